"""CPU test that ties clipper_amd/csrc/icp_rules.hpp to tests/icp_model.py without a GPU: tests/cpp/test_icp_rules.cpp
(g++ -ffp-contract=off) runs whole ICPs on the host from the header, with the addition tree as the kernels run it, and
prints T and the history as bit patterns; here they are compared with the numpy model bit for bit. Run without a case,
the program checks the argument checks of host_icp_check.hpp."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import icp_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("icp_rules") / "test_icp_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_icp_rules.cpp"), "-o", out])
    return out


def test_argument_checks_name_their_values(exe):
    out = subprocess.check_output([exe], timeout=60).decode()
    assert "icp checks ok" in out and "FAILED" not in out, out


def _run(exe, tmp_path, src, tgt, T0, method, normals, max_distance, max_iterations, rel=1e-6):
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<4i3d", method, max_iterations, len(src), len(tgt), max_distance, rel, rel))
        f.write(np.asarray(T0, np.float64).T.tobytes())          # column-major
        f.write(np.ascontiguousarray(src).tobytes())
        f.write(np.ascontiguousarray(tgt).tobytes())
        if method == im.PLANE:
            f.write(np.ascontiguousarray(normals).tobytes())
    lines = subprocess.check_output([exe, str(path)], timeout=300).decode().splitlines()
    head = lines[0].split()
    T = np.array([int(x, 16) for x in lines[1].split()[1:]], np.uint64).view(np.float64).reshape(4, 4).T
    hist = np.array([int(x, 16) for x in lines[2].split()[1:]], np.uint64).view(np.float64).reshape(-1, 3)
    return int(head[1]), int(head[3]), int(head[5]), T, hist


CASES = {
    # name: (recipe arguments, method, max_distance, max_iterations)
    "point": (dict(), im.POINT, 0.1, 30),
    "plane": (dict(), im.PLANE, 0.1, 30),
    "point_noisy": (dict(noise=0.002, seed=1), im.POINT, 0.1, 30),
    "plane_noisy": (dict(noise=0.002, seed=1), im.PLANE, 0.1, 30),
    "point_two_levels": (dict(n_tgt=200, n_src=65537 // 64), im.POINT, 0.1, 4),   # (the tree's second level: 5 partials)
    "point_shifted": (dict(offset=1.0e6), im.POINT, 0.1, 30),
    "too_few": (dict(), im.POINT, 1e-9, 30),
    "evaluate_only": (dict(), im.PLANE, 0.1, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_equals_model_bit_for_bit(exe, tmp_path, name):
    kw, method, maxd, iters = CASES[name]
    src, tgt, _ = im.recipe(**kw)
    normals = im.plane_normals(tgt) if method == im.PLANE else None
    want = im.icp(src, tgt, None, method, normals, maxd, iters)
    status, iterations, count, T, hist = _run(exe, tmp_path, src, tgt, np.eye(4), method, normals, maxd, iters)
    assert (status, iterations, count) == (want.status, want.iterations, want.count)
    assert T.tobytes() == want.T.tobytes()
    assert hist.tobytes() == want.history.tobytes()


def test_degenerate_plane_system(exe, tmp_path):
    """a planar target with parallel normals leaves three degrees of freedom open: DEGENERATE, T untouched"""
    rng = np.random.default_rng(3)
    tgt = np.concatenate([rng.random((400, 2)), np.zeros((400, 1))], axis=1)
    src = tgt[:100] + (0.01, 0.0, 0.02)
    normals = np.tile((0.0, 0.0, 1.0), (400, 1))
    want = im.icp(src, tgt, None, im.PLANE, normals, 0.1, 30)
    status, iterations, count, T, hist = _run(exe, tmp_path, src, tgt, np.eye(4), im.PLANE, normals, 0.1, 30)
    assert status == want.status == im.DEGENERATE and iterations == want.iterations == 0
    assert T.tobytes() == np.eye(4).tobytes() == want.T.tobytes() and hist.tobytes() == want.history.tobytes()
