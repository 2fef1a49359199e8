"""CPU test that ties the generalized part of clipper_amd/csrc/icp_rules.hpp to tests/gicp_model.py without a GPU:
tests/cpp/test_gicp_rules.cpp (g++ -ffp-contract=off) runs whole generalized ICPs and the covariance rule on the host
from the header, with the addition tree as the kernels run it, and prints bit patterns; here they are compared with the
numpy model bit for bit. Run without a case, the program checks the argument checks the two calls add and feeds a pair
with a singular C_b + R C_a R^T to the terms: DEGENERATE, T unchanged."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import features_model as fm
from tests import gicp_model as gm
from tests import icp_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gicp_rules") / "test_gicp_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_gicp_rules.cpp"), "-o", out])
    return out


def test_checks_and_the_singular_pair(exe):
    out = subprocess.check_output([exe], timeout=60).decode()
    assert "gicp checks ok" in out and "FAILED" not in out, out


def _run(exe, tmp_path, src, cs, tgt, ct, T0, max_distance, max_iterations, rel=1e-6):
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<4i3d", max_iterations, len(src), len(tgt), 0, max_distance, rel, rel))
        f.write(np.asarray(T0, np.float64).T.tobytes())          # column-major
        for a in (src, cs, tgt, ct):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    lines = subprocess.check_output([exe, "icp", str(path)], timeout=300).decode().splitlines()
    head = lines[0].split()
    T = np.array([int(x, 16) for x in lines[1].split()[1:]], np.uint64).view(np.float64).reshape(4, 4).T
    hist = np.array([int(x, 16) for x in lines[2].split()[1:]], np.uint64).view(np.float64).reshape(-1, 3)
    return int(head[1]), int(head[3]), int(head[5]), T, hist


QUARTER = im.rigid(90.0, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0))

CASES = {
    # name: (recipe arguments, T_init, max_distance, max_iterations)
    "recipe": (dict(), None, 0.1, 30),
    "noisy": (dict(noise=0.002, seed=1), None, 0.1, 30),
    "shifted": (dict(offset=1.0e6), None, 0.1, 30),
    "odd": (dict(n_src=257, n_tgt=400, seed=2), None, 0.1, 30),
    "quarter_turn": (dict(), QUARTER, 0.1, 30),                  # the covariances of the source in a frame of their own
    "two_levels": (dict(n_tgt=200, n_src=65537 // 64), None, 0.1, 4),     # (the tree's second level: 5 partials)
    "too_few": (dict(), None, 1e-9, 30),
    "evaluate_only": (dict(), None, 0.1, 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_equals_model_bit_for_bit(exe, tmp_path, name):
    kw, T0, maxd, iters = CASES[name]
    src, tgt, _ = im.recipe(**kw)
    if T0 is not None:
        src = np.ascontiguousarray(src @ T0[:3, :3])             # turned back, so that T_init puts it in place
    cs, ct = gm.covariances(src)[0], gm.covariances(tgt)[0]
    want = gm.icp_generalized(src, cs, tgt, ct, T0, maxd, iters)
    status, iterations, count, T, hist = _run(exe, tmp_path, src, cs, tgt, ct, np.eye(4) if T0 is None else T0, maxd, iters)
    assert (status, iterations, count) == (want.status, want.iterations, want.count)
    assert T.tobytes() == want.T.tobytes()
    assert hist.tobytes() == want.history.tobytes()
    if name in ("recipe", "quarter_turn", "noisy"):
        assert want.status == im.CONVERGED and want.iterations >= 3


def test_rank_deficient_system_is_degenerate(exe, tmp_path):
    """ten copies of one source point: ten times the same three equations, a system of rank 3"""
    _, tgt, _ = im.recipe(n_tgt=400, seed=2)
    src = np.tile(tgt[7] + (0.01, -0.005, 0.002), (10, 1))
    cs, ct = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (10, 1)), gm.covariances(tgt)[0]
    want = gm.icp_generalized(src, cs, tgt, ct, None, 0.1, 30)
    status, iterations, count, T, hist = _run(exe, tmp_path, src, cs, tgt, ct, np.eye(4), 0.1, 30)
    assert status == want.status == im.DEGENERATE and iterations == want.iterations == 0 and count == want.count == 10
    assert T.tobytes() == np.eye(4).tobytes() == want.T.tobytes() and hist.tobytes() == want.history.tobytes()


@pytest.mark.parametrize("name,knn,radius,eps", [("bunny", 20, 0.0, 1e-3), ("bunny", 3, 0.0, 1e-3), ("bunny", 32, 0.02, 0.25),
                                                ("radius", 16, 0.25, 1e-3), ("short", 20, 0.0, 1e-3)])
def test_covariance_rule_equals_model_bit_for_bit(exe, tmp_path, name, knn, radius, eps):
    P = {"bunny": fm.bunny, "radius": fm.radius_cloud, "short": lambda: fm.uniform_cloud(10, 3)}[name]()
    P = np.ascontiguousarray(P[:300])
    path = tmp_path / "cov.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<2i2d", len(P), knn, radius, eps))
        f.write(P.tobytes())
    lines = subprocess.check_output([exe, "cov", str(path)], timeout=300).decode().splitlines()
    C = np.array([int(x, 16) for x in lines[0].split()[1:]], np.uint64).view(np.float64).reshape(-1, 6)
    cnt = np.array([int(x) for x in lines[1].split()[1:]])
    want, wcnt, _ = gm.covariances(P, knn, radius, eps)
    assert np.array_equal(cnt, wcnt) and C.tobytes() == want.tobytes()
    if name == "radius":
        assert (cnt < 3).sum() >= 20
