"""CPU test that ties the robust part of clipper_amd/csrc/icp_rules.hpp to tests/icp_robust_model.py without a GPU:
tests/cpp/test_icp_robust_rules.cpp (g++ -ffp-contract=off) runs whole robust and trimmed ICPs on the host from the
header, the trimming threshold found by the header's radix select, and prints T, the history, tau and the sum of the
weights as bit patterns; here they are compared with the numpy model bit for bit. The header's select also runs on crafted
uint64 keys against a sort. Run without a case, the program checks the argument checks of check_robust."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import gicp_model as gm
from tests import icp_model as im
from tests import icp_robust_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("icp_robust_rules") / "test_icp_robust_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_icp_robust_rules.cpp"), "-o", out])
    return out


def test_argument_checks_name_their_values(exe):
    out = subprocess.check_output([exe], timeout=60).decode()
    assert "icp robust checks ok" in out and "FAILED" not in out, out


def _run(exe, tmp_path, src, tgt, method, aux, max_distance, max_iterations, loss, scale, trim, rel=1e-6):
    path = tmp_path / "case.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<6i5d", method, max_iterations, len(src), len(tgt), loss, 0, max_distance, rel, rel, scale, trim))
        f.write(np.eye(4).tobytes())
        f.write(np.ascontiguousarray(src).tobytes())
        f.write(np.ascontiguousarray(tgt).tobytes())
        if method == rm.PLANE:
            f.write(np.ascontiguousarray(aux).tobytes())
        if method == rm.GENERALIZED:
            f.write(np.ascontiguousarray(aux[0]).tobytes())
            f.write(np.ascontiguousarray(aux[1]).tobytes())
    lines = subprocess.check_output([exe, str(path)], timeout=300).decode().splitlines()
    head = lines[0].split()
    T = np.array([int(x, 16) for x in lines[1].split()[1:]], np.uint64).view(np.float64).reshape(4, 4).T
    hist = np.array([int(x, 16) for x in lines[2].split()[1:]], np.uint64).view(np.float64).reshape(-1, 3)
    tau, wsum = np.array([int(x, 16) for x in lines[3].split()[1:]], np.uint64).view(np.float64)
    return (int(head[1]), int(head[3]), int(head[5]), int(head[7])), T, hist, float(tau), float(wsum)


CASES = {
    # name: (clouds, method, loss, scale, trim, max_iterations)
    "point_none": ("recipe", rm.POINT, rm.NONE, 0.0, 1.0, 30),
    "point_huber": ("cluttered", rm.POINT, rm.HUBER, 0.01, 1.0, 40),
    "point_tukey": ("cluttered", rm.POINT, rm.TUKEY, 0.03, 1.0, 40),
    "point_trim": ("cluttered", rm.POINT, rm.NONE, 0.0, 0.6, 40),
    "plane_cauchy": ("cluttered", rm.PLANE, rm.CAUCHY, 0.01, 1.0, 40),
    "plane_geman_mcclure_trim": ("cluttered", rm.PLANE, rm.GEMAN_MCCLURE, 0.01, 0.6, 40),
    "generalized_huber_trim": ("cluttered", rm.GENERALIZED, rm.HUBER, 0.01, 0.6, 40),
    "generalized_none": ("recipe", rm.GENERALIZED, rm.NONE, 0.0, 1.0, 30),
    "two_levels_trim": ("two_levels", rm.POINT, rm.CAUCHY, 0.01, 0.9, 2),          # five partials, 1025 candidates
    "nothing_kept": ("recipe", rm.POINT, rm.HUBER, 0.01, 0.001, 30),                # keep = 0: TOO_FEW
    "zero_weights": ("recipe", rm.PLANE, rm.TUKEY, 1e-9, 1.0, 30),                  # DEGENERATE at iteration 0
    "zero_weights_point": ("recipe", rm.POINT, rm.TUKEY, 1e-9, 1.0, 30),            # 0 / 0 in the centroids
}


def _clouds(name):
    if name == "cluttered":
        return rm.cluttered(0)[:2]
    if name == "two_levels":
        return im.recipe(n_tgt=200, n_src=65537 // 64)[:2]
    return im.recipe()[:2]


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_equals_model_bit_for_bit(exe, tmp_path, name):
    clouds, method, loss, scale, trim, iters = CASES[name]
    src, tgt = _clouds(clouds)
    aux = None
    if method == rm.PLANE:
        aux = im.plane_normals(tgt)
    if method == rm.GENERALIZED:
        aux = (gm.covariances(src)[0], gm.covariances(tgt)[0])
    want = rm.icp_robust(src, tgt, None, method, aux if method == rm.PLANE else None, aux, 0.1, iters, loss=loss,
                         scale=scale, trim=trim)
    head, T, hist, tau, wsum = _run(exe, tmp_path, src, tgt, method, aux, 0.1, iters, loss, scale, trim)
    assert head == (want.status, want.iterations, want.count, want.within)
    assert T.tobytes() == want.T.tobytes() and hist.tobytes() == want.history.tobytes()
    assert (tau, wsum) == (want.trim_sqd, want.weight_sum)
    if name == "nothing_kept":
        assert want.status == im.TOO_FEW and want.count == 0 and want.within > 250 and tau == 0.0
    if name.startswith("zero_weights"):
        assert want.status == im.DEGENERATE and want.iterations == 0 and T.tobytes() == np.eye(4).tobytes()
    if name in ("point_none", "generalized_none"):   # the plain models' bits
        plain = (im.icp(src, tgt, None, im.POINT, None, 0.1, iters) if method == rm.POINT
                 else gm.icp_generalized(src, aux[0], tgt, aux[1], None, 0.1, iters))
        assert T.tobytes() == plain.T.tobytes() and hist.tobytes() == plain.history.tobytes()


def _select(exe, tmp_path, keys, rank):
    path = tmp_path / "keys.bin"
    keys = np.ascontiguousarray(keys, np.uint64)
    with open(path, "wb") as f:
        f.write(struct.pack("<2q", len(keys), rank))
        f.write(keys.tobytes())
    out = subprocess.check_output([exe, "select", str(path)], timeout=60).decode().split()
    return int(out[1], 16)


def test_the_select_on_crafted_keys_against_a_sort(exe, tmp_path):
    rng = np.random.default_rng(11)
    base = np.uint64(0x3FB999999999_0000)
    sets = {
        "lowest byte": base + rng.integers(0, 256, 500).astype(np.uint64),
        "lowest two bytes": base + rng.integers(0, 65536, 500).astype(np.uint64),
        "highest byte": (rng.integers(0, 128, 500).astype(np.uint64) << np.uint64(56)) + np.uint64(0x99999999),
        "all equal": np.full(300, base),
        "every byte": rng.integers(0, 2 ** 63, 1000).astype(np.uint64),
        "one key": np.array([7], np.uint64),
        "squared distances": (rng.random(777) ** 8).view(np.uint64),
    }
    for name, keys in sets.items():
        order = np.sort(keys)
        n = len(keys)
        for rank in sorted(r for r in {1, 2, n // 3 + 1, n // 2, n - 1, n} if 1 <= r <= n):
            assert _select(exe, tmp_path, keys, rank) == int(order[rank - 1]), (name, rank)
