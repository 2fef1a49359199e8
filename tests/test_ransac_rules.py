"""CPU test that ties clipper_amd/csrc/ransac_rules.hpp to tests/ransac_model.py without a GPU:
tests/cpp/test_ransac_rules.cpp (g++ -ffp-contract=off) runs whole RANSAC calls on the host from the header, with the
fold as the kernels run it, and prints what the call returns as bit patterns; here they are compared with the model
bit for bit: per-hypothesis samples, pass flags and counts for one round of 256, then T, the mask and every info field
for whole runs. Run without a case, the program checks the argument checks of host_ransac_check.hpp."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import ransac_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ransac_rules") / "test_ransac_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-pthread", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ransac_rules.cpp"), "-o", out])
    return out


def test_argument_checks_name_their_values(exe):
    out = subprocess.check_output([exe], timeout=60).decode()
    assert "ransac checks ok" in out and "FAILED" not in out, out


def write_case(path, D1, D2, A, kw):
    P, B = rm.gather(D1, D2, A)
    with open(path, "wb") as f:
        f.write(struct.pack("<3dq4iQ", kw["max_distance"], kw.get("edge_similarity", 0.9), kw.get("confidence", 0.999),
                            kw.get("max_hypotheses", 100000), kw.get("hypotheses_per_round", 4096), kw.get("n_sample", 3),
                            kw.get("refine_iterations", 1), len(P), kw.get("seed", 0)))
        f.write(P.tobytes())
        f.write(B.tobytes())


def run_case(exe, path, threads=1):
    lines = subprocess.check_output([exe, "run", str(path), str(threads)], timeout=300).decode().splitlines()
    head = lines[0].split()
    ints = {head[i]: int(head[i + 1]) for i in range(0, len(head), 2)}
    fr = lines[1].split()
    ints["fitness"], ints["inlier_rmse"] = int(fr[1], 16), int(fr[3], 16)
    ints["sample"] = [int(x) for x in lines[2].split()[1:]]
    T = np.array([int(x, 16) for x in lines[3].split()[1:]], np.uint64).view(np.float64).reshape(4, 4).T
    mask = np.array([c == "1" for c in lines[4].split()[1]])
    return ints, T, mask


def as_bits(x):
    return int(np.float64(x).view(np.uint64))


def assert_equals_model(got, T, mask, want):
    for name in ("status", "refined", "evaluated", "checked", "best_hypothesis", "best_count", "count"):
        assert got[name] == getattr(want, name), name
    assert got["sample"] == want.sample
    assert got["fitness"] == as_bits(want.fitness) and got["inlier_rmse"] == as_bits(want.inlier_rmse)
    assert T.tobytes() == np.ascontiguousarray(want.T).tobytes()
    assert np.array_equal(mask, want.inliers)


CASES = {
    # name: (recipe configuration, keyword arguments)
    "default_checker": (0, dict(max_hypotheses=4096, hypotheses_per_round=1024)),
    "carried_best": (0, dict(max_hypotheses=1024, hypotheses_per_round=256, confidence=0.9999999)),
    "checker_off": (0, dict(max_hypotheses=512, hypotheses_per_round=256, edge_similarity=0.0)),
    "four_points": (0, dict(max_hypotheses=2048, hypotheses_per_round=512, n_sample=4)),
    "eight_points": (2, dict(max_hypotheses=512, hypotheses_per_round=256, n_sample=8, edge_similarity=0.5)),
    "no_polish": (1, dict(max_hypotheses=4096, hypotheses_per_round=1024, refine_iterations=0)),
    "three_polishes": (1, dict(max_hypotheses=4096, hypotheses_per_round=1024, refine_iterations=3)),
    "exact": (2, dict(max_hypotheses=2048, hypotheses_per_round=256)),
    "no_model": (3, dict(max_hypotheses=256, hypotheses_per_round=256, max_distance=1e-9)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_header_equals_model_bit_for_bit(exe, tmp_path, name):
    cfg, kw = CASES[name]
    D1, D2, A, _, _ = rm.recipe(*rm.RECIPE[cfg])
    kw = dict(dict(max_distance=rm.MAX_DISTANCE, seed=cfg), **kw)
    want = rm.ransac(D1, D2, A, **kw)
    write_case(tmp_path / "case.bin", D1, D2, A, kw)
    got, T, mask = run_case(exe, tmp_path / "case.bin")
    assert_equals_model(got, T, mask, want)


def test_threads_do_not_change_the_result(exe, tmp_path):
    D1, D2, A, _, _ = rm.recipe(*rm.RECIPE[0])
    kw = dict(max_distance=rm.MAX_DISTANCE, max_hypotheses=2048, hypotheses_per_round=512)
    write_case(tmp_path / "case.bin", D1, D2, A, kw)
    a, b = run_case(exe, tmp_path / "case.bin", 1), run_case(exe, tmp_path / "case.bin", 5)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("n_sample,edge", [(3, 0.9), (3, 0.0), (4, 0.9), (8, 0.0)])
def test_one_round_hypothesis_by_hypothesis(exe, tmp_path, n_sample, edge):
    D1, D2, A, _, _ = rm.recipe(*rm.RECIPE[0])
    kw = dict(max_distance=rm.MAX_DISTANCE, hypotheses_per_round=256, n_sample=n_sample, edge_similarity=edge, seed=5)
    write_case(tmp_path / "case.bin", D1, D2, A, kw)
    rows = [[int(x) for x in line.split()] for line in
            subprocess.check_output([exe, "table", str(tmp_path / "case.bin")], timeout=300).decode().splitlines()]
    P, B = rm.gather(D1, D2, A)
    s, ok, counts, _ = rm.round_table(P, B, 5, 0, 256, n_sample, np.float64(edge) * np.float64(edge),
                                      np.float64(rm.MAX_DISTANCE) * np.float64(rm.MAX_DISTANCE))
    assert len(rows) == 256
    for g, row in enumerate(rows):
        assert row[0] == g and row[1] == int(ok[g]) and row[2] == int(counts[g]), g
        assert row[3:] == [int(x) for x in s[g]], g
    assert ok.any()
