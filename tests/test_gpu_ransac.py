"""GPU tests of clipper_hip_ransac_correspondences against tests/ransac_model.py. Every comparison with the model is an
equality: the bytes of T, the inlier mask, and every integer and double of the info except device_ms. The shapes are the
smallest that reach an edge: one ballot (m = 63, 64, 65), one workgroup and the first level of the polish's fold
(255, 256, 257), the fold's second level (65 537), one round, a second whole round and a best carried across rounds,
survivor tiles with a partial last tile (checker off), rounds without a survivor, every sample size, the polish taken,
refused and switched off, clouds far from the origin."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration as reg
from tests import icp_model as im
from tests import ransac_model as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def data(cfg, m=None, offset=0.0):
    """the recipe's configuration cfg, optionally with another number of associations; offset shifts both clouds"""
    mm, outrat, sigma, seed = rm.RECIPE[cfg]
    D1, D2, A, Agt, T = rm.recipe(mm if m is None else m, outrat, sigma, seed)
    for x in (D1, D2, A, Agt, T):
        x.setflags(write=False)
    return (D1 + offset, D2 + offset, A, Agt, T) if offset else (D1, D2, A, Agt, T)


def info_tuple(info):
    return (info.status, info.refined, info.evaluated, info.checked, info.best_hypothesis, info.best_count, info.count,
            np.float64(info.fitness).tobytes(), np.float64(info.inlier_rmse).tobytes(), list(info.sample))


def model_tuple(r):
    return (r.status, r.refined, r.evaluated, r.checked, r.best_hypothesis, r.best_count, r.count,
            np.float64(r.fitness).tobytes(), np.float64(r.inlier_rmse).tobytes(), list(r.sample))


def check(D1, D2, A, **kw):
    """the device against the model: everything the call returns"""
    want = rm.ransac(D1, D2, A, **kw)
    T, info = reg.ransac_correspondences(D1, D2, A, **kw)
    assert info_tuple(info) == model_tuple(want)
    assert T.tobytes() == np.ascontiguousarray(want.T).tobytes()
    assert info.inliers.dtype == bool and np.array_equal(info.inliers, want.inliers)
    assert info.device_ms > 0.0
    return want, T, info


SMALL = dict(max_distance=rm.MAX_DISTANCE, hypotheses_per_round=256, max_hypotheses=1024)


def test_three_exact_associations_take_the_first_valid_hypothesis():
    D1, D2, A, _, _ = data(2)
    want, _, info = check(D1, D2, A[:3], **dict(SMALL, max_hypotheses=256))
    assert want.best_count == 3 and want.count == 3 and info.inliers.all()
    s2, d2 = np.float64(0.9) * np.float64(0.9), np.float64(rm.MAX_DISTANCE) * np.float64(rm.MAX_DISTANCE)
    ok = rm.round_table(*rm.gather(D1, D2, A[:3]), 0, 0, 256, 3, s2, d2)[1]
    assert want.best_hypothesis == int(np.flatnonzero(ok)[0])          # every valid hypothesis counts 3: the tie rule


@pytest.mark.parametrize("m", [63, 64, 65, 255, 256, 257])
def test_ballot_and_workgroup_edges(m):
    D1, D2, A, _, _ = data(0, m)
    want, _, _ = check(D1, D2, A, **SMALL)
    assert want.status != rm.NO_MODEL


def test_second_level_of_the_fold():
    """65 537 associations: 257 partials, one more than a fold round holds. Half of them repeat the 500 exact pairs."""
    D1, D2, _, _, _ = data(2)
    rng = np.random.default_rng(9)
    good = np.stack([np.arange(500)] * 2, axis=1)
    A = np.concatenate([np.tile(good, (66, 1))[:32768], np.stack([rng.integers(0, 500, 32769), rng.integers(0, 550, 32769)], axis=1)])
    A = np.ascontiguousarray(A[rng.permutation(len(A))].astype(np.int32))
    assert len(A) == 65537
    want, _, _ = check(D1, D2, A, **dict(SMALL, max_hypotheses=256, refine_iterations=2))
    assert want.status == rm.CONVERGED and want.count >= 32768


@pytest.mark.parametrize("max_hypotheses,evaluated,status", [(256, 256, rm.MAX_HYPOTHESES), (257, 512, rm.MAX_HYPOTHESES),
                                                              (1024, 1024, rm.CONVERGED)])
def test_rounds_and_the_stop_rule(max_hypotheses, evaluated, status):
    D1, D2, A, _, _ = data(0)
    want, _, _ = check(D1, D2, A, **dict(SMALL, max_hypotheses=max_hypotheses))
    assert (want.evaluated, want.status) == (evaluated, status)
    assert want.best_hypothesis < 256                                  # the winner sits in round 0 and is carried


def test_winner_in_a_later_round():
    D1, D2, A, _, _ = data(1)
    want, _, _ = check(D1, D2, A, **dict(SMALL, max_hypotheses=16384, seed=1))
    assert want.best_hypothesis >= 256 and want.status == rm.CONVERGED and want.evaluated > 256


def test_checker_off_fills_the_survivor_tiles():
    D1, D2, A, _, _ = data(0)
    want, _, _ = check(D1, D2, A, **dict(SMALL, max_hypotheses=512, edge_similarity=0.0))
    assert all(r > 200 and r % 16 != 0 for r in want.rounds)           # many tiles, the last one partial


def test_rounds_without_a_survivor_give_no_model():
    D1, D2, A, Agt, _ = data(0)
    want, T, info = check(D1, D2, A[len(Agt):], **dict(SMALL, max_hypotheses=512, edge_similarity=0.9999))
    assert want.rounds == [0, 0] and want.status == rm.NO_MODEL
    assert np.array_equal(T, np.eye(4)) and info.best_hypothesis == -1 and list(info.sample) == [-1] * 8


def test_one_shared_source_point_gives_no_model():
    D1, D2, A, _, _ = data(0)
    A = A.copy()
    A[:, 0] = 7
    want, T, _ = check(D1, D2, A, **dict(SMALL, max_hypotheses=512, edge_similarity=0.0))
    assert want.status == rm.NO_MODEL and want.checked == 0 and np.array_equal(T, np.eye(4))


@pytest.mark.parametrize("n_sample", [3, 4, 8])
def test_sample_sizes(n_sample):
    D1, D2, A, _, _ = data(2)
    want, _, _ = check(D1, D2, A[:60], **dict(SMALL, max_hypotheses=512, n_sample=n_sample, edge_similarity=0.5))
    assert want.status != rm.NO_MODEL and want.sample[n_sample - 1] >= 0


@pytest.mark.parametrize("refine_iterations", [0, 1, 3])
def test_polish(refine_iterations):
    D1, D2, A, _, _ = data(1)
    want, _, _ = check(D1, D2, A, **dict(SMALL, max_hypotheses=8192, seed=1, refine_iterations=refine_iterations))
    assert want.refined <= refine_iterations and (refine_iterations == 0 or want.refined >= 1)


def test_a_refused_polish_step_keeps_the_hypothesis():
    D1, D2, A, _, _ = data(0)
    want, T, _ = check(D1, D2, A, **dict(SMALL, seed=1, refine_iterations=3))
    assert want.rejected and want.refined == 0 and T.tobytes() == np.ascontiguousarray(want.T_hypothesis).tobytes()


def test_clouds_far_from_the_origin():
    D1, D2, A, _, _ = data(0, offset=1.0e6)
    want, _, _ = check(D1, D2, A, **SMALL)
    assert want.status != rm.NO_MODEL


def test_same_call_same_bytes_and_seeds_differ():
    D1, D2, A, _, _ = data(0)
    a = reg.ransac_correspondences(D1, D2, A, **SMALL)
    b = reg.ransac_correspondences(D1, D2, A, **SMALL)
    c = reg.ransac_correspondences(D1, D2, A, **dict(SMALL, seed=1))
    assert a[0].tobytes() == b[0].tobytes() and info_tuple(a[1]) == info_tuple(b[1]) and np.array_equal(a[1].inliers, b[1].inliers)
    assert a[1].best_hypothesis != c[1].best_hypothesis


def test_every_surface_gives_the_same_bytes(tmp_path):
    D1, D2, A, _, _ = data(0)
    T, info = reg.ransac_correspondences(D1, D2, A, **SMALL)
    # clipperpy.utils
    cp = clipper_amd.load_clipperpy()
    T2, d = cp.utils.ransac_correspondences(D1, D2, A, **SMALL)
    assert np.asarray(T2).tobytes() == T.tobytes() and np.array_equal(np.asarray(d["inliers"]), info.inliers)
    assert (d["status"], d["refined"], d["evaluated"], d["checked"], d["best_hypothesis"], d["best_count"], d["count"],
            np.float64(d["fitness"]).tobytes(), np.float64(d["inlier_rmse"]).tobytes(), list(d["sample"])) == info_tuple(info)
    # the C ABI, called directly
    L = abi.load_library()
    d1, d2 = np.asfortranarray(D1), np.asfortranarray(D2)
    a = np.ascontiguousarray(A.T).reshape(-1)
    prm = abi.RansacParams(**SMALL)
    T3, mask, inf3 = np.zeros(16), np.zeros(len(A), np.uint8), abi.RansacInfo()
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = L.clipper_hip_ransac_correspondences(0, dp(d1), 500, dp(d2), 550, a.ctypes.data_as(C.POINTER(C.c_int32)), len(A),
                                              C.byref(prm), dp(T3), mask.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(inf3))
    assert rc == 0 and T3.reshape(4, 4).T.tobytes() == T.tobytes() and np.array_equal(mask.astype(bool), info.inliers)
    assert info_tuple(inf3) == info_tuple(info)
    rc = L.clipper_hip_ransac_correspondences(0, dp(d1), 500, dp(d2), 550, a.ctypes.data_as(C.POINTER(C.c_int32)), len(A),
                                              C.byref(prm), dp(T3), None, None)          # the optional outputs left out
    assert rc == 0 and T3.reshape(4, 4).T.tobytes() == T.tobytes()
    # the C++ facade
    exe = str(tmp_path / "test_ransac_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_ransac_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    files = [str(tmp_path / f) for f in ("D1.f64", "D2.f64", "A.i32", "out.bin")]
    d1.T.tofile(files[0])                           # row-major n x 3 = column-major 3 x n
    d2.T.tofile(files[1])
    a.tofile(files[2])
    out = subprocess.run([exe, "500", "550", str(len(A))] + files, capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0 and "ALL RANSAC FACADE TESTS PASSED" in out.stdout, out.stdout[-2000:] + out.stderr
    raw = open(files[3], "rb").read()
    assert np.frombuffer(raw[:128]).reshape(4, 4).T.tobytes() == T.tobytes()
    assert tuple(np.frombuffer(raw[128:184], np.int64)) == info_tuple(info)[:7]
    assert np.array_equal(np.frombuffer(raw[184:], np.uint8).astype(bool), info.inliers)


def test_a_device_out_of_range_is_refused():
    D1, D2, A, _, _ = data(0)
    with pytest.raises(abi.ClipperError, match="device 12345 out of range"):
        reg.ransac_correspondences(D1, D2, A, device=12345, **SMALL)


def test_pipeline_ransac_then_icp():
    """the first recipe configuration: the mask is the ground truth, and ICP over the whole clouds from T converges"""
    D1, D2, A, Agt, T_true = data(0)
    T, info = reg.ransac_correspondences(D1, D2, A, rm.MAX_DISTANCE, max_hypotheses=16384, hypotheses_per_round=1024)
    truth = np.zeros(len(A), bool)
    truth[:len(Agt)] = True
    assert np.array_equal(info.inliers, truth)
    T2, icp_info = reg.icp(D1.T, D2.T, T_init=T, max_distance=0.05)
    assert icp_info.status == abi.ICP_CONVERGED
    e0, e1 = reg.transform_error(T_true, T), reg.transform_error(T_true, T2)
    assert e0[1] < 0.02 and e1[1] < 0.02
    assert im.CONVERGED == abi.ICP_CONVERGED
