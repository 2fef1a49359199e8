"""GPU tests of generalized ICP (clipper_hip_estimate_covariances, clipper_hip_icp_generalized: k_icp.hip.h,
host_icp.hpp) against the numpy model tests/gicp_model.py. Every comparison with the model is an equality of bits:
T_out, every history row, iterations, status and count; every covariance entry. The recipe is the one
tests/test_gicp_model.py shows to be a working refinement; the other clouds are the smallest that reach an edge of the
kernels (the addition tree's 255 / 256 / 257, its second level at 65 537 source points, a T_init that turns the source's
covariances, too few inliers, a rank-deficient system, neighbourhoods below three points). A model run is computed once
and shared."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration
from tests import features_model as fm
from tests import gicp_model as gm
from tests import icp_model as im

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH = {abi.KNN_BRUTE: "brute", abi.KNN_GRID: "grid"}
IDENTITY6 = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0])


@functools.lru_cache(maxsize=None)
def case(name):
    """(src, C_src, tgt, C_tgt, T_init, max_distance, max_iterations) of a named input; the covariances are the model's"""
    T0, maxd, iters, cs = None, 0.1, 30, None
    if name == "recipe":
        src, tgt, _ = im.recipe()
    elif name == "noisy":
        src, tgt, _ = im.recipe(noise=0.002, seed=1)
    elif name == "shifted":
        src, tgt, _ = im.recipe(offset=1.0e6)
    elif name == "identical":
        _, tgt, _ = im.recipe(n_tgt=300)
        src = tgt.copy()
    elif name == "quarter_turn":                     # T_init turns the source, and with it its covariances, by 90 degrees
        src, tgt, _ = im.recipe()
        T0 = im.rigid(90.0, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
        src = np.ascontiguousarray(src @ T0[:3, :3])
    elif name.startswith("n_src_"):
        src, tgt, _ = im.recipe(n_src=int(name[6:]), n_tgt=400, seed=2)
    elif name == "two_levels":                       # 257 partials: the second level's strided add
        src, tgt, _ = im.recipe(n_src=65537, noise=0.001, seed=3)
        nv = np.random.default_rng(9).normal(size=(len(src), 3))
        nv /= np.linalg.norm(nv, axis=1)[:, None]
        cs, iters = gm.covariance_of_normal(nv, 1e-3), 1        # (discs about seeded directions: any definite matrices do)
    elif name == "copies":                           # ten copies of one point: ten times the same three equations
        _, tgt, _ = im.recipe(n_tgt=400, seed=2)
        src = np.tile(tgt[7] + (0.01, -0.005, 0.002), (10, 1))
        cs = np.tile(IDENTITY6, (10, 1))
    elif name == "too_few":                          # two inliers under a tiny max_distance
        _, tgt, _ = im.recipe()
        T0 = np.eye(4)
        T0[:3, 3] = (0.5, 0.25, -0.125)
        src = np.concatenate([tgt[:2] - T0[:3, 3], tgt[10:40] + 7.0])
        cs, maxd = np.tile(IDENTITY6, (len(src), 1)), 1e-6
    else:
        raise KeyError(name)
    if cs is None:
        cs = gm.covariances(src)[0]
    return src, cs, tgt, gm.covariances(tgt)[0], T0, maxd, iters


@functools.lru_cache(maxsize=None)
def model(name):
    src, cs, tgt, ct, T0, maxd, iters = case(name)
    return gm.icp_generalized(src, cs, tgt, ct, T0, maxd, iters)


def gpu(name, mode=None):
    src, cs, tgt, ct, T0, maxd, iters = case(name)
    return registration.icp_generalized(src, tgt, T0, cs, ct, max_distance=maxd, max_iterations=iters,
                                        search=None if mode is None else SEARCH[mode])


def bits(T, info):
    return (T.tobytes(), info.history.tobytes(), info.iterations, info.status, info.count, info.fitness, info.inlier_rmse)


def model_bits(r):
    return (r.T.tobytes(), r.history[:r.iterations + 1].tobytes(), r.iterations, r.status, r.count, r.fitness, r.rmse)


@pytest.mark.parametrize("name", ["recipe", "noisy", "shifted", "identical"])
def test_equals_the_model_on_both_routes_and_twice(name):
    want = model(name)
    assert want.status == im.CONVERGED and want.fitness == 1.0
    runs = {}
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        T, info = gpu(name, mode)
        assert info.route == mode and (info.candidates > 0) == (mode == abi.KNN_GRID)
        assert (min(info.dim) >= 1) == (mode == abi.KNN_GRID) and info.device_ms > 0.0
        runs[mode] = bits(T, info)
        assert runs[mode] == model_bits(want)
    assert bits(*gpu(name, abi.KNN_GRID)) == runs[abi.KNN_GRID]             # the same run twice
    assert bits(*gpu(name)) == runs[abi.KNN_BRUTE]                          # the process's setting: brute force


def test_T_init_turns_the_covariances_of_the_source():
    want = model("quarter_turn")
    assert want.status == im.CONVERGED and want.fitness == 1.0 and want.iterations >= 3
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        assert bits(*gpu("quarter_turn", mode)) == model_bits(want)
    # and it is the recipe's problem in another frame: the same number of iterations, the same alignment to rounding
    src, _, _, _, T0, _, _ = case("quarter_turn")
    T, info = gpu("quarter_turn")
    Tr, inr = gpu("recipe")
    assert info.iterations == inr.iterations and np.abs(T @ np.linalg.inv(T0) - Tr).max() < 1e-9


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_edges_of_the_addition_tree(n):
    want = model(f"n_src_{n}")
    assert want.status == (im.TOO_FEW if n == 1 else im.CONVERGED)
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        assert bits(*gpu(f"n_src_{n}", mode)) == model_bits(want)


def test_second_level_of_the_tree():
    want = model("two_levels")
    assert want.status == im.MAX_ITERATIONS and want.iterations == 1 and want.count > 60000
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        assert bits(*gpu("two_levels", mode)) == model_bits(want)


def test_rank_deficient_system_is_degenerate():
    want = model("copies")
    assert want.status == im.DEGENERATE and want.iterations == 0 and want.count == 10
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        T, info = gpu("copies", mode)
        assert info.status == abi.ICP_DEGENERATE and T.tobytes() == np.eye(4).tobytes() and bits(T, info) == model_bits(want)


def test_too_few_inliers_leave_T_init():
    want = model("too_few")
    assert want.status == im.TOO_FEW and want.count == 2
    T0 = case("too_few")[4]
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        T, info = gpu("too_few", mode)
        assert info.status == abi.ICP_TOO_FEW and T.tobytes() == T0.tobytes() and bits(T, info) == model_bits(want)


# ---- the covariances ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cov_model(name, knn, radius, eps):
    P = {"bunny": fm.bunny, "radius": fm.radius_cloud, "n1": lambda: fm.uniform_cloud(1, 1),
         "n257": lambda: fm.uniform_cloud(257, 41)}[name]()
    return (P,) + gm.covariances(P, knn, radius, eps)


@pytest.mark.parametrize("knn", [3, 20, 32])
def test_covariances_equal_the_model_on_both_routes(knn):
    P, want, cnt, _ = cov_model("bunny", knn, 0.0, 1e-3)
    for mode in ("brute", "grid"):
        got = registration.estimate_covariances(P, knn=knn, search=mode)
        assert got.shape == (len(P), 6) and got.tobytes() == want.tobytes()
    w = np.linalg.eigvalsh(gm.full(got))
    assert np.abs(w - np.array([1e-3, 1.0, 1.0])).max() < 1e-12


@pytest.mark.parametrize("name,knn,radius", [("radius", 16, 0.25), ("n1", 20, 0.0), ("n257", 20, 0.0)])
def test_covariances_of_short_neighbourhoods_and_odd_sizes(name, knn, radius):
    P, want, cnt, _ = cov_model(name, knn, radius, 1e-3)
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        prev = abi.knn_set_search(mode)
        try:
            got, gcnt = abi.estimate_covariances(P.T, knn=knn, radius=radius, return_counts=True)
        finally:
            abi.knn_set_search(prev)
        assert np.array_equal(gcnt, cnt) and np.ascontiguousarray(got.T).tobytes() == want.tobytes()
    few = cnt < 3
    assert few.any() == (name != "n257") and np.array_equal(want[few], np.tile(IDENTITY6, (few.sum(), 1)))


@pytest.mark.parametrize("eps", [1e-3, 0.25, 1.0])
def test_covariances_are_the_rule_over_the_device_normals(eps):
    """the same neighbourhood, the same eigenvector: the normals of clipper_hip_estimate_normals through the rule in
    numpy give the covariances bit for bit (the sign rule of the normals cancels in every product); below three
    neighbours the normal is a fixed one and the covariance the identity"""
    P = fm.radius_cloud()
    prev = abi.knn_set_search(abi.KNN_GRID)
    try:
        N, ncnt = abi.estimate_normals(P.T, knn=16, radius=0.25, return_counts=True)
        got, cnt = abi.estimate_covariances(P.T, knn=16, radius=0.25, epsilon=eps, return_counts=True)
    finally:
        abi.knn_set_search(prev)
    assert np.array_equal(cnt, ncnt) and (cnt < 3).sum() >= 20 and (cnt >= 3).sum() > 250
    want = np.where((cnt < 3)[:, None], IDENTITY6, gm.covariance_of_normal(N.T, eps))
    assert np.ascontiguousarray(got.T).tobytes() == np.ascontiguousarray(want).tobytes()
    if eps == 1.0:
        assert np.array_equal(got.T, np.tile(IDENTITY6, (len(P), 1)))


def test_covariances_left_out_are_estimated_in_the_call():
    src, _, tgt, _, _, _, _ = case("noisy")
    for mode in ("brute", "grid"):
        cs = registration.estimate_covariances(src, knn=12, epsilon=1e-2, search=mode)
        ct = registration.estimate_covariances(tgt, knn=12, epsilon=1e-2, search=mode)
        two = registration.icp_generalized(src, tgt, None, cs, ct, max_distance=0.1, search=mode)
        one = registration.icp_generalized(src, tgt, covariance_knn=12, epsilon=1e-2, max_distance=0.1, search=mode)
        half = registration.icp_generalized(src, tgt, target_covariances=ct, covariance_knn=12, epsilon=1e-2, max_distance=0.1,
                                            search=mode)
        assert bits(*one) == bits(*two) == bits(*half) and one[1].status == abi.ICP_CONVERGED
    cm, ctm = gm.covariances(src, 12, 0.0, 1e-2)[0], gm.covariances(tgt, 12, 0.0, 1e-2)[0]
    assert bits(*one) == model_bits(gm.icp_generalized(src, cm, tgt, ctm, None, 0.1, 30))


# ---- the facades ---------------------------------------------------------------------------------------------------------

def test_python_surfaces_return_the_abi_bits():
    src, cs, tgt, ct, _, _, _ = case("noisy")
    T, info = abi.icp_generalized(src.T, cs.T, tgt.T, ct.T, max_distance=0.1)
    assert bits(T, info) == model_bits(model("noisy"))
    cp = clipper_amd.load_clipperpy()
    f = np.asfortranarray
    Cc = cp.utils.estimate_covariances(f(tgt.T))
    assert np.asarray(Cc).shape == (6, len(tgt)) and np.ascontiguousarray(np.asarray(Cc).T).tobytes() == ct.tobytes()
    Tc, ic = cp.utils.icp_generalized(f(src.T), f(cs.T), f(tgt.T), f(ct.T), np.eye(4), 0.1)
    assert np.asarray(Tc).tobytes() == T.tobytes()
    assert (ic["iterations"], ic["status"], ic["count"], ic["fitness"], ic["inlier_rmse"]) == (
        info.iterations, info.status, info.count, info.fitness, info.inlier_rmse)
    assert np.asarray(ic["history"]).tobytes() == info.history.tobytes()
    with pytest.raises(ValueError, match="max_distance must be positive"):
        cp.utils.icp_generalized(f(src.T), f(cs.T), f(tgt.T), f(ct.T), np.eye(4), 0.0)
    with pytest.raises(ValueError, match="epsilon must be in"):
        cp.utils.estimate_covariances(f(tgt.T), 20, 0.0, 0.0)


def test_cpp_facade_gicp(tmp_path):
    src, cs, tgt, ct, _, _, _ = case("noisy")
    exe = str(tmp_path / "test_gicp_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_gicp_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    files = [str(tmp_path / f) for f in ("src.f64", "tgt.f64", "C_tgt.f64", "T.f64")]
    src.tofile(files[0])                            # row-major n x 3 = column-major 3 x n
    tgt.tofile(files[1])
    out = subprocess.run([exe, str(len(src)), str(len(tgt))] + files, capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "ALL GICP FACADE TESTS PASSED" in out.stdout
    assert np.fromfile(files[2]).reshape(-1, 6).tobytes() == ct.tobytes()
    assert np.fromfile(files[3]).reshape(4, 4).T.tobytes() == model("noisy").T.tobytes()


def test_device_out_of_range_is_refused():
    """as the other stand-alone entries refuse it: the arguments are checked first, then the device"""
    L = abi.load_library()
    dp = abi._dp
    P = np.asfortranarray(np.random.default_rng(8).random((3, 8)))
    I6 = np.asfortranarray(np.tile(IDENTITY6[:, None], (1, 8)))
    T, out = np.zeros(16), np.zeros((6, 8), order="F")
    prm, nb = abi.IcpParams(abi.ICP_GENERALIZED, 0.5, 2), abi.Neighborhood(4)
    rc = L.clipper_hip_icp_generalized(4096, dp(P), dp(I6), 8, dp(P), dp(I6), 8, None, C.byref(prm), dp(T), None, None)
    assert rc == -1 and "device 4096 out of range" in abi._last_error()
    rc = L.clipper_hip_estimate_covariances(-1, dp(P), 8, C.byref(nb), 1e-3, dp(out), None)
    assert rc == -1 and "device -1 out of range" in abi._last_error()
    bad = abi.IcpParams(abi.ICP_GENERALIZED, 0.0, 2)
    rc = L.clipper_hip_icp_generalized(4096, dp(P), dp(I6), 8, dp(P), dp(I6), 8, None, C.byref(bad), dp(T), None, None)
    assert rc == -1 and "max_distance must be positive" in abi._last_error()
    assert L.clipper_hip_estimate_covariances(0, dp(P), 8, C.byref(nb), 1e-3, dp(out), None) == 0
