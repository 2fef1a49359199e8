"""GPU tests of the ICP refinement (clipper_hip_icp, clipper_hip_evaluate_registration: k_icp.hip.h, host_icp.hpp)
against the numpy model tests/icp_model.py. Every comparison with the model is an equality of bits: T_out, every
history row, iterations, status and count. The recipe is the one tests/test_icp_model.py shows to be a working ICP; the
other clouds are the smallest that reach an edge of the kernels (the addition tree's 255 / 256 / 257, its second level
at 65 537 source points, a source outside the grid, clouds far from the origin, too few inliers, a rank-deficient
system). A model run is computed once and shared."""
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
from tests import icp_model as im

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = [im.POINT, im.PLANE]
SEARCH = {abi.KNN_BRUTE: "brute", abi.KNN_GRID: "grid"}


@functools.lru_cache(maxsize=None)
def case(name):
    """(src, tgt, normals, T_init, max_distance, max_iterations) of a named input"""
    if name == "recipe":
        src, tgt, _ = im.recipe()
    elif name == "noisy":
        src, tgt, _ = im.recipe(noise=0.002, seed=1)
    elif name.startswith("n_src_"):
        src, tgt, _ = im.recipe(n_src=int(name[6:]), n_tgt=400, seed=2)
    elif name == "two_levels":                       # 257 partials: the second level's strided add
        src, tgt, _ = im.recipe(n_src=65537, noise=0.001, seed=3)
        return src, tgt, im.plane_normals(tgt), None, 0.1, 1
    elif name == "outside":                          # the source 50 units off the target's box; every point still an inlier
        src, tgt, _ = im.recipe(seed=4)
        T0 = np.eye(4)
        T0[:3, 3] = (50.0, -50.0, 50.0)
        return src, tgt, im.plane_normals(tgt), T0, 200.0, 3
    elif name == "shifted":
        src, tgt, _ = im.recipe(offset=1.0e6)
    elif name == "identical":
        _, tgt, _ = im.recipe(n_tgt=300)
        src = tgt.copy()
    elif name == "one_target":                       # every source point nearest to target point 0
        rng = np.random.default_rng(6)
        tgt = np.concatenate([np.zeros((1, 3)), 10.0 + rng.random((19, 3))])
        src = 0.1 * (rng.random((50, 3)) - 0.5)
        return src, tgt, None, None, 1.0, 5
    elif name == "planar":                           # a planar target with parallel normals: three open degrees of freedom
        rng = np.random.default_rng(3)
        tgt = np.concatenate([rng.random((400, 2)), np.zeros((400, 1))], axis=1)
        src = tgt[:100] + (0.01, 0.0, 0.02)
        return src, tgt, np.tile((0.0, 0.0, 1.0), (400, 1)), None, 0.1, 30
    else:
        raise KeyError(name)
    return src, tgt, im.plane_normals(tgt), None, 0.1, 30


@functools.lru_cache(maxsize=None)
def model(name, method):
    src, tgt, normals, T0, maxd, iters = case(name)
    return im.icp(src, tgt, T0, method, normals if method == im.PLANE else None, maxd, iters)


def gpu(name, method, mode=None):
    src, tgt, normals, T0, maxd, iters = case(name)
    kind = "plane" if method == im.PLANE else "point"
    return registration.icp(src, tgt, T0, kind, normals if method == im.PLANE else None, maxd, iters,
                            search=None if mode is None else SEARCH[mode])


def bits(T, info):
    return (T.tobytes(), info.history.tobytes(), info.iterations, info.status, info.count, info.fitness, info.inlier_rmse)


def model_bits(r):
    return (r.T.tobytes(), r.history[:r.iterations + 1].tobytes(), r.iterations, r.status, r.count, r.fitness, r.rmse)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["recipe", "noisy", "shifted", "identical"])
def test_equals_the_model_on_both_routes_and_twice(name, method):
    want = model(name, method)
    assert want.status == im.CONVERGED and want.fitness == 1.0
    runs = {}
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        T, info = gpu(name, method, mode)
        assert info.route == mode and (info.candidates > 0) == (mode == abi.KNN_GRID)
        assert (min(info.dim) >= 1) == (mode == abi.KNN_GRID) and info.device_ms > 0.0
        runs[mode] = bits(T, info)
        assert runs[mode] == model_bits(want)
    assert bits(*gpu(name, method, abi.KNN_GRID)) == runs[abi.KNN_GRID]             # the same run twice
    assert bits(*gpu(name, method)) == runs[abi.KNN_BRUTE]                          # the process's setting: brute force


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_edges_of_the_addition_tree(n, method):
    want = model(f"n_src_{n}", method)
    assert want.status == (im.TOO_FEW if n == 1 else im.CONVERGED)
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        assert bits(*gpu(f"n_src_{n}", method, mode)) == model_bits(want)


@pytest.mark.parametrize("method", METHODS)
def test_second_level_of_the_tree(method):
    want = model("two_levels", method)
    assert want.status == im.MAX_ITERATIONS and want.iterations == 1 and want.count > 60000
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        assert bits(*gpu("two_levels", method, mode)) == model_bits(want)


@pytest.mark.parametrize("method", METHODS)
def test_source_far_outside_the_grid(method):
    want = model("outside", method)
    assert want.history[0, 1] == 1.0 and want.history[0, 2] > 50.0
    b, g = gpu("outside", method, abi.KNN_BRUTE), gpu("outside", method, abi.KNN_GRID)
    assert g[1].route == abi.KNN_GRID and bits(*g) == bits(*b) == model_bits(want)


def test_evaluate_only_equals_evaluate_registration():
    src, tgt, normals, _, _, _ = case("recipe")
    T0 = im.rigid(3.0, (0.0, 1.0, 0.0), (0.01, 0.0, -0.02))
    want = im.evaluate(src, tgt, T0, 0.05)
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        fit, rmse, cnt, corr = registration.evaluate_registration(src, tgt, T0, 0.05, search=SEARCH[mode], return_correspondences=True)
        assert (fit, rmse, cnt) == want[:3] and np.array_equal(corr, want[3]) and 0 < cnt < len(src)
        T, info = registration.icp(src, tgt, T0, "plane", normals, 0.05, max_iterations=0, search=SEARCH[mode])
        assert info.status == abi.ICP_MAX_ITERATIONS and info.iterations == 0 and T.tobytes() == T0.tobytes()
        assert (info.fitness, info.inlier_rmse, info.count) == (fit, rmse, cnt) and info.history.shape == (1, 3)
        # the correspondences are clipper_hip_knn's K = 1 entries of the moved source, gated by the distance
        idx, sqd = abi.knn(im.transform(T0, src).T, tgt.T, 1)
        assert np.array_equal(corr, np.where(sqd[:, 0] <= np.float64(0.05) * np.float64(0.05), idx[:, 0], -1))


@pytest.mark.parametrize("inliers,method", [(0, im.POINT), (2, im.POINT), (5, im.PLANE)])
def test_too_few_inliers_leave_T_init(inliers, method):
    _, tgt, normals, _, _, _ = case("recipe")
    T0 = np.eye(4)
    T0[:3, 3] = (0.5, 0.25, -0.125)
    src = np.concatenate([tgt[:inliers] - T0[:3, 3], tgt[10:40] + 7.0])
    want = im.icp(src, tgt, T0, method, normals, 1e-6, 30)
    assert want.status == im.TOO_FEW and want.count == inliers
    for mode in ("brute", "grid"):
        T, info = registration.icp(src, tgt, T0, "plane" if method == im.PLANE else "point", normals, 1e-6, search=mode)
        assert info.status == abi.ICP_TOO_FEW and T.tobytes() == T0.tobytes() and bits(T, info) == model_bits(want)


def test_degenerate_inputs():
    want = model("planar", im.PLANE)
    assert want.status == im.DEGENERATE
    T, info = gpu("planar", im.PLANE, abi.KNN_GRID)
    assert info.status == abi.ICP_DEGENERATE and np.all(np.isfinite(T)) and bits(T, info) == model_bits(want)
    want = model("one_target", im.POINT)
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        T, info = gpu("one_target", im.POINT, mode)
        assert np.all(np.isfinite(T)) and bits(T, info) == model_bits(want)


def test_python_surfaces_return_the_abi_bits():
    src, tgt, normals, _, _, _ = case("noisy")
    T, info = abi.icp(src.T, tgt.T, None, abi.ICP_POINT_TO_PLANE, normals.T, 0.1)
    assert bits(T, info) == model_bits(model("noisy", im.PLANE))
    cp = clipper_amd.load_clipperpy()
    Tc, ic = cp.utils.icp(np.asfortranarray(src.T), np.asfortranarray(tgt.T), np.eye(4), "plane", np.asfortranarray(normals.T), 0.1)
    assert np.asarray(Tc).tobytes() == T.tobytes()
    assert (ic["iterations"], ic["status"], ic["count"], ic["fitness"], ic["inlier_rmse"]) == (
        info.iterations, info.status, info.count, info.fitness, info.inlier_rmse)
    assert np.asarray(ic["history"]).tobytes() == info.history.tobytes()
    fit, rmse, cnt = cp.utils.evaluate_registration(np.asfortranarray(src.T), np.asfortranarray(tgt.T), np.asarray(Tc), 0.1)
    assert (fit, rmse, cnt) == abi.evaluate_registration(src.T, tgt.T, T, 0.1)
    with pytest.raises(ValueError, match="max_distance must be positive"):
        cp.utils.icp(np.asfortranarray(src.T), np.asfortranarray(tgt.T), np.eye(4), "point", np.zeros((3, 0), order="F"), 0.0)


def test_cpp_facade_icp(tmp_path):
    src, tgt, normals, _, _, _ = case("noisy")
    exe = str(tmp_path / "test_icp_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_icp_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    files = [str(tmp_path / f) for f in ("src.f64", "tgt.f64", "nrm.f64", "T_point.f64", "T_plane.f64")]
    src.tofile(files[0])                            # row-major n x 3 = column-major 3 x n
    tgt.tofile(files[1])
    normals.tofile(files[2])
    out = subprocess.run([exe, str(len(src)), str(len(tgt))] + files, capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "ALL ICP FACADE TESTS PASSED" in out.stdout
    for f, method in ((files[3], im.POINT), (files[4], im.PLANE)):
        assert np.fromfile(f).reshape(4, 4).T.tobytes() == model("noisy", method).T.tobytes()


def test_end_to_end_with_refinement():
    """tests/test_gpu_features.py's raw-cloud route (normals, FPFH, mutual matches, fill, solve, closed-form transform
    over the selected associations), then the step it stopped short of: ICP over the whole clouds against a NOISY copy
    of the second view (uniform +-1e-4, a thousandth of the model's size), started from the closed-form transform. The
    refined transform equals the model's from the same T_init bit for bit, and its translation error stays below the
    noise amplitude."""
    P = fm.bunny()
    Q, perm, T_true = fm.transformed_copy(P)
    F0 = registration.compute_fpfh(P, knn=16, viewpoint=P.mean(axis=0))
    F1 = registration.compute_fpfh(Q, knn=16, viewpoint=Q.mean(axis=0))
    A, _ = registration.match_descriptors(F0, F1, knn=1, mutual=True)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(P.T, Q.T, A, sigma=5e-6, epsilon=1e-5)
    s = g.solve(np.random.default_rng(4).random(len(A)))
    T0 = abi.estimate_rigid_transform(P.T, Q.T, A[s.nodes])
    amp = 1e-4
    Qn = Q + np.random.default_rng(8).uniform(-amp, amp, Q.shape)
    Nq = registration.estimate_normals(Qn, knn=16, viewpoint=Qn.mean(axis=0))
    for kind, method in (("point", im.POINT), ("plane", im.PLANE)):
        want = im.icp(P, Qn, T0, method, Nq, 0.005, 30)
        T, info = registration.icp(P, Qn, T0, kind, Nq, max_distance=0.005, search="grid")
        assert bits(T, info) == model_bits(want) and info.status == abi.ICP_CONVERGED and info.fitness == 1.0
        rot, trans = im.transform_error(T_true, T)
        print(f"{kind}: {info.iterations} iterations, rmse {info.inlier_rmse:.3g}, rotation error {rot:.3g} rad, translation error {trans:.3g}")
        assert trans < amp
