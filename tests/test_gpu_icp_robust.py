"""GPU tests of robust and trimmed ICP (clipper_hip_icp_robust, clipper_hip_icp_generalized_robust: k_icp.hip.h's weighted
sums, k_select.hip.h's rank select, host_icp.hpp) against the numpy model tests/icp_robust_model.py. Every comparison is
an equality of bits: T_out, every history row, iterations, status, count, fitness, rmse, within and trim_sqd (and the sum
of the weights). The cluttered case is the one tests/test_icp_robust_model.py shows the losses and the trimming to win
on; the other clouds are the smallest that reach an edge of the kernels (the addition tree's 255 / 256 / 257, its second
level and a selection over 33 tiles at 65 537 source points, keys that differ in their lowest bytes only, ties, nothing
kept, all weights zero). A model run is computed once and shared."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration
from tests import gicp_model as gm
from tests import icp_model as im
from tests import icp_robust_model as rm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT, PLANE, GEN = rm.POINT, rm.PLANE, rm.GENERALIZED
METHODS = [POINT, PLANE, GEN]
LOSS_NAMES = {v: k for k, v in rm.LOSSES.items()}
# (loss, scale) at the scales the model's property test uses
LOSSES = [(rm.HUBER, 0.01), (rm.CAUCHY, 0.01), (rm.TUKEY, 0.03), (rm.GEMAN_MCCLURE, 0.01)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(src, tgt, T_init, max_distance, max_iterations) of a named input"""
    T0, maxd, iters = None, 0.1, 30
    if name == "recipe":
        src, tgt, _ = im.recipe()
    elif name == "noisy":
        src, tgt, _ = im.recipe(noise=0.002, seed=1)
    elif name == "cluttered":
        src, tgt, _ = rm.cluttered(0)
        iters = 40
    elif name.startswith("n_src_"):
        src, tgt, _ = im.recipe(n_src=int(name[6:]), n_tgt=400, seed=2)
    elif name == "two_levels":                       # 257 partials, a selection over 33 tiles
        src, tgt, _ = im.recipe(n_src=65537, noise=0.001, seed=3)
        iters = 1
    elif name == "ties":                             # every source point twice
        src, tgt, _ = im.recipe(n_src=150, deg=2.0, shift=0.01, noise=0.001, seed=5)
        src, iters = np.concatenate([src, src]), 0
    elif name == "low_bytes":                        # sqd = (1 + i 2^-52)^2: keys equal in their upper six bytes
        rng = np.random.default_rng(6)
        tgt = np.concatenate([np.zeros((1, 3)), 10.0 + rng.random((19, 3))])
        src = np.zeros((300, 3))
        src[:, 0] = 1.0 + np.arange(300) * 2.0 ** -52
        maxd, iters = 10.0, 0
    elif name == "wide_spread":                      # sqd spread geometrically from 1e-16 to 1e-2
        _, tgt, _ = im.recipe(n_tgt=300)
        r = np.sqrt(np.geomspace(1e-16, 1e-2, 300))
        src, maxd, iters = tgt + np.stack([r, 0 * r, 0 * r], axis=1), 0.2, 0
    elif name == "identical":                        # every sqd is 0
        _, tgt, _ = im.recipe(n_tgt=300)
        src, iters = tgt.copy(), 0
    else:
        raise KeyError(name)
    return src, tgt, T0, maxd, iters


@functools.lru_cache(maxsize=None)
def aux(name):
    """(normals of the target, covariances of the source, of the target): the model's, whatever they are made from"""
    src, tgt, _, _, _ = case(name)
    if name == "two_levels":                         # (discs about seeded directions: any definite matrices do)
        nv = np.random.default_rng(9).normal(size=(len(src), 3))
        nv /= np.linalg.norm(nv, axis=1)[:, None]
        cs = gm.covariance_of_normal(nv, 1e-3)
    else:
        cs = gm.covariances(src)[0]
    return im.plane_normals(tgt), cs, gm.covariances(tgt)[0]


@functools.lru_cache(maxsize=None)
def model(name, method, loss=rm.NONE, scale=0.0, trim=1.0, iters=None):
    src, tgt, T0, maxd, it = case(name)
    n, cs, ct = aux(name) if method != POINT else (None, None, None)
    return rm.icp_robust(src, tgt, T0, method, n, (cs, ct), maxd, it if iters is None else iters, loss=loss, scale=scale,
                         trim=trim)


def gpu(name, method, loss=rm.NONE, scale=0.0, trim=1.0, mode="grid", iters=None):
    """through the ABI's Python functions: the robust entry points whatever the settings"""
    src, tgt, T0, maxd, it = case(name)
    it = it if iters is None else iters
    with registration._knn_search(mode):
        if method == GEN:
            _, cs, ct = aux(name)
            return abi.icp_generalized_robust(src.T, cs.T, tgt.T, ct.T, T0, maxd, it, loss=loss, scale=scale, trim=trim)
        N = aux(name)[0].T if method == PLANE else None
        return abi.icp_robust(src.T, tgt.T, T0, method, N, maxd, it, loss=loss, scale=scale, trim=trim)


def bits(T, info):
    return (T.tobytes(), info.history.tobytes(), info.iterations, info.status, info.count, info.fitness, info.inlier_rmse,
            info.within, info.trim_sqd, info.weight_sum)


def model_bits(r):
    return (r.T.tobytes(), r.history[:r.iterations + 1].tobytes(), r.iterations, r.status, r.count, r.fitness, r.rmse,
            r.within, r.trim_sqd, r.weight_sum)


def plain_bits(T, info):
    return (T.tobytes(), info.history.tobytes(), info.iterations, info.status, info.count, info.fitness, info.inlier_rmse)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["recipe", "noisy"])
def test_none_and_trim_one_equal_the_plain_calls(name, method):
    src, tgt, T0, maxd, iters = case(name)
    for mode in ("brute", "grid"):
        if method == GEN:
            _, cs, ct = aux(name)
            plain = registration.icp_generalized(src, tgt, T0, cs, ct, max_distance=maxd, max_iterations=iters, search=mode)
        else:
            plain = registration.icp(src, tgt, T0, "plane" if method == PLANE else "point",
                                     aux(name)[0] if method == PLANE else None, maxd, iters, search=mode)
        T, info = gpu(name, method, mode=mode)
        assert plain_bits(T, info) == plain_bits(*plain) and info.status == abi.ICP_CONVERGED
        assert info.within == info.count == len(src) and info.trim_sqd == np.float64(maxd) * np.float64(maxd)
        assert info.weight_sum == (float(len(src)) if method == POINT else 0.0)
        assert bits(T, info) == model_bits(model(name, method))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("loss,scale,trim", [(l, s, 1.0) for l, s in LOSSES] + [(rm.NONE, 0.0, 0.6), (rm.HUBER, 0.01, 0.6)],
                         ids=lambda v: LOSS_NAMES.get(v, str(v)) if isinstance(v, int) else str(v))
def test_losses_and_trimming_on_the_cluttered_case(method, loss, scale, trim):
    want = model("cluttered", method, loss, scale, trim)
    assert want.status == im.CONVERGED and 0 < want.count <= want.within < 500
    assert (want.count < want.within) == (trim < 1.0)
    runs = [bits(*gpu("cluttered", method, loss, scale, trim, mode)) for mode in ("brute", "grid", "grid")]
    assert runs[0] == runs[1] == runs[2] == model_bits(want)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_edges_of_the_addition_tree(n, method):
    want = model(f"n_src_{n}", method, rm.HUBER, 0.01, 0.75)
    assert want.status == (im.TOO_FEW if n == 1 else im.CONVERGED)
    for mode in ("brute", "grid"):
        assert bits(*gpu(f"n_src_{n}", method, rm.HUBER, 0.01, 0.75, mode)) == model_bits(want)


@pytest.mark.parametrize("method", METHODS)
def test_second_level_of_the_tree_and_a_selection_over_33_tiles(method):
    want = model("two_levels", method, rm.CAUCHY, 0.01, 0.9)
    assert want.status == im.MAX_ITERATIONS and want.iterations == 1 and 50000 < want.count < want.within
    assert bits(*gpu("two_levels", method, rm.CAUCHY, 0.01, 0.9, "grid")) == model_bits(want)


def _sorted_sqd(name):
    src, tgt, T0, maxd, _ = case(name)
    _, sqd = im.nearest(src if T0 is None else im.transform(T0, src), tgt)
    return np.sort(sqd[sqd <= np.float64(maxd) * np.float64(maxd)])


@pytest.mark.parametrize("name,trim", [("ties", 0.5), ("ties", 0.51), ("low_bytes", 0.5), ("low_bytes", 0.9999), ("low_bytes", 0.001),
                                       ("wide_spread", 0.5), ("wide_spread", 0.05), ("identical", 0.5)])
def test_the_select_against_a_sort(name, trim):
    """evaluate-only: count, within and trim_sqd against np.sort, and the whole result against the model"""
    sqd = _sorted_sqd(name)
    within = len(sqd)
    keep = int(trim * float(within))
    assert within == 300
    T, info = gpu(name, POINT, trim=trim)
    assert info.within == within
    if keep == 0:                                    # nothing kept
        assert (info.status, info.count, info.trim_sqd) == (abi.ICP_TOO_FEW, 0, 0.0)
    else:
        tau = sqd[keep - 1]
        assert info.trim_sqd == tau and info.count == int((sqd <= tau).sum()) and info.status == abi.ICP_MAX_ITERATIONS
    if name == "ties":                               # every distance twice: the count is even, whatever keep is
        assert info.count % 2 == 0 and info.count == keep + keep % 2
    if name == "low_bytes":
        keys = sqd.view(np.uint64)
        assert len(np.unique(keys)) > 100 and len(np.unique(keys >> np.uint64(16))) == 1
        assert keep == {0.5: 150, 0.9999: 299, 0.001: 0}[trim]
    if name == "wide_spread":
        assert len(np.unique(sqd.view(np.uint64) >> np.uint64(56))) > 2      # the first digit already differs
    if name == "identical":
        assert info.trim_sqd == 0.0 and info.count == 300
    assert bits(T, info) == model_bits(model(name, POINT, trim=trim))
    assert bits(*gpu(name, POINT, trim=trim, mode="brute")) == bits(T, info)


@pytest.mark.parametrize("method", METHODS)
def test_all_weights_zero_end_degenerate_with_T_init(method):
    want = model("recipe", method, rm.TUKEY, 1e-9)
    assert want.status == im.DEGENERATE and want.iterations == 0 and want.count > 250 and want.weight_sum == 0.0
    T, info = gpu("recipe", method, rm.TUKEY, 1e-9)
    assert info.status == abi.ICP_DEGENERATE and T.tobytes() == np.eye(4).tobytes()
    assert bits(T, info) == model_bits(want)


def test_facades_return_the_abi_bits(tmp_path):
    src, tgt, T0, maxd, iters = case("cluttered")
    normals = aux("cluttered")[0]
    want = model("cluttered", PLANE, rm.HUBER, 0.01, 0.6)
    T, info = registration.icp(src, tgt, None, "plane", normals, maxd, iters, search="grid", loss="huber", scale=0.01, trim=0.6)
    assert bits(T, info) == model_bits(want)
    cp = clipper_amd.load_clipperpy()
    f = np.asfortranarray
    with registration._knn_search("grid"):
        Tc, ic = cp.utils.icp_robust(f(src.T), f(tgt.T), np.eye(4), "plane", f(normals.T), maxd, iters, loss="huber",
                                     scale=0.01, trim=0.6)
    assert np.asarray(Tc).tobytes() == T.tobytes() and np.asarray(ic["history"]).tobytes() == info.history.tobytes()
    assert (ic["iterations"], ic["status"], ic["count"], ic["fitness"], ic["inlier_rmse"], ic["within"], ic["trim_sqd"],
            ic["weight_sum"]) == (info.iterations, info.status, info.count, info.fitness, info.inlier_rmse, info.within,
                                  info.trim_sqd, info.weight_sum)
    with pytest.raises(ValueError, match=r"trim must be in \(0, 1\] \(trim = 1.5\)"):
        cp.utils.icp_robust(f(src.T), f(tgt.T), np.eye(4), "point", np.zeros((3, 0), order="F"), maxd, iters, trim=1.5)
    with pytest.raises(abi.ClipperError, match=r"trim must be in \(0, 1\] \(trim = 0\)"):
        registration.icp(src, tgt, max_distance=maxd, trim=0.0)
    # the C++ facade
    exe = str(tmp_path / "test_icp_robust_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_icp_robust_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    files = [str(tmp_path / n) for n in ("src.f64", "tgt.f64", "nrm.f64", "cs.f64", "ct.f64", "out_plane.f64", "out_gen.f64")]
    _, cs, ct = aux("cluttered")
    for path, a in zip(files, (src, tgt, normals, cs, ct)):
        a.tofile(path)                               # row-major n x k = column-major k x n
    out = subprocess.run([exe, str(len(src)), str(len(tgt))] + files, capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "ALL ROBUST ICP FACADE TESTS PASSED" in out.stdout
    for path, w in ((files[5], want), (files[6], model("cluttered", GEN, rm.HUBER, 0.01, 0.6))):
        got = np.fromfile(path)                      # T 16, then count, within, trim_sqd, weight_sum
        assert got[:16].reshape(4, 4).T.tobytes() == w.T.tobytes()
        assert tuple(got[16:]) == (float(w.count), float(w.within), w.trim_sqd, w.weight_sum)
