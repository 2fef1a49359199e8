"""GPU tests of user-defined invariants in device source: the built-ins restated as device source give
the built-in fills' matrices bit for bit and their solutions, in every storage; formulas the built-ins cannot express
give the host loop's matrix (a Python PairwiseInvariant with the same formula through clipperpy); column shards; the
C++ and Python facades."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import synth
from oracle import clipper_ref as ref
from tests.custom_invariant_model import ASYM_SRC, asym_py  # asymmetric under i <-> j, + - * / sqrt fabs only

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGES = [abi.STORE_F32, abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC]

# EuclideanDistance in euclidean_distance.cpp's order with EuclidInv::score's fma chain (k_affinity.hip.h); params = {sigma, epsilon, mindist}
EUCLID_SRC = r"""
#include <hip/hip_runtime.h>
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) {
    const double t1 = ai[k] - aj[k];
    const double t2 = bi[k] - bj[k];
    s1 = fma(t1, t1, s1);
    s2 = fma(t2, t2, s2);
  }
  const double l1 = sqrt(s1), l2 = sqrt(s2);
  if (params[2] > 0 && (l1 < params[2] || l2 < params[2])) return 0.0;
  const double c = fabs(l1 - l2);
  return (c < params[1]) ? exp(-0.5 * c * c / (params[0] * params[0])) : 0.0;
}
"""

# PointNormalDistance (pointnormal_distance.cpp:13-35), d = 6; params = {sigp, epsp, sign, epsn}
POINTNORMAL_SRC = r"""
__device__ double dist3(const double* p, const double* q) {
  double s = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double t = p[k] - q[k];
    s = fma(t, t, s);
  }
  return sqrt(s);
}
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  const double l1 = dist3(ai, aj), l2 = dist3(bi, bj);
  const double alpha1 = acos(fma(ai[5], aj[5], fma(ai[4], aj[4], ai[3] * aj[3])));
  const double alpha2 = acos(fma(bi[5], bj[5], fma(bi[4], bj[4], bi[3] * bj[3])));
  const double dp = fabs(l1 - l2), dn = fabs(alpha1 - alpha2);
  if (dp < params[1] && dn < params[3]) {
    const double sp = exp(-0.5 * dp * dp / (params[0] * params[0]));
    const double sn = exp(-0.5 * dn * dn / (params[2] * params[2]));
    return sp * sn;
  }
  return 0.0;
}
"""

# with exp; params[2] > 0: NaN for the pairs with ai[0] - bj[0] < -params[2] (0 * sqrt of a negative number)
EXP_SRC = r"""
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) {
    const double t = (ai[k] - aj[k]) - (bi[k] - bj[k]);
    s = s + t * t;
  }
  const double v = exp(-s / params[0]) * (1.0 + params[1] * fabs(ai[0] - bj[0]));
  return params[2] > 0 ? v + 0.0 * sqrt(ai[0] - bj[0] + params[2]) : v;
}
"""


def _exp_py(d, p):
    def f(ai, aj, bi, bj):
        s = 0.0
        for k in range(d):
            t = (float(ai[k]) - float(aj[k])) - (float(bi[k]) - float(bj[k]))
            s = s + t * t
        v = math.exp(-s / p[0]) * (1.0 + p[1] * abs(float(ai[0]) - float(bj[0])))
        if p[2] > 0:
            w = float(ai[0]) - float(bj[0]) + p[2]
            return v + 0.0 * (math.sqrt(w) if w >= 0 else float("nan"))
        return v
    return f


@pytest.fixture(scope="module")
def clipperpy():
    return clipper_amd.load_clipperpy()


def _host_loop(cp, fn, D1, D2, A, storage=None):
    """the host loop (clipper.cpp:31-64) with a Python PairwiseInvariant: M as the facade uploads it"""
    class Inv(cp.invariants.PairwiseInvariant):
        def __init__(self):
            super().__init__()

        def __call__(self, ai, aj, bi, bj):
            return fn(ai, aj, bi, bj)

    c = cp.CLIPPER(Inv(), cp.Params())
    c.set_storage(storage if storage is not None else cp.Storage.F64)
    c.score_pairwise_consistency(np.asfortranarray(D1), np.asfortranarray(D2), np.asarray(A, dtype=np.int32))
    return c.get_affinity_matrix()


def _custom(inv, p, storage, params, group=None):
    g = abi.HipClipper(storage=storage, group=group)
    g.affinity_custom(inv, p.D1, p.D2, p.A, params)
    return g


def _builtin_euclid(p, storage, **kw):
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **kw)
    return g


def _builtin_pointnormal(p, storage):
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, **p.meta["invariant"])
    return g


def _same_solution(a, b):
    assert a.nodes.tolist() == b.nodes.tolist()
    assert np.array_equal(a.u, b.u)
    assert a.ifinal == b.ifinal and a.n_trials == b.n_trials and a.score == b.score


def _against_builtin(gc, gb, p, sr=None):
    Mc, Mb = gc.get_affinity_matrix(), gb.get_affinity_matrix()
    assert np.array_equal(Mc, Mb), f"{np.count_nonzero(Mc != Mb)} entries differ from the built-in fill"
    assert np.array_equal(gc.get_constraint_matrix(), gb.get_constraint_matrix())
    sc, sb = gc.solve(p.u0), gb.solve(p.u0)
    _same_solution(sc, sb)
    if sr is not None:  # the oracle criteria of the suite (tests/test_gpu_parity.py)
        assert sc.nodes.tolist() == sr.nodes.tolist()
        assert abs(sc.score - sr.score) <= 1e-6 * abs(sr.score)
    return sc


@pytest.fixture(scope="module")
def euclid_inv():
    with abi.HipInvariant(EUCLID_SRC, 3) as inv:
        yield inv


def _euclid_params(kw):
    return [kw["sigma"], kw["epsilon"], kw["mindist"]]


@pytest.mark.parametrize("storage", STORAGES)
def test_euclidean_restated_m600(euclid_inv, storage):
    p = synth.make_euclidean_problem(600, 0.9, seed=4242)
    kw = synth.EUCLID_BENCH_PARAMS
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **kw)
    sr = r.solve(p.u0)
    gc, gb = _custom(euclid_inv, p, storage, _euclid_params(kw)), _builtin_euclid(p, storage, **kw)
    _against_builtin(gc, gb, p, sr)
    t = gc.timings()
    assert t.affinity_kernel_ms > 0 and t.affinity_total_ms >= t.affinity_kernel_ms
    gc.close(), gb.close()


@pytest.mark.parametrize("storage", STORAGES)
def test_euclidean_restated_headline(euclid_inv, storage):
    p = synth.make_euclidean_problem(10000, 0.95, seed=12345)
    kw = synth.EUCLID_BENCH_PARAMS
    gc, gb = _custom(euclid_inv, p, storage, _euclid_params(kw)), _builtin_euclid(p, storage, **kw)
    sr = None
    if storage == abi.STORE_F32_CSC:
        r = ref.RefClipper()
        r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **kw)
        sr = r.solve(p.u0)
    sc = _against_builtin(gc, gb, p, sr)
    if sr is not None:
        assert sc.ifinal == sr.ifinal and sc.n_trials == sr.n_trials
    gc.close(), gb.close()


def test_euclidean_restated_m20000_without_the_sub_problem(euclid_inv):
    """the built-in route takes the live sub-problem at this size, kind 3 cannot (no rectangular fill): the two routes
    are held to the suite's route-equivalence criteria (tests/test_gpu_subproblem.py)"""
    p = synth.make_euclidean_problem(20000, 0.95, seed=4100 + 20000)
    kw = synth.EUCLID_BENCH_PARAMS
    gc, gb = _custom(euclid_inv, p, abi.STORE_F32_CSC, _euclid_params(kw)), _builtin_euclid(p, abi.STORE_F32_CSC, **kw)
    assert np.array_equal(gc.get_affinity_matrix(), gb.get_affinity_matrix())
    sc, sb = gc.solve(p.u0), gb.solve(p.u0)
    stc, stb = gc.view_stats(), gb.view_stats()
    assert stb.sub_entries >= 1 and stc.sub_entries == 0 and stc.sub_passes == 0
    assert sc.nodes.tolist() == sb.nodes.tolist() and sc.ifinal == sb.ifinal
    assert abs(sc.score - sb.score) <= 1e-9 * abs(sb.score)
    print(f"m=20000: kind 3 {stc.view_passes} view passes of {stc.passes}; built-in {stb.sub_passes} sub-problem passes")
    gc.close(), gb.close()


@pytest.mark.parametrize("m", [600, 5000])
@pytest.mark.parametrize("storage", STORAGES)
def test_pointnormal_restated(storage, m):
    p = synth.make_pointnormal_problem(m, 0.8, seed=11 + m)
    iv = p.meta["invariant"]
    sr = None
    if m == 600:
        r = ref.RefClipper()
        r.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, **iv)
        sr = r.solve(p.u0)
    with abi.HipInvariant(POINTNORMAL_SRC, 6) as inv:
        gc = _custom(inv, p, storage, [iv["sigp"], iv["epsp"], iv["sign"], iv["epsn"]])
        gb = _builtin_pointnormal(p, storage)
        _against_builtin(gc, gb, p, sr)
        gc.close(), gb.close()


def _problem(rng, d, n1, n2, m=None):
    D1 = rng.random((d, n1))
    D2 = D1[:, rng.permutation(n1)[:n2]] + rng.normal(0, 0.01, size=(d, n2)) if n2 <= n1 else rng.random((d, n2))
    if m is None:
        A = np.array([(i, j) for i in range(n1) for j in range(n2)], dtype=np.int32)  # all-to-all
    else:  # repeated indices in both columns
        A = np.stack([rng.integers(0, n1, m), rng.integers(0, n2, m)], axis=1).astype(np.int32)
    return D1, D2, A


@pytest.mark.parametrize("d", [1, 2, 5, 7])
def test_asymmetric_formula_is_the_host_loop_bit_for_bit(clipperpy, d):
    rng = np.random.default_rng(100 + d)
    p1, p2 = [0.9, 0.25, 1e-3, 0.3], [1.3, -0.1, 0.0, 0.55]
    with abi.HipInvariant(ASYM_SRC, d) as inv:
        for D1, D2, A in (_problem(rng, d, 40, 30, m=350), _problem(rng, d, 18, 15)):
            # two fills with different params on one compiled handle
            for prm in (p1, p2):
                Mh = _host_loop(clipperpy, asym_py(d, prm), D1, D2, A)
                assert np.count_nonzero(Mh) > 0 and np.count_nonzero(Mh) < Mh.size - Mh.shape[0]
                g = abi.HipClipper(storage=abi.STORE_F64)
                g.affinity_custom(inv, D1, D2, A, prm)
                assert np.array_equal(g.get_affinity_matrix(), Mh)
                assert np.array_equal(g.get_constraint_matrix(), (Mh != 0).astype(float))
                g.close()
            # the staged form: the same inputs, filled again
            g = abi.HipClipper(storage=abi.STORE_F64_CSC)
            g.stage_inputs(D1, D2, A)
            g.affinity_custom_staged(inv, p1)
            assert np.array_equal(g.get_affinity_matrix(), _host_loop(clipperpy, asym_py(d, p1), D1, D2, A))
            g.close()


@pytest.mark.parametrize("d", [1, 2, 5, 7])
def test_formula_with_exp_and_nan_against_the_host_loop(clipperpy, d):
    rng = np.random.default_rng(200 + d)
    eps = abi.Params().affinityeps
    with abi.HipInvariant(EXP_SRC, d) as inv:
        for D1, D2, A in (_problem(rng, d, 40, 30, m=350), _problem(rng, d, 18, 15)):
            for prm, nan in (([0.05 * d, 0.02, 0.0], False), ([0.05 * d, 0.02, 0.3], True)):
                Mh = _host_loop(clipperpy, _exp_py(d, prm), D1, D2, A)
                # no score within 1e-12 of affinityeps: the pattern does not hang on the last ulp
                f = _exp_py(d, prm)
                sc = np.array([f(D1[:, A[i, 0]], D1[:, A[j, 0]], D2[:, A[i, 1]], D2[:, A[j, 1]])
                               for i in range(len(A)) for j in range(i + 1, len(A))
                               if A[i, 0] != A[j, 0] and A[i, 1] != A[j, 1]])
                fin = sc[np.isfinite(sc)]
                assert np.min(np.abs(fin - eps)) > 1e-12
                assert (not nan) or np.count_nonzero(np.isnan(sc)) > 0
                g = abi.HipClipper(storage=abi.STORE_F64)
                g.affinity_custom(inv, D1, D2, A, prm)
                Mg = g.get_affinity_matrix()
                assert np.array_equal(Mg != 0, Mh != 0)
                assert np.all(np.isfinite(Mg))
                nz = Mh != 0
                ulp = np.spacing(np.abs(Mh[nz]))
                assert np.all(np.abs(Mg[nz] - Mh[nz]) <= 2 * ulp)
                g.close()


def test_wrong_dimension_is_refused(euclid_inv):
    p = synth.make_euclidean_problem(200, 0.9, seed=3)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    with pytest.raises(abi.ClipperError, match="d = 3"):
        g.affinity_custom(euclid_inv, np.vstack([p.D1, p.D1[:1]]), np.vstack([p.D2, p.D2[:1]]), p.A, [0.01, 0.06, 0.0])
    g.stage_inputs(p.D1[:2], p.D2[:2], p.A)
    with pytest.raises(abi.ClipperError, match="clipper_hip error -1"):
        g.affinity_custom_staged(euclid_inv, [0.01, 0.06, 0.0])
    with pytest.raises(abi.ClipperError, match="nparams"):
        g.affinity_custom_staged(euclid_inv, np.zeros(17))
    g.close()


def test_column_shards(euclid_inv):
    p = synth.make_euclidean_problem(3000, 0.9, seed=77)
    prm = _euclid_params(synth.EUCLID_BENCH_PARAMS)
    for storage in (abi.STORE_F32_CSC, abi.STORE_F64):
        g1 = _custom(euclid_inv, p, storage, prm)
        g2 = _custom(euclid_inv, p, storage, prm, group=[0, 0])
        assert np.array_equal(g1.get_affinity_matrix(), g2.get_affinity_matrix())
        s1, s2 = g1.solve(p.u0), g2.solve(p.u0)
        assert s1.nodes.tolist() == s2.nodes.tolist() and s1.ifinal == s2.ifinal
        assert abs(s1.score - s2.score) <= 1e-12 * abs(s1.score)
        g1.close(), g2.close()


# the notebook's invariant (examples/python/ex4_bunny.ipynb: EuclideanDistance as a Python subclass), sums as written
NOTEBOOK_SRC = r"""
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) {
    s1 = s1 + (ai[k] - aj[k]) * (ai[k] - aj[k]);
    s2 = s2 + (bi[k] - bj[k]) * (bi[k] - bj[k]);
  }
  const double c = fabs(sqrt(s1) - sqrt(s2));
  return c < params[1] ? exp(-0.5 * c * c / (params[0] * params[0])) : 0.0;
}
"""


def test_clipperpy_device_invariant_matches_the_python_subclass(clipperpy):
    cp = clipperpy
    p = synth.make_euclidean_problem(1000, 0.9, seed=2024)
    sigma, epsilon = 0.015, 0.05

    class Custom(cp.invariants.PairwiseInvariant):
        def __init__(self):
            super().__init__()

        def __call__(self, ai, aj, bi, bj):
            s1 = s2 = 0.0
            for k in range(3):
                s1 = s1 + (float(ai[k]) - float(aj[k])) * (float(ai[k]) - float(aj[k]))
                s2 = s2 + (float(bi[k]) - float(bj[k])) * (float(bi[k]) - float(bj[k]))
            c = abs(math.sqrt(s1) - math.sqrt(s2))
            return math.exp(-0.5 * c * c / (sigma * sigma)) if c < epsilon else 0.0

    dev = cp.invariants.DeviceInvariant(NOTEBOOK_SRC, [sigma, epsilon])
    assert dev.source == NOTEBOOK_SRC and list(dev.params) == [sigma, epsilon]
    with pytest.raises(RuntimeError, match="GPU only"):
        dev(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        cp.CLIPPERBatch(dev, cp.Params())
    out = {}
    for name, inv in (("device", dev), ("python", Custom())):
        c = cp.CLIPPER(inv, cp.Params())
        c.set_storage(cp.Storage.F64)
        c.score_pairwise_consistency(p.D1, p.D2, p.A)
        c.solve(p.u0)
        out[name] = (c.get_affinity_matrix(), c.get_solution())
    (Md, sd), (Mp, sp) = out["device"], out["python"]
    assert np.array_equal(Md != 0, Mp != 0) and np.count_nonzero(Md) > 0
    nz = Mp != 0   # (exp: the device's and the host's libm may differ in the last bit)
    assert np.all(np.abs(Md[nz] - Mp[nz]) <= 2 * np.spacing(np.abs(Mp[nz])))
    assert list(sd.nodes) == list(sp.nodes) and sd.ifinal == sp.ifinal
    assert abs(sd.score - sp.score) <= 1e-12 * abs(sp.score)


def test_cpp_facade(tmp_path):
    exe = str(tmp_path / "test_device_invariant_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_device_invariant_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "batch.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL DEVICE INVARIANT FACADE TESTS PASSED" in out.stdout
