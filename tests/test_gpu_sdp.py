"""GPU tests of the semidefinite relaxation (clipper_hip_sdp, clipper_hip_sdp_solve, CLIPPER::solveAsMSRCSDR with
setDeviceSdp) against the sequential model of tests/sdp_model.py."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import synth
from tests import sdp_model as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGES = (abi.STORE_F32_CSC, abi.STORE_F64_CSC, abi.STORE_F32, abi.STORE_F64)
TIGHT = dict(eps_abs=1e-6, eps_rel=1e-6, max_iters=20000)


def _certificate(M, C, r, eps_abs, eps_rel):
    """The host's check of a device result: the dual bound recomputed, the gap, the violation of P."""
    M = sm.symmetric_lower(M)
    mask = sm.symmetric_lower(np.asarray(C) != 0) != 0
    X, Y = r.X, r.Y
    p = float(np.sum(M * X))
    d = float(np.linalg.eigvalsh(M - Y)[-1])
    assert np.allclose(X, X.T, atol=1e-12)
    assert abs(np.trace(X) - 1.0) < 1e-9
    assert np.linalg.eigvalsh(X)[0] > -1e-9
    assert np.all(Y[mask] <= 1e-12)               # the dual of X_ij >= 0 where C != 0
    assert abs(-r.pobj - p) <= 1e-9 * max(1.0, abs(p))
    assert abs(-r.dobj - d) <= 1e-7 * max(1.0, abs(d))
    assert d >= p - (eps_abs + eps_rel * max(abs(d), abs(p))) - 1e-12 or r.info.converged == 0
    if r.info.converged:
        assert abs(d - p) <= eps_abs + eps_rel * max(abs(d), abs(p)) + 1e-9
    viol = np.sqrt(np.sum(np.where(mask, np.minimum(X, 0.0), X) ** 2))
    assert viol <= r.info.r_prim + 1e-9
    return p, d


def _margin_ok(ev, thr):
    a = np.abs(ev)
    return np.min(np.abs(a - thr)) >= 0.05 * a.max()


def _params(**kw):
    return abi.SdpParams(**kw)


def _euclid_ctx(m, rho, seed, storage):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    return g


def _compare(M, C, r, eps):
    ref = sm.solve(M, C, **eps)
    tol = eps["eps_abs"] + eps["eps_rel"] * abs(ref["pobj"])
    assert abs(r.pobj - ref["pobj"]) <= 2 * tol + 1e-9, (r.pobj, ref["pobj"])
    if _margin_ok(ref["evec1"], ref["thr"]) and _margin_ok(r.evec1, r.thr):
        assert r.nodes.tolist() == ref["nodes"]
    return ref


def _clique_union(n, k, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    K = sorted(perm[:k].tolist())
    A = np.zeros((n, n))
    A[np.ix_(K, K)] = 1
    i = k
    while i < n:
        s = int(min(rng.integers(1, max(2, k)), n - i))
        grp = perm[i:i + s]
        A[np.ix_(grp, grp)] = 1
        i += s
    np.fill_diagonal(A, 1.0)
    return A, K


# ---- the reference's golden problem (test/sdp_test.cpp) ----------------------------------------------------------

def test_golden_20x20_both_entry_points(golden):
    M = np.array(golden["dsd_test_20x20"]["M"])
    Cm = (M > 0).astype(float)
    r = abi.sdp_solve(M, Cm, _params(**TIGHT))
    assert r.info.converged == 1
    _certificate(M, Cm, r, 1e-6, 1e-6)
    ref = _compare(M, Cm, r, TIGHT)
    assert r.nodes.tolist() == ref["nodes"]
    # the context: set_matrix_data stores M and C without their diagonals; the entry point adds the identity back
    g = abi.HipClipper(storage=abi.STORE_F64)
    Moff, Coff = M - np.eye(20), Cm - np.eye(20)
    g.set_matrix_data(Moff, Coff)
    nodes, rc = g.sdp(_params(**TIGHT))
    _certificate(M, Cm, rc, 1e-6, 1e-6)
    assert nodes.tolist() == r.nodes.tolist() and abs(rc.pobj - r.pobj) < 1e-9
    assert g.get_solution().nodes.tolist() == nodes.tolist() and g.get_solution().score == -1
    # lambdas ascending, evec1 its largest entry positive, thr its half
    assert np.all(np.diff(r.lambdas) >= 0) and abs(r.lambdas.sum() - 1) < 1e-9
    assert r.evec1[np.argmax(np.abs(r.evec1))] > 0 and r.thr == pytest.approx(np.abs(r.evec1).max() / 2)
    assert np.allclose(np.linalg.eigvalsh(r.X), r.lambdas, atol=1e-9)


# ---- known answers: a disjoint union of cliques -----------------------------------------------------------------

@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (33, 6), (64, 9), (100, 12), (128, 12)])
def test_clique_union_known_answers(n, k):
    A, K = _clique_union(n, k, seed=n)
    r = abi.sdp_solve(A, A, _params(**TIGHT))
    assert r.info.converged == 1
    assert r.nodes.tolist() == K
    assert abs(r.pobj + k) <= 1e-4 * k
    _certificate(A, A, r, 1e-6, 1e-6)


# ---- scored synthetic problems, every storage ---------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
@pytest.mark.parametrize("m,rho", [(40, 0.5), (97, 0.7), (128, 0.9)])
def test_euclidean_problems(storage, m, rho):
    g = _euclid_ctx(m, rho, seed=m + 3, storage=storage)
    M, Cm = g.get_affinity_matrix(), g.get_constraint_matrix()
    eps = dict(eps_abs=1e-5, eps_rel=1e-5, max_iters=20000)
    nodes, r = g.sdp(_params(**eps))
    assert r.info.converged == 1
    _certificate(M, Cm, r, 1e-5, 1e-5)
    _compare(M, Cm, r, eps)
    assert np.array_equal(g.get_selected_associations(), g.get_initial_associations()[nodes])


def test_pointnormal_problem():
    p = synth.make_pointnormal_problem(80, 0.8, seed=7)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A)
    M, Cm = g.get_affinity_matrix(), g.get_constraint_matrix()
    eps = dict(eps_abs=1e-5, eps_rel=1e-5, max_iters=20000)
    _, r = g.sdp(_params(**eps))
    _certificate(M, Cm, r, 1e-5, 1e-5)
    _compare(M, Cm, r, eps)


# ---- explicit C != pattern(M), lower-triangle semantics ------------------------------------------------------------

def test_explicit_constraint_matrix():
    rng = np.random.default_rng(5)
    n = 50
    up = np.triu(rng.random((n, n)) < 0.4, 1)
    M = np.where(up, rng.uniform(0.1, 1.0, (n, n)), 0.0)
    M = M + M.T + np.eye(n)
    cu = np.triu(rng.random((n, n)) < 0.5, 1)
    Cm = (cu | cu.T).astype(float) + np.eye(n)
    r = abi.sdp_solve(M, Cm, _params(**TIGHT))
    assert np.all(np.abs(r.X[Cm == 0]) <= r.info.r_prim + 1e-12)
    _certificate(M, Cm, r, 1e-6, 1e-6)
    _compare(M, Cm, r, TIGHT)
    # the same through a context with an explicit C, dense and f32 slices
    for storage in (abi.STORE_F64, abi.STORE_F32_CSC):
        g = abi.HipClipper(storage=storage)
        g.set_matrix_data(M - np.eye(n), Cm - np.eye(n))
        _, rc = g.sdp(_params(**TIGHT))
        _certificate(g.get_affinity_matrix(), g.get_constraint_matrix(), rc, 1e-6, 1e-6)
        assert abs(rc.pobj - r.pobj) <= 1e-5 * abs(r.pobj)


def test_lower_triangle_and_zero_diagonal():
    A, K = _clique_union(30, 5, seed=4)
    Mg, Cg = A.copy(), A.copy()
    iu = np.triu_indices(30, 1)
    rng = np.random.default_rng(9)
    Mg[iu] = rng.uniform(-5, 5, len(iu[0]))
    Cg[iu] = rng.integers(0, 2, len(iu[0]))
    r0 = abi.sdp_solve(A, A, _params(**TIGHT))
    r1 = abi.sdp_solve(Mg, Cg, _params(**TIGHT))
    assert np.array_equal(r0.X, r1.X) and r0.nodes.tolist() == r1.nodes.tolist()
    Cz = A.copy()
    Cz[K[0], K[0]] = 0.0
    r2 = abi.sdp_solve(A, Cz, _params(**TIGHT))
    assert abs(r2.X[K[0], K[0]]) <= r2.info.r_prim + 1e-12
    assert -r2.dobj >= len(K) - 1 - 1e-9 and abs(r2.pobj + (len(K) - 1)) < 0.1
    _certificate(A, Cz, r2, 1e-6, 1e-6)


# ---- stop rules, determinism, refusals ----------------------------------------------------------------------------

def test_max_iters_and_time_limit():
    g = _euclid_ctx(128, 0.6, seed=2, storage=abi.STORE_F32_CSC)
    M, Cm = g.get_affinity_matrix(), g.get_constraint_matrix()
    _, r = g.sdp(_params(max_iters=5, eps_abs=1e-9, eps_rel=1e-9))
    assert r.iters == 5 and r.info.converged == 0 and r.info.timed_out == 0 and len(r.nodes) > 0
    _, d5 = _certificate(M, Cm, r, 1e-9, 1e-9)
    _, tight = g.sdp(_params(**TIGHT))
    assert d5 >= -tight.pobj - 1e-4 * abs(tight.pobj)  # still a bound on the optimum
    t0 = time.time()
    _, r = g.sdp(_params(max_iters=10 ** 6, eps_abs=1e-12, eps_rel=1e-12, time_limit_secs=0.3))
    wall = time.time() - t0
    assert r.info.timed_out == 1 and r.info.converged == 0 and wall < 5.0, (wall, r.iters)
    _, d = _certificate(M, Cm, r, 1e-12, 1e-12)
    assert d >= -tight.pobj - 1e-4 * abs(tight.pobj)


def test_deterministic():
    g = _euclid_ctx(90, 0.7, seed=8, storage=abi.STORE_F32_CSC)
    _, a = g.sdp(_params(eps_abs=1e-5, eps_rel=1e-5))
    _, b = g.sdp(_params(eps_abs=1e-5, eps_rel=1e-5))
    for f in ("X", "Y", "lambdas", "evec1"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.nodes.tolist() == b.nodes.tolist() and a.pobj == b.pobj and a.dobj == b.dobj and a.iters == b.iters


def test_refusals():
    big = np.eye(abi.SDP_MAX_N + 1)
    with pytest.raises(abi.ClipperError, match=r"error -7.*limit of 128"):
        abi.sdp_solve(big, big)
    g = _euclid_ctx(200, 0.9, seed=3, storage=abi.STORE_F32_CSC)
    with pytest.raises(abi.ClipperError, match=r"error -7.*limit of 128"):
        g.sdp()
    p = synth.make_euclidean_problem(100, 0.9, seed=3)
    grp = abi.HipClipper(storage=abi.STORE_F32_CSC, group=[0, 0])
    grp.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    with pytest.raises(abi.ClipperError, match=r"error -7.*one-shard"):
        grp.sdp()
    with pytest.raises(abi.ClipperError, match=r"error -5"):
        abi.HipClipper(storage=abi.STORE_F32_CSC).sdp()
    z = np.zeros((4, 4))
    with pytest.raises(abi.ClipperError, match=r"error -1.*diagonal"):
        abi.sdp_solve(z, z)


def test_no_side_effects_on_solve():
    p = synth.make_euclidean_problem(120, 0.8, seed=21)
    fresh = abi.HipClipper(storage=abi.STORE_F32_CSC)
    fresh.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    s0 = fresh.solve(p.u0)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    g.sdp()
    s1 = g.solve(p.u0)
    assert np.array_equal(s1.u, s0.u) and s1.nodes.tolist() == s0.nodes.tolist()


# ---- the reference-facing surfaces ------------------------------------------------------------------------------

def test_clipperpy_sdp(golden):
    cp = clipper_amd.load_clipperpy()
    M = np.array(golden["dsd_test_20x20"]["M"])
    Cm = (M > 0).astype(float)
    prm = cp.SDPParams()
    prm.eps_abs, prm.eps_rel, prm.max_iters = 1e-6, 1e-6, 20000
    s = cp.sdp.solve(M, Cm, prm)
    assert isinstance(s, cp.SDPSolution)
    r = abi.sdp_solve(M, Cm, _params(**TIGHT))
    assert list(s.nodes) == r.nodes.tolist() and np.allclose(np.asarray(s.X), r.X, atol=0)
    assert s.iters == r.iters and s.pobj == pytest.approx(r.pobj, rel=1e-6) and s.dobj == pytest.approx(r.dobj, rel=1e-6)
    assert s.thr == r.thr and np.array_equal(np.asarray(s.evec1), r.evec1) and s.t > 0
    c = cp.CLIPPER(cp.invariants.EuclideanDistance(cp.invariants.EuclideanDistanceParams()), cp.Params())
    c.set_matrix_data(M - np.eye(20), Cm - np.eye(20))
    c.solve_as_msrc_sdr(prm)  # default: the stub, as a reference build without SCS
    assert len(c.get_solution().nodes) == 0
    c.set_device_sdp(True)
    c.solve_as_msrc_sdr(prm)
    sol = c.get_solution()
    assert sorted(sol.nodes) == r.nodes.tolist() and sol.score == -1 and sol.ifinal == 0 and sol.t > 0
    assert np.all(np.asarray(sol.u) == 0) and np.asarray(sol.u).shape == (20,)


def test_cpp_facade_sdp(tmp_path, golden):
    exe = str(tmp_path / "test_sdp_facade")
    mfile = str(tmp_path / "M.txt")
    np.savetxt(mfile, np.array(golden["dsd_test_20x20"]["M"]), fmt="%.17g")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_sdp_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe, mfile], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL SDP FACADE TESTS PASSED" in out.stdout
