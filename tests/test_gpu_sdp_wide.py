"""GPU tests of the wide route of the semidefinite relaxation (clipper_hip_sdp_set_route; DESIGN.md section 11, "The
wide route"): against the workgroup route where both run, against the sequential model of tests/sdp_model.py above
128, known answers, the capped large end, determinism, the time limit, batches and the facades.

The shapes are the smallest at which each piece can go wrong: n = 1, 2 (a single pair), 3 (a pad index), 128 (the old
ceiling), 129 / 130 (the first sizes of the wide route, odd and even), sizes that are no multiple of the step launch's
tile (16 pairs) or of the update's (16 entries), more than one tile each way, and 512 / 1024 capped at a few iterations.
The helpers (_certificate, the 5 % margin rule) are those of tests/test_gpu_sdp.py, restated."""
import functools
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
TIGHT = dict(eps_abs=1e-6, eps_rel=1e-6, max_iters=20000)


@pytest.fixture(autouse=True)
def _default_route():
    """every test of this file leaves the process on the default route (the suite shares one process)"""
    try:
        yield
    finally:
        abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP)


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


def _euclid_ctx(m, rho, seed, storage=abi.STORE_F64):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    return g


@functools.lru_cache(maxsize=None)
def _scored(m, rho, seed):
    """M and C (identity diagonals) of a scored synthetic problem; computed once, never written to"""
    g = _euclid_ctx(m, rho, seed)
    M, Cm = g.get_affinity_matrix(), g.get_constraint_matrix()
    M.setflags(write=False)
    Cm.setflags(write=False)
    return M, Cm


@functools.lru_cache(maxsize=None)
def _model(m, rho, seed, eps, max_iters=20000):
    M, Cm = _scored(m, rho, seed)
    return sm.solve(M, Cm, max_iters=max_iters, eps_abs=eps, eps_rel=eps)


def _under(route, fn, *a, **kw):
    abi.sdp_set_route(route)
    try:
        return fn(*a, **kw)
    finally:
        abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP)


# ---- 1. both routes agree where both run ---------------------------------------------------------------------------

def _both_routes(M, Cm, prm):
    wg = _under(abi.SDP_ROUTE_WORKGROUP, abi.sdp_solve, M, Cm, prm)
    wide = _under(abi.SDP_ROUTE_WIDE, abi.sdp_solve, M, Cm, prm)
    assert wg.info.route == abi.SDP_ROUTE_WORKGROUP and wide.info.route == abi.SDP_ROUTE_WIDE
    dx = float(np.max(np.abs(wide.X - wg.X)))
    dp = abs(wide.pobj - wg.pobj)
    print(f"n = {M.shape[0]}: iters {wg.iters} / {wide.iters}, sweeps {wg.info.sweeps} / {wide.info.sweeps}, "
          f"max|dX| = {dx:.3e}, |dpobj| = {dp:.3e}, |ddobj| = {abs(wide.dobj - wg.dobj):.3e}")
    assert wide.iters == wg.iters and wide.info.converged == wg.info.converged
    if _margin_ok(wg.evec1, wg.thr) and _margin_ok(wide.evec1, wide.thr):
        assert wide.nodes.tolist() == wg.nodes.tolist()
    assert dp <= 1e-9 * max(1.0, abs(wg.pobj))
    # both routes eigendecompose W + E with ||E||_F <= 1e-13 ||W||_F and both projections are non-expansive: over
    # these iteration counts the drift is of order 1e-10; 1e-8 leaves two decades
    assert dx <= 1e-8
    return wg, wide


@pytest.mark.parametrize("n,k", [(1, 1), (2, 1), (3, 2), (7, 3), (33, 6)])
def test_routes_agree_on_clique_unions(n, k):
    A, K = _clique_union(n, k, seed=n)
    wg, wide = _both_routes(A, A, _params(**TIGHT))
    assert wide.info.converged == 1 and wide.nodes.tolist() == K
    _certificate(A, A, wide, 1e-6, 1e-6)


@pytest.mark.parametrize("m,rho,seed", [(64, 0.7, 67), (97, 0.7, 100), (128, 0.9, 131)])
def test_routes_agree_on_scored_problems(m, rho, seed):
    M, Cm = _scored(m, rho, seed)
    wg, wide = _both_routes(M, Cm, _params(eps_abs=1e-5, eps_rel=1e-5, max_iters=20000))
    assert wide.info.converged == 1
    _certificate(M, Cm, wide, 1e-5, 1e-5)


def _scaled_explicit(n, scale):
    """test_explicit_constraint_matrix's generator with seed 3; the scale covers the diagonal of M too"""
    rng = np.random.default_rng(3)
    up = np.triu(rng.random((n, n)) < 0.4, 1)
    M = np.where(up, rng.uniform(0.1, 1.0, (n, n)), 0.0)
    M = (M + M.T + np.eye(n)) * scale
    cu = np.triu(rng.random((n, n)) < 0.5, 1)
    Cm = (cu | cu.T).astype(float) + np.eye(n)
    return M, Cm


def test_penalty_moves_both_ways_on_both_routes():
    """Every branch of the decision that ends an iteration, on both routes: the penalty goes down, it goes up, the dual
    bound is reached after both residuals pass, and the certificate runs at max_iters. The figures are the model's
    (tests/sdp_model.py, on the CPU)."""
    prm = _params(eps_abs=1e-6, eps_rel=1e-6, max_iters=60)
    # n = 9, M small against the penalty: the model halves rho at iterations 10, 20, 30, 40 and 50 (r_p / r_d < 1e-4
    # at each, against 0.1) and converges at iteration 55 with nodes [0, 4] (rounding margin 0.5). 55 is not pinned:
    # the gap test at 1e-6 may fall one iteration either way between Jacobi and eigh; rho does not depend on it.
    M, Cm = _scaled_explicit(9, 0.01)
    for r in _both_routes(M, Cm, prm):
        print(f"n = 9 route {r.info.route}: rho {r.info.rho!r}, iters {r.iters}, converged {r.info.converged}, "
              f"nodes {r.nodes.tolist()}")
        assert r.info.rho == 2.0 ** -5 and r.info.converged == 1 and 50 <= r.iters < 60
    # n = 33, M large against the penalty: the model doubles rho at iterations 10 to 50 (r_p / r_d = 4517, 1107, 266,
    # 60.7, 12.3 against 10), leaves it at iteration 60 (1.65) and stops unconverged: the certificate runs. (The
    # rounding margin is 0.012: _both_routes leaves the nodes out below 0.05.)
    M, Cm = _scaled_explicit(33, 100.0)
    wg, wide = _both_routes(M, Cm, prm)
    for r in (wg, wide):
        print(f"n = 33 route {r.info.route}: rho {r.info.rho!r}, iters {r.iters}, converged {r.info.converged}")
        assert r.info.rho == 32.0 and r.iters == 60 and r.info.converged == 0
    _certificate(M, Cm, wide, 1e-6, 1e-6)


# ---- 2. above 128 against the model, under AUTO --------------------------------------------------------------------
# (model iterations and the margin of the rounding, computed on the CPU with tests/sdp_model.py: 48 / 0.17, 117 / 0.23,
# 47 / 0.11, 95 / 0.14; none of the four sits on a stopping threshold)

def _against_model(M, Cm, r, ref, eps):
    assert r.info.route == abi.SDP_ROUTE_WIDE and r.info.converged == 1
    _certificate(M, Cm, r, eps, eps)
    print(f"n = {M.shape[0]}: iters {r.iters} (model {ref['iters']}), pobj {r.pobj!r} (model {ref['pobj']!r}), "
          f"max|dX| = {np.max(np.abs(r.X - ref['X'])):.3e}")
    assert abs(r.pobj - ref["pobj"]) <= 2 * (eps + eps * abs(ref["pobj"])) + 1e-9
    assert r.nodes.tolist() == ref["nodes"]
    assert r.iters == ref["iters"]


@pytest.mark.parametrize("m,rho,seed,eps", [(130, 0.6, 133, 1e-5), (200, 0.9, 203, 1e-3), (256, 0.8, 259, 1e-3)])
def test_above_128_against_the_model(m, rho, seed, eps):
    M, Cm = _scored(m, rho, seed)
    r = _under(abi.SDP_ROUTE_AUTO, abi.sdp_solve, M, Cm, _params(eps_abs=eps, eps_rel=eps, max_iters=20000))
    _against_model(M, Cm, r, _model(m, rho, seed, eps), eps)


def test_above_128_through_a_context():
    m, rho, seed, eps = 129, 0.7, 132, 1e-3
    g = _euclid_ctx(m, rho, seed)
    prm = _params(eps_abs=eps, eps_rel=eps, max_iters=20000)
    with pytest.raises(abi.ClipperError, match=r"error -7.*limit of 128"):  # the default route still refuses
        g.sdp(prm)
    nodes, r = _under(abi.SDP_ROUTE_AUTO, g.sdp, prm)
    M, Cm = _scored(m, rho, seed)
    _against_model(M, Cm, r, _model(m, rho, seed, eps), eps)
    assert nodes.tolist() == r.nodes.tolist() and g.get_solution().nodes.tolist() == nodes.tolist()
    assert np.array_equal(g.get_selected_associations(), g.get_initial_associations()[nodes])


# ---- 3. known answers ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k", [(129, 12), (191, 14), (384, 20)])
def test_clique_union_known_answers(n, k):
    A, K = _clique_union(n, k, seed=n)
    r = _under(abi.SDP_ROUTE_AUTO, abi.sdp_solve, A, A, _params(**TIGHT))
    assert r.info.route == abi.SDP_ROUTE_WIDE and r.info.converged == 1
    assert r.nodes.tolist() == K
    assert abs(r.pobj + k) <= 1e-4 * k
    _certificate(A, A, r, 1e-6, 1e-6)


# ---- 4. the large end, capped ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,rho,seed,cap", [(512, 0.9, 515, 3), (1024, 0.9, 1027, 2)])
def test_large_end_capped(m, rho, seed, cap):
    M, Cm = _scored(m, rho, seed)
    r = _under(abi.SDP_ROUTE_AUTO, abi.sdp_solve, M, Cm, _params(eps_abs=1e-9, eps_rel=1e-9, max_iters=cap))
    assert r.info.route == abi.SDP_ROUTE_WIDE
    assert r.iters == cap and r.info.converged == 0 and r.info.timed_out == 0
    _certificate(M, Cm, r, 1e-9, 1e-9)
    ref = _model(m, rho, seed, 1e-9, cap)
    dx = float(np.max(np.abs(r.X - ref["X"])))
    print(f"n = {m}: max|dX| = {dx:.3e}, pobj {r.pobj!r} (model {ref['pobj']!r}), sweeps {r.info.sweeps}, "
          f"t_solve {r.info.t_solve:.3f} s")
    assert ref["iters"] == cap
    assert dx <= 1e-8
    assert abs(r.pobj - ref["pobj"]) <= 1e-9 * abs(ref["pobj"])


# ---- 5. explicit C != pattern(M) -------------------------------------------------------------------------------------

def test_explicit_constraint_matrix():
    rng = np.random.default_rng(6)  # (test_gpu_sdp.py::test_explicit_constraint_matrix's generator, its seed plus 1)
    n = 150
    up = np.triu(rng.random((n, n)) < 0.4, 1)
    M = np.where(up, rng.uniform(0.1, 1.0, (n, n)), 0.0)
    M = M + M.T + np.eye(n)
    cu = np.triu(rng.random((n, n)) < 0.5, 1)
    Cm = (cu | cu.T).astype(float) + np.eye(n)
    # (the model needs 6338 iterations to 1e-6 here; 60 exercise the mask of an explicit C just as well, and the
    # certificate's inequalities hold at every iteration)
    r = _under(abi.SDP_ROUTE_AUTO, abi.sdp_solve, M, Cm, _params(eps_abs=1e-6, eps_rel=1e-6, max_iters=60))
    assert r.info.route == abi.SDP_ROUTE_WIDE and r.iters == 60
    assert np.all(np.abs(r.X[Cm == 0]) <= r.info.r_prim + 1e-12) and np.any(Cm == 0)
    assert np.any((Cm != 0) & (M == 0)) and np.any((Cm == 0) & (M != 0))  # C is not the pattern of M
    _certificate(M, Cm, r, 1e-6, 1e-6)
    ref = sm.solve(M, Cm, max_iters=60, eps_abs=1e-6, eps_rel=1e-6)
    assert np.max(np.abs(r.X - ref["X"])) <= 1e-8 and abs(r.pobj - ref["pobj"]) <= 1e-9 * abs(ref["pobj"])


# ---- 6. determinism ----------------------------------------------------------------------------------------------------

def test_deterministic():
    M, Cm = _scored(160, 0.7, 163)
    prm = _params(eps_abs=1e-9, eps_rel=1e-9, max_iters=20)
    a = _under(abi.SDP_ROUTE_AUTO, abi.sdp_solve, M, Cm, prm)
    b = _under(abi.SDP_ROUTE_AUTO, abi.sdp_solve, M, Cm, prm)
    assert a.info.route == abi.SDP_ROUTE_WIDE and a.iters == 20
    for f in ("X", "Y", "lambdas", "evec1"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.nodes.tolist() == b.nodes.tolist() and a.pobj == b.pobj and a.dobj == b.dobj and a.iters == b.iters
    assert a.info.sweeps == b.info.sweeps and a.info.rho == b.info.rho


# ---- 7. the time limit -----------------------------------------------------------------------------------------------

def test_time_limit():
    m, rho, seed = 256, 0.8, 259
    M, Cm = _scored(m, rho, seed)
    abi.sdp_set_route(abi.SDP_ROUTE_AUTO)
    t0 = time.time()
    r = abi.sdp_solve(M, Cm, _params(max_iters=10 ** 6, eps_abs=1e-12, eps_rel=1e-12, time_limit_secs=0.3))
    wall = time.time() - t0
    assert r.info.timed_out == 1 and r.info.converged == 0 and wall < 5.0, (wall, r.iters)
    assert r.iters >= 1 and r.info.route == abi.SDP_ROUTE_WIDE
    _, d = _certificate(M, Cm, r, 1e-12, 1e-12)
    opt = -_model(m, rho, seed, 1e-3)["pobj"]  # within 1e-3 relative of the optimum
    assert d >= opt - 2e-3 * abs(opt)  # dobj is a certified bound on it


# ---- 8. batches --------------------------------------------------------------------------------------------------------

def test_batch_mixes_the_routes():
    sizes = [40, 129, 128, 200, 7]
    probs = [_scored(129, 0.7, 132) if m == 129 else _scored(200, 0.9, 203) if m == 200 else _scored(m, 0.7, m + 3)
             for m in sizes]
    # 50 iterations: the two wide problems converge (48 and 47), the cap stops others: both ends of a batch's solve
    prm = _params(eps_abs=1e-3, eps_rel=1e-3, max_iters=50)
    with pytest.raises(abi.ClipperError, match=r"error -7: problem 1:.*limit of 128"):  # the default route
        abi.sdp_solve_batch(probs, prm)
    abi.sdp_set_route(abi.SDP_ROUTE_AUTO)
    got = abi.sdp_solve_batch(probs, prm)
    assert [r.info.route for r in got] == [0, 2, 0, 2, 0]
    assert got[1].info.converged == 1 and got[3].info.converged == 1
    for (M, Cm), r in zip(probs, got):
        lone = abi.sdp_solve(M, Cm, prm)
        assert lone.info.route == r.info.route
        for f in ("X", "Y", "lambdas", "evec1"):
            assert np.array_equal(getattr(r, f), getattr(lone, f)), (M.shape[0], f)
        assert r.nodes.tolist() == lone.nodes.tolist() and r.thr == lone.thr
        for f in ("iters", "converged", "timed_out", "num_nodes", "sweeps", "pobj", "dobj", "r_prim", "r_dual", "rho"):
            assert getattr(r.info, f) == getattr(lone.info, f), (M.shape[0], f)
    # under WIDE every problem takes the wide driver, and is its lone call too
    abi.sdp_set_route(abi.SDP_ROUTE_WIDE)
    small = [probs[4], probs[0]]
    got = abi.sdp_solve_batch(small, prm)
    assert [r.info.route for r in got] == [2, 2]
    for (M, Cm), r in zip(small, got):
        lone = abi.sdp_solve(M, Cm, prm)
        assert np.array_equal(r.X, lone.X) and np.array_equal(r.evec1, lone.evec1) and r.nodes.tolist() == lone.nodes.tolist()
        assert r.info.iters == lone.info.iters and r.info.pobj == lone.info.pobj and r.info.dobj == lone.info.dobj


def test_context_batch_follows_the_route():
    """clipper_hip_batch_sdp: the children's relaxations, the one above 128 through the wide driver"""
    ps = [synth.make_euclidean_problem(m, 0.7, seed=s) for m, s in ((60, 63), (129, 132))]
    prm = _params(eps_abs=1e-3, eps_rel=1e-3, max_iters=20000)
    b = abi.HipBatch(storage=abi.STORE_F64)
    b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in ps], **synth.EUCLID_BENCH_PARAMS)
    with pytest.raises(abi.ClipperError, match=r"error -7: problem 1:.*limit of 128"):
        b.sdp(prm)
    abi.sdp_set_route(abi.SDP_ROUTE_AUTO)
    got = b.sdp(prm)
    assert [r.info.route for r in got] == [0, 2]
    for p, r, (m, s) in zip(ps, got, ((60, 63), (129, 132))):
        g = _euclid_ctx(m, 0.7, s)
        nodes, lone = g.sdp(prm)
        assert np.array_equal(r.X, lone.X) and np.array_equal(r.Y, lone.Y) and r.nodes.tolist() == nodes.tolist()
        assert r.info.iters == lone.info.iters and r.info.pobj == lone.info.pobj and r.info.dobj == lone.info.dobj


# ---- 9. the facades ----------------------------------------------------------------------------------------------------

def test_clipperpy_route_round_trip():
    cp = clipper_amd.load_clipperpy()
    try:
        assert cp.sdp.route() == cp.sdp.Route.Workgroup
        cp.sdp.set_route(cp.sdp.Route.Auto)
        assert cp.sdp.route() == cp.sdp.Route.Auto and abi.sdp_route() == abi.SDP_ROUTE_AUTO
        A, K = _clique_union(129, 12, seed=129)
        s = cp.sdp.solve(A, A, cp.SDPParams())
        assert list(s.nodes) == K
        cp.sdp.set_route(cp.sdp.Route.Wide)
        assert cp.sdp.route() == cp.sdp.Route.Wide
    finally:
        cp.sdp.set_route(cp.sdp.Route.Workgroup)
    assert abi.sdp_route() == abi.SDP_ROUTE_WORKGROUP
    with pytest.raises(RuntimeError, match=r"limit of 128"):
        cp.sdp.solve(A, A, cp.SDPParams())


def test_cpp_facade_sdp_wide(tmp_path):
    # what the ABI gives under AUTO: sdp_solve at 150 x 150, a context at m = 200
    M150, _ = _clique_union(150, 13, seed=150)
    M200, C200 = _scored(200, 0.9, 203)
    prm = _params()  # sdp::Params' defaults
    r150 = _under(abi.SDP_ROUTE_AUTO, abi.sdp_solve, M150, M150, prm)
    g = abi.HipClipper(storage=abi.STORE_F64)
    g.set_matrix_data(M200 - np.eye(200), C200 - np.eye(200))
    nodes200, _ = _under(abi.SDP_ROUTE_AUTO, g.sdp, prm)
    files = {}
    for name, arr in (("M150", M150), ("C150", M150), ("M200", M200), ("C200", C200)):
        files[name] = str(tmp_path / (name + ".txt"))
        np.savetxt(files[name], arr, fmt="%.17g")
    files["want"] = str(tmp_path / "want.txt")
    with open(files["want"], "w") as f:
        f.write(f"{r150.pobj!r} {len(r150.nodes)} " + " ".join(map(str, r150.nodes.tolist())) + "\n")
        f.write(f"{len(nodes200)} " + " ".join(map(str, nodes200.tolist())) + "\n")
    exe = str(tmp_path / "test_sdp_wide_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_sdp_wide_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe, files["M150"], files["C150"], files["M200"], files["C200"], files["want"]],
                         capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL SDP WIDE FACADE TESTS PASSED" in out.stdout


# ---- the infeasible problem (no diagonal entry of C is nonzero) ------------------------------------------------------

def test_infeasible_problem_is_refused():
    z = np.zeros((4, 4))
    big = np.zeros((130, 130))
    eye = np.eye(5)
    for route, Z in ((abi.SDP_ROUTE_WIDE, z), (abi.SDP_ROUTE_AUTO, big)):
        abi.sdp_set_route(route)
        with pytest.raises(abi.ClipperError, match=r"error -1: sdp: no diagonal"):
            abi.sdp_solve(Z, Z)
    # a batch names its first infeasible problem, whichever route it would have taken
    abi.sdp_set_route(abi.SDP_ROUTE_AUTO)
    with pytest.raises(abi.ClipperError, match=r"error -1: problem 1: sdp: no diagonal"):
        abi.sdp_solve_batch([(eye, eye), (big, big), (z, z)])
    with pytest.raises(abi.ClipperError, match=r"error -1: problem 1: sdp: no diagonal"):
        abi.sdp_solve_batch([(eye, eye), (z, z), (big, big)])
    got = abi.sdp_solve_batch([(eye, eye)])  # the entry points are usable afterwards
    assert got[0].info.converged == 1
