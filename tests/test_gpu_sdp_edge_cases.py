"""GPU tests of the semidefinite relaxation on degenerate graphs and at the value edges (tests/sdp_edge_cases.py;
DESIGN.md section 11): every case through abi.sdp_solve on the workgroup route and under SDP_ROUTE_WIDE, through one
abi.sdp_solve_batch call that mixes all the cases of n <= 128 with an ordinary scored problem, and, for the handed-over
kinds, through HipClipper.sdp() after set_matrix_data and set_sparse_matrix_data on the four storages.
tests/test_sdp_edge_cases_cpu.py shows on the CPU model that each case has the property asked for here.

Bars, in this order of authority:
  1. the certificate (tests/test_gpu_sdp.py::_certificate, imported): d = lambda_max(M - Y) recomputed with numpy, the
     feasibility of X to r_prim, the sign of Y;
  2. the known optimum where the table has one: d >= opt - 1e-9 max(1, |opt|) in every outcome (weak duality for any Y
     of the right sign, plus the eigenvalue error the certificate allows), and when converged
     -pobj >= opt - tol - 1e-9 with tol = eps_abs + eps_rel max(|d|, |p|), since opt <= d <= p + tol. No upper bar on p:
     X leaves the feasible set by up to r_prim;
  3. the model where the model converges: |pobj - pobj_model| <= 2 tol + 1e-9 (test_gpu_sdp.py::_compare's bar),
     converged == 1, the nodes equal where both rounding margins pass. Iteration counts are printed, not asserted:
     Jacobi and eigh may cross a stopping threshold one step apart on degenerate spectra;
  4. between the routes: converged equal and |dpobj| <= 2 tol. Not max|dX| <= 1e-8: that figure was derived for
     spectra with gaps, and the equal cliques and the star have none by construction.
The huge rungs (s >= 2^52: no valid support) have the certificate's own bars alone: status 0, every output finite,
|tr X - 1| <= 1e-9, lambda_min(X) >= -1e-9, Y <= 0 on the mask, viol <= r_prim, the recomputed d within
1e-7 max(1, |d|) of -dobj, and two runs give the same bits. The weak-duality comparison is left out there: its
tolerance means nothing at 2^100.
For every case two calls give the same bits on each route, and every batch problem gives the bits of its lone call.

Measured on one MI355X, seconds per solve (t_solve; a test of a case on a route solves twice), workgroup / wide route:
star-9 0.017 / 0.048, star-17 0.070 / 0.164, star-33 0.25 / 0.50, star-65 1.14 / -, path-33 1.63 / 4.20 (so the wide
route has path-17 instead), path-65 at 200 iterations 0.34 / 0.54, tiefill-33 0.11 / 0.25, tiefill-65 1.50 / 2.29,
ladder-17-2^10 0.28 / 0.74; every quick kind, n = 128 and 129 included, under 0.01. The slowest tests: tiefill-65 on the
wide route 4.6 s, path-33 on the workgroup route 3.6 s, the contexts of tiefill-65 and path-33 3.3 s per storage; the
whole file 80 s."""
import functools

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth
from tests import sdp_edge_cases as ec
from tests import sdp_model as sm
from tests.test_gpu_sdp import _certificate, _margin_ok

pytestmark = pytest.mark.gpu
CASES = ec.by_name()
ROUTE = {ec.WG: abi.SDP_ROUTE_WORKGROUP, ec.WIDE: abi.SDP_ROUTE_WIDE}
STORAGES = (abi.STORE_F32_CSC, abi.STORE_F64_CSC, abi.STORE_F32, abi.STORE_F64)
F32_STORAGES = (abi.STORE_F32_CSC, abi.STORE_F32)
BITS = ("X", "Y", "lambdas", "evec1")
INFO_BITS = ("iters", "converged", "timed_out", "num_nodes", "sweeps", "pobj", "dobj", "r_prim", "r_dual", "rho")
# the batch's one set of parameters: the huge rungs' own, so that their lone results are the batch's to the bit; the
# quick kinds converge under it, the kinds that iterate stop at the cap: both ends of a batch's solve
BATCH_EPS = dict(eps_abs=ec.TIGHT, eps_rel=ec.TIGHT, max_iters=ec.HUGE_MAX_ITERS)


@pytest.fixture(autouse=True)
def _default_route():
    """every test of this file leaves the process on the default route (the suite shares one process)"""
    try:
        yield
    finally:
        abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP)


def _under(route, fn, *a, **kw):
    abi.sdp_set_route(route)
    try:
        return fn(*a, **kw)
    finally:
        abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP)


@functools.lru_cache(maxsize=None)
def _model(name, f32=False):
    """the model's solution of a case (of the matrix an fp32 storage holds of it); computed once, never written to"""
    c = CASES[name]
    M, Cm = (c.handed.rounded_f32().dense() if f32 else (c.M, c.C))
    r = sm.solve(M, Cm, **c.eps)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


_LONE = {}


def _lone(name, route):
    """the lone call's result of a case on a route, solved once and shared (the tests read it, none writes to it)"""
    if (name, route) not in _LONE:
        c = CASES[name]
        _LONE[name, route] = _under(ROUTE[route], abi.sdp_solve, c.M, c.C, abi.SdpParams(**c.eps))
    return _LONE[name, route]


def _same_bits(a, b, what):
    for f in BITS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)
    assert a.nodes.tolist() == b.nodes.tolist() and a.thr == b.thr, what
    for f in INFO_BITS:
        assert getattr(a.info, f) == getattr(b.info, f), (what, f)


def _huge_bars(M, Cm, r):
    mask = sm.symmetric_lower(np.asarray(Cm) != 0) != 0
    for f in BITS:
        assert np.all(np.isfinite(getattr(r, f))), f
    for f in ("pobj", "dobj", "r_prim", "r_dual", "rho"):
        assert np.isfinite(getattr(r.info, f)), f
    assert np.isfinite(r.thr)
    assert abs(np.trace(r.X) - 1.0) <= 1e-9
    assert np.linalg.eigvalsh(r.X)[0] >= -1e-9
    assert np.all(r.Y[mask] <= 0.0)
    viol = np.sqrt(np.sum(np.where(mask, np.minimum(r.X, 0.0), r.X) ** 2))
    assert viol <= r.info.r_prim + 1e-9
    d = float(np.linalg.eigvalsh(sm.symmetric_lower(M) - r.Y)[-1])
    assert abs(-r.dobj - d) <= 1e-7 * max(1.0, abs(d))


def _bars(c, r, M, Cm, ref, opt, what):
    """bars 1 to 3 on one result; M, Cm: what was solved; ref: the model's solution of it (None: no bar); opt: the
    known optimum of it (None: none)"""
    if c.kind == "huge":
        _huge_bars(M, Cm, r)
        return
    p, d = _certificate(M, Cm, r, c.eps_abs, c.eps_rel)
    tol = c.eps_abs + c.eps_rel * max(abs(d), abs(p))
    if opt is not None:
        assert d >= opt - 1e-9 * max(1.0, abs(opt)), (what, d, opt)
        if r.info.converged:
            assert p >= opt - tol - 1e-9, (what, p, opt)
    if ref is not None and c.converges:
        print(f"{what}: iters {r.iters} (model {ref['iters']}), sweeps {r.info.sweeps}, rho {r.info.rho}, "
              f"pobj {r.pobj!r} (model {ref['pobj']!r}), t_solve {r.info.t_solve:.3f} s")
        tol_m = c.eps_abs + c.eps_rel * abs(ref["pobj"])
        assert abs(r.pobj - ref["pobj"]) <= 2 * tol_m + 1e-9, (what, r.pobj, ref["pobj"])
        assert r.info.converged == 1, what
        if c.kind not in ("eqcliques", "tiny") and _margin_ok(ref["evec1"], ref["thr"]) and _margin_ok(r.evec1, r.thr):
            assert r.nodes.tolist() == ref["nodes"], what
        if c.compare_nodes:   # (the CPU test shows the model's margin on these kinds: the comparison does take place)
            assert _margin_ok(r.evec1, r.thr), what
    else:
        print(f"{what}: iters {r.iters}, converged {r.info.converged}, rho {r.info.rho}, pobj {r.pobj!r}, "
              f"t_solve {r.info.t_solve:.3f} s")
    if c.nodes is not None and r.info.converged:
        assert tuple(r.nodes.tolist()) == c.nodes, what     # the larger clique; the planted clique
    if c.kind == "tiny":
        assert r.iters == 1 and r.info.converged == 1
        assert np.max(np.abs(r.X - np.eye(c.n) / c.n)) <= 1e-12
    if not c.converges and c.kind != "huge":
        assert r.iters == c.max_iters and r.info.converged == 0   # path-65: the certificate launch


# ---- 1. every case on every route it runs on, twice --------------------------------------------------------------------

@pytest.mark.parametrize("name,route", [(c.name, rt) for c in ec.all_cases() for rt in c.routes])
def test_case_on_route(name, route):
    c = CASES[name]
    r = _lone(name, route)
    assert r.info.route == ROUTE[route] and r.info.timed_out == 0
    again = _under(ROUTE[route], abi.sdp_solve, c.M, c.C, abi.SdpParams(**c.eps))
    _same_bits(again, r, f"{name} on the {route} route, second call")
    _bars(c, r, c.M, c.C, None if c.kind == "huge" else _model(name), c.opt, f"{name} [{route}]")


# ---- 2. between the routes -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in ec.all_cases() if len(c.routes) == 2 and c.kind != "huge"])
def test_routes_agree(name):
    c = CASES[name]
    wg, wide = _lone(name, ec.WG), _lone(name, ec.WIDE)
    tol = c.eps_abs + c.eps_rel * max(abs(wg.pobj), abs(wg.dobj))
    print(f"{name}: iters {wg.iters} / {wide.iters}, |dpobj| = {abs(wide.pobj - wg.pobj):.3e} (2 tol = {2 * tol:.3e}), "
          f"max|dX| = {np.max(np.abs(wide.X - wg.X)):.3e}")
    assert wide.info.converged == wg.info.converged
    assert abs(wide.pobj - wg.pobj) <= 2 * tol


# ---- 3. one batch that mixes all the cases of n <= 128 with an ordinary problem ---------------------------------------------

@functools.lru_cache(maxsize=None)
def _scored(m=40, rho=0.7, seed=43):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    g = abi.HipClipper(storage=abi.STORE_F64)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    M, Cm = g.get_affinity_matrix(), g.get_constraint_matrix()
    M.setflags(write=False)
    Cm.setflags(write=False)
    return M, Cm


BATCH_NAMES = [c.name for c in ec.all_cases() if c.n <= 128]


@functools.lru_cache(maxsize=None)
def _batch():
    """one call: every case of n <= 128, the scored problem in the middle"""
    probs = [(CASES[n].M, CASES[n].C) for n in BATCH_NAMES]
    mid = len(probs) // 2
    probs.insert(mid, _scored())
    got = abi.sdp_solve_batch(probs, abi.SdpParams(**BATCH_EPS))
    assert len(got) == len(probs)
    ordinary = got.pop(mid)
    return dict(zip(BATCH_NAMES, got)), ordinary


@pytest.mark.parametrize("name", BATCH_NAMES + ["scored"])
def test_batch_problem_is_its_lone_call(name):
    by_name, ordinary = _batch()
    if name == "scored":
        M, Cm = _scored()
        lone = abi.sdp_solve(M, Cm, abi.SdpParams(**BATCH_EPS))
        _same_bits(ordinary, lone, "the scored problem of the batch")
        _certificate(M, Cm, ordinary, BATCH_EPS["eps_abs"], BATCH_EPS["eps_rel"])
        return
    c, rb = CASES[name], by_name[name]
    lone = _lone(name, ec.WG) if c.eps == BATCH_EPS else abi.sdp_solve(c.M, c.C, abi.SdpParams(**BATCH_EPS))
    _same_bits(rb, lone, f"{name} in the batch")
    assert rb.info.route == abi.SDP_ROUTE_WORKGROUP
    if c.kind == "huge":
        _huge_bars(c.M, c.C, rb)
    else:
        _, d = _certificate(c.M, c.C, rb, BATCH_EPS["eps_abs"], BATCH_EPS["eps_rel"])
        if c.opt is not None:
            assert d >= c.opt - 1e-9 * max(1.0, abs(c.opt)), (name, d, c.opt)


# ---- 4. the handed-over kinds through a context: both setters, the four storages ---------------------------------------------

def _context_params():
    out = []
    for c in ec.quick_cases():
        out.append(pytest.param(c.name, STORAGES, id=c.name))
    for c in ec.iterating_cases():   # (seconds each: one storage per test)
        out += [pytest.param(c.name, (s,), id=f"{c.name}-storage{s}") for s in STORAGES]
    return out


def _held_opt(c, M):
    """the known optimum of the matrix a storage holds of the case (unit weights and C = I: the table's own)"""
    if c.opt is None:
        return None
    return float(np.linalg.eigvalsh(M)[-1]) if c.kind == "ccomplete" else c.opt


@pytest.mark.parametrize("name,storages", _context_params())
def test_context_after_both_setters(name, storages):
    c = CASES[name]
    route = abi.SDP_ROUTE_WORKGROUP if c.n <= 128 else abi.SDP_ROUTE_AUTO
    for storage in storages:
        f32 = storage in F32_STORAGES
        held = c.handed.rounded_f32() if f32 else c.handed
        Mh, Ch = held.dense()
        same = np.array_equal(Mh, c.M)
        ref = _model(name) if same else _model(name, True)
        first = None
        for sparse in (False, True):
            g = abi.HipClipper(storage=storage)
            if sparse:
                g.set_sparse_matrix_data(*c.handed.upper_csc())
            else:
                g.set_matrix_data(*c.handed.dense())
            assert np.array_equal(g.get_affinity_matrix(), Mh) and np.array_equal(g.get_constraint_matrix(), Ch)
            nodes, r = _under(route, g.sdp, abi.SdpParams(**c.eps))
            what = f"{name} storage {storage} {'sparse' if sparse else 'dense'} setter"
            assert nodes.tolist() == r.nodes.tolist() and g.get_solution().nodes.tolist() == nodes.tolist(), what
            _bars(c, r, Mh, Ch, ref, _held_opt(c, Mh), what)
            if first is None:
                first = r
            else:   # the same store, however it was handed over: the same solve
                _same_bits(r, first, what + " against the dense one")
            g.close()


# ---- 5. non-finite values at the host-matrix entry points ------------------------------------------------------------------

def test_refusals():
    eye = np.eye(9)
    for bad in (np.nan, np.inf, -np.inf):
        M = eye.copy()
        M[7, 2] = bad
        with pytest.raises(abi.ClipperError, match=r"error -1: sdp: M: non-finite value at row 7, column 2$"):
            abi.sdp_solve(M, eye)
        with pytest.raises(abi.ClipperError, match=r"error -1: sdp: C: non-finite value at row 7, column 2$"):
            abi.sdp_solve(eye, M)
        with pytest.raises(abi.ClipperError, match=r"error -1: problem 3: sdp: M: non-finite value at row 7, column 2$"):
            abi.sdp_solve_batch([(eye, eye)] * 3 + [(M, eye), (eye, eye)])
        with pytest.raises(abi.ClipperError, match=r"error -1: problem 1: sdp: C: non-finite value at row 7, column 2$"):
            abi.sdp_solve_batch([(eye, eye), (eye, M)])
        # only the lower triangle is read, so only it is checked
        U = eye.copy()
        U[2, 7] = bad
        r = abi.sdp_solve(U, U)
        assert r.info.converged == 1 and abs(r.pobj + 1.0) <= 1e-9
        # the next valid calls succeed
        assert abi.sdp_solve(eye, eye).info.converged == 1
        assert abi.sdp_solve_batch([(eye, eye), (U, eye)])[1].info.converged == 1
    for route in (abi.SDP_ROUTE_AUTO, abi.SDP_ROUTE_WIDE):   # before the route matters
        M = eye.copy()
        M[8, 8] = np.nan
        with pytest.raises(abi.ClipperError, match=r"error -1: sdp: M: non-finite value at row 8, column 8$"):
            _under(route, abi.sdp_solve, M, eye)
        assert _under(route, abi.sdp_solve, eye, eye).info.converged == 1
