"""Every affinity fill route on pairs that sit exactly on its thresholds (tests/fill_boundary_gen.py): c == epsilon, one
grid step either side, epsilon one ulp either side of c, mindist exactly at / one ulp above a length — around the
origin and around large dyadic offsets, where the fp32 copies the prefilter works on lose the grid's low bits. Every
route must keep exactly the pairs the oracle keeps (C == pattern(M)): the fp32 prefilter may never reject a pair the
fp64 rule keeps. Routes (CLIPPER_HIP_AFFINITY, storage, shards -> fill kernel):
  default, one shard, fp32 values or fp64 slices, d in {2, 3}  k_affinity_sym<Inv, float | double>
  default, one shard, dense fp64                               k_affinity_compact<T, Inv>
  default, column shards, slices                               k_affinity_rect<Inv, VT, TW> (run_affinity_rect)
  default, column shards, dense                                k_affinity_compact<T, Inv>
  strip                                                        k_affinity_compact<T, Inv>
  plain, or d not in {2, 3}                                    k_affinity_plain<T, Inv>
  row view of M[rows, :] (clipper_hip_view_matvec, solve)      k_affinity_rect<Inv, VT, TW>
(Inv: the invariant's policy type of k_affinity.hip.h — EuclidInv<2 | 3>, EuclidInv<0> for any other d, PointNormalInv.)
The live sub-problem's child fill (k_affinity_sym on the points k_sub_gather_points gathers) runs in the staged test
below, but on no boundary pair: on the problems whose selected set holds the boundary pairs the solve does not hand over.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clipper_amd import _abi as abi
from oracle import clipper_ref as ref
from tests import fill_boundary_gen as gen

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

STORAGES = [abi.STORE_F32, abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC]
F64S = (abi.STORE_F64, abi.STORE_F64_CSC)
CSCS = (abi.STORE_F32_CSC, abi.STORE_F64_CSC)
FLT_MIN = float(np.finfo(np.float32).tiny)
SIGMA = gen.EPS          # boundary scores exp(-1/2): well above affinityeps
PN_PRM = dict(sigp=gen.EPS, sign=0.10, epsn=0.35)


def _route(storage, nshards, mode, d):
    if mode == "plain" or d not in (2, 3):
        return "k_affinity_plain"
    if mode == "strip" or storage == abi.STORE_F64 or (nshards > 1 and storage not in CSCS):
        return "k_affinity_compact"
    return "k_affinity_sym" if nshards == 1 else "k_affinity_rect"


def _fill(obj, p, pointnormal, eps, mindist):
    if pointnormal:
        obj.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, epsp=eps, **PN_PRM)
    else:
        obj.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, sigma=SIGMA, epsilon=eps, mindist=mindist)


def _oracle_checked(p, setting, eps, mindist, pointnormal, params=None):
    """the oracle's M and C — after checking that they keep / drop every couple as the generator's exact arithmetic
    says (so that the problem does hold boundary pairs of every kind)"""
    r = ref.RefClipper(params) if params is not None else ref.RefClipper()
    _fill(r, p, pointnormal, eps, mindist if not pointnormal else 0.0)
    Mr, Cr = r.get_affinity_matrix(), r.get_constraint_matrix()
    counts = {}
    for kind in gen.KINDS:
        if pointnormal and kind in ("md1", "md2"):
            continue  # (PointNormalDistance has no mindist)
        i, j = p.couples[kind][:, 0], p.couples[kind][:, 1]
        want = gen.expected(setting, kind)
        assert i.size > 0
        assert np.all((Mr[i, j] != 0) == want), (setting, kind)
        counts[kind] = (int(i.size), bool(want))
    return r, Mr, Cr, counts


def _check_against(g, Mr, Cr, storage, pointnormal):
    Mg, Cg = g.get_affinity_matrix(), g.get_constraint_matrix()
    assert np.array_equal(Mg != 0, Mr != 0), f"non-zero pattern differs at {np.argwhere((Mg != 0) != (Mr != 0))[:5]}"
    assert np.array_equal(Cg, Cr)
    assert np.array_equal(Mg, Mg.T)
    nz = Mr != 0
    if storage not in F64S:
        assert np.max(np.abs(Mg - Mr.astype(np.float32).astype(np.float64)), initial=0.0) <= 1.2e-7
    else:
        rel = 1e-12 if pointnormal else 4 * 2.3e-16
        assert np.max(np.abs(Mg[nz] - Mr[nz]) / Mr[nz], initial=0.0) <= rel


def _routes(d):
    """(storage, shards, mode) of every route a problem of dimension d goes through"""
    out = []
    for storage in STORAGES:
        for mode in (("sym", "strip", "plain") if d in (2, 3) else ("sym",)):
            out.append((storage, 1, mode))
        for n in (2, 3):
            out.append((storage, n, "sym" if d not in (2, 3) else ("sym" if storage in CSCS else "strip")))
    out.append((abi.STORE_F32_CSC, 2, "plain"))
    return out


def _set_mode(monkeypatch, mode):
    if mode == "sym":
        monkeypatch.delenv("CLIPPER_HIP_AFFINITY", raising=False)
    else:
        monkeypatch.setenv("CLIPPER_HIP_AFFINITY", mode)


CASES = [  # (m, d, offset exponent) — m on and off the 128-row tile / 64-column slice edges
    (127, 2, None), (129, 3, 17), (1037, 3, None), (1037, 2, 10), (2049, 3, 14), (129, 5, 12), (1037, 5, None),
]


@pytest.mark.parametrize("m,d,off", CASES)
def test_every_route_keeps_the_oracles_boundary_pairs(monkeypatch, m, d, off):
    p = gen.make(m, d, off, seed=m + 10 * d)
    for kind in gen.KINDS:  # the generator's lengths are exact
        l1, l2 = gen.lengths(p, kind)
        c = np.abs(l1 - l2)
        assert np.all(c == {"eq": gen.EPS, "below": gen.EPS - gen.H, "above": gen.EPS + gen.H,
                            "md1": gen.EPS / 2, "md2": gen.EPS / 2}[kind])
        if kind.startswith("md"):
            assert np.all(np.minimum(l1, l2) == gen.LMD)
    report = []
    for setting, eps, mindist in gen.SETTINGS:
        r, Mr, Cr, counts = _oracle_checked(p, setting, eps, mindist, False)
        for storage, n, mode in _routes(d):
            _set_mode(monkeypatch, mode)
            g = abi.HipClipper(storage=storage, group=[0] * n if n > 1 else None)
            _fill(g, p, False, eps, mindist)
            _check_against(g, Mr, Cr, storage, False)
            report.append((setting, storage, n, mode, _route(storage, n, mode, d)))
            g.close()
        monkeypatch.delenv("CLIPPER_HIP_AFFINITY", raising=False)
        # the row view's rectangular fill of the rows that hold the boundary pairs
        if d in (2, 3):
            rows = np.unique(np.concatenate([p.couples[k].ravel() for k in gen.KINDS]))
            x = np.random.default_rng(m).random(m) + 0.5
            xm = np.zeros(m)
            xm[rows] = x[rows]
            oM, oC = r.matvec(xm)
            for storage in CSCS:
                g = abi.HipClipper(storage=storage)
                _fill(g, p, False, eps, mindist)
                yM, yC = g.view_matvec(rows, x)
                assert np.max(np.abs(yC - oC)) <= 1e-12 * max(1.0, float(np.max(np.abs(oC))))
                tol = 1e-12 if storage == abi.STORE_F64_CSC else 2e-7
                assert np.max(np.abs(yM - oM)) <= tol * max(1.0, float(np.max(np.abs(oM))))
                report.append((setting, storage, 1, "view", "k_affinity_rect"))
                g.close()
        print(f"m={m} d={d} offset=2^{off} {setting}: couples {counts}")
    print("routes:", sorted({(s, n, mo, k) for _, s, n, mo, k in report}))


@pytest.mark.parametrize("m,off", [(129, 12), (1037, None)])
def test_pointnormal_routes_keep_the_oracles_boundary_pairs(monkeypatch, m, off):
    """identical unit-axis normals on both sides of every pair: acos(+-1) or acos(0) the same on both, dn = 0, and dp
    alone decides at epsp"""
    p = gen.make(m, 3, off, seed=7 * m, pointnormal=True)
    for setting, eps, _ in gen.SETTINGS:
        r, Mr, Cr, counts = _oracle_checked(p, setting, eps, 0.0, True)
        for storage, n, mode in _routes(3):
            _set_mode(monkeypatch, mode)
            g = abi.HipClipper(storage=storage, group=[0] * n if n > 1 else None)
            _fill(g, p, True, eps, 0.0)
            _check_against(g, Mr, Cr, storage, True)
            g.close()
        monkeypatch.delenv("CLIPPER_HIP_AFFINITY", raising=False)
        rows = np.unique(np.concatenate([p.couples[k].ravel() for k in ("eq", "below", "above")]))
        x = np.random.default_rng(m).random(m) + 0.5
        xm = np.zeros(m)
        xm[rows] = x[rows]
        oM, oC = r.matvec(xm)
        g = abi.HipClipper(storage=abi.STORE_F64_CSC)
        _fill(g, p, True, eps, 0.0)
        yM, yC = g.view_matvec(rows, x)
        assert np.max(np.abs(yC - oC)) <= 1e-12 * max(1.0, float(np.max(np.abs(oC))))
        assert np.max(np.abs(yM - oM)) <= 1e-12 * max(1.0, float(np.max(np.abs(oM))))
        g.close()
        print(f"pointnormal m={m} offset=2^{off} {setting}: couples {counts}")


def test_coordinates_so_large_that_fp32_squares_overflow(monkeypatch):
    """Around 2^33 with lengths up to 2^32: the square-root-free prefilter's t = s1 + s2 - E^2 squared overflows fp32.
    The threshold is then infinite (host_solver.hpp, guarded_threshold) and every pair is scored exactly."""
    rng = np.random.default_rng(33)
    m, big = 258, 2.0 ** 33
    P = big + np.round(rng.uniform(-2 ** 32, 2 ** 32, (m, 3)))
    Q = P + np.array([2.0 ** 20, -2.0 ** 21, 2.0 ** 19])
    Q[: m // 2] += rng.integers(-2, 3, (m // 2, 3)) * 2.0 ** 10    # half of them off by up to a few thousand
    A = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.int32)
    D1, D2 = np.ascontiguousarray(P.T), np.ascontiguousarray(Q.T)
    prm = dict(sigma=2.0 ** 12, epsilon=2.0 ** 12, mindist=0.0)
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(D1, D2, A, **prm)
    Mr, Cr = r.get_affinity_matrix(), r.get_constraint_matrix()
    assert np.count_nonzero(Mr) > m * m // 8
    for storage, n, mode in _routes(3):
        _set_mode(monkeypatch, mode)
        g = abi.HipClipper(storage=storage, group=[0] * n if n > 1 else None)
        g.score_pairwise_consistency_euclidean(D1, D2, A, **prm)
        _check_against(g, Mr, Cr, storage, False)
        g.close()
    monkeypatch.delenv("CLIPPER_HIP_AFFINITY", raising=False)


@pytest.mark.parametrize("pointnormal", [False, True])
def test_scores_below_flt_min_keep_the_pattern(monkeypatch, pointnormal):
    """affinityeps = 0 and a small sigma: kept scores from ~1e-30 down to ~1e-300 (fp32: normal, subnormal, and zero
    after rounding — stored as FLT_MIN so that C == pattern(M)), and pairs whose fp64 exp itself underflows to 0
    (dropped on both sides)."""
    m = 1037
    p = gen.make(m, 3, 10, seed=99, pointnormal=pointnormal)
    # exponent -c^2 / (2 sigma^2) of the couples: -200 (c = EPS / 2: fp32 zero, fp64 normal), -783 / -800 / -817
    # (c = EPS -+ H, EPS: fp64 exp underflows to 0); of the inliers (c <= EPS / 4) from -50 up; the cross pairs: anything
    sigma = gen.EPS / 40.0
    params = dict(affinityeps=0.0)
    eps = 2 * gen.EPS
    r = ref.RefClipper(ref.Params(**params))
    if pointnormal:
        r.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, sigp=sigma, epsp=eps, sign=0.1, epsn=0.35)
    else:
        r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, sigma=sigma, epsilon=eps, mindist=0.0)
    Mr, Cr = r.get_affinity_matrix(), r.get_constraint_matrix()
    f32 = Mr.astype(np.float32).astype(np.float64)
    pos = Mr > 0
    zero32 = pos & (f32 == 0)                          # fp32 rounds the score to 0
    sub32 = pos & (f32 != 0) & (f32 < FLT_MIN)         # ... to a subnormal
    assert np.count_nonzero(zero32) > 20 and np.count_nonzero(sub32) > 0 and np.count_nonzero(pos & (Mr >= FLT_MIN)) > 20
    for kind in ("below", "eq", "above"):              # c < eps, but exp(-c^2 / (2 sigma^2)) == 0 in fp64
        i, j = p.couples[kind][:, 0], p.couples[kind][:, 1]
        assert np.all(Mr[i, j] == 0)
    i, j = p.couples["md1"][:, 0], p.couples["md1"][:, 1]
    assert np.all(zero32[i, j])                        # c = EPS / 2: 1.4e-87
    for storage, n, mode in _routes(3):
        _set_mode(monkeypatch, mode)
        g = abi.HipClipper(abi.Params(**params), storage=storage, group=[0] * n if n > 1 else None)
        if pointnormal:
            g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, sigp=sigma, epsp=eps, sign=0.1, epsn=0.35)
        else:
            g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, sigma=sigma, epsilon=eps, mindist=0.0)
        Mg, Cg = g.get_affinity_matrix(), g.get_constraint_matrix()
        assert np.array_equal(Mg != 0, pos) and np.array_equal(Cg, Cr) and np.array_equal(Cg != 0, pos)
        if storage in F64S:  # the oracle's value: 4 ulp (device exp vs libm exp), a few units where it is subnormal
            rel = 1e-12 if pointnormal else 4 * 2.3e-16
            assert np.all(np.abs(Mg[pos] - Mr[pos]) <= np.maximum(rel * Mr[pos], 4 * 2.0 ** -1074))
        else:  # the fp32-rounded oracle to 1 ulp (normal or subnormal); FLT_MIN where that rounding is 0
            assert np.all(Mg[zero32] == FLT_MIN)
            rest = pos & ~zero32
            assert np.all(np.abs(Mg[rest] - f32[rest]) <= np.maximum(f32[rest] * 2.0 ** -23, 2.0 ** -149))
        g.close()
    monkeypatch.delenv("CLIPPER_HIP_AFFINITY", raising=False)


# ---- full solves: views and the live sub-problem ----------------------------------------------------------------------

LIVE = dict(m_synth=5000, rho=0.95, seed=99)          # 5440 associations: past the row view's minimum size (3000)
CHILD_ENV = dict(CLIPPER_HIP_SUBPROBLEM_MIN_M="3000", CLIPPER_HIP_RV_BUILD_SCALE="0.02")


def _child(code):
    """the sub-problem's minimum size and the view's build cost are read once per process: a child process"""
    env = dict(os.environ, **CHILD_ENV)
    env.pop("CLIPPER_HIP_AFFINITY", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def _same_list(nodes, u, sr):
    """the oracle's selected list (utils.cpp:33-55: descending by (value, index)); entries whose u agree to rounding
    may have swapped places (fp32 values move the last digits of u) — as tests/test_gpu_subproblem.py"""
    na, nb = np.asarray(nodes), np.asarray(sr.nodes)
    assert na.size == nb.size and sorted(na.tolist()) == sorted(nb.tolist())
    ua, ub = np.asarray(u), np.asarray(sr.u)
    tol = max(1e-9, 4 * float(np.max(np.abs(ua - ub))))
    for k in np.nonzero(na != nb)[0]:
        assert abs(ua[na[k]] - ua[nb[k]]) < tol and abs(ub[na[k]] - ub[nb[k]]) < tol, (int(k), int(na[k]), int(nb[k]))


def _selected_pairs(p, nodes):
    """per kind: how many boundary pairs have both ends in the selected set"""
    sel = set(int(x) for x in nodes)
    return {k: int(sum(int(a) in sel and int(b) in sel for a, b in p.couples[k])) for k in gen.KINDS}


def _check_live_oracle(p, setting, sr):
    """the oracle selects both ends of the kept boundary pairs (of every kept kind) and never both ends of a dropped one:
    the selected set rests on the boundary decisions"""
    both = _selected_pairs(p, sr.nodes)
    for kind in gen.KINDS:
        assert (both[kind] >= 3) if gen.expected(setting, kind) else (both[kind] == 0), (setting, kind, both)
    return both


_SOLVE_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
from clipper_amd import _abi as abi
from tests import fill_boundary_gen as gen
p = gen.make_live(**{live!r})
out = {{}}
for route in ("noviews", "views", "sub"):
    for storage in (abi.STORE_F32_CSC, abi.STORE_F64_CSC):
        g = abi.HipClipper(storage=storage)
        g.set_row_view(1 if route == "noviews" else 0)
        g.set_subproblem(0 if route == "sub" else 1)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, sigma={sigma!r}, epsilon={eps!r}, mindist={md!r})
        s = g.solve(p.u0)
        st = g.view_stats()
        out[route + str(storage)] = dict(nodes=s.nodes.tolist(), u=s.u.tolist(), score=s.score, ifinal=s.ifinal,
                                         trials=s.n_trials, builds=st.builds, rows=st.rows, view_passes=st.view_passes,
                                         passes=st.passes, sub_entries=st.sub_entries, sub_leaves=st.sub_leaves,
                                         sub_passes=st.sub_passes, sub_rows=st.sub_rows)
        g.close()
print(json.dumps(out))
"""


@pytest.mark.parametrize("setting", [s[0] for s in gen.SETTINGS])
def test_solves_on_views_and_the_sub_problem_keep_the_boundary_pairs(setting):
    """The boundary pairs sit inside the clique the solve selects (tests/fill_boundary_gen.py, make_live): the selected
    set holds both ends of every kept kind, so they are live rows when the solve's row views are filled again from the
    staged points (k_affinity_rect: every column of the view's rows). A boundary pair that fill dropped would break the
    clique: every route (no views, views, views + sub-problem allowed) must give the oracle's list and agree with the
    others. (The solve does not hand over to the live sub-problem on this problem: its child fill is not reached here.)"""
    _, eps, md = next(s for s in gen.SETTINGS if s[0] == setting)
    p = gen.make_live(**LIVE)
    r, _, _, counts = _oracle_checked(p, setting, eps, md, False)
    sr = r.solve(p.u0)
    both = _check_live_oracle(p, setting, sr)
    res = _child(_SOLVE_CHILD.format(root=ROOT, live=LIVE, sigma=SIGMA, eps=eps, md=md))
    for key, s in res.items():
        _same_list(s["nodes"], s["u"], sr)
        assert abs(s["score"] - sr.score) <= 1e-6 * max(1.0, abs(sr.score)), key
        assert s["ifinal"] == sr.ifinal, key
    for storage in (abi.STORE_F32_CSC, abi.STORE_F64_CSC):
        nv, v, sb = (res[f"{route}{storage}"] for route in ("noviews", "views", "sub"))
        assert nv["builds"] == 0 and nv["sub_entries"] == 0
        assert v["builds"] >= 1 and v["view_passes"] >= 1 and v["sub_entries"] == 0, v
        assert sb["builds"] >= 1 and sb["view_passes"] >= 1, sb
        # the three routes: the same point to rounding (as tests/test_gpu_subproblem.py)
        for other in (nv, sb):
            assert other["nodes"] == v["nodes"]
            assert abs(other["score"] - v["score"]) <= 1e-10 * abs(v["score"])
            assert np.allclose(other["u"], v["u"], rtol=0, atol=1e-7)
    print(setting, "boundary pairs with both ends selected:", both, {
        k: {q: v[q] for q in ("builds", "rows", "view_passes", "passes", "sub_entries", "sub_passes", "sub_rows")}
        for k, v in res.items()})


# ---- the staged entry points: one context, filled again and again --------------------------------------------------

def _same_bits(a, b):
    assert a.nodes.tolist() == b.nodes.tolist()
    assert np.array_equal(a.u, b.u)
    assert a.score == b.score and a.ifinal == b.ifinal and a.n_trials == b.n_trials


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_staged_context_filled_again_matches_fresh_one_shot_contexts(storage):
    """stage_inputs once, affinity_*_staged with other (sigma, epsilon, mindist) again and again, stage_u0 +
    solve_staged after each: every result is a fresh context's one-shot result bit for bit, and the oracle's; then
    other problems (smaller, larger, PointNormal) staged on the same context — nothing of the previous fill (its
    maxabs, E^2, slices) may carry over. (Below the row view's minimum size: views and the sub-problem are the next
    test's.)"""
    g = abi.HipClipper(storage=storage)
    problems = [(gen.make(1037, 3, 14, seed=1), False), (gen.make(600, 3, None, seed=2), False),
                (gen.make(2049, 2, 17, seed=3), False), (gen.make(1037, 3, 10, seed=4, pointnormal=True), True)]
    fills = [(gen.EPS, 0.0, gen.EPS)] + [(e, md, 2 * gen.EPS) for _, e, md in gen.SETTINGS] + [(gen.EPS / 2, 0.0, gen.EPS)]
    for p, pn in problems:
        g.stage_inputs(p.D1, p.D2, p.A)
        for eps, md, sigma in fills:
            if pn:
                g.affinity_pointnormal_staged(sigp=sigma, epsp=eps, sign=PN_PRM["sign"], epsn=PN_PRM["epsn"])
            else:
                g.affinity_euclidean_staged(sigma=sigma, epsilon=eps, mindist=md)
            g.stage_u0(p.u0)
            s = g.solve_staged()
            f = abi.HipClipper(storage=storage)
            r = ref.RefClipper()
            for obj in (f, r):
                if pn:
                    obj.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, sigp=sigma, epsp=eps, **{
                        k: PN_PRM[k] for k in ("sign", "epsn")})
                else:
                    obj.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, sigma=sigma, epsilon=eps, mindist=md)
            _same_bits(s, f.solve(p.u0))
            _check_against(g, r.get_affinity_matrix(), r.get_constraint_matrix(), storage, pn)
            sr = r.solve(p.u0)
            _same_list(s.nodes, s.u, sr)
            assert abs(s.score - sr.score) <= 1e-6 * max(1.0, abs(sr.score)) and s.ifinal == sr.ifinal
            f.close()
    g.close()


# (problem, setting) in the order the next test fills them on one context: large, small, large, PointNormal, large
_STAGED_SEQ = [("liveA", "eps"), ("liveA", "eps_up_md"), ("liveA", "eps_down_md_up"), ("small", "eps"),
               ("emb", "eps"), ("emb", "eps_up_md"), ("liveB", "eps_up_md"), ("pn", "eps_up_md"), ("emb", "eps"),
               ("liveA", "eps_up_md")]


def _staged_problems():
    return {"liveA": (gen.make_live(**LIVE), False), "small": (gen.make(1037, 3, 14, seed=1), False),
            "liveB": (gen.make_live(4000, 0.95, 7, offset_exp=None), False),
            "pn": (gen.make(1037, 3, 10, seed=4, pointnormal=True), True),
            "emb": (gen.make_embedded(5000, 0.9, 99, 257, 12), False)}


_STAGED_CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, {root!r})
from clipper_amd import _abi as abi
from tests import fill_boundary_gen as gen
from tests import test_gpu_fill_boundaries as t
probs = t._staged_problems()
settings = {{n: (e, md) for n, e, md in gen.SETTINGS}}
g = abi.HipClipper(storage={storage})
staged = None
out = []
for name, setting in t._STAGED_SEQ:
    p, pn = probs[name]
    eps, md = settings[setting]
    if name != staged:
        g.stage_inputs(p.D1, p.D2, p.A)
        staged = name
    if pn:
        g.affinity_pointnormal_staged(sigp=t.SIGMA, epsp=eps, sign=t.PN_PRM["sign"], epsn=t.PN_PRM["epsn"])
    else:
        g.affinity_euclidean_staged(sigma=t.SIGMA, epsilon=eps, mindist=md)
    g.stage_u0(p.u0)
    s = g.solve_staged()
    st = g.view_stats()
    f = abi.HipClipper(storage={storage})
    t._fill(f, p, pn, eps, md)
    o = f.solve(p.u0)
    fst = f.view_stats()
    f.close()
    out.append(dict(name=name, setting=setting, nodes=s.nodes.tolist(), u=s.u.tolist(), score=s.score, ifinal=s.ifinal,
                    same=bool(s.nodes.tolist() == o.nodes.tolist() and np.array_equal(s.u, o.u) and s.score == o.score
                              and s.ifinal == o.ifinal and s.n_trials == o.n_trials),
                    builds=st.builds, view_passes=st.view_passes, sub_entries=st.sub_entries, sub_passes=st.sub_passes,
                    fresh_builds=fst.builds, fresh_sub_entries=fst.sub_entries))
g.close()
print(json.dumps(out))
"""


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_staged_context_with_views_and_sub_problem_refilled_and_restaged(storage):
    """The staged path at the sizes where the solve builds row views and hands over to the live sub-problem (a child
    process, as above): one context is filled again with other thresholds and re-staged with small, large and
    PointNormal problems, and with the first ones again. Each staged solve must equal a fresh context's one-shot solve
    bit for bit and give the oracle's result. The large problems must have built views on the staged context, and the
    synthetic one with couples appended ("emb", make_embedded) must also have run on the sub-problem: a view, a
    sub-problem, an E^2 or a maxabs left from the previous fill would show."""
    probs = _staged_problems()
    settings = {n: (e, md) for n, e, md in gen.SETTINGS}
    res = _child(_STAGED_CHILD.format(root=ROOT, storage=storage))
    assert [(x["name"], x["setting"]) for x in res] == _STAGED_SEQ
    oracle = {}
    for x in res:
        p, pn = probs[x["name"]]
        eps, md = settings[x["setting"]]
        key = (x["name"], x["setting"])
        if key not in oracle:
            r = ref.RefClipper()
            _fill(r, p, pn, eps, md)
            oracle[key] = r.solve(p.u0)
        sr = oracle[key]
        assert x["same"], key
        _same_list(x["nodes"], x["u"], sr)
        assert abs(x["score"] - sr.score) <= 1e-6 * max(1.0, abs(sr.score)) and x["ifinal"] == sr.ifinal, key
        if x["name"].startswith("live"):
            _check_live_oracle(p, x["setting"], sr)
            assert x["builds"] >= 1 and x["view_passes"] >= 1, x
        elif x["name"] == "emb":
            assert x["builds"] >= 1 and x["view_passes"] >= 1 and x["sub_entries"] >= 1 and x["sub_passes"] >= 1, x
        else:
            assert x["builds"] == 0 and x["sub_entries"] == 0, x
    print({(x["name"], x["setting"]): {k: x[k] for k in ("builds", "view_passes", "sub_entries", "sub_passes")}
           for x in res})
