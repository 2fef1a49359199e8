"""Every solver route on degenerate graphs (tests/degenerate_cases.py) against the oracle: no edge, every edge, every pair
forbidden (u -> 0, no node), disjoint cliques, star, path, and round(F) larger than the number of positive entries of u.
tests/test_degenerate_cases_cpu.py shows on the CPU that each case's oracle result does not move with the order of the
additions — which is what lets this file ask for equality.

Routes (logged per test, and summed up by the last test of the file): the four storages under windows 0 (automatic), 1
and 6; the slices with the resident solver switched off; 2 and 3 column shards; set_matrix_data against
set_sparse_matrix_data; the three rounding modes; rescale_u0 both ways; batched calls that mix the cases with an
ordinary problem; at m > 3000, in a child process, row views built by the slice filter (handed-over matrices) and by
the rectangular fill (point-built ones), and the live sub-problem.

Bars, the project's own: the selected list equal (where the oracle's own u has selected entries within 2e-7 of each
other: the set, and entries that changed places agree to rounding — as tests/test_gpu_subproblem.py), ifinal equal, the
trial count equal on the fp64 storages, |dF| <= 1e-6 max(1, |F|), max|u - u_oracle| <= 1e-7, u finite. The fp32 storages
are compared with the oracle on the values they hold."""
import collections
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth
from oracle import clipper_ref as ref
from oracle import dsd_ref
from tests import degenerate_cases as dc
from tests.test_gpu_fill_boundaries import CHILD_ENV
from tests.test_gpu_parity import F64S, REL_SCORE, STORAGES, _check_solution

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSCS = (abi.STORE_F32_CSC, abi.STORE_F64_CSC)
WEIGHTED = ("tiefill", "uzero", "ccomplete")
ROUTES = collections.Counter()     # what ran, over the whole file
RAN = set()                        # which of the tests that reach the solver routes ran in this process
_ORACLE = {}


def _held(c, storage):
    """the case as `storage` holds it: fp32 storages round the weights (0, 0.5 and 1 are exact)"""
    return c.rounded_f32() if (storage not in F64S and c.kind in WEIGHTED) else c


def _oracle(c, **pkw):
    """the C++ oracle's solution of the case (one solve per case and parameter set, shared by every route)"""
    key = (c.name, tuple(sorted(pkw.items())))
    if key not in _ORACLE:
        r = ref.RefClipper(ref.Params(**pkw))
        if c.from_points:
            r.score_pairwise_consistency_euclidean(c.D1, c.D2, c.A, **dc.POINT_INV)
        else:
            r.set_sparse_matrix_data(*c.upper_csc())
        _ORACLE[key] = r.solve(c.u0)
    return _ORACLE[key]


def _load(g, c, sparse=False):
    if c.from_points:
        g.score_pairwise_consistency_euclidean(c.D1, c.D2, c.A, **dc.POINT_INV)
    elif sparse:
        g.set_sparse_matrix_data(*c.upper_csc())
    else:
        g.set_matrix_data(*c.dense())


def _nodes_match(nodes, u, sr):
    """the oracle's list; where the oracle's own selected entries lie within 2e-7 of each other (degenerate_cases.
    tied_entries) the same set, and entries that changed places agree to rounding"""
    na, nb = np.asarray(nodes), np.asarray(sr.nodes)
    if not dc.tied_entries(sr.u, sr.nodes):
        assert na.tolist() == nb.tolist(), "selected node list differs"
        return
    assert na.size == nb.size and sorted(na.tolist()) == sorted(nb.tolist()), "selected node set differs"
    ua, ub = np.asarray(u), np.asarray(sr.u)
    tol = max(1e-9, 4 * float(np.max(np.abs(ua - ub))))
    for k in np.nonzero(na != nb)[0]:
        assert abs(ua[na[k]] - ua[nb[k]]) < tol and abs(ub[na[k]] - ub[nb[k]]) < tol, (int(k), int(na[k]), int(nb[k]))


def _check(sg, sr, c, storage, what, g=None):
    try:
        assert np.all(np.isfinite(sg.u)) and np.isfinite(sg.score), "u or F is not finite"
        _nodes_match(sg.nodes, sg.u, sr)
        _check_solution(sg, sr, exact_counts=(storage in F64S), ordered=False)
        assert np.max(np.abs(sg.u - sr.u), initial=0.0) <= dc.U_TOL, "u differs"
        if c.kind == "uzero":
            assert not sg.u.any() and sg.score == 0.0 and sg.nodes.size == 0
            if g is not None:
                assert g.get_selected_associations().shape == (0, 2)
    except AssertionError as e:
        raise AssertionError(f"{c.name} [{what}]: {e}\n  gpu: nodes={sg.nodes.tolist()[:40]} F={sg.score!r} ifinal={sg.ifinal} "
                             f"trials={sg.n_trials}\n  oracle: nodes={sr.nodes.tolist()[:40]} F={sr.score!r} ifinal={sr.ifinal} "
                             f"trials={sr.n_trials}\n  max|du|={np.max(np.abs(sg.u - sr.u), initial=0.0):.3g}") from None


def _route(g, shards=1):
    """which solver ran, for the log (storage_in_use: slices or the dense store — an explicit C lives in the latter)"""
    if shards > 1:
        return "column shards"
    if g.last_solver == 1:
        return "resident"
    return "streaming slices" if g.storage_in_use in CSCS else "streaming dense"


def _log(local, route):
    local[route] += 1
    ROUTES[route] += 1


SMALL = dc.small_handed() + dc.small_points()


# ---- small cases: storages, windows, resident on / off, column shards, the two setters ----------------------------------

@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_storages_windows_resident_and_shards(case):
    c, local = case, collections.Counter()
    RAN.add("small")
    explicit = (not c.from_points) and c.explicit_c
    for storage in STORAGES:
        held = _held(c, storage)
        sr = _oracle(held)
        for V in (0, 1, 6):
            g = abi.HipClipper(storage=storage)
            g.set_window(V)
            _load(g, c)
            if V == 0 and not c.from_points:   # the matrix the storage holds is the one its oracle solved
                Mh, Ch = held.dense()
                assert np.array_equal(g.get_affinity_matrix(), Mh) and np.array_equal(g.get_constraint_matrix(), Ch)
            sg = g.solve(c.u0)
            _check(sg, sr, c, storage, f"storage {storage} window {V}", g)
            if explicit or V != 0:
                # an explicit C lives in the dense store, and a forced window is the streaming launches': neither is
                # refused, both run without the resident solver
                assert g.last_solver == 0 and (not explicit or g.storage_in_use not in CSCS)
            _log(local, _route(g))
            if c.kind == "uzero" and V == 0:
                # the same context once more, with another u0 and then with an ordinary matrix: nothing of the zero
                # window (its norms, its hold, its counters) may leak into the next solve
                u1 = dc._u0(77, c.m)
                r1 = ref.RefClipper()
                r1.set_sparse_matrix_data(*held.upper_csc())
                _check(g.solve(u1), r1.solve(u1), c, storage, f"storage {storage}: second solve, another u0", g)
                o = dc.two_cliques(40, 7, 5)
                _load(g, o)
                _check(g.solve(o.u0), _oracle(o), o, storage, f"storage {storage}: an ordinary matrix after {c.name}", g)
            g.close()
        if storage in CSCS:
            g = abi.HipClipper(storage=storage)
            g.set_resident(1)
            _load(g, c)
            sg = g.solve(c.u0)
            assert g.last_solver == 0
            _check(sg, sr, c, storage, f"storage {storage}, resident solver off", g)
            _log(local, _route(g))
            g.close()
    for storage in (abi.STORE_F64, abi.STORE_F64_CSC):
        for n in (2, 3):
            g = abi.HipClipper(storage=storage, group=[0] * n)
            _load(g, c)
            _check(g.solve(c.u0), _oracle(c), c, storage, f"storage {storage}, {n} column shards", g)
            _log(local, _route(g, n))
            g.close()
    if not c.from_points:
        for storage in (abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC):
            a, b = abi.HipClipper(storage=storage), abi.HipClipper(storage=storage)
            _load(a, c)
            _load(b, c, sparse=True)
            assert np.array_equal(a.get_affinity_matrix(), b.get_affinity_matrix())
            assert np.array_equal(a.get_constraint_matrix(), b.get_constraint_matrix())
            sa, sb = a.solve(c.u0), b.solve(c.u0)
            assert sa.nodes.tolist() == sb.nodes.tolist() and np.array_equal(sa.u, sb.u), f"{c.name}: the two setters differ"
            assert sa.score == sb.score and sa.ifinal == sb.ifinal and sa.n_trials == sb.n_trials and a.last_solver == b.last_solver
            _check(sb, _oracle(_held(c, storage)), c, storage, f"storage {storage}, sparse setter", b)
            _log(local, "sparse setter")
            a.close()
            b.close()
    sr = _oracle(c)
    print(f"{c.name}: oracle trials={sr.n_trials} ifinal={sr.ifinal} nodes={len(sr.nodes)} F={sr.score:.6g}; routes {dict(local)}")


# ---- rounding modes: an empty S, k = 0, k above the number of positive entries ------------------------------------------

def _dsd_oracle(c, sr):
    """Rounding::DSD (clipper.cpp:294-300) from the oracle's u: dsd::solve(M, nnz(u)) — an EMPTY list means every node
    (dsd.cpp:278-284)"""
    M, _ = c.dense()
    return dsd_ref.densest_subgraph(M, np.nonzero(sr.u > 0)[0].tolist())


@pytest.mark.parametrize("case", [c for c in dc.small_handed() if c.kind in ("uzero", "tiefill", "edgeless") and c.m <= 129],
                         ids=lambda c: c.name)
def test_rounding_modes(case):
    c = case
    for storage in (abi.STORE_F64, abi.STORE_F32_CSC):
        held = _held(c, storage)
        for rounding in (abi.ROUNDING_NONZERO, abi.ROUNDING_DSD_HEU, abi.ROUNDING_DSD):
            if rounding == abi.ROUNDING_DSD and c.kind == "uzero" and c.m > 65:
                continue   # (the whole graph through the Python restatement of Goldberg's algorithm: seconds)
            g = abi.HipClipper(abi.Params(rounding=rounding), storage=storage)
            _load(g, c)
            sg = g.solve(c.u0)
            if rounding == abi.ROUNDING_DSD:
                sr = _oracle(held)
                want = _dsd_oracle(held, sr)
                assert sg.nodes.tolist() == want, f"{c.name} storage {storage} Rounding::DSD: {sg.nodes.tolist()} != {want}"
                assert sg.ifinal == sr.ifinal and abs(sg.score - sr.score) <= REL_SCORE * max(1.0, abs(sr.score))
                assert np.max(np.abs(sg.u - sr.u), initial=0.0) <= dc.U_TOL
            else:
                sr = _oracle(held, rounding=rounding)
                _check(sg, sr, c, storage, f"storage {storage} rounding {rounding}", g)
                if rounding == abi.ROUNDING_NONZERO:
                    assert sg.nodes.tolist() == np.nonzero(sr.u > 0)[0].tolist()
            ROUTES[f"rounding {rounding}"] += 1
            g.close()
    sr = _oracle(c)
    dsd = "not run" if (c.kind == "uzero" and c.m > 65) else f"{len(_dsd_oracle(c, sr))} nodes"
    print(f"{c.name}: positive entries {int(np.count_nonzero(sr.u > 0))}, round(F) = {int(np.round(sr.score))}, Rounding::DSD: {dsd}")


@pytest.mark.parametrize("case", [c for c in SMALL if c.kind == "cliques0"], ids=lambda c: c.name)
def test_u0_zero_on_the_larger_clique_with_and_without_rescaling(case):
    c = case
    for rescale in (0, 1):
        sr = _oracle(c, rescale_u0=rescale)
        assert sorted(sr.nodes.tolist()) == c.groups[1].tolist() and not sr.u[c.groups[0]].any()
        for storage in (abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC):
            g = abi.HipClipper(abi.Params(rescale_u0=rescale), storage=storage)
            _load(g, c)
            sg = g.solve(c.u0)
            _check(sg, sr, c, storage, f"storage {storage} rescale_u0 {rescale}", g)
            assert not sg.u[c.groups[0]].any()
            ROUTES[f"rescale_u0 {rescale}"] += 1
            g.close()


# ---- batched calls that mix degenerate problems with an ordinary one ----------------------------------------------------

@pytest.mark.parametrize("storage", CSCS)
@pytest.mark.parametrize("sizes", [(64, 65, 129), (300, 3, 65), (1, 2, 300), (129, 300, 3)])
def test_batches_that_mix_degenerate_and_ordinary_problems(storage, sizes):
    me, mc, mg = sizes
    RAN.add("batch")
    p = synth.make_euclidean_problem(300, 0.8, seed=500 + me)
    rp = ref.RefClipper()
    rp.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **dc.POINT_INV)
    sp = rp.solve(p.u0)
    ordinary = dc.Case(f"synth-300-{me}", "ordinary", 300, p.u0, D1=p.D1, D2=p.D2, A=p.A)
    cases = [dc.points_edgeless(me), dc.points_complete(mc), dc.points_two_groups(max(mg, 3)),
             dc.points_two_groups(max(mg, 3), zero_on_larger=True), ordinary]
    b = abi.HipBatch(storage=storage)
    routes = []
    for order in (list(range(len(cases))), [4, 0, 3, 1, 2]):
        probs = [cases[k] for k in order]
        sols = b.solve_euclidean([(c.D1, c.D2, c.A, c.u0) for c in probs], **dc.POINT_INV)
        for i, (c, s) in enumerate(zip(probs, sols)):
            sr = sp if c is ordinary else _oracle(c)
            _check(s, sr, c, storage, f"batch of {[q.name for q in probs]}, problem {i}, storage {storage}")
            sel = b.selected_associations(i)
            assert sel.shape == (len(sr.nodes), 2) and np.array_equal(sel, c.A[s.nodes])
            routes.append(b.route(i))
            ROUTES["batch resident" if routes[-1] == 1 else "batch, solved alone"] += 1
    launches, nb, na = b.stats()
    assert launches >= 1 and nb >= 1, (launches, nb, na)
    print(f"sizes {sizes} storage {storage}: routes {routes}, last call: {launches} launches, {nb} batched, {na} alone")
    b.close()


# ---- m > 3000: row views and the live sub-problem, in a child process ---------------------------------------------------

_LARGE_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r})
from clipper_amd import _abi as abi
from tests import degenerate_cases as dc
out = {{}}
for c in dc.large_handed() + dc.large_points():
    routes = ("noviews", "views", "sub") if c.from_points else ("noviews", "views")
    for route in routes:
        for storage in (abi.STORE_F32_CSC, abi.STORE_F64_CSC):
            g = abi.HipClipper(storage=storage)
            g.set_row_view(1 if route == "noviews" else 0)
            g.set_subproblem(0 if route == "sub" else 1)
            if c.from_points:
                g.score_pairwise_consistency_euclidean(c.D1, c.D2, c.A, **dc.POINT_INV)
            else:
                g.set_sparse_matrix_data(*c.upper_csc())
            s = g.solve(c.u0)
            st = g.view_stats()
            out[c.name + "|" + route + "|" + str(storage)] = dict(
                nodes=s.nodes.tolist(), u=s.u.tolist(), score=s.score, ifinal=s.ifinal, trials=s.n_trials,
                solver=g.last_solver, builds=st.builds, rows=st.rows, view_passes=st.view_passes, passes=st.passes,
                resident_launches=st.resident_launches, sub_entries=st.sub_entries, sub_passes=st.sub_passes,
                sub_rows=st.sub_rows)
            g.close()
print(json.dumps(out))
"""


def test_large_cases_on_views_and_the_sub_problem():
    """One child process (the sub-problem's minimum size and the view's build cost are read once per process; the
    environment of tests/test_gpu_fill_boundaries.py): every large case without views, with views, and — point-built —
    with the sub-problem allowed, on both slice storages. A handed-over matrix builds its views with the slice filter, a
    point-built one with the rectangular fill."""
    RAN.add("large")
    env = dict(os.environ, **CHILD_ENV)
    env.pop("CLIPPER_HIP_AFFINITY", None)
    # (about 40 solves of at most 550 trials at m <= 5601 and as many context set-ups: seconds; the limit is for a hang)
    out = subprocess.run([sys.executable, "-c", _LARGE_CHILD.format(root=ROOT)], env=env, capture_output=True, text=True,
                         timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    cases = {c.name: c for c in dc.large_handed() + dc.large_points()}
    filter_builds = fill_builds = sub_entries = 0
    for key, x in res.items():
        name, route, storage = key.split("|")
        c, storage = cases[name], int(storage)
        sr = _oracle(_held(c, storage))
        sg = abi.Solution(ifinal=x["ifinal"], nodes=np.array(x["nodes"], np.int32), u=np.array(x["u"]), score=x["score"],
                          n_trials=x["trials"])
        print(f"{key}: trials {x['trials']} (oracle {sr.n_trials}) ifinal {x['ifinal']} nodes {len(x['nodes'])} builds {x['builds']} "
              f"rows {x['rows']} view passes {x['view_passes']} of {x['passes']} resident launches {x['resident_launches']} "
              f"sub entries {x['sub_entries']} sub passes {x['sub_passes']}")
        _check(sg, sr, c, storage, key)
        if route == "noviews":
            assert x["builds"] == 0 and x["sub_entries"] == 0, key
        if route != "sub":
            assert x["sub_entries"] == 0, key
        if route != "noviews" and x["builds"] >= 1:
            ROUTES["rect-fill view" if c.from_points else "filter-built view"] += 1
            fill_builds += c.from_points
            filter_builds += not c.from_points
        if x["sub_entries"] >= 1:
            ROUTES["sub-problem"] += 1
            sub_entries += 1
        ROUTES["resident" if x["solver"] == 1 else "streaming slices"] += 1
    assert filter_builds >= 1, "no handed-over large case built a view with the slice filter"
    assert fill_builds >= 1, "no point-built large case built a view"
    assert sub_entries >= 1, "no point-built large case entered the live sub-problem"


def test_every_route_was_reached():
    """(the last test of the file: what the tests above logged; it asks for nothing where only a part of the file ran)"""
    print("routes reached:", dict(sorted(ROUTES.items())))
    if RAN != {"small", "batch", "large"}:
        return
    for route in ("streaming dense", "streaming slices", "resident", "batch resident", "column shards", "filter-built view",
                  "rect-fill view", "sub-problem"):
        assert ROUTES[route] >= 1, f"route never reached: {route}"
