"""GPU tests of the seeded maximum-clique call (clipper_hip_max_clique_seeded, clipper_hip_batch_max_clique_seeded,
maxclique::Params::warm_start; DESIGN.md section 9, "Seeded calls"). Expected lists come from the sequential model
(tests/maxclique_seed_model.py on tests/maxclique_model.py) and from the UNSEEDED device call, never from the seeded
call itself. The problems are rows of the table of DESIGN.md 9 "Batches" (make_euclidean_problem(m, rho, seed), bench
parameters); their contexts, unseeded results and models are those tests/test_gpu_batch_maxclique.py computes once."""
import time

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import synth
from tests import maxclique_model as mm
from tests import maxclique_seed_model as sm
from tests import test_gpu_batch_maxclique as bm

pytestmark = pytest.mark.gpu
CSC = abi.STORE_F32_CSC
INV = synth.EUCLID_BENCH_PARAMS
COUNTERS = ("roots_searched", "roots_pruned", "bb_nodes")
SEED_FIELDS = ("seed_given", "seed_kept", "seed_size", "winner")

_core, _solved = {}, {}


def core_of(row):
    if row not in _core:
        _core[row] = mm.core_numbers_levels(bm.model(row)[0])
    return _core[row]


def solve_nodes(row):
    """the node list of the device's solve() on a lone context (F32 slices); once per row"""
    if row not in _solved:
        g = bm._lone_context(row, CSC)
        _solved[row] = g.solve(bm._problem(row).u0).nodes.tolist()
        g.close()
    return _solved[row]


def unseeded(row, storage=CSC):
    return bm.lone(row, storage, abi.MC_EXACT)[0]


def _context_nodes(g):
    out = np.zeros(max(int(g.m), 1), dtype=np.int32)
    k = g.L.clipper_hip_get_nodes(g.h, abi._ip(out), len(out))
    assert k >= 0
    return out[:k].tolist()


def sfields(s):
    return tuple(getattr(s, f) for f in SEED_FIELDS)


def expect_exact(row, S):
    """(list, winner, heuristic_size) the contract's three cases give for EXACT seeded with S"""
    adj, _, heu, omega = bm.model(row)
    un = unseeded(row)
    assert len(un) == omega
    return sm.seeded_exact(adj, S, un, core_of(row), heu)


# ---- 1. the rule ---------------------------------------------------------------------------------------------------

RULE_ROWS = [(2, 0.0, 14), (64, 0.7, 2), (65, 0.9, 3), (128, 0.9, 4), (129, 0.8, 5), (200, 0.95, 6)]


@pytest.mark.parametrize("row", RULE_ROWS)
def test_seed_only_equals_the_models_seed_clique(row):
    m = row[0]
    adj = bm.model(row)[0]
    core = core_of(row)
    clique = unseeded(row)
    rng = np.random.default_rng(0)
    others = np.setdiff1d(np.arange(m), clique)
    junk = rng.choice(others, min(10, others.size), replace=False).tolist()
    last_bits = [v for v in (63, 64, 127) if v < m] or [m - 1]
    for storage in (bm.STORAGES if m <= 129 else (CSC,)):
        g = bm._lone_context(row, storage)
        sol = g.solve(bm._problem(row).u0).nodes.tolist()
        assert sol == solve_nodes(row)
        seeds = [("solution", sol), (clique, clique), (clique + junk, clique + junk)] + [([v], [v]) for v in last_bits]
        for arg, S in seeds:
            want, kept = sm.seed_clique(adj, core, S)
            nodes, info, si = g.max_clique(abi.MC_SEED_ONLY, seed=arg)
            what = f"row {row}, storage {storage}, seed {S}"
            assert nodes.tolist() == sorted(want), what
            assert sfields(si) == (len(S), kept, len(want), 2), (what, sfields(si))
            assert info.num_nodes == len(want) and info.edges == int(adj.sum()) // 2, what
            assert g.get_selected_associations().tolist() == np.asarray(bm._problem(row).A)[nodes].tolist(), what
        g.close()
    # a clique is kept whole
    q, k = sm.seed_clique(adj, core, clique)
    assert set(clique) <= set(q) and k == len(clique)


# ---- 2. still exact ------------------------------------------------------------------------------------------------

EXACT_ROWS = [(65, 0.9, 3), (96, 0.95, 103), (200, 0.95, 6), (700, 0.95, 9), (1000, 0.95, 11), (2100, 0.95, 15)]


@pytest.mark.parametrize("row", EXACT_ROWS)
def test_seeded_exact_is_still_exact(row):
    adj, _, heu, omega = bm.model(row)
    g = bm._lone_context(row, CSC)
    sol = g.solve(bm._problem(row).u0).nodes.tolist()
    want, winner, b = expect_exact(row, sol)
    q0, kept = sm.seed_clique(adj, core_of(row), sol)
    nodes, info, si = g.max_clique(abi.MC_EXACT, seed="solution")
    g.close()
    print(f"row {row}: solve() {len(sol)} nodes, kept {si.seed_kept}, seed clique {si.seed_size}, HEU {len(heu)}, "
          f"omega {omega}, winner {si.winner}, bb_nodes {info.bb_nodes}, roots searched {info.roots_searched}")
    assert info.num_nodes == len(nodes) == omega and mm.is_clique(adj, nodes), row
    assert nodes.tolist() == want and si.winner == winner and info.heuristic_size == b, (row, si.winner, winner)
    assert sfields(si)[:3] == (len(sol), kept, len(q0)) and info.timed_out == 0, (row, sfields(si))
    if row == (65, 0.9, 3):  # the seed clique is one short of omega: the search must still beat it
        assert si.winner == 0 and nodes.tolist() == unseeded(row) and si.seed_size == 5 and omega == 6


# ---- 3. the incumbent counts ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", [(700, 0.95, 9), (1000, 0.95, 11)])
def test_a_maximum_seed_fixes_the_counters(row):
    seed = unseeded(row)
    runs = []
    for storage in (CSC, abi.STORE_F64):
        g = bm._lone_context(row, storage)
        _, plain = g.max_clique(abi.MC_EXACT)
        for _ in range(2):
            nodes, info, si = g.max_clique(abi.MC_EXACT, seed=seed)
            assert nodes.tolist() == seed and sfields(si) == (len(seed), len(seed), len(seed), 2), (row, sfields(si))
            runs.append(tuple(getattr(info, f) for f in COUNTERS))
            # (a branch cut against a smaller incumbent is also cut against the final one)
            assert info.bb_nodes <= plain.bb_nodes and info.roots_searched <= plain.roots_searched, (row, runs[-1])
        g.close()
        print(f"row {row}, storage {storage}: unseeded bb_nodes {plain.bb_nodes}, roots searched {plain.roots_searched}; "
              f"seeded (searched, pruned, bb_nodes) {runs[-1]}")
    assert len(set(runs)) == 1, runs


# ---- 4. seeds that lose or do nothing ---------------------------------------------------------------------------------

def test_a_seed_that_loses_to_heu():
    row = (300, 0.9, 7)  # HEU = K + 1 = 30
    adj, _, heu, omega = bm.model(row)
    core = core_of(row)
    u = int(min(np.flatnonzero(adj.any(axis=1)), key=lambda x: (int(core[x]), int(x))))
    v = int(min(np.flatnonzero(adj[u]), key=lambda x: (int(core[x]), int(x))))
    want, winner, b = expect_exact(row, [u, v])
    assert winner == 1 and len(heu) == omega == 30 and want == unseeded(row)
    g = bm._lone_context(row, CSC)
    nodes, info, si = g.max_clique(abi.MC_EXACT, seed=[v, u])
    q0, kept = sm.seed_clique(adj, core, [u, v])
    assert nodes.tolist() == want and si.winner == 1 and info.heuristic_size == b == 30
    assert sfields(si)[:3] == (2, 2, len(q0)) and len(q0) < 30
    g.close()


def test_an_empty_seed_is_the_unseeded_call():
    for row in [(300, 0.9, 7), (200, 0.95, 6)]:
        g = bm._lone_context(row, CSC)
        n0, i0 = g.max_clique(abi.MC_EXACT)
        n1, i1, si = g.max_clique(abi.MC_EXACT, seed=[])
        assert n1.tolist() == n0.tolist() == unseeded(row)
        assert bm._fields(i1) == bm._fields(i0) and i1.timed_out == i0.timed_out == 0
        assert sfields(si) == (0, 0, 0, 0 if len(n0) > i0.heuristic_size else 1)
        if row == (300, 0.9, 7):  # (no search: nothing depends on the schedule)
            assert [getattr(i1, f) for f in COUNTERS] == [getattr(i0, f) for f in COUNTERS]
        # a context without a node list: NULL, -1 is an empty list
        fresh = bm._lone_context(row, CSC)
        n2, i2, s2 = fresh.max_clique(abi.MC_EXACT, seed="solution")
        assert n2.tolist() == n0.tolist() and sfields(s2)[:3] == (0, 0, 0)
        fresh.close()
        g.close()


def test_an_edgeless_graph_heu_and_kcore():
    g = bm._lone_context((1, 0.0, 13), CSC)
    for meth in (abi.MC_EXACT, abi.MC_HEU, abi.MC_SEED_ONLY):
        nodes, info, si = g.max_clique(meth, seed=[0])
        assert nodes.tolist() == [] and info.num_nodes == 0 and sfields(si)[:3] == (1, 0, 0), meth
    g.close()
    row = (1000, 0.95, 11)
    adj, kc, heu, omega = bm.model(row)
    g = bm._lone_context(row, CSC)
    sol = g.solve(bm._problem(row).u0).nodes.tolist()
    want, winner, b = sm.seeded_heu(adj, sol, core_of(row), heu)
    q0, kept = sm.seed_clique(adj, core_of(row), sol)
    nodes, info, si = g.max_clique(abi.MC_HEU, seed=sol)
    assert winner == 2 and want == sorted(q0) and len(q0) > len(heu)
    assert nodes.tolist() == want and sfields(si) == (len(sol), kept, len(q0), 2) and info.heuristic_size == b
    nodes, info, si = g.max_clique(abi.MC_KCORE, seed=sol)
    assert nodes.tolist() == kc == bm.lone(row, CSC, abi.MC_KCORE)[0] and si.seed_given == len(sol)
    g.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------

def test_refusals():
    row = (200, 0.95, 6)
    m = row[0]
    g = bm._lone_context(row, CSC)
    sol = g.solve(bm._problem(row).u0).nodes.tolist()
    for bad, pos in (([3, 5, m, 7], 2), ([3, -1], 1), ([3, 5, 9, 5, 3], 3)):
        with pytest.raises(abi.ClipperError, match=rf"error -1: .*seed\[{pos}\]"):
            g.max_clique(abi.MC_EXACT, seed=bad)
        assert _context_nodes(g) == sol  # (a refused call leaves the node list alone)
    nodes, info = g.max_clique(abi.MC_EXACT)
    assert nodes.tolist() == unseeded(row) and bm._fields(info) == bm.lone(row, CSC, abi.MC_EXACT)[1]
    with pytest.raises(abi.ClipperError, match=r"error -1: .*method 3"):
        g.max_clique(abi.MC_SEED_ONLY)
    with pytest.raises(abi.ClipperError, match=r"error -1: .*method 4"):
        g.max_clique(4, seed=[1])
    g.close()
    b = bm._batch([(40, 0.5, 1), (65, 0.9, 3)])
    with pytest.raises(abi.ClipperError, match=r"error -1: .*method 3"):
        b.max_clique(abi.MC_SEED_ONLY)
    b.close()
    p = bm._problem((300, 0.9, 7))
    grp = abi.HipClipper(storage=CSC, group=[0, 0])
    grp.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    with pytest.raises(abi.ClipperError, match="error -7"):
        grp.max_clique(abi.MC_EXACT, seed=[0, 1])
    grp.close()


# ---- 6. nothing else is touched ----------------------------------------------------------------------------------------

def test_no_side_effects_on_solve():
    row = (1000, 0.95, 11)
    p = bm._problem(row)
    g = bm._lone_context(row, CSC)
    s0 = g.solve(p.u0)
    nodes, info, si = g.max_clique(abi.MC_EXACT, seed="solution")
    assert si.seed_given == len(s0.nodes) and len(nodes) == bm.model(row)[3]
    assert np.array_equal(g.get_selected_associations(), np.asarray(p.A)[nodes])
    assert _context_nodes(g) == nodes.tolist()
    s1 = g.solve(p.u0)
    assert np.array_equal(s1.u, s0.u) and s1.nodes.tolist() == s0.nodes.tolist()
    g.close()


# ---- 7. batch ---------------------------------------------------------------------------------------------------------

BATCH_ROWS = bm.SMALL + [(2048, 0.95, 12), (2100, 0.95, 15)]


def _lone_seeded(row, S, meth=abi.MC_EXACT):
    g = bm._lone_context(row, CSC)
    nodes, info, si = g.max_clique(meth, seed=S)
    g.close()
    return nodes.tolist(), info, si


def _assert_equal_to_lone(row, got, want):
    (n, i, s), (ln, li, ls) = got, want
    assert n.tolist() == ln and bm._fields(i) == bm._fields(li) and sfields(s) == sfields(ls), (row, sfields(s), sfields(ls))
    assert i.timed_out == li.timed_out == 0, row
    if s.seed_size == i.num_nodes:  # the incumbent never moved: the counters depend on nothing
        assert [getattr(i, f) for f in COUNTERS] == [getattr(li, f) for f in COUNTERS], row


def test_batch_seeded_from_its_own_solve():
    b = bm._batch(BATCH_ROWS)
    res = b.max_clique(abi.MC_EXACT, seeds="solution")
    assert len(res) == len(BATCH_ROWS) and b.max_clique_stats()[1:] == (len(BATCH_ROWS) - 1, 1)
    for k, (row, got) in enumerate(zip(BATCH_ROWS, res)):
        _assert_equal_to_lone(row, got, _lone_seeded(row, solve_nodes(row)))
        adj, _, _, omega = bm.model(row)
        assert len(got[0]) == omega and (omega == 0 or mm.is_clique(adj, got[0])), row
        assert got[2].seed_given == len(solve_nodes(row)), row
        assert b.get_nodes(k).tolist() == got[0].tolist()
        assert np.array_equal(b.selected_associations(k), np.asarray(bm._problem(row).A)[got[0]].reshape(-1, 2)), row
    b.close()


def test_batch_explicit_seeds_and_refusals():
    rows = [(65, 0.9, 3), (128, 0.9, 4), (200, 0.95, 6), (129, 0.8, 5), (700, 0.95, 9)]
    b = bm._batch(rows)
    sols = [b.get_nodes(k).tolist() for k in range(len(rows))]
    seeds = [solve_nodes(r) for r in rows]
    seeds[2] = []  # the problem in the middle runs unseeded
    res = b.max_clique(abi.MC_EXACT, seeds=seeds)
    for k, (row, got) in enumerate(zip(rows, res)):
        if k == 2:
            ln, lf, _, _ = bm.lone(row, CSC, abi.MC_EXACT)
            assert got[0].tolist() == ln and bm._fields(got[1]) == lf and sfields(got[2])[:3] == (0, 0, 0), row
        else:
            _assert_equal_to_lone(row, got, _lone_seeded(row, seeds[k]))
    only = b.max_clique(abi.MC_SEED_ONLY, seeds=seeds)
    for k, (row, (n, i, s)) in enumerate(zip(rows, only)):
        q0 = sm.seed_clique(bm.model(row)[0], core_of(row), seeds[k])[0]
        assert n.tolist() == sorted(q0) and s.seed_size == len(q0), row
    # an invalid index in problem 3 fails the call naming the problem and the position; the batch stays usable
    b.solve_euclidean(bm._tuples(rows), **INV)
    bad = [list(s) for s in seeds]
    bad[3] = bad[3][:2] + [rows[3][0]]
    with pytest.raises(abi.ClipperError, match=r"error -1: problem 3: .*seed\[2\]"):
        b.max_clique(abi.MC_EXACT, seeds=bad)
    for k in range(len(rows)):
        assert b.get_nodes(k).tolist() == sols[k]
    res = b.max_clique(abi.MC_EXACT)
    for row, (n, i) in zip(rows, res):
        assert n.tolist() == unseeded(row), row
    b.close()


# ---- 8. the time limit -------------------------------------------------------------------------------------------------

def test_time_limit():
    """the 8 problems of the unseeded time-limit test, seeded from the batch's solve, limit 0.05 s: a time-out is not
    asserted, the seeded search may finish"""
    probs = [synth.make_euclidean_problem(2048, 0.98, seed=s) for s in range(77, 85)]
    inv = dict(sigma=0.1, epsilon=bm.TL_EPSILON, mindist=0.0)
    b = abi.HipBatch(storage=CSC)
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **inv)
    t0 = time.time()
    res = b.max_clique(abi.MC_EXACT, time_limit=bm.TL_LIMIT_S, seeds="solution")
    wall = time.time() - t0
    print(f"time limit {bm.TL_LIMIT_S} s, seeded: {wall:.3f} s, timed out {[i.timed_out for _, i, _ in res]}, sizes "
          f"{[len(n) for n, _, _ in res]}, seed cliques {[s.seed_size for _, _, s in res]}, given "
          f"{[s.seed_given for _, _, s in res]}")
    assert wall < 5.0, wall
    for p, sol, (nodes, info, si) in zip(probs, sols, res):
        g = abi.HipClipper(storage=CSC)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **inv)
        adj = mm.adjacency_from_matrix(g.get_constraint_matrix())
        assert mm.is_clique(adj, nodes) and info.num_nodes == len(nodes) >= si.seed_size >= 2
        assert si.seed_given == len(sol.nodes)
        if info.timed_out == 0:  # it finished within the limit, so the unlimited call is as quick
            ln, li, ls = g.max_clique(abi.MC_EXACT, seed=sol.nodes)
            assert info.num_nodes == li.num_nodes and li.timed_out == 0
        g.close()
    b.close()


# ---- 9. facade / clipperpy ------------------------------------------------------------------------------------------------

def _cp_invariant(cp):
    ip = cp.invariants.EuclideanDistanceParams()
    ip.sigma, ip.epsilon, ip.mindist = INV["sigma"], INV["epsilon"], INV["mindist"]
    return cp.invariants.EuclideanDistance(ip)


def test_clipperpy_warm_start():
    cp = clipper_amd.load_clipperpy()
    row = (700, 0.95, 9)
    p = bm._problem(row)
    adj, _, heu, omega = bm.model(row)
    A = np.asarray(p.A).astype(np.int32)
    c = cp.CLIPPER(_cp_invariant(cp), cp.Params())
    c.score_pairwise_consistency(p.D1, p.D2, A)
    warm = cp.MCParams()
    warm.warm_start = True
    with pytest.raises(Exception, match="warm_start"):
        c.solve_as_maximum_clique(warm)  # no node list yet
    c.solve(p.u0)
    sol = sorted(c.get_solution().nodes)
    c.solve_as_maximum_clique(warm)
    s = c.get_solution()
    assert omega == 35 and len(s.nodes) == 35 and mm.is_clique(adj, list(s.nodes)) and s.score == -1 and s.ifinal == 0
    assert list(s.nodes) == expect_exact(row, sol)[0]
    assert np.array_equal(np.asarray(c.get_selected_associations()), A[list(s.nodes)])
    # the explicit seed: a vertex list in any order
    c2 = cp.CLIPPER(_cp_invariant(cp), cp.Params())
    c2.score_pairwise_consistency(p.D1, p.D2, A)
    c2.solve_as_maximum_clique(cp.MCParams(), sol[::-1])
    assert list(c2.get_solution().nodes) == list(s.nodes)
    c2.solve_as_maximum_clique(cp.MCParams(), seed=[])
    assert list(c2.get_solution().nodes) == unseeded(row)
    with pytest.raises(Exception, match=r"seed\[1\]"):
        c2.solve_as_maximum_clique(cp.MCParams(), [0, row[0]])
    # the batch
    rows = [(65, 0.9, 3), (200, 0.95, 6), row]
    cb = cp.CLIPPERBatch(_cp_invariant(cp), cp.Params())
    first = cb.solve([(q.D1, q.D2, np.asarray(q.A).astype(np.int32), q.u0) for q in map(bm._problem, rows)])
    out = cb.solve_as_maximum_clique(warm)
    for i, (r, o) in enumerate(zip(rows, out)):
        assert list(o.nodes) == expect_exact(r, sorted(first[i].nodes))[0], r
        assert o.score == -1 and o.ifinal == 0 and np.all(np.asarray(o.u) == 0)
        sel = np.asarray(cb.get_selected_associations(i)).reshape(-1, 2)
        assert np.array_equal(sel, np.asarray(bm._problem(r).A)[list(o.nodes)].reshape(-1, 2))
