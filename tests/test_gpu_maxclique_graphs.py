"""GPU tests of the maximum-clique kernels (k_maxclique.hip.h) on the structured graphs of tests/maxclique_graphs.py:
every answer against the hand-derived table, HEU's list against the sequential model, and EXACT's LIST against the
tie rule (tests/maxclique_model.py exact_clique): the node list is a function of the graph, whatever the interleaving
of the slots, the storage, and the number of launches the work is cut into (abi.debug_mc_budgets)."""
import functools

import numpy as np
import pytest

from clipper_amd import _abi as abi
from tests import maxclique_graphs as tg
from tests import maxclique_model as mm
from tests import maxclique_seed_model as sm

pytestmark = pytest.mark.gpu
STORAGES = (abi.STORE_F32_CSC, abi.STORE_F64_CSC, abi.STORE_F32, abi.STORE_F64)
METHODS = (abi.MC_KCORE, abi.MC_HEU, abi.MC_EXACT)
SMALL = sorted(tg.SMALL)


@functools.lru_cache(maxsize=None)
def _model(name):
    """(adj, heu, exact) by the sequential model on the hand-derived cores, once per graph"""
    g = tg.SMALL.get(name) or tg.PEEL[name]
    adj = g.adj()
    heu = mm.heu(adj, g.core)
    exact = mm.exact_clique(adj, g.core, g.degrees(), heu, omega_known=g.omega)
    return adj, heu, exact


@pytest.fixture
def budgets():
    """sets the launch budgets, and restores the library's constants afterwards"""
    yield abi.debug_mc_budgets
    abi.debug_mc_budgets(0, 0)


def _context(g, storage, sparse):
    c = abi.HipClipper(storage=storage)
    if sparse:
        c.set_sparse_matrix_data(g.m, *g.csc(), *g.csc())
    else:
        Cm = g.C()
        c.set_matrix_data(Cm, Cm)
    return c


def _check(c, g, heu, exact):
    """Every equality of one context; returns the three lists. An edgeless graph: KCORE lists every vertex, HEU and
    EXACT none, and no search is entered (its counters stay 0)."""
    assert c.core_numbers().tolist() == g.core.tolist()
    kc, info = c.max_clique(abi.MC_KCORE)
    assert kc.tolist() == g.kcore_list()
    assert info.edges == g.edges and info.max_core == int(g.core.max())
    h, info = c.max_clique(abi.MC_HEU)
    assert h.tolist() == list(heu) and info.heuristic_size == len(heu) and info.timed_out == 0
    e, info = c.max_clique(abi.MC_EXACT)
    assert len(e) == (g.omega if g.edges else 0)
    assert e.tolist() == list(exact)
    assert info.timed_out == 0 and info.edges == g.edges and info.max_core == int(g.core.max())
    assert info.heuristic_size == len(heu)
    if g.edges and info.heuristic_size < info.max_core + 1:
        assert info.roots_searched + info.roots_pruned == g.m, (info.roots_searched, info.roots_pruned)
    e2, _ = c.max_clique(abi.MC_EXACT)
    h2, _ = c.max_clique(abi.MC_HEU)
    assert e2.tolist() == e.tolist() and h2.tolist() == h.tolist()
    return kc.tolist(), h.tolist(), e.tolist()


@pytest.mark.parametrize("name", SMALL)
def test_small_graph_on_every_storage(name):
    """set_matrix_data(C, C): C is M's pattern, so the slice storages build the adjacency from the slices and the dense
    ones from the dense store. Word edges: m mod 64 in {0, 1, 63} across the table (asserted in the CPU tests)."""
    g = tg.SMALL[name]
    adj, heu, exact = _model(name)
    if g.exact is not None:
        assert list(g.exact) == exact
    if g.heu_below_omega:
        assert len(heu) < g.omega
    lists = []
    for storage in STORAGES:
        c = _context(g, storage, sparse=False)
        assert c.storage_in_use == storage
        lists.append(_check(c, g, heu, exact))
        c.close()
    assert all(x == lists[0] for x in lists)


@pytest.mark.parametrize("name", sorted(tg.PEEL))
def test_peel_edge_graph(name):
    """Frontiers at, one above and two rounds above MC_PEEL_FCAP (a ring at k = 2: all m vertices at once), and the
    1000 two-vertex rounds of a path."""
    g = tg.PEEL[name]
    adj, heu, exact = _model(name)
    if name in ("ring_2049", "ring_4100"):
        assert int(np.count_nonzero(g.degrees() <= 2)) > tg.FCAP  # the overflow path is taken
    lists = [_check(c, g, heu, exact) for c in (_context(g, abi.STORE_F32_CSC, True), _context(g, abi.STORE_F32, False))]
    assert lists[0] == lists[1]


def test_large_graph_long_rows_overflowing_frontiers_and_a_cut_peel():
    """m = 40 000 through set_sparse_matrix_data: nw = 625 > 64 (the strided loops of the colouring and the branch take
    more than one pass), twenty rounds whose frontier overflows, and a peel launch cut at the default budget
    (MC_PEEL_BUDGET of host_maxclique.hpp: m * nw > 2^24)."""
    g = tg.large_graph()
    nw = (g.m + 63) // 64
    assert nw > 64 and g.m * nw > tg.PEEL_BUDGET and g.m - 17 > 19 * tg.FCAP
    c = _context(g, abi.STORE_F32_CSC, sparse=True)
    assert c.storage_in_use == abi.STORE_F32_CSC
    _check(c, g, g.exact, g.exact)
    # adjacency, degrees and at least two peel launches: 14 rounds of 2048 vertices spend 14 * 2048 * 626 > 2^24
    assert 14 * tg.FCAP * (nw + 1) > tg.PEEL_BUDGET > 13 * tg.FCAP * (nw + 1)
    c.core_numbers()
    assert c.mc_launches() == 2 + 2
    c.close()


# ---- launch cuts ------------------------------------------------------------------------------------------------------

def _three(c):
    """(lists, launches, infos) of the three methods"""
    lists, launches, infos = [], [], []
    for meth in METHODS:
        nodes, info = c.max_clique(meth)
        lists.append(nodes.tolist())
        launches.append(c.mc_launches())
        infos.append(info)
    return lists, launches, infos


@pytest.mark.parametrize("name", SMALL)
def test_launch_cuts_change_no_result(name, budgets):
    """Budgets of 1 and of 64 row-word operations per launch (and of 8 on the graphs EXACT has to search): the three
    methods return what they return at the default budgets, in more launches. The counts, all read here:
      * KCORE's grows by exactly the peel's extra launches (mm.peel_launches: a launch ends at the end of the round
        in which the budget is spent; a raise of the level costs nothing);
      * no method's count shrinks, and every method's is strictly larger wherever the peel is cut (every graph with two
        peeling rounds at budget 1; paths, stars' hubs and the graphs with isolated vertices at 64). A graph that is
        peeled in one round and searched in one step per root (a ring, a biclique) cannot take more launches: there
        the counts are equal;
      * on the HEU-below-omega graphs at budget 1 a slot makes one step per launch, and the winning root needs a step
        per level down to its leaf of omega vertices: EXACT takes at least omega - 1 search launches (and the
        collection) on top of HEU's, against one at the default budget. Every such search went through a resume.
    """
    g = tg.SMALL[name]
    adj, heu, exact = _model(name)
    c = _context(g, abi.STORE_F32_CSC, sparse=False)
    abi.debug_mc_budgets(0, 0)
    want, l0, i0 = _three(c)
    assert want == [g.kcore_list(), list(heu), list(exact)]
    assert mm.peel_launches(adj, tg.PEEL_BUDGET) == 1
    if g.heu_below_omega:
        assert i0[2].bb_nodes * (g.m + 1) + g.m < tg.WAVE_BUDGET and l0[2] - l0[1] == 2
    # (8 on the searching graphs: a slot is cut after a few steps, at whatever depth it has reached by then)
    for b in sorted({max(1, g.budget), max(64, g.budget)} | ({8} if g.heu_below_omega else set())):
        budgets(b, b)
        got, lb, ib = _three(c)
        assert got == want, (b, got, want)
        assert ib[2].timed_out == 0
        if g.edges and ib[2].heuristic_size < ib[2].max_core + 1:
            assert ib[2].roots_searched + ib[2].roots_pruned == g.m
        extra = mm.peel_launches(adj, b) - 1
        print(f"{name}: budget {b}: launches {lb} (default {l0}), peel launches {extra + 1}")
        assert lb[0] - l0[0] == extra, (b, lb, l0)
        for k in range(3):
            assert lb[k] >= l0[k] + extra, (b, lb, l0)
            if extra > 0:
                assert lb[k] > l0[k]
        if g.heu_below_omega and b == 1:
            assert lb[2] - lb[1] >= g.omega and lb[2] > l0[2] + extra, (lb, l0)
        abi.debug_mc_budgets(0, 0)
    c.close()


def test_launch_cuts_reach_every_resume_path():
    """what the table gives the test above: a peel cut at 1 and at 64, and a resumed EXACT search on three graphs"""
    assert mm.peel_launches(_model("path_129")[0], 64) == 9 and mm.peel_launches(_model("path_129")[0], 1) == 65
    assert len(tg.HEU_BELOW_OMEGA) >= 3
    assert all(mm.peel_launches(_model(n)[0], 64) >= 2 for n in tg.HEU_BELOW_OMEGA)
    assert {g.m % 64 for g in tg.WORD_GRAPHS} >= {0, 1, 63}  # vertex m - 1 on bit 63, on bit 0 of a new word, on bit 62


def test_launch_cuts_with_more_seeds_and_roots_than_slots(budgets):
    """ring_4100 at budgets of 1: the peel takes its three rounds (2048, 2048 and 4 vertices) in three launches; HEU has
    4100 seeds and EXACT 4100 roots for min(8 per compute unit, 4100) slots, and a slot finishes one seed, or one step
    of one root, per launch (no seed is skipped: core + 1 = 3 is never below the best size 2), so both phases come back
    for the rest through `head` in ceil(4100 / slots) launches. The lists are those of the default budgets."""
    g = tg.PEEL["ring_4100"]
    adj, heu, exact = _model("ring_4100")
    c = _context(g, abi.STORE_F32_CSC, sparse=True)
    slots = min(8 * c.device_info()[1], g.m)
    rounds = -(-g.m // slots)
    want, l0, _ = _three(c)
    assert want == [g.kcore_list(), list(heu), list(exact)]
    budgets(1, 1)
    got, l1, i1 = _three(c)
    print(f"ring_4100: launches {l1} (default {l0}), {slots} slots")
    assert got == want
    assert i1[2].roots_searched + i1[2].roots_pruned == g.m and i1[2].timed_out == 0
    assert l1[0] - l0[0] == 2
    assert l1[1] - l0[1] >= 2 + (rounds - 1) and l1[2] - l0[2] >= 2 + 2 * (rounds - 1)
    if slots < g.m:
        assert l1[1] > l0[1] + 2 and l1[2] > l1[1]
    c.close()


# ---- seeded calls -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", tg.HEU_BELOW_OMEGA)
def test_seeded_calls_on_heu_below_omega_graphs(name):
    """A seed inside a maximum clique (three vertices of exact_clique's) and a seed that is a maximal but smaller
    clique (HEU's): MC_EXACT returns omega vertices, the list and the winner of the seeded model."""
    g = tg.SMALL[name]
    adj, heu, exact = _model(name)
    assert mm.is_clique(adj, heu) and not any(adj[v][heu].all() for v in range(g.m) if v not in heu)  # maximal
    for storage in (abi.STORE_F32_CSC, abi.STORE_F64):
        c = _context(g, storage, sparse=False)
        for seed in (exact[:3], heu):
            want, winner, b = sm.seeded_exact(adj, seed, exact, core=g.core, heu=heu)
            nodes, info, sinfo = c.max_clique(abi.MC_EXACT, seed=seed)
            assert len(nodes) == len(exact) == g.omega and mm.is_clique(adj, nodes)
            assert sinfo.winner == winner and info.heuristic_size == b and info.timed_out == 0
            assert nodes.tolist() == want
        c.close()
