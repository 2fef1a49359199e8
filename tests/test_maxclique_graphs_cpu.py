"""The graph table of tests/maxclique_graphs.py and the tie rule of tests/maxclique_model.py, without a device: the
hand-derived answers against the sequential model and networkx, exact_clique against a brute-force evaluation of the
rule's graph-theoretic definition, and the conditions the table promises (HEU below omega, ties, the reached edges)."""
import functools

import networkx as nx
import numpy as np
import pytest

from tests import maxclique_graphs as tg
from tests import maxclique_model as mm

SMALL = sorted(tg.SMALL)


@functools.lru_cache(maxsize=None)
def _facts(name):
    """(adj, core, deg, heu) of a small graph by the model, computed once"""
    g = tg.SMALL[name]
    adj = g.adj()
    core = mm.core_numbers(adj)
    return adj, core, adj.sum(axis=1), mm.heu(adj, core)


@functools.lru_cache(maxsize=None)
def _exact(name):
    g = tg.SMALL[name]
    adj, core, deg, heu = _facts(name)
    return mm.exact_clique(adj, core, deg, heu, omega_known=g.omega)


@pytest.mark.parametrize("name", SMALL)
def test_hand_derived_answers(name):
    g = tg.SMALL[name]
    adj, core, deg, heu = _facts(name)
    assert adj.shape == (g.m, g.m) and not adj.diagonal().any() and np.array_equal(adj, adj.T)
    assert len(g.edge_list) == g.edges == int(adj.sum()) // 2
    assert np.array_equal(g.degrees(), deg)
    assert g.core.tolist() == core.tolist()
    assert g.omega == mm.omega(adj)
    G = nx.from_numpy_array(adj)
    cn = nx.core_number(G)
    assert [cn[v] for v in range(g.m)] == g.core.tolist()
    if g.enumerable:
        assert max(len(c) for c in nx.find_cliques(G)) == g.omega
    colptr, rows, vals = g.csc()
    assert colptr[-1] == g.edges and np.all(np.diff(colptr) >= 0) and len(rows) == len(vals) == g.edges
    assert all(np.all(np.diff(rows[colptr[j]:colptr[j + 1]]) > 0) and np.all(rows[colptr[j]:colptr[j + 1]] < j)
               for j in range(g.m))


@pytest.mark.parametrize("name", SMALL)
def test_exact_clique_is_a_maximum_clique(name):
    g = tg.SMALL[name]
    adj, core, deg, heu = _facts(name)
    e = _exact(name)
    if g.edges == 0:
        assert heu == [] and e == []  # (the methods return no vertex for a graph without an edge)
        return
    assert len(e) == g.omega and mm.is_clique(adj, e) and e == sorted(e)
    if g.exact is not None:
        assert e == list(g.exact)
    if len(heu) == g.omega:
        assert e == heu


@pytest.mark.parametrize("name", [n for n in SMALL if tg.SMALL[n].enumerable and tg.SMALL[n].edges > 0])
def test_exact_clique_equals_the_definition_by_enumeration(name):
    adj, core, deg, heu = _facts(name)
    cliques = list(nx.find_cliques(nx.from_numpy_array(adj)))
    assert len(cliques) <= 5000
    assert _exact(name) == mm.exact_clique_by_enumeration(adj, core, deg, heu, cliques)


def test_search_content():
    """At least three graphs on which HEU is smaller than omega, at least two with several maximum cliques whose
    minimum-pos vertices differ (among them graphs on which EXACT has to choose, HEU being smaller)."""
    assert len(tg.HEU_BELOW_OMEGA) >= 3
    for name in tg.HEU_BELOW_OMEGA:
        g = tg.SMALL[name]
        adj, core, deg, heu = _facts(name)
        assert g.m <= 129 and 2 <= len(heu) < g.omega, name
        assert len(heu) < int(core.max()) + 1  # (EXACT is not skipped)
    searched_ties = 0
    for name in tg.TIES:
        g = tg.SMALL[name]
        adj, core, deg, heu = _facts(name)
        pos = mm.root_positions(core, deg)
        firsts = {min(c, key=lambda v: pos[v]) for c in nx.find_cliques(nx.from_numpy_array(adj)) if len(c) == g.omega}
        assert len(firsts) >= 2, name
        searched_ties += g.heu_below_omega
    assert len(tg.TIES) >= 2 and searched_ties >= 2


def test_the_larger_indexed_clique_wins_by_pos():
    """decoy_two_k5_129: the rule is by pos, not by index: the K_5 on 124..128 has the smaller (core, degree)."""
    adj, core, deg, heu = _facts("decoy_two_k5_129")
    pos = mm.root_positions(core, deg)
    assert pos[124] < pos[0] and _exact("decoy_two_k5_129") == [124, 125, 126, 127, 128]


def test_peel_launch_model_and_the_budgets_that_cut():
    """peel_launches: one launch at the default budget for every small graph; with a budget of 64 row-word operations
    the 65 two-vertex rounds of path_129 (2 * (3 + 1) operations each) take nine launches, and every HEU-below-omega
    graph is cut after its first round (its isolated vertices alone cost more than 64)."""
    for g in tg.WORD_GRAPHS:
        assert mm.peel_launches(_facts(g.name)[0], tg.PEEL_BUDGET) == 1
    assert mm.peel_launches(_facts("path_129")[0], 64) == 9
    assert mm.peel_launches(_facts("path_129")[0], 1) == 65
    assert mm.peel_launches(_facts("ring_129")[0], 1) == 1  # (a raise of the level costs nothing: one round, all peeled)
    for name in tg.HEU_BELOW_OMEGA:
        g = tg.SMALL[name]
        assert int(np.count_nonzero(g.core == 0)) * ((g.m + 63) // 64 + 1) > 64
        assert mm.peel_launches(_facts(name)[0], 64) >= 2


def test_word_edge_sizes_are_covered():
    sizes = {g.m for g in tg.WORD_GRAPHS}
    assert set(tg.WORD_SIZES) <= sizes
    for m in (63, 64, 65, 127, 128, 129):
        for family in ("ring", "path", "star"):
            assert f"{family}_{m}" in tg.SMALL
    assert {g.m % 64 for g in tg.WORD_GRAPHS} >= {0, 1, 63}


@pytest.mark.parametrize("g", tg.PEEL_GRAPHS, ids=lambda g: g.name)
def test_peel_graphs(g):
    adj = g.adj()
    assert int(adj.sum()) // 2 == g.edges == len(g.edge_list)
    assert mm.core_numbers(adj).tolist() == g.core.tolist()
    heu = mm.heu(adj, g.core)
    assert len(heu) == g.omega == 2
    assert mm.exact_clique(adj, g.core, adj.sum(axis=1), heu, omega_known=g.omega) == heu


def test_peel_frontiers_reach_the_capacity():
    """the frontier of the first peeling round (every vertex of a ring at k = 2) sits below, at and above FCAP"""
    sizes = sorted(g.m for g in tg.PEEL_GRAPHS if g.name.startswith("ring_"))
    assert sizes == [tg.FCAP - 1, tg.FCAP, tg.FCAP + 1, 4100] and 4100 > 2 * tg.FCAP  # 4100: three rounds


def test_large_graph_by_construction():
    g = tg.large_graph()
    m = g.m
    assert m == 40000 and g.edges == len(g.edge_list) == m + 10 + 36
    e = g.edge_list
    assert len({(int(a), int(b)) for a, b in e}) == g.edges and np.all(e[:, 0] < e[:, 1])
    deg = g.degrees()
    special = sorted(tg.LARGE_K5 + tg.LARGE_K66)
    assert len(set(special)) == 17 and all(b - a > 1 for a, b in zip(special, special[1:])) and special[-1] - special[0] < m - 1
    assert set(deg[list(tg.LARGE_K5)]) == {6} and set(deg[list(tg.LARGE_K66)]) == {8}
    assert np.count_nonzero(deg == 2) == m - 17
    # the core numbers by networkx (sparse): the hand-derived ones
    G = nx.Graph()
    G.add_nodes_from(range(m))
    G.add_edges_from(e.tolist())
    cn = nx.core_number(G)
    assert np.array_equal(np.array([cn[v] for v in range(m)], dtype=np.int32), g.core)
    assert g.kcore_list() == sorted(tg.LARGE_K66)
    cl = [c for c in nx.find_cliques(G) if len(c) > 2]
    assert [sorted(c) for c in cl] == [sorted(tg.LARGE_K5)] and g.omega == 5
    # the edges the graph reaches: rows of more than 64 words, overflowing frontiers, a peel cut at the default budget
    nw = (m + 63) // 64
    assert nw == 625 > 64 and (m - 17) > 19 * tg.FCAP and m * nw > tg.PEEL_BUDGET
    assert max(tg.LARGE_K66) - min(tg.LARGE_K66) > 64 * 64  # the roots' candidates span more than 64 words
