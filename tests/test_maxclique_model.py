"""CPU checks of the maximum-clique model (tests/maxclique_model.py) against networkx, and of the C ABI's max-clique
declarations against the ctypes binding (a C program includes the header; gcc only, no GPU)."""
import ctypes
import os
import subprocess

import networkx as nx
import numpy as np
import pytest

from clipper_amd import _abi as abi
from tests import maxclique_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gnp(n, p, rng):
    a = np.triu(rng.random((n, n)) < p, 1)
    return a | a.T


def _nx(adj):
    return nx.from_numpy_array(adj.astype(int))


@pytest.mark.parametrize("p", [0.05, 0.2, 0.5, 0.8])
def test_model_against_networkx_gnp(p):
    rng = np.random.default_rng(int(p * 100))
    for _ in range(60):
        n = int(rng.integers(1, 81))
        adj = _gnp(n, p, rng)
        g = _nx(adj)
        core = mm.core_numbers(adj)
        assert core.tolist() == [nx.core_number(g)[v] for v in range(n)]
        assert mm.core_numbers_levels(adj).tolist() == core.tolist()
        w = len(nx.max_weight_clique(g, weight=None)[0])
        assert mm.omega(adj) == w
        h = mm.heu(adj, core)
        assert h == mm.heu_plain(adj)
        if adj.any():
            assert mm.is_clique(adj, h) and 2 <= len(h) <= w
        else:
            assert h == []
        assert mm.kcore(adj, core) == [v for v in range(n) if core[v] == core.max()]


def test_model_planted_cliques():
    rng = np.random.default_rng(7)
    for n, k in ((60, 12), (80, 20), (200, 40)):
        adj = _gnp(n, 0.15, rng)
        S = rng.choice(n, k, replace=False)
        adj[np.ix_(S, S)] = True
        np.fill_diagonal(adj, False)
        assert mm.omega(adj) == len(nx.max_weight_clique(_nx(adj), weight=None)[0]) >= k


def test_model_empty_single_complete():
    assert mm.core_numbers(np.zeros((0, 0), bool)).tolist() == [] and mm.heu(np.zeros((0, 0), bool)) == []
    one = np.zeros((1, 1), bool)
    assert mm.core_numbers(one).tolist() == [0] and mm.kcore(one) == [0] and mm.heu(one) == [] and mm.omega(one) == 1
    e = np.zeros((9, 9), bool)
    assert mm.kcore(e) == list(range(9)) and mm.heu(e) == []
    full = ~np.eye(9, dtype=bool)
    assert mm.core_numbers(full).tolist() == [8] * 9 and mm.heu(full) == list(range(9)) and mm.omega(full) == 9


def test_heu_rule_ties_and_order():
    # two disjoint triangles and an edge: the triangle with the smaller seed wins; picks by core, then index
    adj = np.zeros((8, 8), bool)
    for a, b in ((5, 6), (6, 7), (5, 7), (0, 2), (2, 4), (0, 4), (1, 3)):
        adj[a, b] = adj[b, a] = True
    assert mm.heu(adj) == [0, 2, 4]
    assert mm.greedy_clique(adj, mm.core_numbers(adj), 6) == [6, 5, 7]


def test_maxclique_abi_matches_header(tmp_path):
    src = tmp_path / "mc.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){'
                   'printf("%d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   'CLIPPER_HIP_MC_EXACT, CLIPPER_HIP_MC_HEU, CLIPPER_HIP_MC_KCORE, sizeof(clipper_maxclique_info_t),'
                   'offsetof(clipper_maxclique_info_t, num_nodes), offsetof(clipper_maxclique_info_t, max_core),'
                   'offsetof(clipper_maxclique_info_t, heuristic_size), offsetof(clipper_maxclique_info_t, timed_out),'
                   'offsetof(clipper_maxclique_info_t, edges), offsetof(clipper_maxclique_info_t, roots_searched),'
                   'offsetof(clipper_maxclique_info_t, roots_pruned), offsetof(clipper_maxclique_info_t, bb_nodes),'
                   'offsetof(clipper_maxclique_info_t, seconds));return 0;}\n')
    exe = tmp_path / "mc"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [abi.MC_EXACT, abi.MC_HEU, abi.MC_KCORE] == [0, 1, 2]
    S = abi.MaxCliqueInfo
    names = ["num_nodes", "max_core", "heuristic_size", "timed_out", "edges", "roots_searched", "roots_pruned",
             "bb_nodes", "seconds"]
    assert got[3] == ctypes.sizeof(S)
    assert got[4:] == [getattr(S, n).offset for n in names]
    facade = open(os.path.join(ROOT, "include", "clipper", "clipper.h")).read()
    assert "enum class Method { EXACT, HEU, KCORE };" in facade   # the same order as CLIPPER_HIP_MC_*
