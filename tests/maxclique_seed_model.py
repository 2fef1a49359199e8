"""Sequential CPU model of the seeded maximum-clique call ("Seeded calls"), written from the
specification alone on top of tests/maxclique_model.py.

  seed_clique(adj, core, S)      the seed clique Q0 of the vertex list S, in pick order, and seed_kept
  maximum_clique(adj)            some clique of omega vertices (a stand-in for the unseeded EXACT call's list where
                                 no device is at hand)
  seeded_heu(adj, S, ...)        what method HEU returns from S: (list, winner, heuristic_size)
  seeded_exact(adj, S, unseeded) what method EXACT returns from S, given the unseeded call's list: the three cases
"""
from __future__ import annotations

import numpy as np

from tests import maxclique_model as mm


def seed_clique(adj: np.ndarray, core: np.ndarray, S) -> tuple[list[int], int]:
    """Reduce: degS(v) = |N(v) & S| once; candidates S; take the candidate of largest degS (ties: smallest index),
    intersect the candidates with its row, until none is left. Extend: the candidates become the common neighbourhood
    of the vertices taken, over all vertices; go on as greedy_clique does (largest core number, ties smallest index,
    no threshold). Returns (Q0 in pick order, seed_kept); ([], 0) for an empty S."""
    m = adj.shape[0]
    S = sorted(set(int(v) for v in S))
    assert all(0 <= v < m for v in S)
    if not S:
        return [], 0
    inS = np.zeros(m, dtype=bool)
    inS[S] = True
    degS = (adj & inS[None, :]).sum(axis=1)
    cand = inS.copy()
    common = np.ones(m, dtype=bool)
    out = []
    while cand.any():
        c = np.flatnonzero(cand)
        u = int(min(c, key=lambda x: (-int(degS[x]), int(x))))
        out.append(u)
        cand &= adj[u]
        common &= adj[u]
    kept = len(out)
    key = core.astype(np.int64) * (m + 1) + (m - np.arange(m))  # largest core, then smallest index
    c = np.flatnonzero(common)
    while c.size:
        u = int(c[np.argmax(key[c])])
        out.append(u)
        c = c[adj[u, c]]
    return out, kept


def maximum_clique(adj: np.ndarray) -> list[int]:
    """A clique of omega vertices (ascending): branch and bound with the colouring bound of the model."""
    m = adj.shape[0]
    if m == 0 or not adj.any():
        return []
    G = mm._bits(adj)
    best = list(mm.heu(adj))

    def expand(P, path):
        nonlocal best
        vs, cs = mm._colour(G, P)
        for i in range(len(vs) - 1, -1, -1):
            if len(path) + cs[i] <= len(best):
                return
            v = vs[i]
            NP = P & G[v]
            if NP == 0:
                if len(path) + 1 > len(best):
                    best = path + [v]
            else:
                expand(NP, path + [v])
            P &= ~(1 << v)

    expand((1 << m) - 1, [])
    return sorted(best)


def _incumbent(adj, core, S):
    """(Q0 ascending, s as the incumbent sees it: 0 when Q0 has fewer than two vertices, seed_kept, |Q0|)"""
    q0, kept = seed_clique(adj, core, S)
    return sorted(q0), (len(q0) if len(q0) >= 2 else 0), kept, len(q0)


def seeded_heu(adj: np.ndarray, S, core: np.ndarray | None = None, heu: list[int] | None = None):
    """Method HEU from S: HEU's clique when it is larger than Q0, else Q0 (ties go to the seed clique).
    Returns (list ascending, winner: 1 HEU's clique / 2 the seed clique, heuristic_size = max(s, HEU))."""
    if adj.shape[0] == 0 or not adj.any():
        return [], 0, 0
    core = mm.core_numbers(adj) if core is None else core
    heu = mm.heu(adj, core) if heu is None else heu
    q0, s, _, _ = _incumbent(adj, core, S)
    if s >= 2 and s >= len(heu):
        return q0, 2, s
    return list(heu), 1, len(heu)


def seeded_exact(adj: np.ndarray, S, unseeded: list[int], core: np.ndarray | None = None,
                 heu: list[int] | None = None):
    """Method EXACT from S, given the unseeded EXACT call's list (a maximum clique). With b = max(s, HEU):
    omega > b: the unseeded list (winner 0); omega = b and s >= HEU: Q0 (winner 2); omega = b and s < HEU: the unseeded
    list, which is HEU's clique (winner 1). Returns (list ascending, winner, heuristic_size = b)."""
    if adj.shape[0] == 0 or not adj.any():
        return [], 0, 0
    core = mm.core_numbers(adj) if core is None else core
    heu = mm.heu(adj, core) if heu is None else heu
    q0, s, _, _ = _incumbent(adj, core, S)
    b = max(s, len(heu))
    if len(unseeded) > b:
        return sorted(unseeded), 0, b
    if s >= 2 and s >= len(heu):
        return q0, 2, b
    return sorted(unseeded), 1, b
