"""Sequential CPU model of the maximum-clique methods, written from the specification alone.

The graph is a symmetric boolean adjacency matrix `adj` (numpy, m x m, zero diagonal): edge (i, j) when
C(i, j) != 0, i != j.

  core_numbers(adj)   Batagelj-Zaversnik core numbers (bucket peeling; a vectorised level peel for large m)
  kcore(adj)          ROBIN: every vertex whose core number is the maximum (ascending)
  heu(adj)            the greedy clique: every vertex seeds one, candidates N(v), repeatedly take the candidate of
                      largest core number (ties: smallest index) and intersect with its row; the largest clique
                      wins (ties: smallest seed); [] without an edge
  omega(adj)          the clique number, by a bitset branch and bound (greedy colouring bound, Python ints as bitsets)
  exact_clique(adj, core, deg, heu_list)
                      the list method EXACT returns: the tie rule of k_maxclique.hip.h's mc_exact, sequentially
  exact_clique_by_enumeration(adj, core, deg, heu_list, cliques)
                      the same list from the rule's graph-theoretic definition over an enumeration of the maximum cliques
  peel_launches(adj, budget)
                      the launches the core peel takes with a budget of `budget` row-word operations per launch
  is_clique(adj, S)
"""
from __future__ import annotations

import numpy as np


def adjacency_from_matrix(C: np.ndarray) -> np.ndarray:
    """The graph of a (dense, symmetric) constraint matrix: C != 0 off the diagonal."""
    a = np.asarray(C) != 0
    a = a | a.T
    np.fill_diagonal(a, False)
    return a


def core_numbers(adj: np.ndarray) -> np.ndarray:
    """Core numbers: bucket peeling up to m = 3000, the vectorised level peel above (the same numbers)."""
    return core_numbers_bucket(adj) if adj.shape[0] <= 3000 else core_numbers_levels(adj)


def core_numbers_levels(adj: np.ndarray) -> np.ndarray:
    """Level peel: at level k remove every vertex of degree <= k until none is left, then k = least degree."""
    m = adj.shape[0]
    deg = adj.sum(axis=1).astype(np.int64)
    alive = np.ones(m, dtype=bool)
    core = np.zeros(m, dtype=np.int32)
    k = 0
    while alive.any():
        f = np.flatnonzero(alive & (deg <= k))
        if f.size == 0:
            k = int(deg[alive].min())
            continue
        core[f] = k
        alive[f] = False
        deg -= adj[f].sum(axis=0, dtype=np.int64)
    return core


def core_numbers_bucket(adj: np.ndarray) -> np.ndarray:
    """Batagelj-Zaversnik: vertices in buckets by current degree, always peel from the lowest bucket."""
    m = adj.shape[0]
    nbrs = [np.flatnonzero(adj[v]) for v in range(m)]
    deg = np.array([len(n) for n in nbrs], dtype=np.int64)
    core = np.zeros(m, dtype=np.int64)
    if m == 0:
        return core.astype(np.int32)
    maxd = int(deg.max())
    buckets = [set() for _ in range(maxd + 1)]
    for v in range(m):
        buckets[deg[v]].add(v)
    removed = np.zeros(m, dtype=bool)
    d = 0
    for _ in range(m):
        d = max(0, d - 1)  # a peel lowers degrees by one at most
        while not buckets[d]:
            d += 1
        v = min(buckets[d])  # (any choice gives the same core numbers)
        buckets[d].remove(v)
        removed[v] = True
        core[v] = d
        for u in nbrs[v]:
            if not removed[u] and deg[u] > d:
                buckets[deg[u]].remove(u)
                deg[u] -= 1
                buckets[deg[u]].add(u)
    return core.astype(np.int32)


def kcore(adj: np.ndarray, core: np.ndarray | None = None) -> list[int]:
    if adj.shape[0] == 0:
        return []
    core = core_numbers(adj) if core is None else core
    return np.flatnonzero(core == core.max()).tolist()


def greedy_clique(adj: np.ndarray, core: np.ndarray, v: int, thr: int = 0) -> list[int]:
    """The greedy clique of seed v (candidates with core + 1 < thr dropped; thr = 0: none), in pick order."""
    m = adj.shape[0]
    key = core.astype(np.int64) * (m + 1) + (m - np.arange(m))  # largest core, then smallest index
    cand = np.flatnonzero(adj[v] & (core.astype(np.int64) + 1 >= thr))
    out = [v]
    while cand.size:
        u = int(cand[np.argmax(key[cand])])
        out.append(u)
        cand = cand[adj[u, cand]]
    return out


def heu(adj: np.ndarray, core: np.ndarray | None = None) -> list[int]:
    """The HEU rule. Seeds are visited by core descending with the running best as the candidate threshold: a
    pruning that changes no seed able to reach the best size (picks come in non-increasing core order), so the
    result is the plain rule's: largest clique, smallest seed."""
    m = adj.shape[0]
    if m == 0 or not adj.any():
        return []
    core = core_numbers(adj) if core is None else core
    best, best_seed = 0, -1
    for v in sorted(range(m), key=lambda x: (-int(core[x]), x)):
        if core[v] + 1 < best:
            break
        size = len(greedy_clique(adj, core, v, best))
        if size > best or (size == best and v < best_seed):
            best, best_seed = size, v
    return sorted(greedy_clique(adj, core, best_seed))


def heu_plain(adj: np.ndarray) -> list[int]:
    """The HEU rule without any pruning (for the model's own tests)."""
    m = adj.shape[0]
    if m == 0 or not adj.any():
        return []
    core = core_numbers(adj)
    best = max(((len(greedy_clique(adj, core, v)), -v) for v in range(m)))
    return sorted(greedy_clique(adj, core, -best[1]))


def _bits(adj: np.ndarray) -> list[int]:
    m = adj.shape[0]
    rows = []
    for v in range(m):
        packed = np.packbits(adj[v], bitorder="little")
        rows.append(int.from_bytes(packed.tobytes(), "little"))
    return rows


def omega(adj: np.ndarray, lower: int | None = None) -> int:
    """The clique number: for every vertex r (core ascending), the cliques of r and its later neighbours, branch and
    bound with the greedy colouring bound (Tomita's MCQ over bitsets)."""
    m = adj.shape[0]
    if m == 0:
        return 0
    if not adj.any():
        return 1
    core = core_numbers(adj)
    G = _bits(adj)
    best = max(lower or 0, len(heu(adj, core)))
    if best == int(core.max()) + 1:
        return best
    order = sorted(range(m), key=lambda x: (int(core[x]), x))
    later = 0
    for r in reversed(order):
        if core[r] + 1 > best:
            P = G[r] & later
            best = max(best, 1 + _expand(G, P, 0, best - 1))
        later |= 1 << r
    return best


def _colour(G: list[int], P: int):
    """Greedy sequential colouring of P in index order: (vertices, colours), colours non-decreasing."""
    vs, cs = [], []
    Q, k = P, 0
    while Q:
        k += 1
        R = Q
        while R:
            v = (R & -R).bit_length() - 1
            R &= ~G[v] & ~(1 << v)
            Q &= ~(1 << v)
            vs.append(v)
            cs.append(k)
    return vs, cs


def _expand(G: list[int], P: int, size: int, best: int) -> int:
    """Largest clique size (at least `best` + 1, else `best`) of the vertices of P, on top of `size` taken ones."""
    vs, cs = _colour(G, P)
    for i in range(len(vs) - 1, -1, -1):
        if size + cs[i] <= best:
            return best
        v = vs[i]
        NP = P & G[v]
        if NP == 0:
            best = max(best, size + 1)
        else:
            best = max(best, _expand(G, NP, size + 1, best))
        P &= ~(1 << v)
    return best


def root_positions(core, deg) -> np.ndarray:
    """pos[v]: v's place in the order by (core, degree, index) (host_mcplan.hpp root_order)"""
    m = len(core)
    order = sorted(range(m), key=lambda v: (int(core[v]), int(deg[v]), v))
    pos = np.zeros(m, dtype=np.int64)
    pos[order] = np.arange(m)
    return pos


def _root_candidates(G, core, pos, r, h) -> int:
    """P_0 of root r: its neighbours of larger pos and of core >= h, as a bitset"""
    P, bits = 0, G[r]
    while bits:
        x = (bits & -bits).bit_length() - 1
        bits &= bits - 1
        if pos[x] > pos[r] and core[x] >= h:
            P |= 1 << x
    return P


def exact_clique(adj: np.ndarray, core, deg, heu_list, omega_known: int | None = None) -> list[int]:
    """The list method EXACT returns (ascending), from the comment above mc_exact and root_order, sequentially.

    If no clique beats HEU's, HEU's. Else the roots are visited in pos order (pos: the order by (core, degree,
    index)); root r searches the cliques {r} + K with K inside P_0 = the neighbours x of r with pos[x] > pos[r] and
    core[x] >= |HEU|. A level holds the candidates P_L of the clique {r, path}: it is coloured (classes one after the
    other; in a class, repeatedly the lowest-index vertex of R is taken, its neighbours leave R, and it leaves R and
    Q), the LAST vertex coloured is branched on and leaves P_L, P_{L+1} = P_L & N(v), depth first; the level is coloured
    again whenever the search returns to it. The first leaf of omega vertices, in the first root that has one, is the
    answer; a graph without an edge has none ([]). A level whose bound (clique so far + colours) is below omega holds no such leaf and is left at once: the
    only pruning the model does, with the known omega (the kernel prunes against its incumbent, which never cuts a
    branch whose bound reaches omega before the root's own first maximum clique is found)."""
    if not adj.any():
        return []  # (no edge: every method returns no vertex)
    h = len(heu_list)
    w = omega(adj, lower=h) if omega_known is None else omega_known
    if w <= h:
        return sorted(int(v) for v in heu_list)
    G = _bits(adj)
    pos = root_positions(core, deg)

    def search(P, path):
        while True:
            vs, cs = _colour(G, P)
            if not vs or len(path) + cs[-1] < w:
                return None
            v = vs[-1]
            P &= ~(1 << v)
            NP = P & G[v]
            if NP == 0:
                if len(path) + 1 == w:
                    return path + [v]
            else:
                found = search(NP, path + [v])
                if found:
                    return found

    for r in sorted(range(adj.shape[0]), key=lambda v: pos[v]):
        if core[r] + 1 < w:
            continue
        found = search(_root_candidates(G, core, pos, r, h), [r])
        if found:
            return sorted(found)
    raise AssertionError("no root holds a clique of omega vertices")


def exact_clique_by_enumeration(adj: np.ndarray, core, deg, heu_list, cliques) -> list[int]:
    """The same list from the graph-theoretic definition, over `cliques` = every maximum clique of the graph (an
    enumeration from elsewhere, e.g. networkx.find_cliques): no bound, no pruning. The winning root is the vertex of
    smallest pos that is the minimum-pos vertex of a maximum clique; below it the branch vertices of a level come in
    the order the repeated colouring gives them, and the first one that some remaining maximum clique contains is
    taken."""
    cliques = [frozenset(int(v) for v in c) for c in cliques]
    w = max(len(c) for c in cliques)
    if w <= len(heu_list):
        return sorted(int(v) for v in heu_list)
    cliques = [c for c in cliques if len(c) == w]
    G = _bits(adj)
    pos = root_positions(core, deg)
    r = min((min(c, key=lambda v: pos[v]) for c in cliques), key=lambda v: pos[v])
    left = [c for c in cliques if min(c, key=lambda v: pos[v]) == r]
    path, P = [r], _root_candidates(G, core, pos, r, len(heu_list))
    while len(path) < w:
        while True:
            vs, _ = _colour(G, P)
            v = vs[-1]  # (never empty: a clique of `left` is still inside path + P)
            P &= ~(1 << v)
            mine = [c for c in left if v in c]
            if mine:
                break
        left = mine
        path.append(v)
        P &= G[v]
    return sorted(path)


def peel_launches(adj: np.ndarray, budget: int, fcap: int = 2048) -> int:
    """The launches of the core peel (k_maxclique.hip.h mc_peel): a launch runs rounds until `budget` row-word
    operations are spent or every vertex is peeled; a round that peels n vertices costs n (nw + 1), nw = ceil(m / 64),
    a round that only raises the level costs nothing. Exact while no round finds more than `fcap` vertices."""
    m = adj.shape[0]
    nw = (m + 63) // 64
    deg = adj.sum(axis=1).astype(np.int64)
    alive = np.ones(m, dtype=bool)
    k, removed, launches = 0, 0, 0
    while removed < m:
        launches += 1
        work = 0
        while removed < m and work < budget:
            f = np.flatnonzero(alive & (deg <= k))
            assert f.size <= fcap
            if f.size == 0:
                k = max(k, int(deg[alive].min()))
                continue
            alive[f] = False
            deg -= adj[f].sum(axis=0, dtype=np.int64)
            removed += f.size
            work += f.size * (nw + 1)
    return max(launches, 1)


def is_clique(adj: np.ndarray, S) -> bool:
    S = list(S)
    if len(set(S)) != len(S):
        return False
    sub = adj[np.ix_(S, S)]
    return bool(np.all(sub | np.eye(len(S), dtype=bool)))
