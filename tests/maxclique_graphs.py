"""A table of structured graphs for the maximum-clique kernels (k_maxclique.hip.h).

Plain numpy, deterministic. Every entry carries answers DERIVED BY HAND FROM THE CONSTRUCTION, never from a model:
the edge count, every core number and the clique number omega; `why` says in one line where they come from.
tests/test_maxclique_graphs_cpu.py checks them against the sequential model and networkx, the GPU tests check the
kernels against them.

  kind "word"   m <= 193: vertex m - 1 on bit 63 of the last word or on bit 0 of a new one, cliques across word edges
  kind "peel"   the core peel's edges: the frontier capacity MC_PEEL_FCAP = 2048, long cascades, a jump of the level k
  kind "large"  m = 40 000: rows of more than 64 words, overflowing frontiers and a cut peel launch at once

Rules used in the derivations:
  * a vertex of a graph of minimum degree d has core number >= d, and core(v) <= deg(v);
  * core(v) >= k + 1 needs k + 1 neighbours of core >= k + 1, so a vertex whose other neighbours all have a smaller
    core than its clique's keeps the clique's core (ring neighbours of core 2 never raise a planted clique);
  * a vertex of a clique K_t with j extra edges into a part of core >= t - 1 + j has core exactly t - 1 + j = deg(v).
"""
from __future__ import annotations

import dataclasses
import itertools

import numpy as np

FCAP = 2048          # MC_PEEL_FCAP (k_maxclique.hip.h)
PEEL_BUDGET = 1 << 24  # MC_PEEL_BUDGET (host_maxclique.hpp): row-word operations per peel launch
WAVE_BUDGET = 1 << 18  # MC_WAVE_BUDGET (host_maxclique.hpp)
WORD_SIZES = (1, 2, 63, 64, 65, 127, 128, 129)


@dataclasses.dataclass(frozen=True)
class Graph:
    name: str
    m: int
    edge_list: np.ndarray      # (E, 2) int64, i < j, sorted by (j, i), no repeats
    edges: int                 # by hand
    core: np.ndarray           # by hand, int32, one per vertex
    omega: int                 # by hand (an edgeless graph: 1; the methods HEU and EXACT then return [])
    why: str
    kind: str = "word"
    heu_below_omega: bool = False   # the greedy clique is smaller than omega: EXACT has to search
    ties: bool = False              # several maximum cliques whose minimum-pos vertices differ
    enumerable: bool = True         # few maximal cliques by construction: a brute force over them is cheap
    exact: tuple | None = None      # the list EXACT must return where the construction alone gives it
    kcore: tuple | None = None      # KCORE's list where the table states it (else: the vertices of maximum core)
    budget: int = 1                 # the smallest budget of the launch-cut test (raised where budget 1 is slow)

    def adj(self) -> np.ndarray:
        a = np.zeros((self.m, self.m), dtype=bool)
        if len(self.edge_list):
            a[self.edge_list[:, 0], self.edge_list[:, 1]] = True
        return a | a.T

    def C(self) -> np.ndarray:
        """the dense 0/1 constraint matrix with unit diagonal"""
        return self.adj().astype(np.float64) + np.eye(self.m)

    def csc(self):
        """strict-upper CSC (colptr int64, rows int32, values float64) for set_sparse_matrix_data"""
        e = self.edge_list
        colptr = np.zeros(self.m + 1, dtype=np.int64)
        if len(e):
            np.add.at(colptr, e[:, 1] + 1, 1)
        return np.cumsum(colptr), e[:, 0].astype(np.int32), np.ones(len(e), dtype=np.float64)

    def degrees(self) -> np.ndarray:
        d = np.zeros(self.m, dtype=np.int64)
        if len(self.edge_list):
            np.add.at(d, self.edge_list[:, 0], 1)
            np.add.at(d, self.edge_list[:, 1], 1)
        return d

    def kcore_list(self) -> list[int]:
        return list(self.kcore) if self.kcore is not None else np.flatnonzero(self.core == self.core.max()).tolist()


# ---- edge sets --------------------------------------------------------------------------------------------------

def _ring(m):
    return {(min(i, (i + 1) % m), max(i, (i + 1) % m)) for i in range(m)}


def _path(m):
    return {(i, i + 1) for i in range(m - 1)}


def _clique(vs):
    return {(min(a, b), max(a, b)) for a, b in itertools.combinations(vs, 2)}


def _biclique(A, B):
    return {(min(a, b), max(a, b)) for a in A for b in B}


def _multipartite(parts):
    e = set()
    for P, Q in itertools.combinations(parts, 2):
        e |= _biclique(P, Q)
    return e


def _edges(pairs) -> np.ndarray:
    if not pairs:
        return np.zeros((0, 2), dtype=np.int64)
    e = np.array(sorted(pairs, key=lambda p: (p[1], p[0])), dtype=np.int64)
    assert np.all(e[:, 0] < e[:, 1])
    return e


def _ring_edge_array(m) -> np.ndarray:
    i = np.arange(m - 1, dtype=np.int64)
    e = np.stack([i, i + 1], axis=1)
    return np.concatenate([e, np.array([[0, m - 1]], dtype=np.int64)])


def _sorted_edges(e: np.ndarray) -> np.ndarray:
    return e[np.lexsort((e[:, 0], e[:, 1]))]


def _const(m, c):
    return np.full(m, c, dtype=np.int32)


def _cores(m, default, groups):
    c = np.full(m, default, dtype=np.int32)
    for vs, k in groups:
        c[list(vs)] = k
    return c


# ---- the table ---------------------------------------------------------------------------------------------------

def _word_graphs() -> list[Graph]:
    table = []

    def add(name, m, pairs, edges, core, omega, why, **kw):
        table.append(Graph(name, m, _edges(pairs), edges, core, omega, why, **kw))

    add("single_vertex", 1, set(), 0, _const(1, 0), 1, "m = 1: the path, star and ring of one vertex; no edge")
    add("edge_2", 2, {(0, 1)}, 1, _const(2, 1), 2, "m = 2: the path, star and K_{1,1}: one edge")
    add("cocktail_2", 2, set(), 0, _const(2, 0), 1, "K_2 minus its perfect matching: two isolated vertices")
    for m in (63, 64, 65, 127, 128, 129):
        add(f"ring_{m}", m, _ring(m), m, _const(m, 2), 2, "C_m, m > 3: m edges, 2-regular, triangle-free")
        add(f"path_{m}", m, _path(m), m - 1, _const(m, 1), 2, "a tree: m - 1 edges, every core 1, no triangle")
        hub = m - 1 if m % 64 in (0, 1) else 0  # the hub on the last bit where that bit is a word edge
        add(f"star_{m}", m, {(min(hub, v), max(hub, v)) for v in range(m) if v != hub}, m - 1, _const(m, 1), 2,
            "a tree with one hub: m - 1 edges, every core 1 (the leaves bound the hub's), no triangle")
    for a, b in ((32, 32), (32, 33), (63, 64), (64, 65)):
        m = a + b
        add(f"biclique_{a}_{b}", m, _biclique(range(a), range(a, m)), a * b, _const(m, a), 2,
            "K_{a,b}, a <= b, parts contiguous: ab edges; minimum degree a, and the b-side has degree a: every core a")
    add("cocktail_64", 64, _clique(range(64)) - {(i, i + 1) for i in range(0, 64, 2)}, 64 * 62 // 2, _const(64, 62), 32,
        "K_64 minus the matching (2i, 2i + 1): 62-regular, one vertex of every pair: omega 32 (2^32 maximum cliques)",
        enumerable=False)
    add("cocktail_128", 128, _clique(range(128)) - {(i, i + 64) for i in range(64)}, 128 * 126 // 2, _const(128, 126), 64,
        "K_128 minus the matching (i, i + 64), pairs across the word edge: 126-regular, omega 64", enumerable=False)
    # complete t-partite: the core is the minimum degree m - (largest part) for every vertex (a vertex of a smaller part
    # needs every vertex outside its part, the largest part's among them); omega = t; edges = (m^2 - sum of squares) / 2
    for m, t, inter in ((63, 7, True), (65, 4, True), (129, 5, True), (64, 4, False), (127, 3, False), (128, 8, False)):
        if inter:
            parts = [list(range(p, m, t)) for p in range(t)]
        else:
            cut = [round(i * m / t) for i in range(t + 1)]
            parts = [list(range(cut[i], cut[i + 1])) for i in range(t)]
        sizes = [len(p) for p in parts]
        add(f"partite_{m}_{t}_{'interleaved' if inter else 'contiguous'}", m, _multipartite(parts),
            (m * m - sum(s * s for s in sizes)) // 2, _const(m, m - max(sizes)), t,
            "complete t-partite: every core m - (largest part), omega t" + (", vertex i in part i mod t" if inter else ""),
            enumerable=False)
    add("moon_moser_63", 63, _multipartite([list(range(p, 63, 21)) for p in range(21)]), (63 * 63 - 21 * 9) // 2,
        _const(63, 60), 21, "K_{3 x 21}, vertex i in part i mod 21: 60-regular, omega 21, 3^21 maximum cliques",
        enumerable=False)
    add("moon_moser_129", 129, _multipartite([list(range(3 * p, 3 * p + 3)) for p in range(43)]), (129 * 129 - 43 * 9) // 2,
        _const(129, 126), 43, "K_{3 x 43}, contiguous triples: 126-regular, omega 43, 3^43 maximum cliques", enumerable=False)
    for m, s in ((63, 3), (64, 8), (65, 5), (128, 8), (129, 3)):
        t = m // s
        pairs = set()
        for c in range(t):
            pairs |= _clique(range(c * s, c * s + s))
        add(f"cliques_{t}x{s}", m, pairs, t * s * (s - 1) // 2, _const(m, s - 1), s,
            "t disjoint K_s: (s - 1)-regular, t maximum cliques; HEU's is the first (smallest seed), EXACT has nothing to add",
            ties=True, exact=tuple(range(s)))
    for m in (127, 128, 129):
        K = list(range(60, 68))
        add(f"ring_k8_{m}", m, _ring(m) | _clique(K), m + 28 - 7, _cores(m, 2, [(K, 7)]), 8,
            "C_m plus K_8 on 60..67 (7 of its 28 edges are the ring's): ring vertices degree 2; the K_8 across the word "
            "edge keeps core 7 (its other neighbours have core 2)", exact=tuple(K))
    K = [0, 63, 64, 127, 128]
    add("ring_k5_word_edges_129", 129, _ring(129) | _clique(K), 129 + 10 - 3, _cores(129, 2, [(K, 4)]), 5,
        "C_129 plus a clique on {0, 63, 64, 127, 128 = m - 1}: the ring already holds 63-64, 127-128 and 128-0", exact=tuple(K))
    K = [0, 63, 64, 127, 128, 192]
    add("ring_k6_word_edges_193", 193, _ring(193) | _clique(K), 193 + 15 - 3, _cores(193, 2, [(K, 5)]), 6,
        "C_193 plus K_6 on {0, 63, 64, 127, 128, m - 1 = 192}: the ring already holds 63-64, 127-128 and 192-0",
        exact=tuple(K))
    add("edgeless_k51", 100, _clique(range(49, 100)), 51 * 50 // 2, _cores(100, 0, [(range(49, 100), 50)]), 51,
        "49 isolated vertices and a K_51: the peel's level jumps from 0 to 50 in one step", exact=tuple(range(49, 100)))

    # ---- HEU below omega: a decoy of high core and small clique number draws every greedy pick away ----------------
    # Every vertex a of the clique part T has one (or two) neighbours in the decoy, of larger core than T's: the greedy
    # clique of seed a takes that neighbour first and is left with nothing; a decoy seed stays inside the decoy.
    X, Y = list(range(0, 8)), list(range(8, 24))
    T6 = list(range(61, 67))
    add("decoy_k6_100", 100, _multipartite([X, Y[:8], Y[8:]]) | _clique(T6) | {(i, 61 + i) for i in range(6)},
        192 + 15 + 6, _cores(100, 0, [(range(24), 16), (T6, 6)]), 6,
        "K_{8,8,8} on 0..23 (core 16, omega 3), K_6 on 61..66 across the word edge, 61 + i joined to i: degree 6 with "
        "every neighbour of core >= 6, so core 6; the rest isolated. HEU finds a triangle of the decoy",
        heu_below_omega=True, exact=tuple(T6))
    X, Y = list(range(40, 52)), list(range(52, 64))
    T1, T2 = list(range(0, 5)), list(range(124, 129))
    add("decoy_two_k5_129", 129,
        _biclique(X, Y) | _clique(T1) | _clique(T2) | {(i, 40 + 2 * i) for i in range(5)} | {(i, 41 + 2 * i) for i in range(5)}
        | {(52 + i, 124 + i) for i in range(5)},
        144 + 10 + 10 + 10 + 5, _cores(129, 0, [(X + Y, 12), (T1, 6), (T2, 5)]), 5,
        "K_{12,12} on 40..63 (core 12, omega 2); K_5 on 0..4, each with two decoy neighbours (core 6); K_5 on 124..128, "
        "each with one (core 5): two maximum cliques, and the one of LARGER indices has the smaller (core, degree): "
        "its vertex 124 is the first root in pos order that holds a maximum clique",
        heu_below_omega=True, ties=True, exact=tuple(T2))
    X, Y = list(range(0, 12)), list(range(12, 24))
    T = list(range(60, 68))
    add("decoy_k2222_70", 70, _biclique(X, Y) | _multipartite([[60 + p, 64 + p] for p in range(4)]) | {(i, 60 + i) for i in range(8)},
        144 + 24 + 8, _cores(70, 0, [(X + Y, 12), (T, 7)]), 4,
        "K_{12,12} on 0..23; K_{2,2,2,2} on 60..67 (parts {60 + p, 64 + p}, 6-regular, 16 maximum cliques), 60 + i joined "
        "to i: degree 7, core 7. Eight maximum cliques start at vertex 60, eight at 64",
        heu_below_omega=True, ties=True)
    X, Y = list(range(100, 112)), list(range(112, 124))
    T = list(range(58, 70))
    add("decoy_k3333_129", 129,
        _biclique(X, Y) | _multipartite([list(range(58 + p, 70, 4)) for p in range(4)]) | {(58 + i, 100 + i) for i in range(12)},
        144 + 54 + 12, _cores(129, 0, [(X + Y, 12), (T, 10)]), 4,
        "K_{12,12} on 100..123; Moon-Moser K_{3,3,3,3} on 58..69 (part i mod 4, 9-regular, 81 maximum cliques) across the "
        "word edge, 58 + i joined to 100 + i: degree 10, core 10",
        heu_below_omega=True, ties=True)
    return table


def _peel_graphs() -> list[Graph]:
    T = []
    for m in (2047, 2048, 2049, 4100):
        T.append(Graph(f"ring_{m}", m, _sorted_edges(_ring_edge_array(m)), m, _const(m, 2), 2,
                       "C_m: the round at k = 2 finds all m vertices at once: a frontier of m against a capacity of 2048",
                       kind="peel"))
    i = np.arange(1999, dtype=np.int64)
    T.append(Graph("path_2000", 2000, np.stack([i, i + 1], axis=1), 1999, _const(2000, 1), 2,
                   "a path: every round at k = 1 peels the two end vertices: 1000 rounds", kind="peel"))
    return T


LARGE_M = 40000
LARGE_K5 = (64, 4159, 8191, 20480, 39999)
LARGE_K66 = tuple(3000 * i + 100 for i in range(12))


def large_graph() -> Graph:
    """m = 40 000: a ring, a K_5 on five pairwise non-adjacent ring vertices and a K_{6,6} (even i against odd i) on
    twelve more, spread over the whole index range. Ring-only vertices: degree 2, core 2. K_5 vertices: degree 6, core 4
    (their ring neighbours have core 2). K_{6,6} vertices: degree 8, core 6. omega = 5 = the K_5, which HEU finds (the
    seeds of core 6 give an edge, the first seed of core 4 the K_5). HEU (5) < max_core + 1 (7): EXACT runs over the
    twelve roots of core >= 5, whose rows span 625 words, and must return the K_5."""
    m = LARGE_M
    A, B = LARGE_K66[0::2], LARGE_K66[1::2]
    extra = _edges(_clique(LARGE_K5) | _biclique(A, B))
    e = _sorted_edges(np.concatenate([_ring_edge_array(m), extra]))
    core = _cores(m, 2, [(LARGE_K5, 4), (LARGE_K66, 6)])
    return Graph("ring_k5_k66_40000", m, e, m + 10 + 36, core, 5, large_graph.__doc__, kind="large",
                 exact=tuple(sorted(LARGE_K5)), kcore=tuple(sorted(LARGE_K66)))


WORD_GRAPHS = _word_graphs()
PEEL_GRAPHS = _peel_graphs()
SMALL = {g.name: g for g in WORD_GRAPHS}
PEEL = {g.name: g for g in PEEL_GRAPHS}
assert len(SMALL) == len(WORD_GRAPHS) and len(PEEL) == len(PEEL_GRAPHS)
HEU_BELOW_OMEGA = [g.name for g in WORD_GRAPHS if g.heu_below_omega]
TIES = [g.name for g in WORD_GRAPHS if g.ties]
