"""Degenerate graphs for the solver (tests/test_degenerate_cases_cpu.py, tests/test_gpu_degenerate.py): no edge, every
edge, every pair forbidden, disjoint cliques, stars, paths, and weights above 1 whose round(F) exceeds the number of
positive entries of u. Named cases with fixed seeds, in two families:

  * HANDED OVER: the symmetric (M, C) with unit diagonals for set_matrix_data, and the strict upper triangle of the
    same as CSC lists for set_sparse_matrix_data (Case.dense(), Case.upper_csc());
  * BUILT FROM POINTS: (D1, D2, A) for the Euclidean scorer at POINT_INV, so that the batch, the rectangular-fill row
    views and the live sub-problem can be reached:
      edgeless    every association is (i, 0): a shared endpoint gives M = C = 0 (clipper.cpp:35-38)
      complete    D2 = D1 bit for bit, A = (i, i): every score is exp(0) = 1
      two groups  D2 = D1 with 64.0 added to the second group's points, all on a grid of 2^-20: differences inside a
                  group are exact (score 1), across the groups |l1 - l2| > 60 (score 0)

Case.kind names the property the case is there for; the CPU test checks it on the oracle before any GPU test may ask for
equality:
  "edgeless"   random u0 > 0, no edge: one positive entry, one node, F = 1
  "complete"   M = 1 everywhere, random u0: all m nodes, F = m
  "uniform"    complete with M_off = 0.5 and u0 = 1 at dyadic 1 / sqrt(m): every sum is exact, every entry of u bit-equal,
               the selected nodes are the heap's tie rule alone
  "cliques"    two disjoint cliques and isolated vertices, random u0: the larger clique
  "cliques0"   the same with u0 zero on the larger clique: the smaller one
  "star", "path"   two nodes after hundreds of trials
  "tiefill"    weights in [2, 5], C = pattern(M): round(F) exceeds the number of positive entries of u, so
               findIndicesOfkLargest (utils.cpp:33-55) fills up with zero entries by its heap's tie rule
  "uzero"      weights in [0.5, 3], C = I (every pair forbidden): the iteration accepts an all-zero candidate, u == 0,
               F = 0, no node
  "ccomplete"  weights in [0.5, 3], C complete: no active constraint (clipper.cpp:203-204, 269-279), one outer iteration
  "emptyrows"  rows without an entry in front of an ordinary synthetic problem (points_embedded_empty_rows): the large
               point-built case on which views are built and the live sub-problem is entered — the purely degenerate
               point-built cases end within a few trials or hold no bytes a view could save
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

POINT_INV = dict(sigma=0.015, epsilon=0.05, mindist=0.0)
SMALL_M = (1, 2, 3, 64, 65, 129, 300)   # one vertex, one pair, a pad index, one slice, one slice + 1, two words + 1
LARGE_M = 3001                           # just above the row view's minimum size (RV_MIN_M = 3000)


@dataclass
class Case:
    name: str
    kind: str
    m: int
    u0: np.ndarray
    # handed over: strict upper triangle as coordinate lists sorted by (column, row); values of C are 1
    Mi: np.ndarray | None = None
    Mj: np.ndarray | None = None
    Mv: np.ndarray | None = None
    Ci: np.ndarray | None = None
    Cj: np.ndarray | None = None
    # built from points
    D1: np.ndarray | None = None
    D2: np.ndarray | None = None
    A: np.ndarray | None = None
    groups: tuple = field(default_factory=tuple)   # cliques / two groups: (larger, smaller) as index arrays

    @property
    def from_points(self) -> bool:
        return self.A is not None

    @property
    def explicit_c(self) -> bool:
        """C != pattern(M) off the diagonal"""
        return not (self.Mi.size == self.Ci.size and np.array_equal(self.Mi, self.Ci) and np.array_equal(self.Mj, self.Cj))

    def dense(self):
        """(M, C) symmetric with unit diagonals, as set_matrix_data takes them"""
        M, C = np.eye(self.m), np.eye(self.m)
        M[self.Mi, self.Mj] = self.Mv
        M[self.Mj, self.Mi] = self.Mv
        C[self.Ci, self.Cj] = 1.0
        C[self.Cj, self.Ci] = 1.0
        return M, C

    def upper_csc(self):
        """(m, Mcolptr, Mrow, Mval, Ccolptr, Crow, Cval) of the strict upper triangles, as set_sparse_matrix_data takes them"""
        def colptr(j):
            return np.concatenate([[0], np.cumsum(np.bincount(j, minlength=self.m))]).astype(np.int64)
        return (self.m, colptr(self.Mj), self.Mi.astype(np.int32), self.Mv.astype(np.float64),
                colptr(self.Cj), self.Ci.astype(np.int32), np.ones(self.Ci.size))

    def matvec(self, x):
        """(M_off x, C_off x) from the lists: what the solver's products are, without a dense matrix"""
        if getattr(self, "_ops", None) is None:
            import scipy.sparse as sp
            def sym(i, j, v):
                U = sp.csr_matrix((v, (i, j)), shape=(self.m, self.m))
                return (U + U.T).tocsr()
            self._ops = (sym(self.Mi, self.Mj, self.Mv), sym(self.Ci, self.Cj, np.ones(self.Ci.size)))
        return self._ops[0] @ x, self._ops[1] @ x

    def rounded_f32(self) -> "Case":
        """the matrix an fp32 storage holds of this case (value_edges.held: the cast, and a non-zero value never 0)"""
        import dataclasses
        from tests.value_edges import STORE_F32, held
        return dataclasses.replace(self, name=self.name + "/f32", Mv=held(self.Mv, STORE_F32))


def _lists(mask_or_values):
    """strict upper triangle of a dense array -> (i, j, v) sorted by (column, row)"""
    U = np.triu(mask_or_values, 1)
    j, i = np.nonzero(U.T)
    return i.astype(np.int64), j.astype(np.int64), U[i, j].astype(np.float64)


def _handed(name, kind, m, u0, W, Cmask=None, groups=()):
    Mi, Mj, Mv = _lists(W)
    if Cmask is None:
        Ci, Cj = Mi, Mj
    else:
        Ci, Cj, _ = _lists(Cmask)
    return Case(name, kind, m, np.asarray(u0, float), Mi=Mi, Mj=Mj, Mv=Mv, Ci=Ci, Cj=Cj, groups=groups)


def _u0(seed, m):
    return np.random.default_rng(seed).random(m) * 0.9 + 0.1     # > 0 everywhere


def edgeless(m, seed=1):
    return _handed(f"edgeless-{m}", "edgeless", m, _u0(seed + m, m), np.zeros((m, m)))


def complete_ones(m, seed=2):
    return _handed(f"complete-{m}", "complete", m, _u0(seed + m, m), np.ones((m, m)))


def complete_half_uniform(m):
    assert float(np.sqrt(m)) == int(np.sqrt(m)) and (int(np.sqrt(m)) & (int(np.sqrt(m)) - 1)) == 0, "1 / sqrt(m) must be dyadic"
    return _handed(f"uniform-{m}", "uniform", m, np.ones(m), np.full((m, m), 0.5))


def two_cliques(m, a, b, zero_on_larger=False, seed=3):
    """cliques of a > b vertices among m, scattered by a permutation; the rest isolated"""
    assert a > b and a + b <= m
    rng = np.random.default_rng(seed + m)
    perm = rng.permutation(m)
    big, small = np.sort(perm[:a]), np.sort(perm[a:a + b])
    W = np.zeros((m, m))
    W[np.ix_(big, big)] = 1.0
    W[np.ix_(small, small)] = 1.0
    u0 = _u0(seed + 7 * m, m)
    if zero_on_larger:
        u0[big] = 0.0
    kind = "cliques0" if zero_on_larger else "cliques"
    return _handed(f"{kind}-{m}", kind, m, u0, W, groups=(big, small))


def star(m=50, seed=11):
    """(the seed: one of the few whose oracle result does not move with the order of the additions — with most u0 the
    star takes thousands of trials to a single node, and their count rests on rounding)"""
    W = np.zeros((m, m))
    W[0, 1:] = 1.0
    return _handed(f"star-{m}", "star", m, _u0(seed + m, m), W)


def path(m, seed=5):
    i = np.arange(m - 1, dtype=np.int64)
    return Case(f"path-{m}", "path", m, _u0(seed + m, m), Mi=i, Mj=i + 1, Mv=np.ones(m - 1), Ci=i, Cj=i + 1)


def _weights(rng, m, density, lo, hi):
    """random strict-upper weights in [lo, hi) at the given density, as lists (no dense array: m may be large)"""
    n = int(round(density * m * (m - 1) / 2))
    code = np.unique(rng.integers(0, m, n * 2) * m + rng.integers(0, m, n * 2))
    i, j = code // m, code % m
    keep = i < j
    pick = rng.permutation(int(keep.sum()))[:n]
    i, j = i[keep][pick], j[keep][pick]
    order = np.lexsort((i, j))
    i, j = i[order], j[order]
    return i.astype(np.int64), j.astype(np.int64), lo + (hi - lo) * rng.random(i.size)


def weights_tiefill(m, density, seed=6):
    rng = np.random.default_rng(seed + m)
    i, j, v = _weights(rng, m, density, 2.0, 5.0)
    return Case(f"tiefill-{m}", "tiefill", m, _u0(seed + 3 * m, m), Mi=i, Mj=j, Mv=v, Ci=i, Cj=j)


def weights_c_identity(m, density=0.3, seed=7):
    rng = np.random.default_rng(seed + m)
    i, j, v = _weights(rng, m, density, 0.5, 3.0)
    e = np.zeros(0, np.int64)
    return Case(f"uzero-{m}", "uzero", m, _u0(seed + 3 * m, m), Mi=i, Mj=j, Mv=v, Ci=e, Cj=e)


def weights_c_complete(m, density=0.3, seed=8):
    rng = np.random.default_rng(seed + m)
    i, j, v = _weights(rng, m, density, 0.5, 3.0)
    Ci, Cj, _ = _lists(np.ones((m, m)))
    return Case(f"ccomplete-{m}", "ccomplete", m, _u0(seed + 3 * m, m), Mi=i, Mj=j, Mv=v, Ci=Ci, Cj=Cj)


# ---- built from points -------------------------------------------------------------------------------------------------

def _grid_points(rng, n):
    return np.ascontiguousarray((rng.integers(0, 1 << 20, (n, 3)) * 2.0 ** -20).T)     # 3 x n in [0, 1)


def points_edgeless(m, seed=11):
    rng = np.random.default_rng(seed + m)
    D1, D2 = _grid_points(rng, m), _grid_points(rng, 2)
    A = np.stack([np.arange(m), np.zeros(m, int)], axis=1).astype(np.int32)
    return Case(f"points-edgeless-{m}", "edgeless", m, _u0(seed + 3 * m, m), D1=D1, D2=D2, A=A)


def points_complete(m, seed=12):
    rng = np.random.default_rng(seed + m)
    D1 = _grid_points(rng, m)
    A = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.int32)
    return Case(f"points-complete-{m}", "complete", m, _u0(seed + 3 * m, m), D1=D1, D2=D1.copy(), A=A)


def points_two_groups(m, a=None, zero_on_larger=False, seed=13):
    """the first a associations one group, the other m - a < a the second"""
    a = (9 * m) // 16 + 1 if a is None else a
    assert a > m - a >= 1
    rng = np.random.default_rng(seed + m)
    D1 = _grid_points(rng, m)
    D2 = D1.copy()
    D2[:, a:] += 64.0
    A = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.int32)
    u0 = _u0(seed + 3 * m, m)
    if zero_on_larger:
        u0[:a] = 0.0
    kind = "cliques0" if zero_on_larger else "cliques"
    return Case(f"points-{kind}-{m}", kind, m, u0, D1=D1, D2=D2, A=A, groups=(np.arange(a), np.arange(a, m)))


def points_embedded_empty_rows(m_synth=5000, rho=0.9, seed=99, n_empty=601):
    """n_empty associations whose rows hold no entry at all, in front of a synthetic registration problem
    (clipper_amd.synth: the shape on which a solve builds row views and hands over to the live sub-problem): their
    points of the first set lie 64 away from the unit cube and they share one point of the second set, so they are
    inconsistent with each other (a shared endpoint) and with every other association (|l1 - l2| > 60). The first
    slices of the matrix hold no entry, the views' rows of these associations none, and u0 > 0 keeps them live at first."""
    from clipper_amd import synth
    s = synth.make_euclidean_problem(m_synth, rho, seed=seed)
    rng = np.random.default_rng(seed + 2)
    n1, n2 = s.D1.shape[1], s.D2.shape[1]
    far = 64.0 + _grid_points(rng, n_empty)
    D1, D2 = np.hstack([s.D1, far]), np.hstack([s.D2, np.full((3, 1), 0.5)])
    E = np.stack([n1 + np.arange(n_empty), np.full(n_empty, n2)], axis=1).astype(np.int32)
    m = n_empty + m_synth
    return Case(f"points-emptyrows-{m}", "emptyrows", m, np.concatenate([_u0(seed + 3, n_empty), s.u0]),
                D1=np.ascontiguousarray(D1), D2=np.ascontiguousarray(D2), A=np.vstack([E, s.A]).astype(np.int32),
                groups=(np.arange(n_empty),))


def expected_point_matrix(c: Case):
    """what the scorer must give on a point-built case, exactly: the strict-upper pattern (every kept score is 1)"""
    W = np.zeros((c.m, c.m))
    if c.kind == "complete":
        W[:] = 1.0
    elif c.kind in ("cliques", "cliques0"):
        for g in c.groups:
            W[np.ix_(g, g)] = 1.0
    return np.triu(W, 1)


# ---- the lists ---------------------------------------------------------------------------------------------------------

def small_handed():
    out = [edgeless(m) for m in SMALL_M] + [complete_ones(m) for m in SMALL_M]
    out += [complete_half_uniform(4), complete_half_uniform(64)]
    for m, a, b in ((40, 7, 5), (65, 30, 20), (130, 20, 19), (300, 70, 60)):
        out += [two_cliques(m, a, b), two_cliques(m, a, b, zero_on_larger=True)]
    out += [star(50), path(50)]
    out += [weights_tiefill(m, dens) for m, dens in ((65, 0.3), (80, 0.3), (129, 0.2), (200, 0.1), (300, 0.1))]
    out += [weights_c_identity(m) for m in (20, 65, 80, 129, 300)]
    out += [weights_c_complete(m) for m in (3, 65, 129)]
    return out


def small_points():
    out = [points_edgeless(m) for m in SMALL_M] + [points_complete(m) for m in SMALL_M]
    for m in SMALL_M[2:]:
        out += [points_two_groups(m), points_two_groups(m, zero_on_larger=True)]
    return out


def large_handed():
    return [edgeless(LARGE_M), path(LARGE_M), weights_tiefill(LARGE_M, 0.01)]


def large_points():
    return [points_edgeless(LARGE_M), points_two_groups(LARGE_M, a=1600), points_embedded_empty_rows()]


def by_name():
    return {c.name: c for c in small_handed() + small_points() + large_handed() + large_points()}


# ---- how a selected list may be compared -------------------------------------------------------------------------------

U_TOL = 1e-7   # the cap on max|u - u_oracle| the GPU tests use


def tied_entries(u, nodes):
    """True where the ORDER of the selected list rests on rounding: two positive selected entries of u within 2 U_TOL of
    each other (a u within U_TOL of this one may list them the other way round). The list is then compared as a set.
    Zero entries are exact zeros on every path (the projection's), and their order is the heap's tie rule."""
    v = np.sort(np.asarray(u)[np.asarray(nodes, dtype=int)])
    v = v[v > 0]
    return bool(v.size > 1 and np.min(np.diff(v)) <= 2 * U_TOL)


def boundary_gap(u, nodes):
    """smallest selected entry minus largest unselected one (inf where there is none, or where both are exact zeros):
    the selected SET is safe from rounding where this exceeds 2 U_TOL"""
    u = np.asarray(u)
    sel = np.zeros(u.size, bool)
    sel[np.asarray(nodes, dtype=int)] = True
    if sel.all() or not sel.any():
        return float("inf")
    lo, hi = float(u[sel].min()), float(u[~sel].max())
    return float("inf") if lo == 0.0 and hi == 0.0 else lo - hi
