"""Handed-over matrices at fp32's value edges (tests/test_value_edges_cpu.py, tests/test_gpu_value_edges.py): what a
storage must hold of a caller's double, a ladder of values around FLT_MIN, the subnormals, the values that round to fp32
zero and FLT_MAX, and named cases that carry the ladder on the rows and columns where the slices' geometry changes.

THE STORED-VALUE RULE (store_value in k_affinity.hip.h): C == pattern(M) is implicit in every
store, so a storage never lets a non-zero value become 0.
  fp64 storages hold v.
  fp32 storages hold float64(float32(v)) — a value whose fp32 rounding is subnormal stays that subnormal — except where
  that is 0 and v != 0: then copysign(FLT_MIN, v).
held() below is that rule in numpy; every setter is a single cast, so the GPU test compares with np.array_equal.

The cases behave like degenerate_cases.Case (dense(), upper_csc()). "edges-m" at m in (65, 129, 300) — one slice + 1, two
words + 1, several chunks — holds
  * the ladder on rows and columns 0, 63, 64, 127, 128, m - 1 (where they exist): every pair among them, and each rung
    once more between one of them and a row in between;
  * ZERO_COLUMN: a column whose every entry rounds to fp32 zero, and BLOCK_COLUMN, whose entries in rows 0..63 all do
    (it has ordinary entries below): were the pattern lost, a group or a slice would come out empty;
  * an ordinary sparse background, density about 0.1, values in [0.1, 1).
"edges-m-explicitC" is the same M with a C that holds one pair M does not and lacks one pair of M.

"tinyedge" is the one case that is solved: a clique of ordinary weights in which one member's edges to half of the
others are 1e-50, over a sparse background, u0 > 0. With C == pattern(M) the reference allows that member next to
all of the clique (with about zero affinity to half of it); were its tiny entries lost, it would be forbidden next to
half of the clique. TINYEDGE (sizes and seed) was picked on the CPU — tests/test_value_edges_cpu.py shows that the
oracle selects different node sets for M and for M without the underflowed entries, neither on a tie."""
from __future__ import annotations

import numpy as np

from tests import degenerate_cases as dc

STORE_F32, STORE_F64, STORE_F32_CSC, STORE_F64_CSC = 0, 1, 2, 3     # clipper_amd._abi's (checked by the GPU test)
F64S = (STORE_F64, STORE_F64_CSC)
FLT_MIN = 2.0 ** -126
FLT_MAX = (2.0 - 2.0 ** -23) * 2.0 ** 127
FLT_TRUE_MIN = 2.0 ** -149


def held(v, storage):
    """the value(s) `storage` must hold for the caller's v (float64 array or scalar)"""
    v = np.asarray(v, dtype=np.float64)
    if storage in F64S:
        return v.copy()
    with np.errstate(over="ignore", under="ignore"):
        r = v.astype(np.float32).astype(np.float64)
    return np.where((r == 0.0) & (v != 0.0), np.copysign(FLT_MIN, v), r)


def value_class(v):
    """by the fp32 rounding of v: 'normal', 'subnormal', 'zero' (v != 0 rounds to 0), 'top' (at or above FLT_MAX, finite)"""
    with np.errstate(over="ignore", under="ignore"):
        r = abs(float(np.float32(v)))
    assert v != 0.0 and np.isfinite(r), v
    if r == 0.0:
        return "zero"
    if r < FLT_MIN:
        return "subnormal"
    return "top" if r >= FLT_MAX else "normal"


# name -> value; the negative counterparts of a few rungs at the end
LADDER = {
    "0.1": 0.1, "0.37": 0.37, "0.9": 0.9, "1": 1.0, "2.5": 2.5,
    "FLT_MIN": FLT_MIN, "FLT_MIN(1-2^-25)": FLT_MIN * (1.0 - 2.0 ** -25), "1e-40": 1e-40, "2^-149": FLT_TRUE_MIN,
    "2^-150": 2.0 ** -150, "2^-150(1+2^-52)": 2.0 ** -150 * (1.0 + 2.0 ** -52),
    "1e-50": 1e-50, "1e-300": 1e-300, "5e-324": 5e-324,
    "FLT_MAX": FLT_MAX, "FLT_MAX(1+2^-25)": FLT_MAX * (1.0 + 2.0 ** -25),
    "-0.37": -0.37, "-FLT_MIN": -FLT_MIN, "-1e-40": -1e-40, "-2^-150": -(2.0 ** -150), "-1e-50": -1e-50, "-5e-324": -5e-324,
    "-FLT_MAX": -FLT_MAX,
}
TO_ZERO = [v for v in LADDER.values() if value_class(v) == "zero"]      # six of them, two negative

SIZES = (65, 129, 300)
EDGE_LINES = (0, 63, 64, 127, 128)      # and m - 1
ZERO_COLUMN, BLOCK_COLUMN = 17, 40      # (neither an edge line)


def edge_lines(m):
    return sorted({p for p in EDGE_LINES + (m - 1,) if p < m})


def _edges(m, seed=21):
    """the strict-upper entries of "edges-m" as {(i, j): v}, the positions of the ladder's rungs, an absent pair"""
    rng = np.random.default_rng(seed + m)
    bi, bj, bv = dc._weights(rng, m, 0.1, 0.1, 1.0)
    E = {(int(i), int(j)): float(v) for i, j, v in zip(bi, bj, bv)}
    special = (ZERO_COLUMN, BLOCK_COLUMN)
    P = edge_lines(m)
    rungs = list(LADDER.items())
    at = {}
    # every pair among the edge lines: the rungs in turn, starting with those that round to zero
    order = sorted(range(len(rungs)), key=lambda k: value_class(rungs[k][1]) != "zero")
    pairs = [(a, b) for x, a in enumerate(P) for b in P[x + 1:]]
    for n, pos in enumerate(pairs):
        name, v = rungs[order[n % len(rungs)]]
        E[pos] = v
        at.setdefault(name, []).append(pos)
    # each rung once more: one edge line, and a row or column off the lines
    taken = set(pairs)
    for k, (name, v) in enumerate(rungs):
        a = P[k % len(P)]
        b = (a + 2 + 5 * k) % m
        while b in P or b in special or tuple(sorted((a, b))) in taken:
            b = (b + 1) % m
        pos = tuple(sorted((a, b)))
        taken.add(pos)
        E[pos] = v
        at.setdefault(name, []).append(pos)
    # ZERO_COLUMN: nothing but values that round to fp32 zero; BLOCK_COLUMN: the same in rows 0..63, ordinary below
    for pos in [p for p in E if ZERO_COLUMN in p or (BLOCK_COLUMN in p and min(p) < 64 and max(p) < 64)]:
        assert pos not in taken
        del E[pos]
    for n, r in enumerate(range(1, m, 9)):
        if r != ZERO_COLUMN and r not in P:
            E[tuple(sorted((r, ZERO_COLUMN)))] = TO_ZERO[n % len(TO_ZERO)]
    for n, r in enumerate(range(2, 64, 7)):
        if r not in special and r not in P:
            E[tuple(sorted((r, BLOCK_COLUMN)))] = TO_ZERO[(n + 1) % len(TO_ZERO)]
    E[(BLOCK_COLUMN, 64)] = 0.625
    absent = next((i, j) for j in range(m - 2, 0, -1) for i in range(j - 1, -1, -1)
                  if (i, j) not in E and not {i, j} & set(special))
    return E, at, absent


def _case(name, m, E, C_pairs=None):
    keys = sorted(E, key=lambda p: (p[1], p[0]))
    Mi, Mj = (np.array([p[k] for p in keys], np.int64) for k in (0, 1))
    Mv = np.array([E[p] for p in keys], np.float64)
    if C_pairs is None:
        Ci, Cj = Mi, Mj
    else:
        ck = sorted(C_pairs, key=lambda p: (p[1], p[0]))
        Ci, Cj = (np.array([p[k] for p in ck], np.int64) for k in (0, 1))
    return dc.Case(name, "edges", m, dc._u0(31 + m, m), Mi=Mi, Mj=Mj, Mv=Mv, Ci=Ci, Cj=Cj)


def edges(m):
    E, at, _ = _edges(m)
    c = _case(f"edges-{m}", m, E)
    c.rungs_at = at
    return c


def edges_explicit_c(m):
    """the same M; C = pattern(M) without one ordinary pair of M and with one pair M does not hold"""
    E, at, absent = _edges(m)
    dropped = next(p for p in sorted(E, key=lambda p: (p[1], p[0]))
                   if 0.1 <= E[p] < 1.0 and not set(p) & set(edge_lines(m)))
    c = _case(f"edges-{m}-explicitC", m, E, (set(E) - {dropped}) | {absent})
    c.rungs_at, c.c_only, c.m_only = at, absent, dropped
    return c


def cases():
    return [f(m) for m in SIZES for f in (edges, edges_explicit_c)]


def held_case(c, storage):
    """the case as `storage` holds it (the lists of C untouched: the pattern of the fp64 M, or the explicit C)"""
    import dataclasses
    return dataclasses.replace(c, name=f"{c.name}/held{storage}", Mv=held(c.Mv, storage))


def expected_matrices(c, storage):
    """(M, C) as get_affinity_matrix / get_constraint_matrix must return them: held values, unit diagonals"""
    M, C = c.dense()
    return held(M, storage), C


def probe_columns(c, limit=16):
    """the columns whose unit-vector products are checked: 0, 63, 64, m - 1, the two special columns, then those that
    hold most of the ladder's rungs"""
    cols = [p for p in (0, 63, 64, c.m - 1, ZERO_COLUMN, BLOCK_COLUMN) if p < c.m]
    count = {}
    for ps in c.rungs_at.values():
        for p in ps:
            for k in p:
                count[k] = count.get(k, 0) + 1
    for k in sorted(count, key=lambda k: (-count[k], k)):
        if k not in cols:
            cols.append(k)
    return cols[:limit]


# ---- the solve case ----------------------------------------------------------------------------------------------------

TINYEDGE = dict(m=120, clique=12, density=0.05, seed=7)     # picked on the CPU: test_value_edges_cpu.py


def tinyedge(m, clique, density, seed, drop_underflowed=False):
    """a clique of `clique` vertices with weights in [0.6, 1), scattered by a permutation; its first member's edges to
    half of the others are 1e-50; the other vertices a sparse background of weights in [0.1, 0.5) among themselves.
    drop_underflowed: the matrix an fp32 store without the stored-value rule would hold (those edges gone)."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(m)
    K, rest = np.sort(perm[:clique]), np.sort(perm[clique:])
    W = np.zeros((m, m))
    bi, bj, bv = dc._weights(rng, rest.size, density, 0.1, 0.5)
    W[rest[bi], rest[bj]] = bv
    W[np.ix_(K, K)] = 0.6 + 0.4 * rng.random((clique, clique))
    W = np.triu(W, 1)
    W = W + W.T
    w, others = K[0], K[1:]
    tiny = others[: others.size // 2]
    W[w, others[others.size // 2:]] = W[others[others.size // 2:], w] = 1.0     # (its other edges: the strongest)
    W[w, tiny] = W[tiny, w] = 0.0 if drop_underflowed else 1e-50
    u0 = dc._u0(seed + 5, m)
    c = dc._handed("tinyedge" + ("-dropped" if drop_underflowed else ""), "tinyedge", m, u0, W, groups=(K, tiny))
    return c
