"""The reference of a fill with a user-defined invariant, in plain numpy and fp64, shared by
tests/test_custom_invariant_model.py (no device) and tests/test_gpu_custom_invariant_edges.py (the device against it).

The contract, stated once:
  the pair rule   the formula is called on (i, j) with i < j, with ai = D1[:, A[i,0]], aj = D1[:, A[j,0]],
                  bi = D2[:, A[i,1]], bj = D2[:, A[j,1]]; not at all when the two associations share an index in either
                  column; M is symmetric and its diagonal is 0
  the keep rule   score > affinityeps (NaN is not), and C = pattern(M)
  the store rule  fp64 storages keep the score; fp32 storages keep float32(score), or FLT_MIN where that rounds to 0

Every formula is given twice: as device source and as a numpy function of whole arrays f(ai, aj, bi, bj, params) whose
data are (d, npairs) arrays. PLANT, ASYM and WIDE use + - * / sqrt fabs only: each is exactly rounded in IEEE
arithmetic, so with -ffp-contract=off the device must give numpy's bits. tests/test_custom_invariant_model.py holds the
scalar transcriptions the vectorised forms are checked against.
"""
import math

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)                            # 2^-126, the smallest normal
SUB_MAX = float(np.nextafter(np.float32(FLT_MIN), np.float32(0.0)))   # the largest fp32 subnormal
NPARAMS = 16

# ---- the formulas: device source -----------------------------------------------------------------------------------

# d = 2, datum = (label, x), all 16 params. Two associations whose first data carry the same label l >= 1 score
# params[l]; every other pair scores the generic value, asymmetric under i <-> j.
PLANT_SRC = r"""
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  const int l = static_cast<int>(ai[0]);
  if (ai[0] == aj[0] && l >= 1 && l <= 15) return params[l];
  return params[0] / (1.0 + sqrt(fabs((ai[1] - bj[1]) * (aj[1] + 0.25)))) - 0.3;
}
"""

# A formula the built-ins cannot express: asymmetric under i <-> j, uses params[0..3]
ASYM_SRC = r"""
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) s = s + (ai[k] - bj[k]) * (aj[k] + params[1]);
  const double t = sqrt(fabs(s) + params[2]);
  return params[0] / (1.0 + t) - params[3];
}
"""

# d = 16 and d = 32, all 16 params: every coordinate of the four data and every param enters a sum
WIDE_SRC = r"""
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s = 0.0, u = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) {
    s = s + (ai[k] - bj[k]) * (aj[k] + params[k % 16]);
    u = u + (bi[k] - aj[k]) * (bj[k] + params[(k + 5) % 16]);
  }
  const double t = sqrt((fabs(s) + fabs(u)) / CLIPPER_D);
  return 1.0 / (1.0 + t) - 0.72;
}
"""

# ---- the formulas: numpy, on (d, npairs) arrays --------------------------------------------------------------------


def plant_np(ai, aj, bi, bj, p):
    p = np.asarray(p, dtype=np.float64)
    lab = ai[0].astype(np.int64)
    same = (ai[0] == aj[0]) & (lab >= 1) & (lab <= 15)
    generic = p[0] / (1.0 + np.sqrt(np.abs((ai[1] - bj[1]) * (aj[1] + 0.25)))) - 0.3
    return np.where(same, p[np.clip(lab, 0, 15)], generic)


def asym_np(ai, aj, bi, bj, p):
    s = np.zeros(ai.shape[1])
    for k in range(ai.shape[0]):
        s = s + (ai[k] - bj[k]) * (aj[k] + p[1])
    t = np.sqrt(np.abs(s) + p[2])
    return p[0] / (1.0 + t) - p[3]


def asym_py(d, p):
    """ASYM_SRC transcribed for one pair at a time (plain Python floats: what a host PairwiseInvariant computes)"""
    def f(ai, aj, bi, bj):
        s = 0.0
        for k in range(d):
            s = s + (float(ai[k]) - float(bj[k])) * (float(aj[k]) + p[1])
        t = math.sqrt(abs(s) + p[2])
        return p[0] / (1.0 + t) - p[3]
    return f


def wide_np(ai, aj, bi, bj, p):
    d = ai.shape[0]
    s, u = np.zeros(ai.shape[1]), np.zeros(ai.shape[1])
    for k in range(d):
        s = s + (ai[k] - bj[k]) * (aj[k] + p[k % 16])
        u = u + (bi[k] - aj[k]) * (bj[k] + p[(k + 5) % 16])
    t = np.sqrt((np.abs(s) + np.abs(u)) / d)
    return 1.0 / (1.0 + t) - 0.72


def euclid_np(ai, aj, bi, bj, p):
    """EuclideanDistance (euclidean_distance.cpp:13-31); p = (sigma, epsilon, mindist). Ties the pair rule to the
    oracle; its exp is not exactly rounded, so it is compared to a few ulp, never to the device."""
    l1 = np.sqrt(((ai - aj) ** 2).sum(0))
    l2 = np.sqrt(((bi - bj) ** 2).sum(0))
    c = np.abs(l1 - l2)
    scr = np.where(c < p[1], np.exp(-0.5 * c * c / (p[0] * p[0])), 0.0)
    if p[2] > 0:
        scr = np.where((l1 < p[2]) | (l2 < p[2]), 0.0, scr)
    return scr


def pad_params(params):
    """the fill's 16 doubles: the ones given, the rest 0"""
    p = np.zeros(NPARAMS)
    q = np.asarray(params, dtype=np.float64).reshape(-1)
    p[: q.size] = q
    return p


# ---- the contract --------------------------------------------------------------------------------------------------


def distinct_pairs(A):
    """(i, j), i < j, of the pairs the formula is called on"""
    A = np.asarray(A)
    i, j = np.triu_indices(A.shape[0], 1)
    ok = (A[i, 0] != A[j, 0]) & (A[i, 1] != A[j, 1])
    return i[ok], j[ok]


def pair_data(D1, D2, A, i, j):
    A = np.asarray(A)
    return D1[:, A[i, 0]], D1[:, A[j, 0]], D2[:, A[i, 1]], D2[:, A[j, 1]]


def scores(formula, D1, D2, A, params):
    """(i, j, score) of every call"""
    D1, D2 = np.asarray(D1, dtype=np.float64), np.asarray(D2, dtype=np.float64)
    i, j = distinct_pairs(A)
    with np.errstate(invalid="ignore"):
        s = formula(*pair_data(D1, D2, A, i, j), pad_params(params))
    return i, j, np.asarray(s, dtype=np.float64)


def fill(formula, D1, D2, A, params, affinityeps):
    """M and C as an fp64 storage holds them"""
    m = np.asarray(A).shape[0]
    i, j, s = scores(formula, D1, D2, A, params)
    with np.errstate(invalid="ignore"):
        kept = s > affinityeps
    M = np.zeros((m, m))
    M[i[kept], j[kept]] = s[kept]
    M[j[kept], i[kept]] = s[kept]
    return M, (M != 0).astype(np.float64)


def store_f32(M):
    """M as an fp32 storage holds it (read back as doubles)"""
    with np.errstate(under="ignore"):
        v = M.astype(np.float32).astype(np.float64)
    v[(M != 0) & (v == 0)] = FLT_MIN
    return v


# ---- PLANT's data, parameter sets and kinds ------------------------------------------------------------------------

PLANT_KINDS = ("eps", "eps_up", "eps_down", "eps_half", "zero", "neg_zero", "minus_one", "nan", "1e-46", "2^-150",
               "1e-40", "flt_min", "sub_max", "one", "two")   # label l = 1 + index


def plant_values(e):
    """the 15 planted scores of a fill whose affinityeps is e"""
    return [e, float(np.nextafter(e, 1.0)), float(np.nextafter(e, 0.0)), e / 2, 0.0, -0.0, -1.0, math.nan,
            1e-46, 2.0 ** -150, 1e-40, FLT_MIN, SUB_MAX, 1.0, 2.0]


# (scale params[0] of the generic value, affinityeps). The generic value's offset 0.3 is a literal of the source, so
# the sparse set raises it relative to the scale: the pair survives iff sqrt(...) < scale / (0.3 + e) - 1.
PLANT_SETS = {"default": (0.55, 1e-4), "eps0": (0.55, 0.0), "sparse": (0.354, 1e-4)}


def plant_params(which):
    scale, e = PLANT_SETS[which]
    return [scale] + plant_values(e), e


def labelled_problem(m, seed, d=2):
    """data tables of max(m // 3, 4) points (label = index mod 16 in coordinate 0, the rest uniform in [0, 1)) and a
    random association list: indices repeat in both columns; its first two associations are distinct in both, so that
    every m >= 2 calls the formula"""
    rng = np.random.default_rng(seed)
    n = max(m // 3, 4)
    D1, D2 = rng.random((d, n)), rng.random((d, n))
    D1[0] = np.arange(n) % 16
    D2[0] = (np.arange(n) + 7) % 16
    A = np.stack([rng.integers(0, n, m), rng.integers(0, n, m)], axis=1).astype(np.int32)
    A[:2] = [[0, 0], [1, 1]][:m]
    u0 = rng.random(m) + 0.5
    return D1, D2, A, u0


def wide_problem(m, d, seed):
    rng = np.random.default_rng(seed)
    n = max(m // 3, 2)
    D1, D2 = rng.random((d, n)), rng.random((d, n))
    A = np.stack([rng.integers(0, n, m), rng.integers(0, n, m)], axis=1).astype(np.int32)
    return D1, D2, A


def planted_pairs(D1, A):
    """kind -> (i, j) of the distinct-association pairs whose first data carry that kind's label"""
    i, j = distinct_pairs(A)
    A = np.asarray(A)
    li, lj = D1[0, A[i, 0]], D1[0, A[j, 0]]
    return {kind: (i[(li == l) & (lj == l)], j[(li == l) & (lj == l)]) for l, kind in enumerate(PLANT_KINDS, start=1)}


def plant_kept(which):
    """kind -> whether the model keeps it under that parameter set"""
    _, e = PLANT_SETS[which]
    return {kind: bool(v > e) for kind, v in zip(PLANT_KINDS, plant_values(e))}


# ---- the fill's geometry -------------------------------------------------------------------------------------------


def shard_geometry(m, shards=1):
    """W = round_up(ceil(m / shards), 64); per shard its first column and its valid columns; the column blocks of 1024
    per shard and the threads (4 columns each) of the last one"""
    W = -(-(-(-m // shards)) // 64) * 64
    valid = [int(min(max(m - k * W, 0), W)) for k in range(shards)]
    blocks = -(-W // 1024)
    return dict(W=W, c0=[k * W for k in range(shards)], valid=valid, column_blocks=blocks,
                last_block_threads=(W - 1024 * (blocks - 1)) // 4, row_strips=-(-m // 32))


# ---- the cases of tests/test_gpu_custom_invariant_edges.py, with what each claims ----------------------------------
# tests/test_custom_invariant_model.py checks every claim without a device: a case cannot pass vacuously.

ASYM_PARAMS = [0.9, 0.25, 1e-3, 0.3]
WIDE_PARAMS = [0.05 * (k + 1) for k in range(16)]
MIN_PLANTED = 8          # distinct-association pairs of every planted kind a case must hold


def case_seed(m):
    return 7000 + m


VALUE_M = 1029           # value edges: every planted kind, three parameter sets, four storages

# lone fills: m -> what the size is there for (W, column blocks, row strips: checked from shard_geometry)
TILE_CASES = {
    1: dict(W=64, row_strips=1), 2: dict(W=64, row_strips=1), 3: dict(W=64, row_strips=1), 5: dict(W=64, row_strips=1),
    31: dict(W=64, row_strips=1), 32: dict(W=64, row_strips=1), 33: dict(W=64, row_strips=2),
    63: dict(W=64, row_strips=2), 64: dict(W=64, row_strips=2), 65: dict(W=128, row_strips=3),
    1023: dict(W=1024, column_blocks=1), 1024: dict(W=1024, column_blocks=1, row_strips=32),
    1025: dict(W=1088, column_blocks=2, last_block_threads=16, row_strips=33),
    1089: dict(W=1152, column_blocks=2, last_block_threads=32),
}
TILE_ALL_STORAGES = (1025, 5)

# column shards: (m, shards) -> the geometry claimed
SHARD_CASES = {
    (127, 3): dict(valid=[64, 63, 0]),                       # last shard empty
    (129, 3): dict(valid=[64, 64, 1]),                       # last shard holds one valid column
    (1089, 3): dict(valid=[384, 384, 321]),                  # uneven split, c0 not 0
    (2051, 2): dict(W=1088, valid=[1088, 963], column_blocks=2, last_block_threads=16),
    (127, 2): dict(valid=[64, 63]), (129, 2): dict(valid=[128, 1]), (1089, 2): dict(valid=[576, 513]),
    (2051, 3): dict(valid=[704, 704, 643]),
}

WIDE_M = 133             # d = 16 and d = 32; two shards: W = 128, valid [128, 5]
BATCH_MS = (3, 33, 64, 65, 1025, 130, 2)
