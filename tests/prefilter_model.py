"""Executable model (numpy) of the fp32 PREFILTER of the affinity fill (clipper_amd/csrc/k_affinity.hip.h) and of the
threshold it is given (guarded_threshold / guarded_threshold_sq, clipper_amd/csrc/host_solver.hpp). Test
infrastructure: tests/test_prefilter_model.py checks on the CPU that neither prefilter form ever rejects a pair the
exact fp64 rule |l1 - l2| < eps keeps (the promise behind C == pattern(M)); the kernels themselves are checked on the
GPU (tests/test_gpu_fill_boundaries.py).

  strip form     (k_affinity_compact):
                 keep  <=>  |sqrt(s1) - sqrt(s2)| < E                       (raw v_sqrt_f32)
  sqrt-free form (prefilter_close: k_affinity_sym and k_affinity_rect through tile_score_rows):
                 keep  <=>  t <= 0  or  t*t < (4 * 1.0000038147f) * (s1*s2),  t = (s1 + s2) - E^2

s1, s2 are the squared lengths, summed in fp32 by a sequential fmaf chain from the fp32 copies of the points
(k_gather_points); E = guarded_threshold(eps, maxabs, d), E^2 = guarded_threshold_sq(E). Every fp32 operation is
emulated with np.float32 (IEEE, round to nearest even); fmaf with the exact fp64 product and one rounding of the sum.
"""
from __future__ import annotations

import math

import numpy as np

F32_INF = np.float32(np.inf)

# host_solver.hpp, guarded_threshold: `std::ldexp(128.0 * (d + 1), -24) * maxabs`
GUARD_FACTOR = 128.0     # 128 (d + 1)
GUARD_EXP = -24          # 2^-24
# host_solver.hpp, guarded_threshold: `if (!(t < 3.0e38)) return infinity`
THRESHOLD_INF = 3.0e38
# host_solver.hpp, guarded_threshold: `smax = 8.0 * d * maxabs * maxabs; if (!(smax * smax < 1.0e38)) return infinity`
SQUARES_INF = 1.0e38
# host_solver.hpp, guarded_threshold_sq: `if (!(E < 1.0e19f)) return infinity`
THRESHOLD_SQ_INF = np.float32(1.0e19)
# k_affinity.hip.h, prefilter_close (the one place in device code): `t * t < (4.0f * 1.0000038147f) * (s1 * s2)`
MARGIN = np.float32(1.0000038147)  # = 1 + 2^-18


def guarded_threshold(eps: float, maxabs: float, d: int) -> np.float32:
    """eps + 128 (d + 1) 2^-24 maxabs, rounded to fp32 and then one step up; infinity from 3e38 on, and where the
    square-root-free form's fp32 t^2 could overflow (maxabs ~ 6e8 at d = 3)."""
    smax = 8.0 * d * maxabs * maxabs
    if not smax * smax < SQUARES_INF:
        return F32_INF
    guard = math.ldexp(GUARD_FACTOR * (d + 1), GUARD_EXP) * maxabs
    t = eps + guard
    if not t < THRESHOLD_INF:
        return F32_INF
    return np.nextafter(np.float32(t), F32_INF)


def guarded_threshold_sq(E: np.float32) -> np.float32:
    """E^2 (exact in fp64), rounded to fp32 and then one step up; infinity from E = 1e19 on."""
    E = np.float32(E)
    if not E < THRESHOLD_SQ_INF:
        return F32_INF
    e2 = float(E) * float(E)
    return np.nextafter(np.float32(e2), F32_INF)


# ---- fp32 / fp64 arithmetic ----------------------------------------------------------------------------------------

def _round_to_odd_sum(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """a + b (fp64 arrays) rounded to odd in fp64: rounding that once more to fp32 is the correctly rounded fp32 sum
    (53 >= 24 + 2 bits), without the double-rounding error of a plain fp64 sum."""
    a, b = np.broadcast_arrays(np.atleast_1d(a), np.atleast_1d(b))
    s = a + b
    bb = s - a
    err = (a - (s - bb)) + (b - bb)  # TwoSum: a + b == s + err exactly
    inexact = err != 0
    even = (s.view(np.int64) & 1) == 0
    fix = inexact & even
    s = s.copy()
    s[fix] = np.nextafter(s[fix], np.where(err[fix] > 0, np.inf, -np.inf))
    return s


def fmaf(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp32 fused multiply-add: the fp32 x fp32 product is exact in fp64, the sum is rounded once."""
    a, b, c = (np.asarray(x, np.float32) for x in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    r = _round_to_odd_sum(p, c.astype(np.float64)).astype(np.float32)
    return r.reshape(np.broadcast(a, b, c).shape)


def _two_prod(a: np.ndarray, b: np.ndarray):
    """Dekker: a * b == p + e exactly (no overflow / underflow in the range the model draws from)."""
    p = a * b
    sp = 134217729.0  # 2^27 + 1
    ah = a * sp
    ah = ah - (ah - a)
    al = a - ah
    bh = b * sp
    bh = bh - (bh - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def fma64(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fp64 fma, to within the last bit (the exact product plus c, summed in two steps)."""
    p, e = _two_prod(a, b)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    return s + (err + e)


def sqrt_f32_bounds(s: np.ndarray):
    """v_sqrt_f32 (__builtin_amdgcn_sqrtf, not correctly rounded): the correctly rounded root +- 1 ulp."""
    r = np.sqrt(np.asarray(s, np.float32))
    return np.nextafter(r, -F32_INF), np.nextafter(r, F32_INF)


# ---- the rules -------------------------------------------------------------------------------------------------------

def squared_lengths_f32(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """p, q: [..., d] fp64 points. The fp32 copies (k_gather_points), t = row - column in fp32, the sequential fmaf
    chain of the prefilter."""
    pf, qf = p.astype(np.float32), q.astype(np.float32)
    s = np.zeros(p.shape[:-1], np.float32)
    for k in range(p.shape[-1]):
        t = pf[..., k] - qf[..., k]
        s = fmaf(t, t, s)
    return s


def length_f64(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """euclidean_distance.cpp:18-19 as the exact score evaluates it: sequential fp64 fma chain, correctly rounded sqrt."""
    s = np.zeros(p.shape[:-1])
    for k in range(p.shape[-1]):
        t = p[..., k] - q[..., k]
        s = fma64(t, t, s)
    return np.sqrt(s)


def keep_f64(l1: np.ndarray, l2: np.ndarray, eps) -> np.ndarray:
    """euclidean_distance.cpp:28-30: the pair is scored when |l1 - l2| < eps (strict)."""
    return np.abs(l1 - l2) < eps


def keep_strip(s1: np.ndarray, s2: np.ndarray, E) -> np.ndarray:
    """The strip kernels' test `fabsf(sqrt(s1) - sqrt(s2)) < E`, with each v_sqrt_f32 at the end of its +-1 ulp range
    that makes the difference largest: kept here => kept on the device whatever the root's last bit."""
    E = np.asarray(E, np.float32)
    lo1, hi1 = sqrt_f32_bounds(s1)
    lo2, hi2 = sqrt_f32_bounds(s2)
    lo1, lo2 = np.maximum(lo1, np.float32(0)), np.maximum(lo2, np.float32(0))
    worst = np.maximum(np.abs(hi1 - lo2), np.abs(lo1 - hi2))
    return worst < E


def keep_sqrt_free(s1: np.ndarray, s2: np.ndarray, E2) -> np.ndarray:
    """prefilter_close (k_affinity_sym, k_affinity_rect): `t <= 0 || t * t < (4.0f * 1.0000038147f) * (s1 * s2)`."""
    s1, s2 = np.asarray(s1, np.float32), np.asarray(s2, np.float32)
    t = (s1 + s2) - np.asarray(E2, np.float32)
    k = np.float32(4.0) * MARGIN
    with np.errstate(over="ignore"):
        return (t <= np.float32(0)) | (t * t < k * (s1 * s2))
