"""CPU tests of the fp32 prefilter's SPECIFICATION (tests/prefilter_model.py): neither prefilter form may reject a pair
the exact fp64 rule |l1 - l2| < eps keeps — on a seeded adversarial search that puts |l1 - l2| within 1e-15 relative
of eps, on both sides, far from the origin — and the threshold it is given is never below eps. No GPU, no oracle."""
import math

import numpy as np
import pytest

from tests import prefilter_model as pm


def _adversarial_pairs(rng, n, d, log_off=(-2.0, 5.0), log_eps=(-8.0, 0.0), log_len_min=-6.0):
    """n pairs (p_r, p_c), (q_r, q_c) of d-dimensional points: coordinates around +-offset (offset log-uniform),
    l1 log-uniform from 1e-6 up to the offset, l2 = l1 +- c with c log-uniform in the eps range; eps is then set
    within 1e-15 relative of the pair's own fp64 |l1 - l2|, on either side."""
    off = 10.0 ** rng.uniform(*log_off, n)
    sgn = lambda: rng.choice([-1.0, 1.0], (n, d))
    pr = sgn() * off[:, None] * rng.uniform(0.5, 1.0, (n, d))
    qr = sgn() * off[:, None] * rng.uniform(0.5, 1.0, (n, d))
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)
    u1, u2 = unit(rng.normal(size=(n, d))), unit(rng.normal(size=(n, d)))
    l1 = 10.0 ** rng.uniform(log_len_min, np.log10(off))
    c = 10.0 ** rng.uniform(*log_eps, n)
    shorter = (rng.random(n) < 0.5) & (c < l1)
    l2 = np.where(shorter, l1 - c, l1 + c)
    pc, qc = pr + l1[:, None] * u1, qr + l2[:, None] * u2
    L1, L2 = pm.length_f64(pr, pc), pm.length_f64(qr, qc)
    C = np.abs(L1 - L2)
    eps = C * (1.0 + rng.uniform(-1e-15, 1e-15, n))
    maxabs = np.max(np.abs(np.concatenate([pr, pc, qr, qc], axis=1)), axis=1)  # the pair's own: the smallest guard
    return pr, pc, qr, qc, L1, L2, eps, maxabs


def _check_no_false_rejection(pr, pc, qr, qc, L1, L2, eps, maxabs, d):
    keep = pm.keep_f64(L1, L2, eps)
    s1, s2 = pm.squared_lengths_f32(pr, pc), pm.squared_lengths_f32(qr, qc)
    E = np.array([pm.guarded_threshold(e, a, d) for e, a in zip(eps, maxabs)], np.float32)
    E2 = np.array([pm.guarded_threshold_sq(x) for x in E], np.float32)
    strip, sqfree = pm.keep_strip(s1, s2, E), pm.keep_sqrt_free(s1, s2, E2)
    bad_strip, bad_sqfree = np.flatnonzero(keep & ~strip), np.flatnonzero(keep & ~sqfree)
    for name, bad in (("strip", bad_strip), ("sqrt-free", bad_sqfree)):
        if bad.size:
            i = bad[0]
            raise AssertionError(f"{name} prefilter rejects {bad.size} kept pairs, e.g. d={d} eps={eps[i]!r} "
                                 f"l1={L1[i]!r} l2={L2[i]!r} maxabs={maxabs[i]!r} E={E[i]!r} s1={s1[i]!r} s2={s2[i]!r}")
    return keep


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6])
def test_no_false_rejection_on_adversarial_pairs(d):
    rng = np.random.default_rng(1000 + d)
    kept = total = 0
    for _ in range(4):  # 4 x 10 000 pairs per dimension: 200 000 in all
        args = _adversarial_pairs(rng, 10_000, d)
        keep = _check_no_false_rejection(*args, d)
        kept, total = kept + int(keep.sum()), total + keep.size
    # the search sits on the boundary: both sides of it are well populated
    assert 0.25 * total < kept < 0.75 * total


@pytest.mark.parametrize("d", [2, 3])
def test_no_false_rejection_where_the_fp32_squares_overflow(d):
    """Coordinates from 1e6 to 1e12 (world coordinates in small units): t = s1 + s2 - E^2, t*t and s1*s2 of the
    square-root-free form overflow fp32 once the lengths reach a few 1e9. The threshold is then infinite: every
    pair is scored exactly."""
    rng = np.random.default_rng(77 + d)
    args = _adversarial_pairs(rng, 20_000, d, log_off=(6.0, 12.0), log_len_min=0.0)
    keep = _check_no_false_rejection(*args, d)
    assert 0.25 * keep.size < keep.sum() < 0.75 * keep.size
    # (a threshold that stayed finite here would let t*t overflow: the pairs in question exist in this sample)
    pr, pc, qr, qc = args[:4]
    s1, s2 = pm.squared_lengths_f32(pr, pc), pm.squared_lengths_f32(qr, qc)
    with np.errstate(over="ignore"):
        assert np.any(np.isinf((s1 + s2) * (s1 + s2)))


@pytest.mark.parametrize("d", [2, 3, 5])
def test_guarded_threshold_bounds_eps_and_grows_with_maxabs(d):
    rng = np.random.default_rng(5 + d)
    for eps in 10.0 ** rng.uniform(-12, 3, 300):
        prev = np.float32(0)
        for maxabs in [0.0] + sorted(10.0 ** rng.uniform(-3, 12, 40)):
            E = pm.guarded_threshold(eps, maxabs, d)
            assert E >= eps and E > np.float32(eps)             # at least eps, and strictly above its fp32 rounding
            assert E >= prev                                   # monotone in maxabs
            prev = E
            E2 = pm.guarded_threshold_sq(E)
            assert float(E2) >= float(E) * float(E)            # rounded up
    # the guard itself: 128 (d + 1) 2^-24 maxabs on top of eps
    assert float(pm.guarded_threshold(0.0, 2.0 ** 24, d)) >= 128.0 * (d + 1)
    assert float(pm.guarded_threshold(0.0, 2.0 ** 24, d)) == float(np.nextafter(np.float32(128.0 * (d + 1)), np.inf))


def test_infinite_thresholds():
    inf = np.float32(np.inf)
    # t = eps + guard >= 3e38: no finite fp32 threshold
    assert pm.guarded_threshold(3.0e38, 0.0, 3) == inf
    assert pm.guarded_threshold(1.0, 1e45, 3) == inf
    assert pm.guarded_threshold(2.9e38, 0.0, 3) < inf
    # E >= 1e19: E^2 is not an fp32 number
    assert pm.guarded_threshold_sq(np.float32(1e19)) == inf
    assert pm.guarded_threshold_sq(inf) == inf
    assert pm.guarded_threshold_sq(np.nextafter(np.float32(1e19), np.float32(0))) < inf
    # ... and the forms keep every pair with finite squares under an infinite threshold
    s = np.float32([0.0, 1e-30, 1.0, 1e18, 1e30])
    s1, s2 = np.meshgrid(s, s)
    assert pm.keep_strip(s1, s2, inf).all()
    assert pm.keep_sqrt_free(s1, s2, inf).all()
    assert pm.keep_sqrt_free(s1, s2, pm.guarded_threshold_sq(np.float32(2e19))).all()


def test_the_fp32_emulation():
    # fmaf: one rounding (a plain fp32 multiply-add rounds twice and loses the low product bits)
    a = np.float32(1 + 2.0 ** -12)
    assert pm.fmaf(a, a, np.float32(-1.0)) == np.float32(2.0 ** -11 + 2.0 ** -24)
    assert (a * a) - np.float32(1.0) == np.float32(2.0 ** -11)
    rng = np.random.default_rng(3)
    x, y, z = (rng.normal(size=20000).astype(np.float32) for _ in range(3))
    from fractions import Fraction
    for i in range(0, 20000, 97):
        exact = Fraction(float(x[i])) * Fraction(float(y[i])) + Fraction(float(z[i]))
        got = pm.fmaf(x[i:i + 1], y[i:i + 1], z[i:i + 1])[0]
        lo, hi = np.nextafter(got, -np.inf), np.nextafter(got, np.inf)
        assert abs(Fraction(float(got)) - exact) <= min(abs(Fraction(float(lo)) - exact),
                                                        abs(Fraction(float(hi)) - exact))
    # fp64 fma: to the last bit of the exactly rounded result
    u, v, w = rng.normal(size=(3, 5000))
    for i in range(0, 5000, 37):
        exact = Fraction(u[i]) * Fraction(v[i]) + Fraction(w[i])
        assert abs(Fraction(float(pm.fma64(u[i:i + 1], v[i:i + 1], w[i:i + 1])[0])) - exact) <= \
            abs(Fraction(math.ulp(float(exact))))
