"""CPU tests of tests/icp_robust_model.py, the model the robust and trimmed ICP is held to: with no loss and no trimming
it is tests/icp_model.py and tests/gicp_model.py bit for bit; each weight function equals a Python-float restatement below,
at and above the scale; the trimming rule on ties; and the property that makes the feature worth having: on a cluttered
source from a close start every loss and the trimming end at most half as far from the truth as plain ICP."""
import math

import numpy as np
import pytest

from tests import gicp_model as gm
from tests import icp_model as im
from tests import icp_robust_model as rm

# (name, loss, scale, trim): the variants of the property test
VARIANTS = [("huber", rm.HUBER, 0.01, 1.0), ("cauchy", rm.CAUCHY, 0.01, 1.0), ("tukey", rm.TUKEY, 0.03, 1.0),
            ("geman_mcclure", rm.GEMAN_MCCLURE, 0.01, 1.0), ("trim", rm.NONE, 0.0, 0.6)]


def _same(a, b):
    return (a.T.tobytes(), a.history.tobytes(), a.iterations, a.status, a.count, a.fitness, a.rmse) == (
        b.T.tobytes(), b.history.tobytes(), b.iterations, b.status, b.count, b.fitness, b.rmse)


@pytest.mark.parametrize("kw", [dict(), dict(noise=0.002, seed=1)], ids=["recipe", "noisy"])
def test_no_loss_and_no_trimming_is_the_plain_model_bit_for_bit(kw):
    src, tgt, _ = im.recipe(**kw)
    normals = im.plane_normals(tgt)
    for method in (im.POINT, im.PLANE):
        r = rm.icp_robust(src, tgt, None, method, normals, None, 0.1, 30)
        assert _same(r, im.icp(src, tgt, None, method, normals, 0.1, 30))
        assert r.within == r.count and r.trim_sqd == np.float64(0.1) * np.float64(0.1)
        assert r.weight_sum == (float(r.count) if method == im.POINT else 0.0)
    cs, ct = gm.covariances(src)[0], gm.covariances(tgt)[0]
    r = rm.icp_robust(src, tgt, None, rm.GENERALIZED, None, (cs, ct), 0.1, 30)
    assert _same(r, gm.icp_generalized(src, cs, tgt, ct, None, 0.1, 30))


def _weight(loss, e, scale):
    """the rules of the issue on Python floats"""
    k2 = scale * scale
    if loss == rm.HUBER:
        return 1.0 if e <= k2 else scale / math.sqrt(e)
    if loss == rm.CAUCHY:
        return 1.0 / (1.0 + e / k2)
    if loss == rm.TUKEY:
        if e < k2:
            u = 1.0 - e / k2
            return u * u
        return 0.0
    if loss == rm.GEMAN_MCCLURE:
        g = k2 / (k2 + e)
        return g * g
    return 1.0


@pytest.mark.parametrize("loss", sorted(rm.LOSSES.values()))
def test_weights_below_at_and_above_the_scale(loss):
    scale = 0.03
    k2 = scale * scale
    es = [0.0, k2 / 3.0, math.nextafter(k2, 0.0), k2, math.nextafter(k2, 1.0), 7.0 * k2, 1e6 * k2]
    got = rm.weight(loss, np.array(es), scale)
    assert [float(x) for x in got] == [_weight(loss, e, scale) for e in es]
    assert got[0] == 1.0 and np.all(np.diff(got) <= 0.0) and np.all(got >= 0.0)
    at = {rm.NONE: 1.0, rm.HUBER: 1.0, rm.CAUCHY: 0.5, rm.TUKEY: 0.0, rm.GEMAN_MCCLURE: 0.25}[loss]
    assert got[3] == at
    if loss == rm.TUKEY:
        assert got[2] > 0.0 and np.all(got[3:] == 0.0)
    if loss == rm.HUBER:
        assert got[2] == 1.0 and got[4] < 1.0 and got[5] == scale / math.sqrt(7.0 * k2)
    assert math.isnan(float(rm.weight(rm.HUBER, np.array([np.nan]), scale)[0]))


def test_trimmed_counts_on_ties():
    sqd = np.array([4.0, 1.0, 1.0, 9.0, 2.0, 2.0, 2.0, 0.5, 100.0, 3.0])
    inl = sqd <= 50.0                                      # nine within
    for trim, keep, tau, count in [(1.0, 9, 50.0, 9), (0.5, 4, 2.0, 6), (0.34, 3, 1.0, 3), (0.25, 2, 1.0, 3),
                                   (0.12, 1, 0.5, 1), (0.1, 0, 0.0, 0), (0.999, 8, 4.0, 8)]:
        kept, within, t = rm.trim_threshold(sqd, inl, trim, 50.0)
        assert within == 9 and t == tau and int(kept.sum()) == count and count >= min(keep, 9), (trim, t, kept.sum())
        assert not kept[8] and (trim == 1.0 or keep == int(trim * 9.0))
    kept, within, t = rm.trim_threshold(np.zeros(5), np.ones(5, bool), 0.5, 1.0)     # all equal: all kept
    assert (within, t, int(kept.sum())) == (5, 0.0, 5)


@pytest.mark.parametrize("method", [im.POINT, im.PLANE], ids=["point", "plane"])
@pytest.mark.parametrize("seed", [0, 1])
def test_losses_and_trimming_beat_plain_icp_on_clutter(seed, method):
    """the cluttered close start (2 degrees, 0.01; 300 source points and 200 clutter points): every variant ends with
    rotation and translation errors at most half of plain ICP's"""
    src, tgt, T_true = rm.cluttered(seed)
    normals = im.plane_normals(tgt)
    plain = im.icp(src, tgt, None, method, normals, 0.1, 40)
    pr, pt = im.transform_error(T_true, plain.T)
    assert 2e-3 < pr < 4e-2
    for name, loss, scale, trim in VARIANTS:
        r = rm.icp_robust(src, tgt, None, method, normals, None, 0.1, 40, loss=loss, scale=scale, trim=trim)
        rr, rt = im.transform_error(T_true, r.T)
        print(f"seed {seed} method {method} {name}: rotation {pr:.3g} -> {rr:.3g} ({pr / rr:.1f}x), "
              f"translation {pt:.3g} -> {rt:.3g} ({pt / rt:.1f}x), {r.iterations} iterations")
        assert r.status == im.CONVERGED and rr <= 0.5 * pr and rt <= 0.5 * pt, name


def test_far_start_of_the_redescending_losses_is_recorded():
    """An observation, not a claim of quality: from the recipe's default start (10 degrees, 0.05) on the cluttered
    source the redescending losses (Tukey 0.03, Geman-McClure 0.01) give the far pairs next to no weight in point-to-point
    and settle on a wrong alignment, where Huber, Cauchy and trimming still end ten times closer than plain ICP. Measured
    with this model, seed 0, 40 iterations at most (rotation error in rad / translation error, all CONVERGED): plain
    6.0e-3 / 6.0e-3, huber 5.8e-4 / 5.7e-4, cauchy 2.1e-4 / 6.1e-5, trimming at 0.6 4.7e-4 / 2.7e-4; tukey 0.19 / 0.076,
    geman_mcclure 0.18 / 0.072. A property of those losses, not of the code: start them close (from the 2 degree start
    they beat plain ICP 16 to 62 times, above). The test prints the numbers and checks only that every run ends with a
    finite transform and a status."""
    src, tgt, T_true = rm.cluttered(0, deg=10.0, shift=0.05)
    plain = im.icp(src, tgt, None, im.POINT, None, 0.1, 40)
    print("plain", im.transform_error(T_true, plain.T), plain.iterations, plain.status)
    for name, loss, scale, trim in VARIANTS:
        r = rm.icp_robust(src, tgt, None, im.POINT, None, None, 0.1, 40, loss=loss, scale=scale, trim=trim)
        print(name, im.transform_error(T_true, r.T), r.iterations, r.status)
        assert np.all(np.isfinite(r.T)) and r.status in (im.CONVERGED, im.MAX_ITERATIONS, im.TOO_FEW, im.DEGENERATE)
