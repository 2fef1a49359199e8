"""CPU tests of tests/ransac_model.py, the model clipper_hip_ransac_correspondences is held to: the counter-based draw
pinned as integers, the sample's rules, the stop rule at its edges, and that the model is a working RANSAC on the
registration recipe (the condition is exact: the final inlier mask is the ground truth)."""
import numpy as np
import pytest

from clipper_amd import registration as reg
from tests import ransac_model as rm


def test_draws_are_pinned():
    # (seed, h, t, m) -> index: the finalizer of splitmix64 over seed + 0x9E3779B97F4A7C15 (64 h + t + 1), high-half multiply
    assert rm.draw(0, 0, 0, 1000) == 883
    assert rm.draw(0, 1, 0, 1000) == 165
    assert rm.draw(1, 5, 63, 257) == 125
    assert rm.draw(12345, 100000, 7, 65537) == 41824
    assert rm.draw(2 ** 64 - 1, 2 ** 31, 3, 2 ** 31 - 1) == 1881065087
    assert rm.mix(0) == 0 and rm.mix(1) == 0x5692161D100B05E5


def test_vectorised_draw_equals_the_scalar_one():
    for seed, h0, m, n in [(0, 0, 1000, 3), (7, 65536 * 3, 5, 4), (2 ** 64 - 1, 2 ** 31, 9, 8), (3, 0, 3, 3)]:
        s, valid = rm.samples_round(seed, h0, 64, m, n)
        for g in range(64):
            want, ok = rm.sample(seed, h0 + g, m, n)
            assert [int(x) for x in s[g]] == want and bool(valid[g]) == ok


def test_samples_are_distinct_and_in_range():
    s, valid = rm.samples_round(11, 0, 1024, 10, 8)
    assert valid.any()
    for row, ok in zip(s, valid):
        got = [int(x) for x in row if x >= 0]
        assert len(set(got)) == len(got) and all(0 <= x < 10 for x in got)
        assert ok == (len(got) == 8)


def test_exhausted_attempts_mark_the_hypothesis_invalid():
    # three slots cannot fill from two indices: all 64 attempts are spent
    for h in range(32):
        s, ok = rm.sample(0, h, 2, 3)
        assert not ok and s[2] == -1 and sorted(s[:2]) == [0, 1]
    _, valid = rm.samples_round(0, 0, 32, 2, 3)
    assert not valid.any()
    # eight slots from eight indices fill only when 64 draws reach every index: both outcomes occur
    _, valid = rm.samples_round(0, 0, 4096, 8, 8)
    assert valid.any()


def test_needed_at_its_edges():
    assert rm.needed(10, 10, 3, 0.999) == 1                       # w = 1
    assert rm.needed(40, 200, 3, 0.999) == 861
    assert rm.needed(3, 1000, 3, 0.999) == 255842785              # beyond any max_hypotheses of the tests
    assert rm.needed(3, 2 ** 31 - 1, 3, 0.999) == rm.INT64_MAX    # 1 - w^n rounds to 1
    assert rm.stop(3, 16384, 1000, 3, 0.999, 16384) == rm.MAX_HYPOTHESES
    assert rm.stop(2, 16384, 1000, 3, 0.999, 16384) == rm.NO_MODEL
    assert rm.stop(40, 1024, 200, 3, 0.999, 16384) == rm.CONVERGED
    assert rm.stop(40, 512, 200, 3, 0.999, 16384) is None


def _check(cfg, **kw):
    D1, D2, A, Agt, T = rm.recipe(*cfg)
    args = dict(max_hypotheses=16384, hypotheses_per_round=1024, seed=cfg[3])
    args.update(kw)
    r = rm.ransac(D1, D2, A, rm.MAX_DISTANCE, **args)
    truth = np.zeros(len(A), bool)
    truth[:len(Agt)] = True           # (the recipe lists the correct pairs first)
    assert r.status in (rm.CONVERGED, rm.MAX_HYPOTHESES)
    assert np.array_equal(r.inliers, truth)                      # precision = recall = 1
    assert r.count == len(Agt) and r.evaluated % args["hypotheses_per_round"] == 0
    e0, e1 = reg.transform_error(T, r.T_hypothesis), reg.transform_error(T, r.T)
    assert e1[0] <= e0[0] and e1[1] <= e0[1]                     # the polish moves no farther from the truth
    return r


@pytest.mark.parametrize("cfg", rm.RECIPE)
def test_model_is_a_working_ransac(cfg):
    _check(cfg)


def test_model_without_the_checker_and_with_four_points():
    a = _check(rm.RECIPE[0], edge_similarity=0.0)
    assert a.checked > 900                                        # nearly every hypothesis is scored
    b = _check(rm.RECIPE[0], n_sample=4)
    assert b.sample[3] >= 0 and b.sample[4] == -1


def test_no_model_is_the_identity():
    D1, D2, A, _, _ = rm.recipe(*rm.RECIPE[3])
    r = rm.ransac(D1, D2, A, 1e-9, max_hypotheses=256, hypotheses_per_round=256)
    assert r.status == rm.NO_MODEL and np.array_equal(r.T, np.eye(4)) and r.best_hypothesis == -1 and r.refined == 0
