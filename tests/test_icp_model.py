"""CPU checks of tests/icp_model.py: the model the GPU tests compare with bit for bit is itself a working ICP, on the
recipe tests/test_gpu_icp.py uses (the bunny sample in the unit cube, 1025 target points, 300 of them as the source,
moved by the inverse of a rotation about (1, 2, 3) plus a translation; max_distance 0.1).

Measured with this draw (seed 0; noisy: seed 1): noise-free, 10 degrees / 0.05: fitness 0.993 at iteration 0, CONVERGED
after 10 (point-to-point) and 5 (point-to-plane) iterations at fitness 1.0, transform error below 1e-15. Uniform noise
+-0.002: translation error 1.5e-4 / 7.0e-4, rotation error 1.8e-4 / 1.1e-3 rad. 20 degrees / 0.1: fitness 0.73 at
iteration 0, CONVERGED after 15 / 6. Both clouds shifted by 1e6: every source point within 1e-9 of its true place.
The bounds asserted are not these figures: they are stated with each test."""
import numpy as np
import pytest

from oracle import bm_utils_ref as ref
from tests import icp_model as im

METHODS = [im.POINT, im.PLANE]


def _run(method, **kw):
    src, tgt, T_true = im.recipe(**kw)
    normals = im.plane_normals(tgt) if method == im.PLANE else None
    return im.icp(src, tgt, None, method, normals, 0.1, 30), src, tgt, T_true


@pytest.mark.parametrize("method", METHODS)
def test_noise_free_converges_to_the_truth(method):
    r, _, _, T_true = _run(method)
    assert r.status == im.CONVERGED and r.iterations < 20 and r.fitness == 1.0
    rot, tr = im.transform_error(T_true, r.T)
    assert rot < 1e-9 and tr < 1e-9
    assert r.history[0, 1] < 1.0 and np.all(r.history[r.iterations + 1:] == 0.0)


@pytest.mark.parametrize("method", METHODS)
def test_noisy_run_stays_within_the_noise(method):
    """bounds: the translation within the noise amplitude 0.002; the rotation within amplitude / radius of the cloud
    (0.002 / 0.5)"""
    r, _, _, T_true = _run(method, noise=0.002, seed=1)
    assert r.status == im.CONVERGED and r.fitness == 1.0
    rot, tr = im.transform_error(T_true, r.T)
    assert tr < 0.002 and rot < 0.004


@pytest.mark.parametrize("method", METHODS)
def test_far_start_still_converges(method):
    r, _, _, T_true = _run(method, deg=20.0, shift=0.1)
    assert r.status == im.CONVERGED and r.iterations < 30 and r.fitness == 1.0 and r.history[0, 1] < 0.8
    rot, tr = im.transform_error(T_true, r.T)
    assert rot < 1e-6 and tr < 1e-9


@pytest.mark.parametrize("method", METHODS)
def test_shifted_clouds_lose_nothing_in_the_sums(method):
    """Both clouds 1e6 away from the origin. The sums are taken about the centre of the target's box, so what is left is
    the rounding of the coordinates themselves: magnitude 1.7e6 * 2^-53 = 2e-10 per operation, some tens of operations
    per update, at most 30 updates: every source point lands within 1e-7 of where the truth puts it (a one-pass sum
    about the world's origin would lose 1e6^2 * 2^-53 = 1e-4 relative to the unit-size terms and miss this)."""
    r, src, _, T_true = _run(method, offset=1.0e6)
    assert r.status == im.CONVERGED and r.fitness == 1.0
    moved, true = im.transform(r.T, src), im.transform(T_true, src)
    assert np.abs(moved - true).max() < 1e-7
    assert r.rmse < 1e-7


def test_fast_search_equals_the_oracle():
    rng = np.random.default_rng(5)
    Q, B = rng.random((700, 3)), np.round(rng.random((300, 3)), 1)      # (rounded: many equal distances)
    idx, sqd = ref.knn_bruteforce(Q, B, 1)
    j, d = im.nearest_fast(Q, B, chunk=256)
    assert np.array_equal(j, idx[:, 0]) and d.tobytes() == sqd[:, 0].tobytes()
    Bq = np.round(rng.random((50, 3)), 1)
    idx, sqd = ref.knn_bruteforce(Bq, B, 1)
    j, d = im.nearest_fast(Bq, B)
    assert np.array_equal(j, idx[:, 0]) and d.tobytes() == sqd[:, 0].tobytes()


def test_fold_is_the_stated_tree():
    """257 partials (65 537 rows) exercise the second level's strided add; the result is close to, and in general not
    equal to, numpy's own order of addition"""
    rng = np.random.default_rng(7)
    t = rng.normal(size=(65537, 2))
    got = im.fold(t)
    part = [sum_tree(t[b * 256:(b + 1) * 256]) for b in range(257)]
    lanes = [part[i] + part[256] if i == 0 else part[i] for i in range(256)]       # lane 0: 0 + p0 + p256
    want = sum_tree(np.array(lanes))
    assert np.array_equal(np.array(got), want)
    assert np.allclose(got, t.sum(axis=0), rtol=0, atol=1e-9)


def sum_tree(v):
    v = np.concatenate([v, np.zeros((256 - len(v), v.shape[1]))])
    s = 128
    while s:
        v = v[:s] + v[s:2 * s]
        s >>= 1
    return v[0]


def test_too_few_and_evaluate_only():
    src, tgt, _ = im.recipe()
    r = im.icp(src, tgt, None, im.POINT, None, 1e-9, 30)
    assert r.status == im.TOO_FEW and r.iterations == 0 and np.array_equal(r.T, np.eye(4)) and r.count < 3
    fit, rmse, cnt, corr = im.evaluate(src, tgt, None, 0.1)
    r0 = im.icp(src, tgt, None, im.PLANE, im.plane_normals(tgt), 0.1, 0)
    assert r0.status == im.MAX_ITERATIONS and (r0.fitness, r0.rmse, r0.count) == (fit, rmse, cnt)
    assert (corr >= 0).sum() == cnt
