"""CPU checks of tests/gicp_model.py, the model the generalized ICP on the device is compared with bit for bit: its 30
sums against an independent direct evaluation, that it is a working refinement on the recipe of tests/test_gpu_gicp.py,
that it beats point-to-point where generalized ICP is meant to (two disjoint samples of one surface), and the rule of
the per-point covariances.

Measured with these draws: the recipe cases end CONVERGED after 4 to 6 iterations at fitness 1.0, the smallest
det(C_b + R C_a R^T) over all pairs and iterations 0.008 (noise-free), transform error below 1e-13 on the noise-free
recipe. Disjoint samples, seeds 100 to 103: rotation error 0.0017 .. 0.0050 rad in 4 to 6 iterations against
point-to-point's 0.0094 .. 0.021 in 13 to 30, translation error 0.0006 .. 0.0038 against 0.0061 .. 0.015. (How the two
samples are drawn matters at this size: with rng.permutation(4096)[:3072] in place of rng.choice(4096, 3072,
replace=False) seed 102 gave a rotation error of 0.00534 against point-to-point's 0.00498, the translation error
0.00389 against 0.00399; the other three seeds held.) The bounds asserted are not these figures: they are stated with
each test."""
import numpy as np
import pytest

from tests import features_model as fm
from tests import gicp_model as gm
from tests import icp_model as im


def _covs(src, tgt):
    return gm.covariances(src)[0], gm.covariances(tgt)[0]


def _skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def test_sums_equal_a_direct_evaluation():
    """T_init a quarter turn about z and the source turned back by it: the covariances of the source are taken in its
    own frame, so a model that used C_a unrotated, or R^T C_a R, would miss these sums by far more than rounding. The
    direct evaluation: np.linalg.inv, plain matrix products, J as a 3 x 6 array, numpy's own order of addition. Bound:
    1e-10 relative (the model's and numpy's rounding differ by some n * 2^-53 = 3e-14 of the sums' own size, times the
    condition of C_b + R C_a R^T, at most 1 / epsilon = 1e3)."""
    src, tgt, _ = im.recipe()
    T0 = im.rigid(90.0, (0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
    src0 = src @ T0[:3, :3]                           # rows: R^T p, so that T0 puts them back
    cs, ct = _covs(src0, tgt)
    o = im.origin(tgt)
    S, corr, det = gm.sums(src0, cs, tgt, ct, T0, 0.1, o)
    R = T0[:3, :3]
    q = im.transform(T0, src0)

    def direct(rotate):
        A, g, c, sq, n = np.zeros((6, 6)), np.zeros(6), 0.0, 0.0, 0
        for i, j in enumerate(corr):
            if j < 0:
                continue
            M = np.linalg.inv(gm.full(ct[j]) + rotate(gm.full(cs[i])))
            J = np.concatenate([-_skew(q[i] - o), np.eye(3)], axis=1)
            d = q[i] - tgt[j]
            A, g, c, sq, n = A + J.T @ M @ J, g + J.T @ M @ d, c + d @ M @ d, sq + d @ d, n + 1
        return [float(n)] + [A[i, j] for i in range(6) for j in range(i, 6)] + list(g) + [c, sq]

    want = direct(lambda Ca: R @ Ca @ R.T)
    assert want[0] == S[0] and 250 < S[0] <= 300 and det > 1e-3
    assert np.allclose(S, want, rtol=1e-10, atol=0.0), np.abs(np.array(S) / np.array(want) - 1.0).max()
    # the two mistakes this case is for
    assert not np.allclose(S, direct(lambda Ca: Ca), rtol=1e-3, atol=0.0)
    assert not np.allclose(S, direct(lambda Ca: R.T @ Ca @ R), rtol=1e-3, atol=0.0)


RECIPES = {"recipe": dict(), "noisy": dict(noise=0.002, seed=1), "shifted": dict(offset=1.0e6),
           "odd": dict(n_src=257, n_tgt=400, seed=2)}


@pytest.mark.parametrize("name", sorted(RECIPES))
def test_it_is_a_working_refinement(name):
    src, tgt, T_true = im.recipe(**RECIPES[name])
    cs, ct = _covs(src, tgt)
    r = gm.icp_generalized(src, cs, tgt, ct, None, 0.1, 30)
    rot, tr = im.transform_error(T_true, r.T)
    print(f"{name}: {r.iterations} iterations, smallest det {r.min_det:.3g}, rotation error {rot:.3g}, translation error {tr:.3g}")
    assert r.status == im.CONVERGED and r.fitness == 1.0 and r.iterations < 20
    assert np.all(r.history[r.iterations + 1:] == 0.0)
    if name == "recipe":                              # tests/test_icp_model.py's bound for the other two methods
        assert rot < 1e-9 and tr < 1e-9


def disjoint_samples(seed):
    """two disjoint samples of the bunny in the unit cube: 2048 target points, 1024 other points as the source, moved by
    the inverse of 5 degrees about (1, 2, 3) through the cloud's centre and 0.02 along (1, 1, 1) / sqrt 3"""
    rng = np.random.default_rng(seed)
    P = im.bunny_unit()
    pick = rng.choice(len(P), 3072, replace=False)    # (the draw of im.recipe)
    tgt, own = P[pick[:2048]], P[pick[2048:]]
    c = tgt.mean(axis=0)
    C, Ci = np.eye(4), np.eye(4)
    C[:3, 3], Ci[:3, 3] = c, -c
    T_true = C @ im.rigid(5.0, (1.0, 2.0, 3.0), np.full(3, 0.02 / np.sqrt(3.0))) @ Ci
    Ti = np.linalg.inv(T_true)
    return np.ascontiguousarray(own @ Ti[:3, :3].T + Ti[:3, 3]), np.ascontiguousarray(tgt), T_true


@pytest.mark.parametrize("seed", [100, 101, 102, 103])
def test_disjoint_samples_are_refined_better_than_by_point_to_point(seed):
    """no source point has a partner in the target: point-to-point pulls every point to a neighbour's place, the
    generalized metric lets it slide within the surface"""
    src, tgt, T_true = disjoint_samples(seed)
    cs, ct = _covs(src, tgt)
    g = gm.icp_generalized(src, cs, tgt, ct, None, 0.05, 30)
    p = im.icp(src, tgt, None, im.POINT, None, 0.05, 30)
    (grot, gtr), (prot, ptr) = im.transform_error(T_true, g.T), im.transform_error(T_true, p.T)
    print(f"seed {seed}: generalized {grot:.3g} rad / {gtr:.3g} in {g.iterations}; point-to-point {prot:.3g} rad / {ptr:.3g} in {p.iterations}")
    assert g.status in (im.CONVERGED, im.MAX_ITERATIONS) and grot < prot and gtr < ptr


def test_covariances_follow_the_rule():
    eps = 1e-3
    P = fm.bunny()
    C, cnt, N = gm.covariances(P, 20, 0.0, eps)
    assert np.all(cnt == 20)
    F = gm.full(C)
    assert np.array_equal(F, np.swapaxes(F, 1, 2))
    w = np.linalg.eigvalsh(F)
    assert np.abs(w - np.array([eps, 1.0, 1.0])).max() < 1e-12
    assert np.abs(np.linalg.norm(N, axis=1) - 1.0).max() < 1e-15
    # the rule applied to the model's own normal, entry by entry; and the same surface normal as features_model's eigh
    want = np.array([[(1.0 if r == c else 0.0) - (1.0 - eps) * (nv[r] * nv[c]) for r in range(3) for c in range(r, 3)] for nv in N])
    assert want.tobytes() == C.tobytes()
    Nf, _, gap = fm.normals(P, 20)
    sure = gap > 0.05
    assert sure.sum() > 500 and fm.sin_angle(N[sure], Nf[sure]).max() < 1e-12
    # the sign of the normal cancels
    assert gm.covariance_of_normal(-N, eps).tobytes() == C.tobytes()
    # epsilon = 1: the identity whatever the normal
    assert np.array_equal(gm.covariances(P[:50], 8, 0.0, 1.0)[0], np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (50, 1)))


def test_fewer_than_three_neighbours_give_the_identity():
    P = fm.radius_cloud()
    C, cnt, _ = gm.covariances(P, 16, 0.25, 1e-3)
    few = cnt < 3
    assert few.sum() >= 20 and set(cnt[few]) == {1, 2} and (~few).sum() > 250      # (8 lone points, 6 pairs at the least)
    assert np.array_equal(C[few], np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (few.sum(), 1)))
    assert np.all(np.linalg.eigvalsh(gm.full(C[~few]))[:, 0] < 0.5)
    r = gm.covariances(np.random.default_rng(1).random((2, 3)), 3)
    assert np.array_equal(r[0], np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (2, 1))) and list(r[1]) == [2, 2]
