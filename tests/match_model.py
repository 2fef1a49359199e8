"""TEST INFRASTRUCTURE — the model clipper_hip_match_descriptors is held to: the filters of
clipper_amd/csrc/host_match_select.hpp restated in numpy on top of oracle/bm_utils_ref.knn_bruteforce (any d, distances
added in coordinate order, ties by index). Row (i, nn_k(i)), k < knn, is kept iff all of
    nn_k(i) >= 0
    max_sqdist <= 0  or  sqd_k(i) <= max_sqdist
    ratio <= 0  or  nn_1(i) < 0  or  sqd_0(i) < (ratio * ratio) * sqd_1(i)     (knn == 1; forward lists of 2)
    not mutual  or  i in bn(nn_k(i))[0 .. knn)
with i ascending, then k ascending. Also the shared data recipes of tests/test_match_model.py and
tests/test_gpu_match.py."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import bm_utils_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (knn, mutual, ratio, max_sqdist)
CONFIGS = [(1, 1, 0.0, 0.0), (1, 0, 0.8, 0.0), (1, 1, 0.8, 0.0), (3, 1, 0.0, 0.0), (1, 0, 0.0, 0.12), (2, 1, 0.0, 0.12)]


def match_model(F0, F1, knn=1, mutual=True, ratio=0.0, max_sqdist=0.0):
    """F0: n0 x d, F1: n1 x d (rows = descriptors). Returns (A n x 2 int32, sqd n, idx n0 x knn, lsq n0 x knn): the
    associations, their squared distances, and the forward lists before the filters (-1 / inf where F1 is short)."""
    if ratio > 0 and knn != 1:
        raise ValueError("the ratio test needs knn == 1")
    F0, F1 = np.asarray(F0, np.float64), np.asarray(F1, np.float64)
    fi, fd = ref.knn_bruteforce(F0, F1, 2 if ratio > 0 else knn)
    bi = ref.knn_bruteforce(F1, F0, knn)[0] if mutual else None
    r2 = ratio * ratio
    rows, sqd = [], []
    for i in range(len(F0)):
        if ratio > 0 and not (fi[i, 1] < 0 or fd[i, 0] < r2 * fd[i, 1]):
            continue
        for k in range(knn):
            j = int(fi[i, k])
            if j < 0:
                continue
            if max_sqdist > 0 and not fd[i, k] <= max_sqdist:
                continue
            if mutual and i not in bi[j, :knn].tolist():
                continue
            rows.append((i, j))
            sqd.append(fd[i, k])
    return (np.array(rows, dtype=np.int32).reshape(-1, 2), np.array(sqd, dtype=np.float64), fi[:, :knn].astype(np.int32),
            fd[:, :knn])


def filter_recipe():
    """400 x 500 descriptors of 33 numbers: 250 points of F1 are noisy copies of points of F0, 250 are random.
    Returns (F0, F1, truth) with truth the set of (i, j) true pairs."""
    rng = np.random.default_rng(11)
    n0, n1, d = 400, 500, 33
    F0 = rng.random((n0, d))
    src = rng.permutation(n0)[:250]
    F1 = np.concatenate([F0[src] + rng.normal(0, 0.05, (250, d)), rng.random((n1 - 250, d))])
    return F0, F1, {(int(i), j) for j, i in enumerate(src)}


def bunny_recipe(seed=5):
    """The end-to-end data: the bunny sample in the unit cube, a noisy copy (as the reference benchmark's recipe), one
    random 32-number descriptor per point; the second view's descriptors are the first's plus N(0, 0.05^2), a seeded
    30 % of them replaced by fresh random ones. Returns (pts, noisy, F0, F1, Agt) with Agt the pairs (i, i) whose
    descriptor was kept."""
    pts = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "bunny_points.json")))["points"])
    pts = ref.scale_to_cube(pts, 1.0)
    rng = np.random.default_rng(seed)
    n = len(pts)
    noisy = pts + ref.generate_bounded_normal_noise(n, 0.01, 0.0554, rng)
    F0 = rng.random((n, 32))
    F1 = F0 + rng.normal(0, 0.05, (n, 32))
    lost = rng.permutation(n)[:int(round(0.3 * n))]
    F1[lost] = rng.random((len(lost), 32))
    kept = np.setdiff1d(np.arange(n), lost)
    return pts, noisy, F0, F1, np.stack([kept, kept], axis=1).astype(np.int32)
