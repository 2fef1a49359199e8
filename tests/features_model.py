"""TEST INFRASTRUCTURE — the model clipper_hip_estimate_normals / clipper_hip_compute_fpfh are held to: the contract of
clipper_amd/csrc/features_rules.hpp restated in numpy on top of oracle/bm_utils_ref.knn_bruteforce.

Neighbourhood of point i: the first knn entries of its list in the cloud itself (i included, recognised by j == i), with
radius > 0 only those with sqd <= radius * radius. cnt(i) = kept entries.
Normal: cnt < 3 -> (0, 0, 1); else the eigenvector (numpy eigh) of the smallest eigenvalue of the two-pass centred
covariance, signed towards the viewpoint or with its largest component positive.
Pair feature, bins, SPFH and FPFH: every dot product (a0*b0 + a1*b1) + a2*b2, every sum in the stated order, so that
numpy's IEEE operations give the device's bits (atan2 alone may differ by ulps: `margin` says how far every bin
coordinate is from a bin edge). Also the shared inputs of tests/test_features_model.py and tests/test_gpu_features.py."""
from __future__ import annotations

import json
import os

import numpy as np

from oracle import bm_utils_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS, DIM = 11, 33


def neighborhoods(P, knn, radius=0.0):
    """P: n x 3. Returns (idx n x knn int64, sqd n x knn, kept n x knn bool, cnt n): kept entries are a prefix."""
    P = np.asarray(P, np.float64)
    idx, sqd = ref.knn_bruteforce(P, P, knn)
    kept = idx >= 0
    if radius > 0:
        r2 = np.float64(radius) * np.float64(radius)
        kept &= sqd <= r2
    return idx, sqd, kept, kept.sum(axis=1).astype(np.int32)


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def covariance(Q):
    """two-pass centred sums of products of the rows of Q (cnt x 3), in row order; not divided by cnt"""
    m = np.zeros(3)
    for q in Q:
        m = m + q
    m = m / float(len(Q))
    C = np.zeros((3, 3))
    for q in Q:
        d = q - m
        C = C + np.outer(d, d)
    return C


def orient(nv, p, viewpoint):
    if viewpoint is not None:
        flip = dot(nv, np.asarray(viewpoint, np.float64) - p) < 0
    else:
        flip = nv[int(np.argmax(np.abs(nv)))] < 0        # argmax: the first component on ties
    return -nv if flip else nv


def normals(P, knn, radius=0.0, viewpoint=None):
    """Returns (N n x 3, cnt n, gap n): gap = (l1 - l0) / l2 of the covariance's ascending eigenvalues (0 where the
    normal is the fixed one or l2 == 0): how well the data determine the normal."""
    P = np.asarray(P, np.float64)
    idx, _, kept, cnt = neighborhoods(P, knn, radius)
    N = np.zeros((len(P), 3))
    gap = np.zeros(len(P))
    for i in range(len(P)):
        if cnt[i] < 3:
            N[i] = (0.0, 0.0, 1.0)
            continue
        w, V = np.linalg.eigh(covariance(P[idx[i, :cnt[i]]]))
        gap[i] = (w[1] - w[0]) / w[2] if w[2] > 0 else 0.0
        N[i] = orient(V[:, 0], P[i], viewpoint)
    return N, cnt, gap


def pair_features(p1, n1, p2, n2):
    """(theta, alpha, phi) of m pairs (arrays m x 3); (0, 0, 0) for a pair without a line or without a frame"""
    with np.errstate(divide="ignore", invalid="ignore"):
        dp = p2 - p1
        L = np.sqrt(dot(dp, dp))
        a1, a2 = dot(n1, dp) / L, dot(n2, dp) / L
        swap = np.abs(a1) < np.abs(a2)
        s3 = swap[:, None]
        m1, m2, d = np.where(s3, n2, n1), np.where(s3, n1, n2), np.where(s3, -dp, dp)
        phi = np.where(swap, -a2, a1)
        v = cross(d, m1)
        vl = np.sqrt(dot(v, v))
        v = v / vl[:, None]
        w = cross(m1, v)
        f = np.stack([np.arctan2(dot(w, m2), dot(m1, m2)), dot(v, m2), phi], axis=1)
    f[(L == 0) | (vl == 0)] = 0.0
    return f


def bin_coords(f):
    """where the features fall on their 11-bin axes, before the floor (m x 3)"""
    return np.stack([11.0 * (f[:, 0] + np.pi) / (2.0 * np.pi), 11.0 * (f[:, 1] + 1.0) * 0.5,
                     11.0 * (f[:, 2] + 1.0) * 0.5], axis=1)


def bins(f):
    """the three counters (of 33) each feature adds one to (m x 3 ints)"""
    b = np.clip(np.floor(bin_coords(f)), 0, 10).astype(np.int64)
    return b + np.array([0, BINS, 2 * BINS])


def fpfh(P, N, knn, radius=0.0):
    """Returns (F n x 33, SPFH n x 33, cnt n, margin n): margin[i] = the smallest distance of a bin coordinate of any
    pair of point i to an integer (inf without pairs)."""
    P, N = np.asarray(P, np.float64), np.asarray(N, np.float64)
    n = len(P)
    idx, sqd, kept, cnt = neighborhoods(P, knn, radius)
    S = np.zeros((n, DIM))
    margin = np.full(n, np.inf)
    for i in range(n):
        if cnt[i] < 2:
            continue
        js = idx[i, :cnt[i]]
        js = js[js != i]
        if len(js) == 0:
            continue
        pi, ni = np.repeat(P[i][None], len(js), 0), np.repeat(N[i][None], len(js), 0)
        f = pair_features(pi, ni, P[js], N[js])
        c = bin_coords(f)
        margin[i] = np.abs(c - np.round(c)).min()
        counts = np.bincount(bins(f).reshape(-1), minlength=DIM).astype(np.float64)
        S[i] = counts * (100.0 / float(cnt[i] - 1))
    F = np.zeros((n, DIM))
    for i in range(n):
        f = np.zeros(DIM)
        for k in range(cnt[i]):
            j, sd = idx[i, k], sqd[i, k]
            if j == i or sd == 0.0:
                continue
            f = f + S[j] / sd
        for g in range(3):
            s = 0.0
            for b in range(g * BINS, (g + 1) * BINS):
                s = s + f[b]
            if s != 0.0:
                f[g * BINS:(g + 1) * BINS] = f[g * BINS:(g + 1) * BINS] * (100.0 / s)
        F[i] = f + S[i]
    return F, S, cnt, margin


def sin_angle(A, B):
    """sine of the angle between the rows of A and B (unit vectors), sign ignored"""
    return np.linalg.norm(np.cross(A, B), axis=1)


# ---- shared inputs ------------------------------------------------------------------------------------------------

def bunny():
    """the committed 600-point sample of the bunny, n x 3"""
    return np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "bunny_points.json")))["points"], np.float64)


def uniform_cloud(n=300, seed=21):
    return np.random.default_rng(seed).random((n, 3))


def random_pairs(m=2000, seed=7):
    """m pairs of oriented points (p1, n1, p2, n2), each m x 3; a few of them degenerate on purpose: equal points, the
    line along the frame's normal"""
    rng = np.random.default_rng(seed)
    p1, p2 = rng.random((m, 3)), rng.random((m, 3))
    n1, n2 = rng.normal(size=(m, 3)), rng.normal(size=(m, 3))
    n1 /= np.linalg.norm(n1, axis=1)[:, None]
    n2 /= np.linalg.norm(n2, axis=1)[:, None]
    p2[:5] = p1[:5]
    n1[5:10] = (0.0, 0.0, 1.0)
    n2[5:10] = (0.0, 1.0, 0.0)
    p2[5:10] = p1[5:10] + np.array([0.0, 0.0, 0.25])
    return p1, n1, p2, n2


def grid_cloud():
    """18 points on a grid of pitch 0.5 (power-of-two coordinates: every squared distance is exact). With radius 0.5
    the axis neighbours sit exactly on the radius (sqd == 0.25 == radius * radius) and are kept; the diagonal ones
    (sqd == 0.5) are not."""
    g = np.array([[x, y, z] for x in range(3) for y in range(3) for z in range(2)], np.float64)
    return g * 0.5


def doubled_cloud(n=150, seed=33):
    """every point twice (indices i and i + n): sqd == 0 with j != i"""
    P = np.random.default_rng(seed).random((n, 3))
    return np.concatenate([P, P])


def radius_cloud(seed=21):
    """280 uniform points in the unit cube, 8 lone points and 6 close pairs far from it and from each other, shuffled:
    with radius 0.25 the lone points keep 1 entry (themselves), the pairs 2, the cube's points 3 to 16"""
    rng = np.random.default_rng(seed)
    P = rng.random((280, 3))
    singles = np.array([[3.0 + 2 * k, 0.5, 0.5] for k in range(8)]) + rng.random((8, 3)) * 0.1
    a = np.array([[0.5, 3.0 + 2 * k, 0.5] for k in range(6)]) + rng.random((6, 3)) * 0.1
    b = a + rng.normal(size=(6, 3)) * 0.03
    Q = np.concatenate([P, singles, a, b])
    return Q[rng.permutation(len(Q))]


def transformed_copy(P, seed=3):
    """(Q, perm, T): Q[perm[i]] = R P[i] + t for a seeded rotation R, translation t and permutation; T the 4 x 4"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    t = rng.normal(size=3)
    perm = rng.permutation(len(P))
    Q = np.zeros_like(P)
    Q[perm] = P @ q.T + t
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, t
    return Q, perm, T


def _line3():
    return np.outer(np.array([0.0, 1.0, 2.5]), np.array([0.3, -0.7, 0.45])) + np.array([0.1, 0.2, 0.3])


def _plane4():
    return np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])


def _rand(n, seed):
    return lambda: np.random.default_rng(seed).random((n, 3))


# ---- the clouds of tests/test_gpu_features.py -------------------------------------------------------------------------
# Neighbourhoods of two or three points make pairs whose theta is 0 or +-pi to rounding (two neighbours with the same
# kept set have the same normal up to the sign rule; two neighbours with three kept points each have both normals at
# right angles to the line between them), and +-pi is the edge between the first and the last bin. The generic inputs
# below have no such pair: tests/test_features_model.py checks the margin of every one of them.
# name -> (cloud, knn, radius, viewpoint, generic). generic: a cloud in general position, on which the gap cap and the
# bit-for-bit comparison of the histograms apply (the others are degenerate on purpose: their normals are checked by
# what is known about them)
GPU_CASES = {
    "n1": (_rand(1, 1), 3, 0.0, None, True),                       # a lone point: cnt 1
    "n2": (_rand(2, 2), 3, 0.0, (0.5, 0.5, 4.0), True),            # cnt 2: the fixed normal, an SPFH of one pair
    "line3": (_line3, 3, 0.0, None, False),                        # rank-one covariance
    "plane4": (_plane4, 4, 0.0, None, False),                      # the normal known exactly
    "n10_k16": (_rand(10, 3), 16, 0.0, None, True),                # lists shorter than K
    "n257_k8": (_rand(257, 41), 8, 0.0, (0.5, 0.5, 0.5), True),    # the second query block
    "n1025_k16": (_rand(1025, 5), 16, 0.0, None, True),            # the second chunk and the merge
    "n2100_k32": (_rand(2100, 6), 32, 0.0, (2.0, -1.0, 0.5), True),  # three chunks, the K = 32 search
    "doubled_k8": (doubled_cloud, 8, 0.0, None, True),          # sqd == 0 with j != i
    "radius": (radius_cloud, 16, 0.25, None, True),             # cnt of 1 and 2 among the points, and 3 to 16
    "on_radius": (grid_cloud, 8, 0.5, None, False),             # sqd == radius^2 exactly
    "uniform": (uniform_cloud, 16, 0.0, None, True),
    "bunny_k16": (bunny, 16, 0.0, None, True),
    "bunny_k32_r": (bunny, 32, 0.02, (0.0, 0.1, 1.0), True),
}

_models = {}


def case_model(name):
    """the numpy model of a case, computed once"""
    if name not in _models:
        make, knn, radius, view, generic = GPU_CASES[name]
        P = make()
        N, cnt, gap = normals(P, knn, radius, view)
        F, S, fcnt, margin = fpfh(P, N, knn, radius)
        assert np.array_equal(cnt, fcnt)
        _models[name] = dict(P=P, knn=knn, radius=radius, view=view, generic=generic, N=N, cnt=cnt, gap=gap, F=F, S=S,
                             margin=margin)
    return _models[name]
