"""TEST INFRASTRUCTURE — the model clipper_hip_icp_robust / clipper_hip_icp_generalized_robust are held to: the robust
losses and the trimming of clipper_amd/csrc/icp_rules.hpp restated in numpy on top of tests/icp_model.py and
tests/gicp_model.py (their search, terms, fold, steps and recipe; neither file is changed).

The weight of a kept pair is written in the header's order with nothing fused; the weighted terms are w * t[a] for every
term but the count and the last one; point-to-point carries the sum of the weights at position 16 (18 terms) and its
centroids divide by it. The trimming threshold is stated as a sort: tau = np.sort(sqd[within])[keep - 1], where the
header states a radix select; both are exact, so they agree bit for bit."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests import gicp_model as gm
from tests import icp_model as im

NONE, HUBER, CAUCHY, TUKEY, GEMAN_MCCLURE = 0, 1, 2, 3, 4
LOSSES = {"none": NONE, "huber": HUBER, "cauchy": CAUCHY, "tukey": TUKEY, "geman_mcclure": GEMAN_MCCLURE}
POINT, PLANE, GENERALIZED = im.POINT, im.PLANE, gm.GENERALIZED
MIN_COUNT = {POINT: 3, PLANE: 6, GENERALIZED: 3}
WEIGHT_SUM = 16          # position of sum w in the 18 point-to-point terms


# ---- the weight of a pair ----------------------------------------------------------------------------------------------

def weight(loss, e, scale):
    """icp_rules.hpp's icp_weight over an array of squared residuals e"""
    e = np.asarray(e, np.float64)
    scale = np.float64(scale)
    k2 = scale * scale
    with np.errstate(all="ignore"):
        if loss == HUBER:
            return np.where(e <= k2, 1.0, scale / np.sqrt(e))
        if loss == CAUCHY:
            return 1.0 / (1.0 + e / k2)
        if loss == TUKEY:
            u = 1.0 - e / k2
            return np.where(e < k2, u * u, 0.0)
        if loss == GEMAN_MCCLURE:
            g = k2 / (k2 + e)
            return g * g
    return np.ones_like(e)


# ---- trimming ----------------------------------------------------------------------------------------------------------

def trim_threshold(sqd, inl, trim, d2):
    """(kept mask, within, tau): the header's trimming rule, the select stated as a sort"""
    within = int(inl.sum())
    if trim == 1.0:
        return inl.copy(), within, float(d2)
    keep = int(float(trim) * float(within))
    if keep == 0:
        return np.zeros_like(inl), within, 0.0
    tau = np.sort(sqd[inl])[keep - 1]
    return inl & (sqd <= tau), within, float(tau)


# ---- the sums ----------------------------------------------------------------------------------------------------------

def sums(method, src, tgt, aux, T, max_distance, o, loss, scale, trim):
    """aux: the target's normals (PLANE), (cs, ct) (GENERALIZED), None (POINT). Returns (S, within, tau)."""
    q = im.transform(T, src)
    j, sqd = im.nearest(q, tgt)
    d2 = np.float64(max_distance) * np.float64(max_distance)
    inl = (j >= 0) & (sqd <= d2)
    kept, within, tau = trim_threshold(sqd, inl, trim, d2)
    b = tgt[j]
    with np.errstate(all="ignore"):
        if method == POINT:
            t = im.point_terms(q, b, sqd, o)
            w = weight(loss, sqd, scale)
            terms = np.concatenate([t[:, :1], w[:, None] * t[:, 1:16], w[:, None], t[:, 16:17]], axis=1)
        else:
            if method == PLANE:
                terms = im.plane_terms(q, b, aux[j], sqd, o)
            else:
                terms, _ = gm.generalized_terms(q, b, aux[0], aux[1][j], T, sqd, o)
            w = weight(loss, terms[:, 28], scale)
            terms[:, 1:29] = w[:, None] * terms[:, 1:29]
    terms[~kept] = 0.0
    return im.fold(terms), within, tau


def step_point_by(S, n, o):
    """icp_rules.hpp's icp_step_point_by: icp_model.step_point with the centroids divided by n (0 / 0 is not a number)"""
    with np.errstate(all="ignore"):
        n = np.float64(n)
        mq = [float(np.float64(S[1 + a]) / n) for a in range(3)]
        mb = [float(np.float64(S[4 + a]) / n) for a in range(3)]
    H = [S[7 + r * 3 + c] - S[4 + r] * mq[c] for r in range(3) for c in range(3)]
    R = im.rotation_from_cross_covariance(H)
    v = [mb[a] - ((R[a * 3 + 0] * mq[0] + R[a * 3 + 1] * mq[1]) + R[a * 3 + 2] * mq[2]) for a in range(3)]
    return im.about_origin(R, v, o), abs(im.det3(R) - 1.0) <= im.DET_TOL


# ---- the loop ----------------------------------------------------------------------------------------------------------

@dataclass
class Result:
    T: np.ndarray
    history: np.ndarray      # (max_iterations + 1) x 3: count, fitness, rmse over the kept points
    iterations: int
    status: int
    count: int
    fitness: float
    rmse: float
    within: int              # of the last history row: the points within max_distance before trimming
    trim_sqd: float          # tau of the last row: max_distance^2 untrimmed, 0 when nothing was kept
    weight_sum: float        # sum w of the last row (point-to-point; 0 otherwise)


def icp_robust(src, tgt, T_init=None, method=POINT, normals=None, covariances=None, max_distance=0.1, max_iterations=30,
               rel_fitness=1e-6, rel_rmse=1e-6, loss=NONE, scale=0.0, trim=1.0) -> Result:
    """method POINT / PLANE (normals) / GENERALIZED (covariances = (cs, ct), n x 6 each)"""
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    aux = normals if method == PLANE else None
    if method == GENERALIZED:
        aux = (np.ascontiguousarray(covariances[0], np.float64), np.ascontiguousarray(covariances[1], np.float64))
    T = np.eye(4) if T_init is None else np.array(T_init, np.float64)
    o = im.origin(tgt)
    ol = [float(x) for x in o]
    hist = np.zeros((max_iterations + 1, 3))
    prev = (0.0, 0.0)
    k = 0
    while True:
        S, within, tau = sums(method, src, tgt, aux, T, max_distance, o, loss, scale, trim)
        cnt = S[0]
        fitness = cnt / float(len(src))
        rmse = math.sqrt(S[-1] / cnt) if cnt > 0.0 else 0.0
        hist[k] = (cnt, fitness, rmse)
        status = None
        if k >= 1 and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            status = im.CONVERGED
        elif cnt < MIN_COUNT[method]:
            status = im.TOO_FEW
        elif k >= max_iterations:
            status = im.MAX_ITERATIONS
        else:
            dT, ok = step_point_by(S, S[WEIGHT_SUM], ol) if method == POINT else im.step_plane(S, ol)
            N = im.compose(dT, T) if dT is not None else None
            if ok and np.all(np.isfinite(N)):
                T = N
            else:
                status = im.DEGENERATE
        prev = (fitness, rmse)
        if status is not None:
            return Result(T, hist, k, status, int(cnt), fitness, rmse, within, tau,
                          S[WEIGHT_SUM] if method == POINT else 0.0)
        k += 1


# ---- the shared cluttered case -----------------------------------------------------------------------------------------

def cluttered(seed=0, deg=2.0, shift=0.01, n_src=300, n_clutter=200):
    """the recipe's close start with clutter: n_clutter points uniform in the target's bounding box, moved by the inverse
    of T_true and appended to the source. Returns (src, tgt, T_true)."""
    src, tgt, T_true = im.recipe(n_src=n_src, deg=deg, shift=shift, noise=0.001, seed=seed)
    rng = np.random.default_rng(100 + seed)
    c = rng.uniform(tgt.min(axis=0), tgt.max(axis=0), (n_clutter, 3))
    Ti = np.linalg.inv(T_true)
    c = c @ Ti[:3, :3].T + Ti[:3, 3]
    return np.ascontiguousarray(np.concatenate([src, c])), tgt, T_true
