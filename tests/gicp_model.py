"""TEST INFRASTRUCTURE — the model clipper_hip_estimate_covariances / clipper_hip_icp_generalized are held to: the
generalized part of clipper_amd/csrc/icp_rules.hpp restated in numpy on top of tests/icp_model.py (its transform,
nearest, fold, step_plane, compose and loop rules) and tests/features_model.py (the neighbourhood and its covariance).

Every expression is written in the header's order with nothing fused: the 3 x 3 Jacobi of the smallest eigenvector runs
on Python floats (IEEE doubles with +, -, *, /, sqrt only), the 30 terms of a pair are numpy element-wise operations over
all pairs at once, so the model gives the device's bits. Clouds are n x 3, covariances n x 6 (xx, xy, xz, yy, yz, zz),
T is a 4 x 4 numpy matrix."""
from __future__ import annotations

import math

import numpy as np

from tests import features_model as fm
from tests import icp_model as im

GENERALIZED = 2
MIN_COUNT = 3
MAX_SWEEPS, JACOBI_TOL = 16, 1e-16


# ---- the covariance of a point ---------------------------------------------------------------------------------------

def _rotation(apq, app, aqq):
    """sdp_rules.hpp's sdp_rotation"""
    c, s, tn = 1.0, 0.0, 0.0
    if apq != 0.0:
        theta = (aqq - app) / (2.0 * apq)
        at = abs(theta)
        tn = 0.5 / at if at > 1e150 else 1.0 / (at + math.sqrt(theta * theta + 1.0))
        if theta < 0.0:
            tn = -tn
        c = 1.0 / math.sqrt(tn * tn + 1.0)
        s = tn * c
    return c, s, tn


def _rotate(app, aqq, apq, arp, arq, vp, vq):
    """features_rules.hpp's feat_rotate: returns (app, aqq, apq, arp, arq); vp and vq turn in place"""
    c, s, tn = _rotation(apq, app, aqq)
    app = app - tn * apq
    aqq = aqq + tn * apq
    rp, rq = arp, arq
    arp = c * rp - s * rq
    arq = s * rp + c * rq
    for k in range(3):
        x, y = vp[k], vq[k]
        vp[k] = c * x - s * y
        vq[k] = s * x + c * y
    return app, aqq, 0.0, arp, arq


def smallest_eigenvector(C):
    """features_rules.hpp's feat_smallest_eigenvector of the symmetric 3 x 3 C, statement for statement: the unit
    eigenvector of the smallest eigenvalue by cyclic Jacobi, no sign rule"""
    a00, a01, a02, a11, a12, a22 = (float(C[0][0]), float(C[0][1]), float(C[0][2]), float(C[1][1]), float(C[1][2]),
                                    float(C[2][2]))
    v0, v1, v2 = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
    for _ in range(MAX_SWEEPS):
        off = 2.0 * ((a01 * a01 + a02 * a02) + a12 * a12)
        whole = ((a00 * a00 + a11 * a11) + a22 * a22) + off
        if not off > JACOBI_TOL * JACOBI_TOL * whole:
            break
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12, v0, v1)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12, v0, v2)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02, v1, v2)
    pick1 = a11 < a00
    best = a11 if pick1 else a00
    nv = list(v1 if pick1 else v0)
    if a22 < best:
        nv = list(v2)
    ln = math.sqrt((nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2])
    return [nv[0] / ln, nv[1] / ln, nv[2] / ln]


def covariance_of_normal(nv, epsilon):
    """C = I - (1 - epsilon) nv nv^T as (xx, xy, xz, yy, yz, zz); nv: (..., 3)"""
    nv = np.asarray(nv, np.float64)
    w = np.float64(1.0) - np.float64(epsilon)
    x, y, z = nv[..., 0], nv[..., 1], nv[..., 2]
    return np.stack([1.0 - w * (x * x), 0.0 - w * (x * y), 0.0 - w * (x * z), 1.0 - w * (y * y), 0.0 - w * (y * z),
                     1.0 - w * (z * z)], axis=-1)


def covariances(P, knn=20, radius=0.0, epsilon=1e-3):
    """Returns (C n x 6, cnt n, N n x 3): the regularised covariance of every point over features_model's
    neighbourhood, the neighbours kept, and the normal it was made from ((0, 0, 0) with the identity below 3)"""
    P = np.asarray(P, np.float64)
    idx, _, _, cnt = fm.neighborhoods(P, knn, radius)
    N = np.zeros((len(P), 3))
    C = np.tile(np.array([1.0, 0.0, 0.0, 1.0, 0.0, 1.0]), (len(P), 1))
    for i in range(len(P)):
        if cnt[i] < 3:
            continue
        N[i] = smallest_eigenvector(fm.covariance(P[idx[i, :cnt[i]]]))
        C[i] = covariance_of_normal(N[i], epsilon)
    return C, cnt, N


def full(C):
    """n x 6 -> n x 3 x 3"""
    C = np.asarray(C, np.float64)
    return np.stack([np.stack([C[..., 0], C[..., 1], C[..., 2]], -1), np.stack([C[..., 1], C[..., 3], C[..., 4]], -1),
                     np.stack([C[..., 2], C[..., 4], C[..., 5]], -1)], -2)


# ---- the terms of the pairs ------------------------------------------------------------------------------------------

def generalized_terms(q, b, ca, cb, T, sqd, o):
    """icp_rules.hpp's icp_generalized_terms over m pairs at once: q, b m x 3; ca, cb m x 6 -> m x 30"""
    R = [[np.float64(T[r, c]) for c in range(3)] for r in range(3)]
    A = [[ca[:, 0], ca[:, 1], ca[:, 2]], [ca[:, 1], ca[:, 3], ca[:, 4]], [ca[:, 2], ca[:, 4], ca[:, 5]]]
    with np.errstate(all="ignore"):
        X = [[(R[r][0] * A[0][c] + R[r][1] * A[1][c]) + R[r][2] * A[2][c] for c in range(3)] for r in range(3)]

        def y(r, c):
            return (X[r][0] * R[c][0] + X[r][1] * R[c][1]) + X[r][2] * R[c][2]

        s00, s01, s02 = cb[:, 0] + y(0, 0), cb[:, 1] + y(0, 1), cb[:, 2] + y(0, 2)
        s11, s12, s22 = cb[:, 3] + y(1, 1), cb[:, 4] + y(1, 2), cb[:, 5] + y(2, 2)
        k00, k01, k02 = s11 * s22 - s12 * s12, s02 * s12 - s01 * s22, s01 * s12 - s02 * s11
        k11, k12, k22 = s00 * s22 - s02 * s02, s01 * s02 - s00 * s12, s00 * s11 - s01 * s01
        det = (s00 * k00 + s01 * k01) + s02 * k02
        m00, m01, m02, m11, m12, m22 = k00 / det, k01 / det, k02 / det, k11 / det, k12 / det, k22 / det
        M = [np.stack(row, axis=1) for row in ((m00, m01, m02), (m01, m11, m12), (m02, m12, m22))]
        qo, d = q - o, q - b
        G = [np.concatenate([im.cross(qo, M[r]), M[r]], axis=1) for r in range(3)]           # M J, row by row: m x 6
        H = np.zeros((len(q), 6, 6))
        for j in range(6):
            g = np.stack([G[0][:, j], G[1][:, j], G[2][:, j]], axis=1)
            H[:, :3, j] = im.cross(qo, g)
            H[:, 3:, j] = g
        e = np.stack([im.dot(M[0], d), im.dot(M[1], d), im.dot(M[2], d)], axis=1)
        x = im.cross(qo, e)
        cols = [np.ones(len(q))] + [H[:, i, j] for i in range(6) for j in range(i, 6)]
        cols += [x[:, a] for a in range(3)] + [e[:, a] for a in range(3)] + [im.dot(d, e), sqd]
    return np.stack(cols, axis=1), det


def sums(src, cs, tgt, ct, T, max_distance, o):
    """the 30 sums under T in the header's order of addition, the correspondences and the smallest det among the inliers"""
    q = im.transform(T, src)
    j, sqd = im.nearest(q, tgt)
    d2 = np.float64(max_distance) * np.float64(max_distance)
    inl = (j >= 0) & (sqd <= d2)
    terms, det = generalized_terms(q, tgt[j], cs, ct[j], T, sqd, o)
    terms[~inl] = 0.0
    return im.fold(terms), np.where(inl, j, -1).astype(np.int32), (float(det[inl].min()) if inl.any() else math.inf)


# ---- the loop: tests/icp_model.py's, with the sums above and the 6 x 6 step ----------------------------------------------

def icp_generalized(src, cs, tgt, ct, T_init=None, max_distance=0.1, max_iterations=30, rel_fitness=1e-6,
                    rel_rmse=1e-6) -> im.Result:
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    cs, ct = np.ascontiguousarray(cs, np.float64), np.ascontiguousarray(ct, np.float64)
    T = np.eye(4) if T_init is None else np.array(T_init, np.float64)
    o = im.origin(tgt)
    ol = [float(x) for x in o]
    hist = np.zeros((max_iterations + 1, 3))
    prev = (0.0, 0.0)
    min_det = math.inf
    k = 0
    while True:
        S, corr, det = sums(src, cs, tgt, ct, T, max_distance, o)
        min_det = min(min_det, det)
        cnt = S[0]
        fitness = cnt / float(len(src))
        rmse = math.sqrt(S[-1] / cnt) if cnt > 0.0 else 0.0
        hist[k] = (cnt, fitness, rmse)
        status = None
        if k >= 1 and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            status = im.CONVERGED
        elif cnt < MIN_COUNT:
            status = im.TOO_FEW
        elif k >= max_iterations:
            status = im.MAX_ITERATIONS
        else:
            dT, ok = im.step_plane(S, ol)
            N = im.compose(dT, T) if dT is not None else None
            if ok and np.all(np.isfinite(N)):
                T = N
            else:
                status = im.DEGENERATE
        prev = (fitness, rmse)
        if status is not None:
            r = im.Result(T, hist, k, status, int(cnt), fitness, rmse, corr)
            r.min_det = min_det
            return r
        k += 1
