"""TEST INFRASTRUCTURE — the model clipper_hip_icp / clipper_hip_evaluate_registration are held to: the contract of
clipper_amd/csrc/icp_rules.hpp restated in numpy on top of oracle/bm_utils_ref.knn_bruteforce.

Every expression is written in the header's order with nothing fused, the per-point terms are added by the header's
halving tree (256 per partial, then partials t, t + 256, ... per lane, then the tree again), and the step (one-sided
Jacobi of the 3 x 3 cross-covariance; LDL^T of the 6 x 6 system and the Cayley map) runs on Python floats: IEEE
doubles with +, -, *, /, sqrt only, so the model gives the device's bits. Clouds are n x 3 (rows = points), T is a
4 x 4 numpy matrix. Also the shared recipe of tests/test_icp_model.py, tests/test_icp_rules.py and tests/test_gpu_icp.py."""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np

from oracle import bm_utils_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINT, PLANE = 0, 1
CONVERGED, MAX_ITERATIONS, TOO_FEW, DEGENERATE = 0, 1, 2, 3
BLOCK = 256
RANK_TOL, DET_TOL = 1e-10, 1e-9
MIN_COUNT = {POINT: 3, PLANE: 6}


# ---- the search: the K = 1 entry of the contract -------------------------------------------------------------------

def nearest_fast(Q, B, chunk=4096):
    """knn_bruteforce(Q, B, 1) for large clouds: the same distance ((0 + dx dx) + dy dy) + dz dz, the lowest index among
    equal distances (argmin returns the first minimum); checked against the oracle in tests/test_icp_model.py"""
    idx = np.empty(len(Q), np.int64)
    sqd = np.empty(len(Q))
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk]
        d2 = np.zeros((len(q), len(B)))
        for k in range(3):
            df = q[:, k, None] - B[None, :, k]
            d2 = d2 + df * df
        j = np.argmin(d2, axis=1)
        idx[s:s + chunk] = j
        sqd[s:s + chunk] = d2[np.arange(len(q)), j]
    return idx, sqd


def nearest(Q, B):
    if len(Q) * len(B) > 1 << 21:
        return nearest_fast(Q, B)
    idx, sqd = ref.knn_bruteforce(Q, B, 1)
    return idx[:, 0], sqd[:, 0]


# ---- the rules ---------------------------------------------------------------------------------------------------------

def transform(T, P):
    """q_a = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3, rows of P"""
    x, y, z = P[:, 0], P[:, 1], P[:, 2]
    return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def origin(B):
    return (B.min(axis=0) + B.max(axis=0)) * 0.5


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def point_terms(q, b, sqd, o):
    qo, bo = q - o, b - o
    cols = [np.ones(len(q))] + [qo[:, a] for a in range(3)] + [bo[:, a] for a in range(3)]
    cols += [bo[:, r] * qo[:, c] for r in range(3) for c in range(3)] + [sqd]
    return np.stack(cols, axis=1)


def plane_terms(q, b, n, sqd, o):
    qo, d = q - o, q - b
    J = np.concatenate([cross(qo, n), n], axis=1)
    r = dot(d, n)
    cols = [np.ones(len(q))] + [J[:, i] * J[:, j] for i in range(6) for j in range(i, 6)]
    cols += [J[:, i] * r for i in range(6)] + [r * r, sqd]
    return np.stack(cols, axis=1)


def tree(v):
    """v: (groups, 256, terms) -> (groups, terms): v[i] = v[i] + v[i + s], s = 128 .. 1"""
    v = v.copy()
    s = BLOCK // 2
    while s > 0:
        v[:, :s] = v[:, :s] + v[:, s:2 * s]
        s >>= 1
    return v[:, 0]


def fold(terms):
    """terms: (n_src, T), a non-inlier's row +0.0 -> the T sums in the header's order of addition"""
    n, T = terms.shape
    nb = -(-n // BLOCK)
    pad = np.zeros((nb * BLOCK, T))
    pad[:n] = terms
    part = tree(pad.reshape(nb, BLOCK, T))
    rounds = -(-nb // BLOCK)
    pp = np.zeros((rounds * BLOCK, T))
    pp[:nb] = part
    acc = np.zeros((BLOCK, T))
    for r in pp.reshape(rounds, BLOCK, T):
        acc = acc + r
    return [float(x) for x in tree(acc[None])[0]]


def det3(M):
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6])


def rotation_from_cross_covariance(H):
    """H, R: 9 floats row-major (icp_rules.hpp's function, statement for statement)"""
    A, V = list(H), [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for _ in range(60):
        offn = 0.0
        for p in range(2):
            for q in range(p + 1, 3):
                a = b = c = 0.0
                for i in range(3):
                    a += A[i * 3 + p] * A[i * 3 + p]
                    b += A[i * 3 + q] * A[i * 3 + q]
                    c += A[i * 3 + p] * A[i * 3 + q]
                rel = abs(c) / (math.sqrt(a * b) + 1e-300)
                offn = rel if offn < rel else offn
                if abs(c) <= 1e-300:
                    continue
                zeta = (b - a) / (2.0 * c)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
                cs = 1.0 / math.sqrt(1.0 + t * t)
                sn = cs * t
                for i in range(3):
                    ap, aq = A[i * 3 + p], A[i * 3 + q]
                    A[i * 3 + p] = cs * ap - sn * aq
                    A[i * 3 + q] = sn * ap + cs * aq
                    vp, vq = V[i * 3 + p], V[i * 3 + q]
                    V[i * 3 + p] = cs * vp - sn * vq
                    V[i * 3 + q] = sn * vp + cs * vq
        if offn < 1e-15:
            break
    s = [math.sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]) for j in range(3)]
    smallest, least = 0, s[0]
    for j in (1, 2):
        if s[j] < least:
            smallest, least = j, s[j]
    U = [0.0] * 9
    for j in range(3):
        for i in range(3):
            U[i * 3 + j] = A[i * 3 + j] / s[j] if s[j] > 1e-300 else 0.0
    if least <= 1e-300 * (s[0] + s[1] + s[2]) or least == 0.0:
        m, a, b = smallest, (smallest + 1) % 3, (smallest + 2) % 3
        U[0 * 3 + m] = U[1 * 3 + a] * U[2 * 3 + b] - U[2 * 3 + a] * U[1 * 3 + b]
        U[1 * 3 + m] = U[2 * 3 + a] * U[0 * 3 + b] - U[0 * 3 + a] * U[2 * 3 + b]
        U[2 * 3 + m] = U[0 * 3 + a] * U[1 * 3 + b] - U[1 * 3 + a] * U[0 * 3 + b]
    sgn = -1.0 if det3(U) * det3(V) < 0 else 1.0
    R = [0.0] * 9
    for i in range(3):
        for j in range(3):
            r = 0.0
            for k in range(3):
                r += U[i * 3 + k] * (sgn if k == smallest else 1.0) * V[j * 3 + k]
            R[i * 3 + j] = r
    return R


def about_origin(R, v, o):
    """x -> R (x - o) + o + v as a 4 x 4 list of rows"""
    dT = [[0.0] * 4 for _ in range(4)]
    for a in range(3):
        Ro = (R[a * 3 + 0] * o[0] + R[a * 3 + 1] * o[1]) + R[a * 3 + 2] * o[2]
        for c in range(3):
            dT[a][c] = R[a * 3 + c]
        dT[a][3] = v[a] + (o[a] - Ro)
    dT[3][3] = 1.0
    return dT


def step_point(S, o):
    n = S[0]
    mq = [S[1] / n, S[2] / n, S[3] / n]
    mb = [S[4] / n, S[5] / n, S[6] / n]
    H = [S[7 + r * 3 + c] - S[4 + r] * mq[c] for r in range(3) for c in range(3)]
    R = rotation_from_cross_covariance(H)
    v = [mb[a] - ((R[a * 3 + 0] * mq[0] + R[a * 3 + 1] * mq[1]) + R[a * 3 + 2] * mq[2]) for a in range(3)]
    return about_origin(R, v, o), abs(det3(R) - 1.0) <= DET_TOL


def cayley(w):
    a = [w[0] * 0.5, w[1] * 0.5, w[2] * 0.5]
    aa = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
    s = 2.0 / (1.0 + aa)
    K = [0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0]
    return [(1.0 if r == c else 0.0) + s * (K[r * 3 + c] + (a[r] * a[c] - (aa if r == c else 0.0)))
            for r in range(3) for c in range(3)]


def step_plane(S, o):
    A = [[0.0] * 6 for _ in range(6)]
    at = 1
    for i in range(6):
        for j in range(i, 6):
            A[i][j] = A[j][i] = S[at]
            at += 1
    big = A[0][0]
    for i in range(1, 6):
        big = A[i][i] if A[i][i] > big else big
    L = [[0.0] * 6 for _ in range(6)]
    D, y, x = [0.0] * 6, [0.0] * 6, [0.0] * 6
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = np.float64(A[j][j])          # (numpy scalars: a zero pivot divides to inf / nan as the device does)
            for k in range(j):
                d = d - L[j][k] * (L[j][k] * D[k])
            ok = ok and bool(d > RANK_TOL * big)
            D[j] = d
            for i in range(j + 1, 6):
                s = np.float64(A[i][j])
                for k in range(j):
                    s = s - L[i][k] * (L[j][k] * D[k])
                L[i][j] = s / d
        for i in range(6):
            s = np.float64(-S[22 + i])
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s
        for i in range(5, -1, -1):
            s = y[i] / D[i]
            for k in range(i + 1, 6):
                s = s - L[k][i] * x[k]
            x[i] = s
    if not ok:
        return None, False
    x = [float(t) for t in x]
    return about_origin(cayley(x[:3]), x[3:], o), True


def compose(dT, T):
    N = np.zeros((4, 4))
    for c in range(4):
        for r in range(3):
            v = (dT[r][0] * T[0, c] + dT[r][1] * T[1, c]) + dT[r][2] * T[2, c]
            N[r, c] = v + dT[r][3] if c == 3 else v
    N[3, 3] = 1.0
    return N


# ---- the loop ----------------------------------------------------------------------------------------------------------

@dataclass
class Result:
    T: np.ndarray
    history: np.ndarray      # (max_iterations + 1) x 3: count, fitness, rmse; rows never reached are 0
    iterations: int
    status: int
    count: int
    fitness: float
    rmse: float
    corr: np.ndarray         # of the last row: target index, -1 = no inlier


def sums(src, tgt, normals, T, method, max_distance, o):
    q = transform(T, src)
    j, sqd = nearest(q, tgt)
    d2 = np.float64(max_distance) * np.float64(max_distance)
    inl = (j >= 0) & (sqd <= d2)
    b = tgt[j]
    terms = plane_terms(q, b, normals[j], sqd, o) if method == PLANE else point_terms(q, b, sqd, o)
    terms[~inl] = 0.0
    return fold(terms), np.where(inl, j, -1).astype(np.int32)


def icp(src, tgt, T_init=None, method=POINT, normals=None, max_distance=0.1, max_iterations=30, rel_fitness=1e-6,
        rel_rmse=1e-6) -> Result:
    src, tgt = np.ascontiguousarray(src, np.float64), np.ascontiguousarray(tgt, np.float64)
    T = np.eye(4) if T_init is None else np.array(T_init, np.float64)
    o = origin(tgt)
    ol = [float(x) for x in o]
    hist = np.zeros((max_iterations + 1, 3))
    prev = (0.0, 0.0)
    k = 0
    while True:
        S, corr = sums(src, tgt, normals, T, method, max_distance, o)
        cnt = S[0]
        fitness = cnt / float(len(src))
        rmse = math.sqrt(S[-1] / cnt) if cnt > 0.0 else 0.0
        hist[k] = (cnt, fitness, rmse)
        status = None
        if k >= 1 and abs(fitness - prev[0]) < rel_fitness and abs(rmse - prev[1]) < rel_rmse:
            status = CONVERGED
        elif cnt < MIN_COUNT[method]:
            status = TOO_FEW
        elif k >= max_iterations:
            status = MAX_ITERATIONS
        else:
            dT, ok = step_plane(S, ol) if method == PLANE else step_point(S, ol)
            N = compose(dT, T) if dT is not None else None
            if ok and np.all(np.isfinite(N)):
                T = N
            else:
                status = DEGENERATE
        prev = (fitness, rmse)
        if status is not None:
            return Result(T, hist, k, status, int(cnt), fitness, rmse, corr)
        k += 1


def evaluate(src, tgt, T=None, max_distance=0.1):
    r = icp(src, tgt, T, POINT, None, max_distance, 0)
    return r.fitness, r.rmse, r.count, r.corr


# ---- the shared recipe -------------------------------------------------------------------------------------------------

def bunny_unit():
    P = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_points_4096.f32"), dtype="<f4").reshape(-1, 3).astype(np.float64)
    P = P - P.min(axis=0)
    return P / (P.max(axis=0)).max()


def rigid(deg, axis, t):
    """4 x 4 rotation by deg about axis, then the translation t"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def plane_normals(tgt, knn=12):
    """unit normals of the target for the point-to-plane runs: the smallest eigenvector of the covariance of the knn
    nearest points (numpy; the GPU tests and the model take the same array, so how it is made does not matter)"""
    idx, _ = ref.knn_bruteforce(tgt, tgt, knn)
    N = np.zeros_like(tgt)
    for i, nb in enumerate(idx):
        Q = tgt[nb] - tgt[nb].mean(axis=0)
        w, v = np.linalg.eigh(Q.T @ Q)
        N[i] = v[:, 0] / np.linalg.norm(v[:, 0])
    return N


def recipe(n_tgt=1025, n_src=300, deg=10.0, shift=0.05, noise=0.0, seed=0, offset=0.0):
    """the shared recipe: bunny in the unit cube, n_tgt target points, n_src of them as the source, the source moved by
    the inverse of (deg about (1, 2, 3), translation `shift` along (1, 1, 1) / sqrt 3), uniform noise +-noise on the
    source; offset: both clouds shifted by it. Returns (src, tgt, T_true): T_true moves the source onto the target."""
    rng = np.random.default_rng(seed)
    P = bunny_unit()
    tgt = P[rng.choice(len(P), n_tgt, replace=False)]
    pick = rng.choice(n_tgt, n_src, replace=n_src > n_tgt)
    T_true = rigid(deg, (1.0, 2.0, 3.0), np.full(3, shift / np.sqrt(3.0)))
    c = tgt.mean(axis=0)            # (rotate about the cloud's centre, so that `deg` alone sets the displacement)
    C = np.eye(4)
    C[:3, 3] = c
    Ci = np.eye(4)
    Ci[:3, 3] = -c
    T_true = C @ T_true @ Ci
    Ti = np.linalg.inv(T_true)
    src = tgt[pick] @ Ti[:3, :3].T + Ti[:3, 3]
    if noise > 0:
        src = src + rng.uniform(-noise, noise, src.shape)
    if offset:
        O = np.eye(4)
        O[:3, 3] = offset
        Oi = np.eye(4)
        Oi[:3, 3] = -offset
        T_true = O @ T_true @ Oi
        src, tgt = src + offset, tgt + offset
    return np.ascontiguousarray(src), np.ascontiguousarray(tgt), T_true


def transform_error(T_true, T):
    """(rotation error [rad], translation error) of T against the truth"""
    E = np.linalg.inv(T_true) @ T
    c = min(max((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0), 1.0)
    return abs(float(np.arccos(c))), float(np.linalg.norm(E[:3, 3]))
