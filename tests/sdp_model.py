"""Sequential CPU model of the semidefinite relaxation solver, written from the specification
alone. numpy fp64; numpy.linalg.eigh stands in for the device's Jacobi eigensolver.

Problem (only the lower triangle of M and C is read, and taken as symmetric):

    maximize <M, X>  s.t.  tr X = 1,  X psd,  X_ij = 0 where C_ij = 0,  X_ij >= 0 elsewhere

ADMM on the split X = Z, X in the spectraplex S, Z in the polyhedral set P, scaled dual U:

    X+ = proj_S(Z - U + M / rho)        eigendecompose, project the eigenvalues onto the simplex, rebuild
    Z+ = proj_P(X+ + U)                 0 where C = 0, max(., 0) elsewhere
    U+ = U + X+ - Z+

  solve(M, C, ...)      the iteration, the stopping rule and the rounding; returns a dict of the sdp::Solution
                        fields plus the certificate (d, Y, r_prim, r_dual, rho, converged, timed_out)
  symmetric_lower(A)    the symmetric matrix the lower triangle of A stands for
  project_simplex(v)    Euclidean projection onto {x >= 0, sum x = 1}
"""
from __future__ import annotations

import numpy as np

RHO0 = 1.0          # the initial penalty
ADAPT_EVERY = 10    # residual balancing: checked every ADAPT_EVERY iterations at first ...
ADAPT_MU = 10.0     # ... when one residual exceeds ADAPT_MU times the other ...
ADAPT_TAU = 2.0     # ... rho is multiplied or divided by ADAPT_TAU (and U divided or multiplied);
# the interval between checks doubles each time a move reverses the last one (up after down, down after up), so the
# penalty cannot cycle; a check that moves nothing changes neither the interval nor the remembered direction
ADAPT_MAX_EVERY = 1 << 30   # (the interval's cap)


def symmetric_lower(A: np.ndarray) -> np.ndarray:
    A = np.asarray(A, dtype=np.float64)
    L = np.tril(A)
    return L + np.tril(A, -1).T


def project_simplex(v: np.ndarray) -> np.ndarray:
    """tau: the largest k with v_(k) > (sum_{j<=k} v_(j) - 1) / k (v sorted descending); x = max(v - tau, 0).
    In exact arithmetic k = 1 always passes (v > v - 1). In fp64 it fails once v - 1 rounds back to v (v past 2^53) or
    v is not a number; then no k passes, and the projection is weight 1 on the first index of the largest entry (what
    a scan with a strict > from index 0 finds; a NaN gives way to the first number after it) and 0 elsewhere."""
    u = np.sort(v)[::-1]
    cs = np.cumsum(u)
    k = np.arange(1, v.size + 1)
    with np.errstate(invalid="ignore"):
        ok = u > (cs - 1.0) / k
    if not ok.any():
        top = 0
        for j in range(1, v.size):
            if v[j] > v[top] or (np.isnan(v[top]) and not np.isnan(v[j])):
                top = j
        x = np.zeros(v.size)
        x[top] = 1.0
        return x
    K = int(k[ok][-1])
    tau = (cs[K - 1] - 1.0) / K
    return np.maximum(v - tau, 0.0)


def tolerances(n, eps_abs, eps_rel, X, Z, U, rho):
    """Boyd's stopping tolerances for a variable of n * n entries."""
    e_pri = n * eps_abs + eps_rel * max(np.linalg.norm(X), np.linalg.norm(Z))
    e_dual = n * eps_abs + eps_rel * rho * np.linalg.norm(U)
    return e_pri, e_dual


def solve(M, C, max_iters=2000, eps_abs=1e-3, eps_rel=1e-3):
    """The device solver's iteration (the time limit aside, which the model has no use for)."""
    M = symmetric_lower(M)
    mask = symmetric_lower(np.asarray(C, dtype=np.float64) != 0) != 0
    n = M.shape[0]
    dmask = np.diag(mask).astype(np.float64)
    if dmask.sum() == 0:
        raise ValueError("no diagonal entry of C is nonzero: the problem is infeasible")
    Z = np.diag(dmask / dmask.sum())
    U = np.zeros_like(M)
    X = Z.copy()
    Q = np.eye(n)
    mu = np.diag(Z).copy()
    rho = RHO0
    d = np.nan
    r_p = r_d = np.inf
    converged = False
    it = 0
    next_check, interval, last_dir = ADAPT_EVERY, ADAPT_EVERY, 0
    while it < max_iters:
        W = Z - U + M / rho
        lam, Q = np.linalg.eigh(W)
        mu = project_simplex(lam)
        pos = mu > 0
        X = (Q[:, pos] * mu[pos]) @ Q[:, pos].T
        Zn = np.where(mask, np.maximum(X + U, 0.0), 0.0)
        U = U + X - Zn
        r_p = np.linalg.norm(X - Zn)
        r_d = rho * np.linalg.norm(Zn - Z)
        Z = Zn
        it += 1
        e_pri, e_dual = tolerances(n, eps_abs, eps_rel, X, Z, U, rho)
        if r_p <= e_pri and r_d <= e_dual:
            d = np.linalg.eigvalsh(M - rho * U)[-1]
            p = float(np.sum(M * X))
            if abs(d - p) <= eps_abs + eps_rel * max(abs(d), abs(p)):
                converged = True
                break
        if it == next_check:
            move = 1 if r_p > ADAPT_MU * r_d else (-1 if r_d > ADAPT_MU * r_p else 0)
            if move > 0:
                rho *= ADAPT_TAU
                U /= ADAPT_TAU
            elif move < 0:
                rho /= ADAPT_TAU
                U *= ADAPT_TAU
            if move != 0:
                if last_dir == -move and interval <= ADAPT_MAX_EVERY // 2:
                    interval *= 2
                last_dir = move
            next_check = it + interval
    if not converged:
        d = np.linalg.eigvalsh(M - rho * U)[-1]
    p = float(np.sum(M * X))
    # rounding (sdp.cpp:244-261); the eigenpairs of X are those of the last projection
    order = np.argsort(mu, kind="stable")
    lambdas = mu[order]
    top = int(np.argmax(mu))  # (the first of equal largest weights)
    evec1 = Q[:, top].copy()
    big = int(np.argmax(np.abs(evec1)))
    if evec1[big] < 0:
        evec1 = -evec1
    thr = float(np.max(np.abs(evec1)) / 2.0)
    nodes = [i for i in range(n) if abs(evec1[i]) > thr]
    return dict(X=X, Y=rho * U, Z=Z, lambdas=lambdas, evec1=evec1, thr=thr, nodes=nodes, iters=it,
                pobj=-p, dobj=-d, d=d, r_prim=r_p, r_dual=r_d, rho=rho, converged=converged, timed_out=False)
