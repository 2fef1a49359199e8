"""CPU checks of the sequential model of the semidefinite relaxation (tests/sdp_model.py):
known answers on perfect graphs, the certificate on random problems, the lower-triangle semantics."""
import numpy as np
import pytest

from tests import sdp_model as sm

TIGHT = dict(eps_abs=1e-7, eps_rel=1e-7, max_iters=20000)


def _clique_union(n, k, seed):
    """A disjoint union of cliques (a perfect graph: the relaxation is exact) with one largest clique K of size k."""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(n)
    K = sorted(perm[:k].tolist())
    A = np.zeros((n, n))
    A[np.ix_(K, K)] = 1
    i = k
    while i < n:
        s = int(min(rng.integers(1, max(2, k)), n - i))
        grp = perm[i:i + s]
        A[np.ix_(grp, grp)] = 1
        i += s
    np.fill_diagonal(A, 1.0)
    return A, K


def _random_problem(n, p, seed):
    rng = np.random.default_rng(seed)
    up = np.triu(rng.random((n, n)) < p, 1)
    M = np.where(up, rng.uniform(0.05, 1.0, (n, n)), 0.0)
    M = M + M.T + np.eye(n)
    return M, (M != 0).astype(float)


@pytest.mark.parametrize("n,k", [(1, 1), (7, 3), (33, 6), (64, 9), (100, 12), (128, 12)])
def test_known_answers_on_clique_unions(n, k):
    A, K = _clique_union(n, k, seed=n)
    r = sm.solve(A, A, **TIGHT)
    assert r["converged"]
    assert r["nodes"] == K
    assert r["pobj"] == pytest.approx(-k, abs=1e-5 * k)
    assert r["dobj"] == pytest.approx(-k, abs=1e-5 * k)


@pytest.mark.parametrize("seed", range(6))
def test_certificate_on_random_problems(seed):
    n = [12, 25, 40, 60, 90, 128][seed]
    M, C = _random_problem(n, [0.5, 0.3, 0.2, 0.15, 0.1, 0.08][seed], seed)
    eps = 1e-6
    r = sm.solve(M, C, eps_abs=eps, eps_rel=eps, max_iters=20000)
    assert r["converged"]
    X, Y = r["X"], r["Y"]
    p = float(np.sum(M * X))
    d = float(np.linalg.eigvalsh(M - Y)[-1])
    assert d == pytest.approx(r["d"], rel=1e-12, abs=1e-12)
    tol = eps + eps * max(abs(d), abs(p))
    assert d >= p - tol                          # weak duality, up to the primal residual
    assert abs(d - p) <= tol                     # the relative gap
    assert np.all(Y[C != 0] <= 0)                # Y is the dual of X_ij >= 0 where C != 0
    viol = np.sqrt(np.sum(np.where(C != 0, np.minimum(X, 0.0), X) ** 2))
    assert viol <= r["r_prim"] + 1e-15          # X leaves P by at most the reported residual
    assert abs(np.trace(X) - 1) < 1e-12 and np.linalg.eigvalsh(X)[0] > -1e-12
    assert np.all(np.diff(r["lambdas"]) >= 0) and abs(r["lambdas"].sum() - 1) < 1e-12
    assert r["evec1"][np.argmax(np.abs(r["evec1"]))] > 0
    assert r["thr"] == np.abs(r["evec1"]).max() / 2
    assert r["nodes"] == [i for i in range(n) if abs(r["evec1"][i]) > r["thr"]]


def test_lower_triangle_semantics():
    A, K = _clique_union(30, 5, seed=4)
    Mg, Cg = A.copy(), A.copy()
    iu = np.triu_indices(30, 1)
    rng = np.random.default_rng(9)
    Mg[iu] = rng.uniform(-5, 5, len(iu[0]))
    Cg[iu] = rng.integers(0, 2, len(iu[0]))
    r0 = sm.solve(A, A, **TIGHT)
    r1 = sm.solve(Mg, Cg, **TIGHT)
    assert np.array_equal(r0["X"], r1["X"]) and r0["nodes"] == r1["nodes"] and r0["iters"] == r1["iters"]
    Cz = A.copy()
    Cz[K[0], K[0]] = 0.0  # a zero C(i, i) is a zero constraint: X(i, i) = 0
    r2 = sm.solve(A, Cz, **TIGHT)
    assert abs(r2["X"][K[0], K[0]]) <= r2["r_prim"] + 1e-15
    assert r2["Z"][K[0], K[0]] == 0.0
    # the optimum is the clique K without i; d bounds it from above (X keeps a little weight next to i, within r_prim)
    assert r2["d"] >= len(K) - 1 - 1e-9 and abs(r2["pobj"] + (len(K) - 1)) < 0.1


def test_stop_rules_and_infeasible():
    M, C = _random_problem(40, 0.2, 1)
    r = sm.solve(M, C, max_iters=5, eps_abs=1e-12, eps_rel=1e-12)
    assert r["iters"] == 5 and not r["converged"]
    assert r["d"] == pytest.approx(np.linalg.eigvalsh(M - r["Y"])[-1])
    with pytest.raises(ValueError):
        sm.solve(np.zeros((3, 3)), np.zeros((3, 3)))


def test_project_simplex():
    rng = np.random.default_rng(0)
    for _ in range(20):
        v = rng.normal(size=rng.integers(1, 30)) * 3
        x = sm.project_simplex(v)
        assert abs(x.sum() - 1) < 1e-12 and np.all(x >= 0)
        # optimality: x = max(v - tau, 0) with one tau
        tau = (v - x)[x > 0]
        assert np.ptp(tau) < 1e-12 and np.all(v[x == 0] <= tau[0] + 1e-12)
    assert sm.project_simplex(np.array([2.0, 2.0, -1.0])).tolist() == [0.5, 0.5, 0.0]
