"""The conditions on the degenerate cases (tests/degenerate_cases.py), checked on the CPU: what entitles
tests/test_gpu_degenerate.py to demand equality with the oracle.

Every case is solved by the C++ oracle under its three summation modes (the reference's order, reversed, extended
precision), by ref.numpy_solve and by the model below; all must agree on the selected list, ifinal and the trial count,
and u must be finite. A result that moved with the order of the additions could not be asked of a kernel that adds in
another order again. Each case must also show the property it is there for (degenerate_cases.Case.kind):
  uzero      at least one all-zero candidate is accepted; at every all-zero candidate reached from a non-zero u,
             max_i(u_i + alpha gradF_i) <= -1e-9: 1e7 ulps of an entry of a unit vector, so no order of the sums moves it
             across zero (a candidate from u == 0 has gradF == 0 exactly: 0 + alpha 0, no sum involved); u == 0, F == 0.0
  tiefill    round(F) exceeds the number of positive entries of u
  uniform    every entry of the final u is bit-equal
  edgeless   exactly one positive entry
  ccomplete  ifinal == 0: the penalty update finds no active constraint
The weighted cases are checked once more on the values an fp32 storage holds of them.
"""
import numpy as np
import pytest

from oracle import clipper_ref as ref
from tests import degenerate_cases as dc

MARGIN = -1e-9
WEIGHTED = ("tiefill", "uzero", "ccomplete")


def model_solve(mv, u0, p):
    """findDenseClique (clipper.cpp:172-323) restated on mv(x) -> (M_off x, C_off x), recording every candidate that the
    projection u + alpha gradF -> max(., 0) sends to the zero vector: (max_i(u_i + alpha gradF_i), u was already zero)"""
    def grad(x, d):
        a, b = mv(x)
        return (1 + d) * x - d * x.sum() + a + b * d

    def penalty(x, first):
        a, b = mv(x)
        Cbu = x.sum() - b - x
        idx = (Cbu > p.eps) & (x > p.eps)
        if not idx.any():
            return None
        q = (a + x)[idx] / Cbu[idx]
        return float(np.mean(q if first else np.abs(q)))

    u = mv(u0)[0] + u0 if p.rescale_u0 else u0.copy()
    u = u / np.linalg.norm(u)
    d = penalty(u, True) or 0.0
    F, trials, zeros, i = 0.0, 0, [], 0
    for i in range(p.maxoliters + 1):
        if i == p.maxoliters:
            break
        g = grad(u, d)
        F = float(u @ g)
        for _ in range(p.maxiniters):
            alpha, Fnew, dF = 1.0, 0.0, 0.0
            for _ in range(p.maxlsiters):
                t = u + alpha * g
                un = np.maximum(t, 0)
                z = float(un @ un)
                if z > 0:
                    un = un / np.sqrt(z)
                else:
                    zeros.append((float(t.max()), not u.any() and not g.any()))
                gn = grad(un, d)
                trials += 1
                Fnew = float(un @ gn)
                dF = Fnew - F
                if dF < -p.eps:
                    alpha *= p.beta
                else:
                    break
            du = float(np.linalg.norm(un - u))
            F, u, g = Fnew, un, gn
            if du < p.tol_u or abs(dF) < p.tol_F:
                break
        inc = penalty(u, False)
        if inc is None:
            break
        d += inc
    k = int(np.floor(F + 0.5)) if F >= 0 else -int(np.floor(-F + 0.5))
    return dict(nodes=ref.numpy_k_largest(u, k).tolist(), ifinal=i, trials=trials, u=u, F=F, k=k, zeros=zeros)


def _cases():
    out = []
    for c in dc.small_handed() + dc.small_points() + dc.large_handed() + dc.large_points():
        out.append(c)
        if c.kind in WEIGHTED:
            out.append(c.rounded_f32())
    return out


def _oracle_on(c):
    r = ref.RefClipper()
    if c.from_points:
        r.score_pairwise_consistency_euclidean(c.D1, c.D2, c.A, **dc.POINT_INV)
        if c.kind == "emptyrows":
            want = np.triu(r.get_affinity_matrix(), 1)
            e = c.groups[0]
            assert not want[e, :].any() and not want[:, e].any() and np.count_nonzero(want) > c.m
        else:
            want = dc.expected_point_matrix(c)
            assert np.array_equal(np.triu(r.get_affinity_matrix(), 1), want), "the scorer's matrix is not the stated one"
        assert np.array_equal(np.triu(r.get_constraint_matrix(), 1), (want != 0).astype(float))
        i, j, v = dc._lists(want)
        c = dc.Case(c.name, c.kind, c.m, c.u0, Mi=i, Mj=j, Mv=v, Ci=i, Cj=j, groups=c.groups)
    else:
        r.set_sparse_matrix_data(*c.upper_csc())
    return r, c


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c.name)
def test_case_is_stable_and_shows_its_property(case):
    r, c = _oracle_on(case)
    p = ref.Params()
    sols = []
    for mode in (0, 1, 2):
        r.set_sum_mode(mode)
        s = r.solve(c.u0)
        sols.append(dict(nodes=s.nodes.tolist(), ifinal=s.ifinal, trials=s.n_trials, u=s.u, F=s.score))
    sn = ref.numpy_solve(None, None, c.u0, p, matvec=c.matvec)
    sols.append(dict(nodes=sn.nodes.tolist(), ifinal=sn.ifinal, trials=sn.n_trials, u=sn.u, F=sn.score))
    mo = model_solve(c.matvec, c.u0, p)
    sols.append(mo)
    s0 = sols[0]
    tied = dc.tied_entries(s0["u"], s0["nodes"])
    for k, s in enumerate(sols):
        assert np.all(np.isfinite(s["u"])) and np.isfinite(s["F"]), k
        assert (sorted(s["nodes"]) == sorted(s0["nodes"])) if tied else (s["nodes"] == s0["nodes"]), (k, s["nodes"], s0["nodes"])
        assert s["ifinal"] == s0["ifinal"] and s["trials"] == s0["trials"], (k, s["ifinal"], s["trials"], s0["ifinal"], s0["trials"])
        assert abs(s["F"] - s0["F"]) <= 1e-9 * max(1.0, abs(s0["F"])) and np.max(np.abs(s["u"] - s0["u"]), initial=0.0) <= 1e-9
    u, nodes, npos = s0["u"], s0["nodes"], int(np.count_nonzero(s0["u"] > 0))
    if c.kind != "uniform":   # (there every entry is bit-equal by exact arithmetic, and the set is the tie rule's)
        assert dc.boundary_gap(u, nodes) > 2 * dc.U_TOL, "the selected set itself rests on rounding"
    line = f"{c.name}: m={c.m} trials={s0['trials']} ifinal={s0['ifinal']} nodes={len(nodes)} positive={npos} F={s0['F']:.6g} tied={tied}"
    if c.kind == "uzero":
        from_u = [mx for mx, was_zero in mo["zeros"] if not was_zero]
        assert from_u, "no all-zero candidate was accepted"
        assert max(from_u) <= MARGIN, from_u
        line += f" zero candidates={len(mo['zeros'])} margin={max(from_u):.3g}"
        for s in sols:
            assert not s["u"].any() and s["F"] == 0.0 and s["nodes"] == []
    else:
        assert not mo["zeros"], "an all-zero candidate in a case that is not there for it"
    if c.kind == "tiefill":
        assert mo["k"] > npos >= 1 and len(nodes) == mo["k"], (mo["k"], npos)
        line += f" round(F)={mo['k']}"
    if c.kind == "uniform":
        for s in sols:
            assert np.all(s["u"] == s["u"][0])
        assert sorted(nodes) == list(range(mo["k"]))   # the lowest indices: utils.cpp:33-55 replaces only on a larger value
    if c.kind == "edgeless":
        assert npos == 1 and len(nodes) == 1 and abs(s0["F"] - 1.0) <= 1e-12
    if c.kind == "complete":
        assert sorted(nodes) == list(range(c.m)) and s0["ifinal"] == 0
    if c.kind == "ccomplete":
        assert s0["ifinal"] == 0
    if c.kind in ("cliques", "cliques0") and min(len(g) for g in c.groups) > 1:
        want = c.groups[1 if c.kind == "cliques0" else 0]
        assert sorted(nodes) == want.tolist()
    if c.kind == "emptyrows":
        assert not u[c.groups[0]].any() and len(nodes) > 100
    if c.kind in ("star", "path"):
        assert len(nodes) == 2
    print(line)
