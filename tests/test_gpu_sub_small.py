"""The selection a real solve makes for its live sub-problem, read back (clipper_hip_debug_sub_last) and compared with
tests/subproblem_model.py on the matrix the context stores — at the smallest sizes at which a solve hands itself over once
the size threshold is out of the way (clipper_hip_debug_sub_min_m; set_row_view(2) keeps the resident solver off the view).

The exactness of the hand-over rests on two integer facts: cnt[c] is at least the stored entries of column
c among the view's rows, and the N the decision is given — max(1, ncol) + (nS - view rows) — is at least the stored entries
any column outside S has among the rows of S. Both are asserted here on the pattern itself; the whole solves are compared
with the oracle and with each other under the tolerances of tests/test_gpu_subproblem.py.

The pinned cases (found on the device by stepping m up from RV_MIN_M = 3000; DESIGN.md §3e holds what each one read):
below m = 3000 no view exists; at m = 3000 one of eight Euclidean problems builds one (rho = 0.7); from m = 4000 on every
one does and nearly all hand themselves over; PointNormal problems end within 18 passes and build no view below m = 8000.
The dense fp32 store needs nS >= 1024 and 3 nS <= m, that is rho = 0.7: those problems run many trials at d ~ 3e4 and their
trial count moves with the order of the sums on every route, the views alone included (m = 3500, seed 1: 219 trials on the
views, 198 with the sub-problem, 190 in the oracle), so the dense case is one on which the routes agree.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth
from tests import subproblem_model as sm
from tests.test_gpu_subproblem import _oracle, _same_list

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _no_size_threshold():
    abi.debug_sub_min_m(1)
    yield
    abi.debug_sub_min_m(0)


def _problem(kind, m, rho, seed):
    if kind == "pointnormal":
        return synth.make_pointnormal_problem(m, rho, seed=seed), {}
    return synth.make_euclidean_problem(m, rho, seed=seed), synth.EUCLID_BENCH_PARAMS


def _solve(p, prm, kind, storage, route):
    g = abi.HipClipper(storage=storage)
    g.set_row_view(2)                                          # views, but never the resident solver on one
    g.set_subproblem({"views": 1, "sub": 0, "sub_slices": 2}[route])
    if kind == "pointnormal":
        g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, **prm)
    else:
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **prm)
    s = g.solve(p.u0)
    return g, s, g.view_stats()


def _needed_N(pattern, flags):
    """the most stored entries a column outside S has among the rows of S"""
    S = np.asarray(flags[:pattern.shape[0]], dtype=bool)
    return 0 if S.all() else int(pattern[S][:, ~S].sum(axis=0).max())


def _assert_selection(L, pattern):
    """the read-back against the model on the stored pattern, and the premise of the exactness argument"""
    m = pattern.shape[0]
    rows = L["rows"]
    need = _needed_N(pattern, L["flags"])
    print(f"  view {len(rows)} rows, s = {L['s']:.6f}: nS {L['nS']}, ncol {L['ncol']}, n0 {L['n0']}, entries {L['entries']}, "
          f"N_used {L['N_used']:.0f} (the matrix needs {need})")
    assert L["N_used"] == max(1, L["ncol"]) + L["nS"] - len(rows)
    assert L["N_used"] >= need, (L["N_used"], need)
    assert np.all(L["cnt"][:m] >= pattern[rows].sum(axis=0))
    want = sm.select(pattern, rows, L["s"])
    assert L["mp"] == want["mp"] and L["nrows"] == len(rows)
    for k in ("cnt", "flags", "colmap", "pos"):
        assert L[k].shape == want[k].shape and np.array_equal(L[k].astype(np.int64), want[k].astype(np.int64)), k
    for k in ("nS", "ncol", "n0", "entries"):
        assert L[k] == want[k], (k, L[k], want[k])


# (kind, m, rho, seed, dense): dense = the sub-problem is kept as a dense fp32 store under STORE_F32_CSC
CASES = [("euclidean", 3000, 0.7, 1, 0),      # the smallest: 877 view rows, S of 920 (< 1024: slices)
         ("euclidean", 4000, 0.7, 4, 1),      # S of 1237, mostly non-zero, 3 nS <= m: the dense store
         ("euclidean", 4000, 0.95, 2, 0),     # a thin view (200 rows), S a quarter larger
         ("euclidean", 4500, 0.8, 1, 0),      # most passes run on the sub-problem
         ("euclidean", 5000, 0.95, 1, 0),     # the decision hands the solve back once and over again
         ("pointnormal", 8000, 0.97, 2, 0)]   # the smallest PointNormal problem found that builds a view at all


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
@pytest.mark.parametrize("kind,m,rho,seed,dense", CASES)
def test_the_selection_of_a_small_solve(kind, m, rho, seed, dense, storage):
    p, prm = _problem(kind, m, rho, seed)
    sr = _oracle(p, pointnormal=(kind == "pointnormal"), **prm)   # (one CPU solve per problem: the storages share it)
    g0, s0, st0 = _solve(p, prm, kind, storage, "views")
    g1, s1, st1 = _solve(p, prm, kind, storage, "sub")
    g2, s2, st2 = _solve(p, prm, kind, storage, "sub_slices")
    print(f"{kind} m={m} rho={rho} seed={seed} storage={storage}: view {st1.rows} rows, sub-problem of {st1.sub_rows}, "
          f"{st1.sub_entries} hand-overs, {st1.sub_leaves} back, {st1.sub_passes} of {st1.passes} passes on it (dense {st1.sub_dense}); "
          f"trials {s1.n_trials} / views {s0.n_trials} / slices {s2.n_trials} / oracle {sr.n_trials}")
    assert st0.sub_entries == 0 and st0.sub_passes == 0
    for st in (st1, st2):
        assert st.sub_entries >= 1 and st.sub_passes > 0, "the solve never ran on the sub-problem"
    assert st2.sub_dense == 0 and st1.sub_dense == (dense if storage == abi.STORE_F32_CSC else 0)
    pattern = g1.get_constraint_matrix() != 0
    np.fill_diagonal(pattern, False)
    for g, s, st in ((g1, s1, st1), (g2, s2, st2)):
        L = g.debug_sub_last()
        assert L["built"] and L["entered"] and L["nS"] == st.sub_rows
        _assert_selection(L, pattern)
        if st.sub_leaves == 0:
            assert np.all(s.u[L["flags"][:m] == 0] == 0.0)     # exactly zero outside S
    with pytest.raises(abi.ClipperError):
        g0.debug_sub_last()                                    # (no selection on the route without the sub-problem)
    # the three routes against the oracle and each other (the tolerances of tests/test_gpu_subproblem.py)
    for s in (s0, s1, s2):
        _same_list(s, sr)
        assert abs(s.score - sr.score) <= 1e-6 * abs(sr.score)
        assert s.ifinal == sr.ifinal
    for s in (s1, s2):
        assert abs(s.score - s0.score) <= 1e-10 * abs(s0.score)
        assert np.allclose(s.u, s0.u, rtol=0, atol=1e-7)
        assert np.allclose(s.u, sr.u, rtol=0, atol=1e-7)
        assert abs(s.n_trials - s0.n_trials) <= max(3, s0.n_trials // 20), (s.n_trials, s0.n_trials, sr.n_trials)
        assert abs(s.n_trials - sr.n_trials) <= max(4, sr.n_trials // 10), (s.n_trials, s0.n_trials, sr.n_trials)
    # the same context solves again: the same bits, the same selection
    L1 = g1.debug_sub_last()
    s1b = g1.solve(p.u0)
    assert np.array_equal(s1b.u, s1.u) and s1b.n_trials == s1.n_trials and s1b.nodes.tolist() == s1.nodes.tolist()
    L1b = g1.debug_sub_last()
    assert all(np.array_equal(L1[k], L1b[k]) for k in ("cnt", "flags", "colmap", "pos", "rows")) and L1["s"] == L1b["s"]
    for g in (g0, g1, g2):
        g.close()


_CHILD = r"""
import sys, json
import numpy as np
sys.path.insert(0, {root!r})
from clipper_amd import _abi as abi
from clipper_amd import synth
from tests import subproblem_model as sm
p = synth.make_euclidean_problem({m}, {rho}, seed={seed})
g = abi.HipClipper(storage=abi.STORE_F32_CSC)
g.set_row_view(2)
g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
s = g.solve(p.u0)
st = g.view_stats()
L = g.debug_sub_last()
pattern = g.get_constraint_matrix() != 0
np.fill_diagonal(pattern, False)
want = sm.select(pattern, L["rows"], L["s"])
S = L["flags"][:{m}] != 0
need = int(pattern[S][:, ~S].sum(axis=0).max())
print(json.dumps(dict(nodes=s.nodes.tolist(), score=s.score, ifinal=s.ifinal, trials=s.n_trials, entries=st.sub_entries,
                      leaves=st.sub_leaves, sub_passes=st.sub_passes, built=L["built"], entered=L["entered"],
                      lists_equal=[bool(np.array_equal(L[k].astype(np.int64), want[k].astype(np.int64))) for k in ("cnt", "flags", "colmap", "pos")],
                      record=[[L[k], want[k]] for k in ("nS", "ncol", "n0", "entries")], nrows=L["nrows"],
                      N_used=L["N_used"], need=need)))
"""


def test_the_selection_after_a_hand_back_and_a_second_hand_over():
    """CLIPPER_HIP_SUB_TEST_LEAVE = 2 (read once per process: a fresh child): the second launch after every hand-over is
    told that a column outside the sub-problem could come back to life; the solve is handed back, runs the pending pass on
    the view and is handed over again. What the read-back reports afterwards is still the model's selection for the rows it
    reports. CLIPPER_HIP_SUBPROBLEM_MIN_M in the child's environment: the threshold's initial value."""
    m, rho, seed = 4000, 0.9, 1
    res = {}
    for k in ("0", "2"):
        e = dict(os.environ, CLIPPER_HIP_SUBPROBLEM_MIN_M="1", CLIPPER_HIP_SUB_TEST_LEAVE=k)
        out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, m=m, rho=rho, seed=seed)], env=e,
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        res[k] = json.loads(out.stdout.strip().splitlines()[-1])
    base, dist = res["0"], res["2"]
    print({k: {f: r[f] for f in ("entries", "leaves", "sub_passes", "trials", "nrows", "record", "N_used", "need")} for k, r in res.items()})
    assert base["entries"] == 1 and base["leaves"] == 0
    assert dist["leaves"] >= 1 and dist["entries"] >= 2, dist
    for r in (base, dist):
        assert r["built"] and r["entered"] and all(r["lists_equal"]) and all(a == b for a, b in r["record"])
        assert r["N_used"] == max(1, r["record"][1][0]) + r["record"][0][0] - r["nrows"] and r["N_used"] >= r["need"]
    assert sorted(dist["nodes"]) == sorted(base["nodes"]) and dist["ifinal"] == base["ifinal"]
    assert abs(dist["score"] - base["score"]) <= 1e-10 * abs(base["score"])
