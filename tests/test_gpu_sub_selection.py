"""The selection of the live sub-problem by itself (clipper_hip_debug_sub_select: exactly the launches a solve makes
between a view's build and the decision to build the sub-problem — k_sub_colcount, k_sub_flags, k_rv_scan / k_rv_scatter,
k_sub_publish) against tests/subproblem_model.py. Every comparison is an equality of integers; the pattern is the one
the context's own storage holds (get_constraint_matrix), so a count below the stored entries cannot hide.

The shapes are the smallest that reach an edge of the kernels (SL_W = 64 columns per group, four groups per workgroup
of k_sub_colcount, eight headers in flight; RV_BLK = 1024 associations per workgroup of k_sub_flags / k_rv_scatter):

  m = 64    40 random rows            one column group, one chunk
  m = 65    40 random rows            a second column group holding one real column; the c < mp store guard
  m = 257   one row                   five column groups: the second workgroup has one live wave; counts are 0 or 4
  m = 1025  every even row (513)      5 chunks; the second block of k_sub_flags holds one association
  m = 1153  the first 897/1024/1025   7, 8, 9 chunks: a short trip, a full trip, a second trip of one header (clamped index)
  m = 1153  all rows                  nothing outside the view: ncol = 0, S = everything
  m = 4097  the inliers; a random third   five blocks through k_rv_scan / k_rv_scatter; colmap ascending across block edges
"""
import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth
from tests import subproblem_model as sm

pytestmark = pytest.mark.gpu

_CTX = {}


@pytest.fixture(scope="module", autouse=True)
def _contexts():
    yield
    for g, _ in _CTX.values():
        g.close()
    _CTX.clear()


def _context(storage, m):
    """one context and its stored pattern per (storage, m): the cases share them"""
    if (storage, m) not in _CTX:
        p = synth.make_euclidean_problem(m, 0.5, seed=7000 + m)
        g = abi.HipClipper(storage=storage)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
        assert g.storage_in_use == storage
        pattern = g.get_constraint_matrix() != 0
        np.fill_diagonal(pattern, False)
        assert np.array_equal(pattern, pattern.T) and pattern.any()
        pattern.setflags(write=False)
        _CTX[(storage, m)] = (g, pattern)
    return _CTX[(storage, m)]


def _rows(m, what):
    rng = np.random.default_rng(100 + m)
    if what == "random40":
        return np.sort(rng.choice(m, 40, replace=False))
    if what == "one":
        return np.array([m - 3])   # (an inlier: its row has entries)
    if what == "even":
        return np.arange(0, m, 2)
    if what == "all":
        return np.arange(m)
    if what == "inliers":
        return np.arange(m - int(round(m * 0.5)), m)   # (synth: the outliers first, then the inliers)
    if what == "third":
        return np.sort(rng.choice(m, m // 3, replace=False))
    return np.arange(int(what))   # "897": the first 897 rows


def _assert_equals_model(got, want, pattern, rows):
    m = pattern.shape[0]
    assert got["mp"] == want["mp"] and got["nrows"] == len(rows)
    for k in ("cnt", "flags", "colmap", "pos"):   # cnt, flags, pos over all of [0, mp); colmap over [0, nS)
        assert got[k].shape == want[k].shape and np.array_equal(got[k].astype(np.int64), want[k].astype(np.int64)), k
    for k in ("nS", "ncol", "n0", "entries"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.all(got["cnt"][:m] >= pattern[rows].sum(axis=0))
    assert np.all(got["cnt"] % 4 == 0)


CASES = [(64, "random40"), (65, "random40"), (257, "one"), (1025, "even"), (1153, "897"), (1153, "1024"), (1153, "1025"),
         (1153, "all"), (4097, "inliers"), (4097, "third")]


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
@pytest.mark.parametrize("m,what", CASES)
def test_selection_equals_the_model(storage, m, what):
    g, pattern = _context(storage, m)
    rows = _rows(m, what)
    outside = np.setdiff1d(np.arange(m), rows)
    cnt0 = sm.select(pattern, rows, 0.0)["cnt"][:m]
    if outside.size:
        distinct = np.setdiff1d(np.unique(cnt0[outside]), [0])
        assert distinct.size, "no column outside the view has an entry in it: the case checks nothing"
        v = int(distinct[(distinct.size - 1) // 2])     # the median of the distinct positive counts outside the view
    else:
        v = int(np.median(np.unique(cnt0)))             # (all rows: nothing is outside, no threshold can move a column)
    s_out, s_in = float(np.sqrt((v + 0.5) / 0.4)), float(np.sqrt((v - 0.5) / 0.4))
    res = {}
    for s in (0.0, s_out, s_in, 5.0, 1e6):
        want = sm.select(pattern, rows, s)
        got = g.debug_sub_select(rows, s)
        _assert_equals_model(got, want, pattern, rows)
        assert got["s"] == s
        again = g.debug_sub_select(rows, s)
        for k in ("cnt", "flags", "colmap", "pos"):
            assert got[k].tobytes() == again[k].tobytes(), k
        assert {k: got[k] for k in ("nS", "ncol", "n0", "entries")} == {k: again[k] for k in ("nS", "ncol", "n0", "entries")}
        res[s] = got
    assert res[0.0]["n0"] == 0 and res[5.0]["n0"] == 10 and res[1e6]["n0"] == 2_000_000_000
    assert res[s_out]["n0"] == v and res[s_in]["n0"] == v - 1
    assert np.array_equal(np.flatnonzero(res[1e6]["flags"]), rows) and res[1e6]["nS"] == len(rows)   # S is the view
    assert np.array_equal(res[0.0]["flags"][:m] != 0, (cnt0 > 0) | np.isin(np.arange(m), rows))
    if outside.size:
        # the comparison is a strict >: the columns with exactly v entries stay out at n0 = v and join at n0 = v - 1
        moved = (res[s_in]["flags"] != 0) & (res[s_out]["flags"] == 0)
        assert moved.any() and np.all(cnt0[np.flatnonzero(moved)] == v)
        assert res[s_out]["ncol"] >= v
    else:
        assert all(r["nS"] == m and r["ncol"] == 0 for r in res.values())
    if m > 1024:
        cm = res[0.0]["colmap"]
        assert np.all(np.diff(cm) > 0) and cm[0] < 1024 <= cm[-1]   # ascending across the blocks' edges


def test_refusals_leave_the_context_usable():
    m = 257
    g, pattern = _context(abi.STORE_F32_CSC, m)
    rows = np.array([3, 77, 200])
    bad = [(np.array([5, 5]), 1.0), (np.array([9, 4]), 1.0), (np.array([-1, 4]), 1.0), (np.array([4, m]), 1.0),
           (rows, float("nan")), (rows, float("inf")), (rows, -1.0)]
    for r, s in bad:
        with pytest.raises(abi.ClipperError) as e:
            g.debug_sub_select(r, s)
        assert "rows must be ascending" in str(e.value) or "sum(u) must be finite" in str(e.value)
        got = g.debug_sub_select(rows, 2.0)
        _assert_equals_model(got, sm.select(pattern, rows, 2.0), pattern, rows)
    # no matrix; a dense storage
    p = synth.make_euclidean_problem(m, 0.5, seed=7000 + m)
    for storage in (abi.STORE_F32, abi.STORE_F64):
        d = abi.HipClipper(storage=storage)
        with pytest.raises(abi.ClipperError) as e:
            d.debug_sub_select(rows, 2.0)
        assert "needs slices" in str(e.value)
        d.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
        with pytest.raises(abi.ClipperError) as e:
            d.debug_sub_select(rows, 2.0)
        assert "needs slices" in str(e.value)
        with pytest.raises(abi.ClipperError):
            d.debug_sub_last()
        s = d.solve(p.u0)       # still a working context
        assert s.nodes.size > 0
        d.close()
    g2 = abi.HipClipper(storage=abi.STORE_F32_CSC)   # the slices storage, but nothing built yet
    with pytest.raises(abi.ClipperError) as e:
        g2.debug_sub_select(rows, 2.0)
    assert "needs slices" in str(e.value)
    g2.close()
    # a solve on the context the selections ran on: the view they left behind is not taken for a solve's
    sol = g.solve(p.u0)
    ref = abi.HipClipper(storage=abi.STORE_F32_CSC)
    ref.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    sol_ref = ref.solve(p.u0)
    assert np.array_equal(sol.u, sol_ref.u) and sol.nodes.tolist() == sol_ref.nodes.tolist()
    ref.close()
