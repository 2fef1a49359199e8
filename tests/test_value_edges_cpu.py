"""The value-edge cases (tests/value_edges.py) on the CPU: what entitles tests/test_gpu_value_edges.py to ask for
equality. The ladder reaches every class of fp32 rounding and held() is the stored-value rule; every case carries every
rung and the two special columns; the oracle's two setters agree on every case; and the solve case "tinyedge"
discriminates: the oracle selects another node set once the entries that underflow in fp32 are gone, no result sits on
a tie, and none moves with the order of the additions."""
import numpy as np
import pytest

from oracle import clipper_ref as ref
from tests import degenerate_cases as dc
from tests import value_edges as ve

F32, F64 = ve.STORE_F32, ve.STORE_F64


def test_ladder_reaches_every_class_and_held_is_the_rule():
    classes = {name: ve.value_class(v) for name, v in ve.LADDER.items()}
    print(classes)
    assert set(classes.values()) == {"normal", "subnormal", "zero", "top"}
    for cls in ("subnormal", "zero", "top", "normal"):
        assert any(c == cls and ve.LADDER[n] < 0 for n, c in classes.items()), f"no negative rung of class {cls}"
    v = np.array(list(ve.LADDER.values()))
    for storage in (ve.STORE_F32, ve.STORE_F64, ve.STORE_F32_CSC, ve.STORE_F64_CSC):
        h = ve.held(v, storage)
        assert np.array_equal(ve.held(h, storage), h), "held is not idempotent"
        assert np.all(np.isfinite(h)) and np.array_equal(h != 0, v != 0) and np.array_equal(np.sign(h), np.sign(v))
    assert np.array_equal(ve.held(v, F64), v)
    h = dict(zip(ve.LADDER, ve.held(v, F32).tolist()))
    # written out by hand: the tie 2^-150 goes to even (zero, so FLT_MIN is kept), one ulp above it goes up to 2^-149;
    # FLT_MIN less a quarter of a subnormal step rounds back to FLT_MIN; the top rungs both round to FLT_MAX
    assert h["2^-150"] == ve.FLT_MIN and h["-2^-150"] == -ve.FLT_MIN and h["2^-150(1+2^-52)"] == ve.FLT_TRUE_MIN
    assert h["1e-50"] == h["1e-300"] == h["5e-324"] == ve.FLT_MIN and h["-1e-50"] == h["-5e-324"] == -ve.FLT_MIN
    assert h["2^-149"] == ve.FLT_TRUE_MIN and h["FLT_MIN"] == h["FLT_MIN(1-2^-25)"] == ve.FLT_MIN
    assert h["1e-40"] == 71362 * ve.FLT_TRUE_MIN and h["-1e-40"] == -h["1e-40"]      # round(1e-40 / 2^-149) = 71362
    assert h["FLT_MAX"] == h["FLT_MAX(1+2^-25)"] == ve.FLT_MAX and h["-FLT_MAX"] == -ve.FLT_MAX
    assert h["1"] == 1.0 and h["2.5"] == 2.5 and h["0.1"] == float(np.float32(0.1)) != 0.1
    assert ve.held(0.0, F32) == 0.0 and ve.held(1e39, F64) == 1e39


@pytest.mark.parametrize("case", ve.cases(), ids=lambda c: c.name)
def test_case_carries_the_ladder_and_the_oracles_setters_agree(case):
    c = case
    assert c.m in ve.SIZES and np.all(c.Mi < c.Mj) and np.all(c.Mv != 0) and np.all(np.isfinite(c.Mv))
    M, C = c.dense()
    lines = ve.edge_lines(c.m)
    # every rung, each on an edge line, every edge line with rungs of the class that rounds to zero or below FLT_MIN
    for name, v in ve.LADDER.items():
        assert c.rungs_at[name], name
        for i, j in c.rungs_at[name]:
            assert M[i, j] == v and (i in lines or j in lines)
    for p in lines:
        small = [abs(x) for x in M[p] if x != 0 and abs(x) < ve.FLT_MIN]
        assert small, f"no value below FLT_MIN on line {p}"
    # the two special columns
    z = M[:, ve.ZERO_COLUMN].copy()
    z[ve.ZERO_COLUMN] = 0
    assert np.count_nonzero(z) >= 5 and all(ve.value_class(x) == "zero" for x in z[z != 0])
    b = M[:, ve.BLOCK_COLUMN].copy()
    b[ve.BLOCK_COLUMN] = 0
    assert np.count_nonzero(b[:64]) >= 5 and all(ve.value_class(x) == "zero" for x in b[:64][b[:64] != 0])
    assert any(ve.value_class(x) == "normal" for x in b[64:][b[64:] != 0])
    # an ordinary background
    ordinary = (c.Mv >= 0.1) & (c.Mv < 1.0)
    assert 0.05 < np.count_nonzero(ordinary) / (c.m * (c.m - 1) / 2) < 0.15
    # C: the pattern of the fp64 M, or that with one pair more and one less
    pat = (M != 0).astype(float)
    if c.explicit_c:
        (i, j), (k, l) = c.c_only, c.m_only
        assert M[i, j] == 0 and C[i, j] == 1 and M[k, l] != 0 and C[k, l] == 0
        D = C != pat
        assert np.count_nonzero(D) == 4
    else:
        assert np.array_equal(C, pat)
    # held: nothing leaves the pattern, and on fp32 something would have
    Mh, _ = ve.expected_matrices(c, F32)
    with np.errstate(under="ignore"):
        lost = np.count_nonzero((M != 0) & (M.astype(np.float32) == 0))
    assert np.array_equal(Mh != 0, M != 0) and lost >= 20
    # the oracle: both setters hold the same matrices, and they are the handed-over ones
    a, s = ref.RefClipper(), ref.RefClipper()
    a.set_matrix_data(M, C)
    s.set_sparse_matrix_data(*c.upper_csc())
    assert np.array_equal(a.get_affinity_matrix(), s.get_affinity_matrix())
    assert np.array_equal(a.get_constraint_matrix(), s.get_constraint_matrix())
    assert np.array_equal(s.get_affinity_matrix(), M) and np.array_equal(s.get_constraint_matrix(), C)
    x = np.arange(1, c.m + 1) * 2.0 ** -10
    (am, ac), (sm, sc) = a.matvec(x), s.matvec(x)
    assert np.array_equal(ac, sc) and np.array_equal(ac, (C - np.eye(c.m)) @ x)
    assert np.allclose(am, sm, rtol=1e-12, atol=0)
    assert len(ve.probe_columns(c)) == 16
    print(f"{c.name}: {c.Mv.size} entries, {lost // 2} of them round to fp32 zero, lines {lines}")


def _solve_all_modes(c):
    r = ref.RefClipper()
    r.set_sparse_matrix_data(*c.upper_csc())
    sols = []
    for mode in (0, 1, 2):
        r.set_sum_mode(mode)
        sols.append(r.solve(c.u0))
    s0 = sols[0]
    for s in sols[1:]:
        assert s.nodes.tolist() == s0.nodes.tolist() and s.ifinal == s0.ifinal and s.n_trials == s0.n_trials, c.name
        assert np.max(np.abs(s.u - s0.u)) <= 1e-9 and abs(s.score - s0.score) <= 1e-9 * max(1.0, abs(s0.score))
    assert np.all(np.isfinite(s0.u))
    assert not dc.tied_entries(s0.u, s0.nodes), f"{c.name}: the order of the selected list rests on rounding"
    assert dc.boundary_gap(s0.u, s0.nodes) > 2 * dc.U_TOL, f"{c.name}: the selected set rests on rounding"
    return s0


def test_tinyedge_discriminates():
    c = ve.tinyedge(**ve.TINYEDGE)
    gone = ve.tinyedge(**ve.TINYEDGE, drop_underflowed=True)
    K, tiny = c.groups
    M, _ = c.dense()
    assert np.all(M[K[0], tiny] == 1e-50) and tiny.size == (K.size - 1) // 2 and np.all(c.u0 > 0)
    assert np.all(M[np.ix_(K, K)] != 0) and np.all(c.Mv > 0) and c.Mv.max() <= 1.0     # no negative or top rung in a solve
    Mg, _ = gone.dense()
    assert np.array_equal(Mg, np.where(M == 1e-50, 0.0, M))      # only the entries that underflow in fp32 are gone
    s = _solve_all_modes(c)
    sg = _solve_all_modes(gone)
    assert sorted(s.nodes.tolist()) != sorted(sg.nodes.tolist()), "losing the underflowed entries changes nothing"
    # the matrix an fp32 storage holds (FLT_MIN for 1e-50, the other weights rounded) is as safe to compare on
    s32 = _solve_all_modes(ve.held_case(c, F32))
    assert sorted(s32.nodes.tolist()) == sorted(s.nodes.tolist())
    print(f"tinyedge {ve.TINYEDGE}: nodes {sorted(s.nodes.tolist())} (trials {s.n_trials}, gap {dc.boundary_gap(s.u, s.nodes):.3g}), "
          f"without the underflowed entries {sorted(sg.nodes.tolist())} (trials {sg.n_trials}, gap {dc.boundary_gap(sg.u, sg.nodes):.3g})")


def test_rounded_f32_is_held():
    c = dc.weights_tiefill(65, 0.3)
    assert np.array_equal(c.rounded_f32().Mv, c.Mv.astype(np.float32).astype(np.float64))
    t = ve.tinyedge(**ve.TINYEDGE)
    assert np.array_equal(t.rounded_f32().Mv, ve.held(t.Mv, F32)) and np.all(t.rounded_f32().Mv != 0)
