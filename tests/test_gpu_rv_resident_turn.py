"""A turn of the resident solver on a row view (csrc/k_rv_resident.hip.h) after its latency chain was cut: the column
sums combined without a branch per wave, the counts of a one-group unit published by its wave 0 without a round
through LDS, the barriers that the exchange's own barrier already covers dropped. None of this changes a sum, so the
launch must give what the streamed view (mode 2) and the oracle give, on the units the plan makes for the headline's
view (one column group each) and on a view of more column groups than the chip holds units (so some unit holds
several groups: its waves' counts meet in LDS), and the same bits from solve to solve."""
import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth
from oracle import clipper_ref as ref

pytestmark = pytest.mark.gpu

PROBLEMS = [(10000, 0.95, 12345), (10000, 0.95, 4), (6000, 0.9, 6777), (12000, 0.97, 5)]


def _oracle(p):
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    return r.solve(p.u0)


def _solve(p, storage, mode):
    g = abi.HipClipper(storage=storage)
    g.set_row_view(mode)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    s = g.solve(p.u0)
    st = g.view_stats()
    again = g.solve(p.u0)
    g.close()
    return s, st, again


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
@pytest.mark.parametrize("m,rho,seed", PROBLEMS)
def test_turn_gives_the_streamed_views_and_the_oracles_answer(m, rho, seed, storage):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    sr = _oracle(p)
    s1, st1, s1b = _solve(p, storage, 0)
    s2, st2, _ = _solve(p, storage, 2)
    assert st2.resident_launches == 0
    if st2.rows <= 1024 and st2.builds == 1:
        assert st1.resident_launches >= 1, (st1.builds, st1.rows, st1.resident_launches)
    for s in (s1, s2):
        assert s.nodes.tolist() == sr.nodes.tolist()
        assert s.ifinal == sr.ifinal
        assert abs(s.score - sr.score) <= 1e-6 * abs(sr.score)
    assert abs(s1.score - s2.score) <= 1e-10 * abs(s2.score)
    assert np.allclose(s1.u, s2.u, rtol=0, atol=1e-8)
    assert abs(s1.n_trials - sr.n_trials) <= max(2, sr.n_trials // 20)
    # the same bits from solve to solve
    assert np.array_equal(s1b.u, s1.u) and s1b.n_trials == s1.n_trials and s1b.n_passes == s1.n_passes
    if (m, rho, seed) == PROBLEMS[0] and storage == abi.STORE_F32_CSC:
        # the headline: one launch, the oracle's ordered list and its 66 trials
        assert st1.resident_launches == 1
        assert s1.n_trials == sr.n_trials == 66 and s1.ifinal == sr.ifinal


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_units_of_several_column_groups(storage):
    """m = 22 246: 348 column groups, more than the chip holds units, so some unit holds several groups (the counts
    of its waves meet in LDS, the path a one-group unit skips). Same node set, ifinal and score as the streamed view
    and the oracle."""
    m, rho, seed = 22246, 0.985, 694087
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    sr = _oracle(p)
    s1, st1, s1b = _solve(p, storage, 0)
    s2, st2, _ = _solve(p, storage, 2)
    assert st1.resident_launches >= 1 and st2.resident_launches == 0
    assert 0 < st1.resident_units < (m + 63) // 64, (st1.resident_units, m)  # (fewer units than groups)
    for s in (s1, s2):
        assert sorted(s.nodes.tolist()) == sorted(sr.nodes.tolist())
        assert s.ifinal == sr.ifinal
        assert abs(s.score - sr.score) <= 1e-6 * abs(sr.score)
    assert abs(s1.score - s2.score) <= 1e-9 * abs(s2.score)
    assert np.array_equal(s1b.u, s1.u) and s1b.n_trials == s1.n_trials
