"""CPU checks of tests/subproblem_model.py, the model the selection kernels of the live sub-problem are compared with
on the GPU (tests/test_gpu_sub_selection.py, tests/test_gpu_sub_small.py). The exactness argument (DESIGN.md §3e,
tests/test_subproblem_bound.py) needs two integer facts of a selection; the contract as the model states it implies both:

  cnt[c]  >= stored entries of column c among the view's rows                (what k_sub_colcount reads off the headers)
  N_used  >= stored entries any column outside S has among the rows of S     (what the decision's bound is given)
"""
import numpy as np
import pytest

from clipper_amd import synth
from oracle import clipper_ref as ref
from tests import subproblem_model as sm


def _random_pattern(m, density, rng):
    up = np.triu(rng.random((m, m)) < density, 1)
    return up | up.T


def _needed_N(pattern, flags):
    """the most stored entries a column outside S has among the rows of S"""
    S = np.asarray(flags[:pattern.shape[0]], dtype=bool)
    return 0 if S.all() else int(pattern[S][:, ~S].sum(axis=0).max())


def _check(pattern, rows, s):
    m = pattern.shape[0]
    r = sm.select(pattern, rows, s)
    true_cnt = pattern[rows].sum(axis=0)
    assert r["mp"] % 64 == 0 and m <= r["mp"] < m + 64
    assert np.all(r["cnt"][:m] >= true_cnt) and np.all(r["cnt"][:m] < true_cnt + 4 * -(-len(rows) // 128))
    assert np.all(r["cnt"] % 4 == 0) and np.all(r["cnt"][m:] == 0)
    assert np.all(r["flags"][rows]) and not r["flags"][m:].any()
    assert r["nS"] == r["flags"].sum() == len(r["colmap"]) and np.all(np.diff(r["colmap"]) > 0)
    assert np.array_equal(r["pos"][r["colmap"]], np.arange(r["nS"])) and np.all(r["pos"][~r["flags"]] == -1)
    assert r["N_used"] == max(1, r["ncol"]) + r["nS"] - len(rows)
    assert r["N_used"] >= _needed_N(pattern, r["flags"])
    return r


@pytest.mark.parametrize("m,density,nrows,seed", [(64, 0.3, 40, 1), (65, 0.5, 40, 2), (257, 0.2, 1, 3), (300, 0.05, 129, 4),
                                                 (513, 0.6, 257, 5), (700, 0.1, 700, 6)])
def test_counts_and_N_cover_the_matrix_on_random_patterns(m, density, nrows, seed):
    rng = np.random.default_rng(seed)
    pattern = _random_pattern(m, density, rng)
    rows = np.sort(rng.choice(m, nrows, replace=False))
    outside = np.setdiff1d(np.unique(sm.select(pattern, rows, 0.0)["cnt"][:m][np.setdiff1d(np.arange(m), rows)]), [0])
    v = int(np.median(outside)) if outside.size else 4
    joined = []
    for s in (0.0, np.sqrt((v + 0.5) / 0.4), np.sqrt((v - 0.5) / 0.4), 5.0, 1e6):
        r = _check(pattern, rows, s)
        joined.append(r["nS"])
    assert joined[0] >= joined[2] >= joined[1] >= joined[4] == nrows   # a larger threshold never adds a column
    assert sm.select(pattern, rows, np.sqrt((v + 0.5) / 0.4))["n0"] == v
    assert sm.select(pattern, rows, np.sqrt((v - 0.5) / 0.4))["n0"] == v - 1
    assert sm.select(pattern, rows, 5.0)["n0"] == 10 and sm.select(pattern, rows, 1e6)["n0"] == 2_000_000_000


def test_counts_and_N_cover_the_matrix_of_a_registration_problem():
    p = synth.make_euclidean_problem(1200, 0.9, seed=11)
    Mup, _ = ref.numpy_affinity_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    pattern = (Mup + Mup.T) != 0
    assert not pattern.diagonal().any()
    rng = np.random.default_rng(7)
    inliers = np.arange(1200 - 120, 1200)   # (synth places the inliers last)
    for rows in (inliers, np.sort(rng.choice(1200, 400, replace=False)), np.arange(1200)):
        for s in (0.0, 3.0, 5.0, 9.0, 1e6):
            r = _check(pattern, rows, s)
            if len(rows) == 1200:
                assert r["nS"] == 1200 and r["ncol"] == 0 and r["N_used"] == 1


def test_a_count_of_the_first_of_two_sub_blocks_is_no_bound():
    """The hazard of k_sub_colcount: it reads the quads of a slice's sub-block 0. Were a chunk two sub-blocks of 128 rows
    (SL_H = 2: chunks of 256 view rows, the header one byte per lane and sub-block), that would be the count of every other
    128 rows. A column whose entries sit in view rows 128..255 then counts 0: it stays outside S with N too small."""
    m = 400
    pattern = np.zeros((m, m), dtype=bool)
    c = 399
    rows = np.arange(0, 300)
    pattern[130:190, c] = True
    pattern[c, 130:190] = True
    r = sm.select(pattern, rows, 5.0)         # n0 = 10
    assert r["cnt"][c] == 60 and r["flags"][c] and r["N_used"] >= 0
    # the same count over sub-block 0 of each 256-row chunk alone: view rows [0, 128) and [256, 300)
    short = np.zeros(m, dtype=np.int64)
    for k in (0, 2):
        short += 4 * ((pattern[rows[128 * k:128 * k + 128]].sum(axis=0) + 3) // 4)
    assert short[c] == 0 < pattern[rows, c].sum()            # not a bound on the column's entries
    S_short = np.zeros(m, dtype=bool)
    S_short[rows] = True                                     # (c does not join: 0 > 10 is false)
    N_short = max(1, int(short[~S_short].max())) + 0
    assert N_short < pattern[S_short][:, ~S_short].sum(axis=0).max() == 60   # ... and N no bound for the decision
