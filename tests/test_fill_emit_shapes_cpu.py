"""The constructions of tests/fill_emit_shapes_gen.py on the CPU oracle: the affinity matrix of every case is exactly
the stated one — 1.0 on K x K off the diagonal, 0 elsewhere, the constraint matrix its pattern, the products the exact
integer sums — and the cases reach every per-column entry count the device test is meant to reach. The construction is
proven here on the reference before tests/test_gpu_fill_emit_shapes.py lets it judge the device."""
import numpy as np
import pytest

from oracle import clipper_ref as ref
from tests import fill_emit_shapes_gen as gen


def _oracle(p):
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **gen.PARAMS)
    return r


@pytest.mark.parametrize("name", list(gen.CASES))
def test_the_oracle_gives_exactly_the_stated_matrix(name):
    p = gen.make(name)
    r = _oracle(p)
    E = p.expected()
    M, Cm = r.get_affinity_matrix(), r.get_constraint_matrix()
    off = ~np.eye(p.m, dtype=bool)
    assert np.array_equal(M[off], E[off])          # bit for bit: 1.0 or 0
    assert np.array_equal(Cm[off], E[off])
    assert np.array_equal(M, M.T)
    # the far pairs are far by much more than epsilon, the near ones have c = 0 exactly
    i, j = np.nonzero(off)
    l1 = np.linalg.norm(p.D1[:, i] - p.D1[:, j], axis=0)
    l2 = np.linalg.norm(p.D2[:, i] - p.D2[:, j], axis=0)
    c = np.abs(l1 - l2)
    near = E[i, j] != 0
    assert np.all(c[near] == 0.0) and np.all(c[~near] > 100 * gen.EPS)


@pytest.mark.parametrize("name", list(gen.CASES))
def test_the_oracles_products_are_the_exact_integer_sums(name):
    p = gen.make(name)
    r = _oracle(p)
    rows, x = p.rows_in_and_out(), p.x()
    inK = np.isin(rows, p.K)
    if p.K.size and p.K.size < p.m:
        assert inK.any() and (~inK).any()          # rows from inside and from outside K
    xm = np.zeros(p.m)
    xm[rows] = x[rows]
    oM, oC = r.matvec(xm)
    want = p.expected() @ xm                       # (the oracle's products are those of the off-diagonal parts)
    assert np.array_equal(oM, want)
    assert np.array_equal(oC, want)


def test_the_cases_reach_every_wanted_count_and_size():
    got = set()
    for name in gen.CASES:
        got |= gen.make(name).counts()
    assert gen.WANTED_COUNTS <= got, sorted(gen.WANTED_COUNTS - got)
    assert {m for m, _ in gen.CASES.values()} == {127, 128, 129, 257, 385}
    # a 64-column group that holds full columns beside empty ones (maxq = 32 while most lanes have nothing)
    p = gen.make("m385_sparse_cols")
    E = p.expected()
    block = E[0:gen.CHUNK, 2 * gen.GROUP:3 * gen.GROUP]   # chunk 0, the column group of row 128 + 3
    per_col = np.count_nonzero(block, axis=0)
    assert per_col.max() == 128 and np.count_nonzero(per_col) == 1
    # the row masks' words: a chunk with rows in the outer words only, and one with a single inner word
    p = gen.make("m257_words")
    words = lambda k: {int(r) % gen.CHUNK // 32 for r in p.K if r // gen.CHUNK == k}
    assert words(0) == {0, 3} and words(1) == {1}
    p = gen.make("m257_halves")
    words = lambda k: {int(r) % gen.CHUNK // 32 for r in p.K if r // gen.CHUNK == k}
    assert words(0) == {0, 1} and words(1) == {2, 3}
