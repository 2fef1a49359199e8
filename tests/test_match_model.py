"""CPU tests of the model the descriptor matcher is held to (tests/match_model.py): every configuration the GPU tests
run keeps a good part of the unfiltered rows and drops a good part, so that no GPU test of a filter can pass on an
empty or an untouched list; the model without filters is oracle/bm_utils_ref.knn_bruteforce; and the CPU twin of the
end-to-end test of tests/test_gpu_match.py: the model's associations through the CPU oracle."""
import numpy as np
import pytest

from oracle import bm_utils_ref as ref
from oracle import clipper_ref
from tests import match_model as mm


@pytest.fixture(scope="module")
def recipe():
    return mm.filter_recipe()


@pytest.mark.parametrize("knn,mutual,ratio,max_sqdist", mm.CONFIGS)
def test_every_configuration_keeps_and_drops_rows(recipe, knn, mutual, ratio, max_sqdist):
    F0, F1, truth = recipe
    A, sqd, idx, lsq = mm.match_model(F0, F1, knn, bool(mutual), ratio, max_sqdist)
    unfiltered = len(F0) * knn
    assert idx.shape == (len(F0), knn) and np.all(idx >= 0)
    assert len(A) == len(sqd) and len(A) >= 200 and unfiltered - len(A) >= 100
    assert np.all(np.diff(A[:, 0]) >= 0)                       # i ascending
    got = {(int(a), int(b)) for a, b in A}
    assert len(got) == len(A)
    if max_sqdist <= 0:                                        # a noisy copy is far closer than any random descriptor
        assert truth <= got
    else:
        assert np.all(sqd <= max_sqdist)


def test_model_without_filters_is_the_brute_force_search():
    rng = np.random.default_rng(2)
    P0, P1 = rng.random((60, 3)), rng.random((45, 3))
    A, sqd, idx, lsq = mm.match_model(P0, P1, knn=1, mutual=False)
    ridx, rsqd = ref.knn_bruteforce(P0, P1, 1)
    assert np.array_equal(A, np.stack([np.arange(60), ridx[:, 0]], axis=1))
    assert np.array_equal(sqd, rsqd[:, 0]) and np.array_equal(idx, ridx) and np.array_equal(lsq, rsqd)


def test_ratio_needs_one_neighbour_and_short_sets_pad():
    rng = np.random.default_rng(3)
    F0, F1 = rng.random((5, 9)), rng.random((1, 9))
    with pytest.raises(ValueError):
        mm.match_model(F0, F1, knn=2, ratio=0.8)
    A, _, idx, lsq = mm.match_model(F0, F1, knn=1, mutual=False, ratio=0.5)   # no second neighbour: the test passes
    assert A.tolist() == [[i, 0] for i in range(5)]
    A, _, idx, lsq = mm.match_model(F0, F1, knn=3, mutual=False)
    assert A.tolist() == [[i, 0] for i in range(5)] and np.all(idx[:, 1:] == -1) and np.all(np.isinf(lsq[:, 1:]))


def test_end_to_end_on_the_cpu_oracle():
    """tests/test_gpu_match.py::test_end_to_end with the oracle in the GPU's place: match (model), Euclidean fill
    (sigma 0.015, epsilon 0.05), solve; the bounds are those of test_reference_benchmark_recipe_end_to_end."""
    pts, noisy, F0, F1, Agt = mm.bunny_recipe()
    A = mm.match_model(F0, F1, knn=1, mutual=False)[0]
    assert len(A) == len(pts)
    c = clipper_ref.RefClipper()
    c.score_pairwise_consistency_euclidean(pts.T, noisy.T, A, sigma=0.015, epsilon=0.05)
    s = c.solve(np.random.default_rng(4).random(len(A)))
    p, r = ref.get_precision_recall(A[s.nodes], Agt)
    print(f"precision {p:.3f} recall {r:.3f} of {len(Agt)} true pairs, {len(s.nodes)} selected")
    assert p >= 0.9 and r >= 0.5
