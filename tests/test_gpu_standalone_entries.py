"""GPU tests of what the stand-alone calls share (host_call.hpp, host_knn_k.hpp, host_knn.hpp): a device number out of
range at every entry point, and every (route, K) pair of the search's dispatch tables against the numpy brute force
(oracle/bm_utils_ref.knn_bruteforce), by (distance, index), bit for bit. The shapes: 300 queries (no multiple of a
block of 256), a searched cloud of K - 1 points (the list's tail is -1 / 1e300) and one of 1100 (more than a tile of
1024: two chunks merge) in which every point occurs twice (exact ties: the lower index first)."""
import numpy as np
import pytest

from clipper_amd import _abi as abi
from oracle import bm_utils_ref as ref
from tests import features_model as fm
from tests import standalone_entries as se

pytestmark = pytest.mark.gpu

ROUTES = [("brute", abi.KNN_BRUTE), ("grid", abi.KNN_GRID)]


@pytest.fixture
def search_mode():
    """hands the test the setter and puts the process-wide mode back as it was found"""
    before = abi.knn_search()
    try:
        yield abi.knn_set_search
    finally:
        abi.knn_set_search(before)


@pytest.mark.parametrize("entry", se.ENTRIES, ids=lambda e: e[0])
def test_device_out_of_range(entry):
    rc, msg = se.call(entry, 99)
    assert rc == se.E_INVALID and "device 99 out of range" in msg, (rc, msg)


def _clouds(d, n1, seed):
    """300 queries and a searched cloud of n1 points, rows = points; from 4 points on every point occurs twice"""
    rng = np.random.default_rng(seed)
    half = rng.random((n1 // 2, d))
    P1 = np.concatenate([half, half, rng.random((n1 % 2, d))]) if n1 >= 4 else rng.random((n1, d))
    return rng.random((300, d)), P1


@pytest.fixture(scope="module")
def searches():
    """(d, n1) -> (queries, searched cloud, the reference's lists at 16 entries): computed once, read by every K"""
    out = {}
    for d in (2, 3):
        for n1 in (1, 3, 7, 15, 1100):
            Q, P1 = _clouds(d, n1, 100 * d + n1)
            out[d, n1] = (Q, P1) + ref.knn_bruteforce(Q, P1, 16)
    return out


def _check_lists(idx, sqd, ridx, rsqd, knn):
    """nearest-K lists are nested: the reference's first knn columns"""
    ridx, rsqd = ridx[:, :knn], rsqd[:, :knn]
    have = ridx >= 0
    assert idx.shape == ridx.shape and np.array_equal(idx, ridx.astype(np.int32))
    assert np.array_equal(sqd[have].view(np.uint64), rsqd[have].view(np.uint64))
    assert np.all(sqd[~have] == 1e300)


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize("knn", [1, 2, 4, 8, 16])
def test_every_k_in_three_dimensions(search_mode, searches, knn, route):
    search_mode(route[1])
    for n1 in (max(knn - 1, 1), 1100):                 # (K = 1: a cloud of one point, the shortest there is)
        Q, P1, ridx, rsqd = searches[3, n1]
        idx, sqd = abi.knn(Q.T, P1.T, knn)
        st = abi.knn_last_search()
        assert st.route == route[1] and st.queries == 300
        _check_lists(idx, sqd, ridx, rsqd, knn)
        if n1 == 1100:                                 # the twins are a tie at every rank: the lower index first
            assert knn == 1 or np.all(idx[:, 1] == idx[:, 0] + 550)
        else:
            assert np.all(idx[:, knn - 1] == (-1 if knn > 1 else 0))


@pytest.mark.parametrize("knn", [1, 2, 4, 8, 16])
def test_every_k_in_two_dimensions(searches, knn):
    for n1 in (max(knn - 1, 1), 1100):
        Q, P1, ridx, rsqd = searches[2, n1]
        idx, sqd = abi.knn(Q.T, P1.T, knn)
        assert abi.knn_last_search().route == abi.KNN_BRUTE
        _check_lists(idx, sqd, ridx, rsqd, knn)


@pytest.mark.parametrize("knn", [1, 2, 4, 8])
def test_every_k_of_the_descriptor_search(knn):
    for n1 in (max(knn - 1, 1), 1100):
        F0, F1 = _clouds(33, n1, 3300 + n1)
        ridx, rsqd = ref.knn_bruteforce(F0, F1, knn)
        _, _, idx, lsq = abi.match_descriptors(F0.T, F1.T, knn=knn, mutual=False, return_lists=True)
        _check_lists(idx, lsq, ridx, rsqd, knn)


@pytest.fixture(scope="module")
def k32_models():
    return {}


@pytest.mark.parametrize("route", ROUTES, ids=lambda r: r[0])
@pytest.mark.parametrize("n", [31, 1100])
def test_k32_through_fpfh_from_points(search_mode, k32_models, n, route):
    """the lists of 32 entries cannot be read directly (clipper_hip_knn stops at 16): the descriptors built from them,
    against the model over the reference's lists and the normals the call returned. n = 31: every list ends in -1."""
    P = _clouds(3, n, 32 + n)[1]
    search_mode(route[1])
    F, N = abi.fpfh_from_points(P.T, normal_knn=32, knn=32)
    assert abi.knn_last_search().route == route[1]
    if n not in k32_models:                            # (the two routes return the same normals: one model serves both)
        k32_models[n] = (N.copy(),) + fm.fpfh(P, N.T, 32)
    N0, Fm, _, cnt, margin = k32_models[n]
    assert np.array_equal(N.view(np.uint64), N0.view(np.uint64))
    assert np.all(cnt == min(n, 32))
    assert np.all(np.isinf(margin) | (margin >= 1e-9)), "the input sits on a bin edge: choose another"
    assert np.array_equal(F.T, Fm)
