"""GPU tests of the grid route of the d = 3 nearest-neighbour search (clipper_hip_knn_set_search; DESIGN.md section 9,
"The grid route of the search"). The route keeps the brute-force route's contract — fp64 distances added in coordinate
order with nothing fused, lists ascending by (distance, index), -1 / 1e300 where the searched cloud is short — so every
check here is an equality: against oracle/bm_utils_ref.knn_bruteforce, against the brute-force route on the device, and
of every caller's output under the two routes. No tolerances. One cap keeps "exact by visiting everything" from
passing: on the uniform 20 000-point cloud at K = 32 a query visits at most n1 / 8 candidates on average."""
import json
import os

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration
from oracle import bm_utils_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def search_mode():
    """hands the test the setter and puts the process-wide mode back as it was found"""
    before = abi.knn_search()
    try:
        yield abi.knn_set_search
    finally:
        abi.knn_set_search(before)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _check_against_oracle(P0, P1, knn):
    """abi.knn (rows = points here) against the oracle: indices, and the bits of the distances"""
    idx, sqd = abi.knn(P0.T, P1.T, knn)
    ridx, rsqd = ref.knn_bruteforce(P0, P1, knn)
    assert np.array_equal(idx, ridx.astype(np.int32))
    have = ridx >= 0
    assert np.array_equal(_bits(sqd[have]), _bits(rsqd[have]))
    assert np.all(sqd[~have] == 1e300)
    return idx, sqd


def _grid_ran(n0):
    st = abi.knn_last_search()
    assert st.route == abi.KNN_GRID and st.queries == n0 and min(st.dim) >= 1
    return st


# ---- 1. against the oracle ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n0,n1,knn", [(1, 1, 1), (5, 3, 4), (257, 1023, 1), (300, 1025, 3), (1000, 2500, 5), (64, 5000, 16)])
def test_grid_knn_against_the_oracle(search_mode, n0, n1, knn):
    rng = np.random.default_rng(n0 + n1)
    P0, P1 = rng.random((n0, 3)), rng.random((n1, 3))
    search_mode(abi.KNN_GRID)
    _check_against_oracle(P0, P1, knn)
    st = _grid_ran(n0)
    assert 0 < st.candidates <= n0 * n1 and st.dim[0] * st.dim[1] * st.dim[2] <= max(1, n1)


def _edge_clouds():
    """(name, queries, searched cloud), rows = points: the clouds of tests/cpp/test_knn_grid_rules.cpp"""
    rng = np.random.default_rng(20240611)
    P, Q = rng.random((700, 3)), rng.random((150, 3))
    out = [("uniform", Q, P), ("self-search", P, P), ("uniform shifted by 1e6", Q + 1e6, P + 1e6),
           ("self-search shifted by 1e6", P + 1e6, P + 1e6)]
    g = np.arange(8.0)
    L = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)[rng.permutation(512)]
    out.append(("integer lattice, shuffled", L, L))
    T = np.concatenate([P[:200]] * 3)
    out.append(("every point three times", T, T))
    F, Qf = P.copy(), Q.copy()
    F[:, 2] = 0.0
    Qf[:, 2] = 0.0
    out += [("planar", Qf, F), ("planar, queries off the plane", Q, F)]
    Cl, Qc = P.copy(), Q.copy()
    Cl[:, 1:] = 0.5
    Qc[:, 1:] = 0.5
    out.append(("collinear", Qc, Cl))
    t = rng.random(300)
    D = np.stack([t, 2.0 * t, -t], axis=1)
    out.append(("collinear, diagonal", D, D))
    I = np.full((40, 3), 0.25)
    out += [("40 identical points", I, I), ("40 identical points, other queries", Q, I)]
    far = np.where(np.arange(450).reshape(150, 3) % 2 == 1, -1.0, 1.0) * (5.0 + 100.0 * Q)
    out.append(("queries well outside the box", far, P))
    out += [("3 points, knn larger", Q, P[:3]), ("1 point", Q, P[:1])]
    W = np.repeat((np.arange(400) % 2).astype(np.float64)[:, None], 3, axis=1) + 1e-3 * rng.random((400, 3))
    out.append(("two clusters of width 1e-3 a unit apart", W, W))
    return out


@pytest.mark.parametrize("case", _edge_clouds(), ids=lambda c: c[0])
def test_grid_knn_edge_clouds_against_the_oracle(search_mode, case):
    _, Q, P = case
    search_mode(abi.KNN_GRID)
    for knn in (1, 4, 16):
        _check_against_oracle(Q, P, knn)
        _grid_ran(len(Q))


SCAN_CHUNK = 1024  # cells one round of the cell table's scan takes (ROW_SCAN_THREADS, k_wave.hip.h)


@pytest.mark.parametrize("cells", [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1, 2 * SCAN_CHUNK + 1])
def test_grid_knn_cell_table_around_the_scan_chunk(search_mode, cells):
    """A cloud with extent along x only plans dim = (floor(n1 / 4), 1, 1): n1 = 4 cells + 2 puts the cell table just
    below, at and just above one chunk of its scan, and just above two, where the scan's carry goes from chunk to chunk.
    The plan is read back, so the case cannot pass by missing the boundary."""
    rng = np.random.default_rng(cells)
    n1 = 4 * cells + 2
    P1 = np.full((n1, 3), 0.5)
    P1[:, 0] = rng.random(n1)
    P0 = np.full((200, 3), 0.5)
    P0[:, 0] = rng.random(200)
    search_mode(abi.KNN_GRID)
    for knn in (1, 4):
        _check_against_oracle(P0, P1, knn)
        st = _grid_ran(len(P0))
        assert tuple(st.dim) == (cells, 1, 1)


# ---- 2. against the brute-force route on the device, and the pruning cap ----------------------------------------------

@pytest.fixture(scope="module")
def uniform20k():
    return np.random.default_rng(20000).random((20000, 3))


def _both_routes(P0, P1, knn):
    before = abi.knn_search()
    try:
        abi.knn_set_search(abi.KNN_BRUTE)
        bi, bd = abi.knn(P0.T, P1.T, knn)
        assert abi.knn_last_search().route == abi.KNN_BRUTE and abi.knn_last_search().candidates == 0
        abi.knn_set_search(abi.KNN_GRID)
        gi, gd = abi.knn(P0.T, P1.T, knn)
        st = _grid_ran(len(P0))
    finally:
        abi.knn_set_search(before)
    return (bi, bd), (gi, gd), st


def test_grid_equals_brute_force_20000_uniform(uniform20k):
    rng = np.random.default_rng(1)
    Q = rng.random((20000, 3))
    (bi, bd), (gi, gd), _ = _both_routes(Q, uniform20k, 16)
    assert np.array_equal(bi, gi) and _same_bits(bd, gd)


def _bunny(n, seed=3):
    """n points on the bunny's surface: the fixture's 600 resampled with a jitter of a hundredth of its extent"""
    pts = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "bunny_points.json")))["points"], np.float64)
    rng = np.random.default_rng(seed)
    ext = (pts.max(axis=0) - pts.min(axis=0)).max()
    return pts[rng.integers(0, len(pts), n)] + rng.normal(0.0, 0.01 * ext, (n, 3))


def test_grid_lists_of_a_surface_cloud_at_k32(search_mode):
    """3 000 points from the bunny searched in themselves at K = 32: the lists behind the features (abi.knn stops at
    16), read through estimate_normals' counts and compute_fpfh's SPFH, and the first 16 entries through abi.knn"""
    P = _bunny(3000)
    (bi, bd), (gi, gd), _ = _both_routes(P, P, 16)
    assert np.array_equal(bi, gi) and _same_bits(bd, gd)
    N = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, len(P)))
    r = 0.06 * (P.max(axis=0) - P.min(axis=0)).max()
    out = {}
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        search_mode(mode)
        out[mode] = abi.compute_fpfh(P.T, N, knn=32, radius=r, return_spfh=True)
        assert abi.knn_last_search().route == mode
    for a, b in zip(out[abi.KNN_BRUTE], out[abi.KNN_GRID]):
        assert _same_bits(a.astype(np.float64), b.astype(np.float64))
    cnt = out[abi.KNN_GRID][2]
    assert cnt.min() < 32 <= cnt.max()                 # the radius cuts some lists and leaves others whole


def test_grid_prunes(search_mode, uniform20k):
    """candidates visited / queries <= n1 / 8 on the uniform 20 000-point cloud at K = 32 (the lists of the features):
    a host prototype visits about 120 per query at two points per cell; the cap leaves room for cells several times
    coarser, and none for visiting everything."""
    search_mode(abi.KNN_GRID)
    abi.estimate_normals(uniform20k.T, knn=32)
    st = _grid_ran(len(uniform20k))
    per_query = st.candidates / st.queries
    print(f"grid {st.dim[0]} x {st.dim[1]} x {st.dim[2]}, {per_query:.1f} candidates per query of n1 = {len(uniform20k)}")
    assert 32 <= per_query <= len(uniform20k) / 8


# ---- 3. the callers, under BRUTE and then GRID ----------------------------------------------------------------------

def _under_both(search_mode, call):
    out = []
    for mode in (abi.KNN_BRUTE, abi.KNN_GRID):
        search_mode(mode)
        out.append(call())
        st = abi.knn_last_search()
        assert st.route == mode and st.queries > 0
    return out


@pytest.fixture(scope="module")
def clouds2000():
    rng = np.random.default_rng(2000)
    P = rng.random((2000, 3))
    return P, P[rng.permutation(2000)] + rng.normal(0.0, 0.004, (2000, 3))


@pytest.mark.parametrize("knn,one_to_one", [(1, False), (1, True), (4, False), (4, True)])
def test_distance_based_correspondences_equal_under_both_routes(search_mode, clouds2000, knn, one_to_one):
    P0, P1 = clouds2000
    a, b = _under_both(search_mode, lambda: abi.distance_based_correspondences(P0.T, P1.T, knn, 0.03, one_to_one))
    assert len(a) > 100 and np.array_equal(a, b)


def test_estimate_normals_equal_under_both_routes(search_mode, clouds2000):
    P = clouds2000[0]
    (Na, ca), (Nb, cb) = _under_both(search_mode, lambda: abi.estimate_normals(P.T, knn=16, radius=0.12, return_counts=True))
    assert _same_bits(Na, Nb) and np.array_equal(ca, cb)
    assert ca.min() < 16 == ca.max()                   # the radius cuts some lists


def test_compute_fpfh_equal_under_both_routes(search_mode, clouds2000):
    P = clouds2000[0]
    search_mode(abi.KNN_BRUTE)
    N = abi.estimate_normals(P.T, knn=16)
    (Fa, Sa, ca), (Fb, Sb, cb) = _under_both(search_mode, lambda: abi.compute_fpfh(P.T, N, knn=32, radius=0.2, return_spfh=True))
    assert _same_bits(Fa, Fb) and _same_bits(Sa, Sb) and np.array_equal(ca, cb)
    assert ca.min() < 32 == ca.max()


def test_fpfh_from_points_equal_under_both_routes(search_mode, clouds2000):
    P = clouds2000[0]
    (Fa, Na), (Fb, Nb) = _under_both(search_mode, lambda: abi.fpfh_from_points(P.T, normal_knn=16, normal_radius=0.12, knn=32,
                                                                              radius=0.2))
    assert _same_bits(Fa, Fb) and _same_bits(Na, Nb)
    # and the counts, through the two single-stage calls on the grid route
    search_mode(abi.KNN_GRID)
    _, cn = abi.estimate_normals(P.T, knn=16, radius=0.12, return_counts=True)
    _, _, cf = abi.compute_fpfh(P.T, Nb, knn=32, radius=0.2, return_spfh=True)
    search_mode(abi.KNN_BRUTE)
    _, cn0 = abi.estimate_normals(P.T, knn=16, radius=0.12, return_counts=True)
    _, _, cf0 = abi.compute_fpfh(P.T, Nb, knn=32, radius=0.2, return_spfh=True)
    assert np.array_equal(cn, cn0) and np.array_equal(cf, cf0)


def test_two_dimensional_search_runs_brute_force_under_grid(search_mode):
    rng = np.random.default_rng(2)
    P0, P1 = rng.random((300, 2)), rng.random((1500, 2))
    search_mode(abi.KNN_GRID)
    _check_against_oracle(P0, P1, 8)
    st = abi.knn_last_search()
    assert st.route == abi.KNN_BRUTE and st.candidates == 0 and st.queries == 300


# ---- 4. AUTO --------------------------------------------------------------------------------------------------------

def test_auto_takes_the_grid_from_the_documented_size_on(search_mode):
    thr = int(abi.knn_last_search().auto_min_n)        # read from the library, not written down here
    assert thr >= 2
    rng = np.random.default_rng(4)
    P1, Q = rng.random((thr, 3)), rng.random((64, 3))
    search_mode(abi.KNN_AUTO)
    below = abi.knn(Q.T, P1[:thr - 1].T, 1)
    assert abi.knn_last_search().route == abi.KNN_BRUTE
    at = abi.knn(Q.T, P1.T, 1)
    assert abi.knn_last_search().route == abi.KNN_GRID
    search_mode(abi.KNN_BRUTE)
    for got, cloud in ((below, P1[:thr - 1]), (at, P1)):
        want = abi.knn(Q.T, cloud.T, 1)
        assert np.array_equal(got[0], want[0]) and _same_bits(got[1], want[1])
    assert abi.knn_last_search().route == abi.KNN_BRUTE
    # two dimensions: brute force under AUTO as well, whatever the size
    search_mode(abi.KNN_AUTO)
    abi.knn(Q[:, :2].T, P1[:, :2].T, 1)
    assert abi.knn_last_search().route == abi.KNN_BRUTE


# ---- 5. the facades -------------------------------------------------------------------------------------------------

def test_clipperpy_knn_search_round_trip(clouds2000):
    cp = clipper_amd.load_clipperpy()
    before = abi.knn_search()
    try:
        assert cp.utils.knn_search() == cp.utils.KnnSearch.Brute
        cp.utils.set_knn_search(cp.utils.KnnSearch.Grid)
        assert cp.utils.knn_search() == cp.utils.KnnSearch.Grid and abi.knn_search() == abi.KNN_GRID
        P = np.asfortranarray(clouds2000[0][:500].T)
        Ng = cp.utils.estimate_normals(P, 16, 0.0, [])
        assert abi.knn_last_search().route == abi.KNN_GRID
        cp.utils.set_knn_search(cp.utils.KnnSearch.Auto)
        assert cp.utils.knn_search() == cp.utils.KnnSearch.Auto and abi.knn_search() == abi.KNN_AUTO
        cp.utils.set_knn_search(cp.utils.KnnSearch.Brute)
        Nb = cp.utils.estimate_normals(P, 16, 0.0, [])
        assert abi.knn_last_search().route == abi.KNN_BRUTE and _same_bits(np.asarray(Ng), np.asarray(Nb))
    finally:
        abi.knn_set_search(before)
    assert abi.knn_search() == before


def test_registration_search_argument_leaves_the_mode_as_it_found_it(search_mode, clouds2000):
    P0, P1 = clouds2000
    search_mode(abi.KNN_BRUTE)
    want = registration.ground_truth_associations(P0, P1, 0.03)
    assert abi.knn_last_search().route == abi.KNN_BRUTE
    got = registration.ground_truth_associations(P0, P1, 0.03, search="grid")
    assert abi.knn_last_search().route == abi.KNN_GRID and abi.knn_search() == abi.KNN_BRUTE
    assert len(want) > 100 and np.array_equal(want, got)
    search_mode(abi.KNN_AUTO)
    N = registration.estimate_normals(P0, knn=16, search="grid")
    assert abi.knn_last_search().route == abi.KNN_GRID and abi.knn_search() == abi.KNN_AUTO
    F = registration.compute_fpfh(P0, N, search="brute")
    assert abi.knn_last_search().route == abi.KNN_BRUTE and abi.knn_search() == abi.KNN_AUTO and F.shape == (2000, 33)
