"""GPU test of who owns what a cloud on the device holds (host_cloud.hpp, host_knn_grid.hpp's KnnTarget): a round of
every stage on clouds and of the stand-alone calls beside them leaves no device buffer, pinned buffer or event behind
(the method of test_gpu_buffer_lifetime.py on what that round does not open); an attachment can be downloaded exactly
when clipper_hip_cloud_info reports it and exactly when the stage that owns it has run; and a cloud keeps the
brute-force route's bounding box and the grid route's index side by side, each made once.

Sizes: clouds of 300 and 200 points, as the other cloud tests use: several grid cells, two workgroups, lists that are
not all padding."""
import ctypes as C

import numpy as np
import pytest

from clipper_amd import _abi as abi

pytestmark = pytest.mark.gpu

NS, NT = 200, 300
MAXD = 0.25
VOXEL = 1e-3   # (finer than the sampling: nearly every point is a voxel of its own)
HELD = ("device_buffers", "device_bytes", "pinned_buffers", "events")
E_STATE = -5
ROUTES = [abi.KNN_BRUTE, abi.KNN_GRID]


@pytest.fixture(scope="module")
def scene():
    """a wavy sheet sampled twice: the target, and a source that is a moved, jittered part of it (made once)"""
    rng = np.random.default_rng(42)
    xy = rng.random((2, NT))
    tgt = np.asfortranarray(np.vstack([xy, 0.2 * np.sin(3.0 * xy[0]) * np.cos(2.0 * xy[1])]))
    a = 0.05
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    src = np.asfortranarray(R @ tgt[:, :NS] + np.array([[0.02], [-0.01], [0.015]]) + 1e-3 * rng.normal(size=(3, NS)))
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, 0.0, -0.01]
    F = {n: np.asfortranarray(rng.random((8, n))) for n in (NS, NT)}   # descriptors from elsewhere
    return src, tgt, T0, F


@pytest.fixture(params=ROUTES, ids=["brute", "grid"])
def route(request):
    prev = abi.knn_set_search(request.param)
    yield request.param
    abi.knn_set_search(prev)


def _held(c):
    return {k: c[k] for k in HELD}


def _round(scene):
    """every stage on two clouds and the stand-alone calls beside them, all closed again; returns the counts as they
    stood while the clouds, the pairs and the context were open"""
    src, tgt, T0, F = scene
    with abi.DeviceCloud(src) as raw_s, abi.DeviceCloud(tgt) as raw_t, \
            raw_s.voxel_down_sample(VOXEL, return_trace=True) as cs, raw_t.voxel_down_sample(VOXEL, return_trace=True) as ct:
        for c in (cs, ct):
            c.estimate_normals(knn=12)
            c.compute_fpfh(knn=16)
            c.fpfh_from_points(normal_knn=12, knn=16)
            c.estimate_covariances(knn=12)
        with cs.match(ct, knn=1, mutual=False) as fpfh_pairs:
            assert len(fpfh_pairs) == len(cs)
        cs.set_descriptors(F[NS][:, :len(cs)])
        ct.set_descriptors(F[NT][:, :len(ct)])
        with cs.match(ct, knn=1, mutual=False) as pairs:
            A = pairs.download(with_sqd=False)
            g = abi.HipClipper(storage=abi.STORE_F32_CSC)
            g.stage_inputs_clouds(cs, ct, pairs)
            g.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
            g.stage_u0(np.full(len(pairs), 1.0))
            g.solve_staged()
            cs.gather_points(A[:, 0])
            cs.icp(ct, T_init=T0, method=abi.ICP_POINT_TO_PLANE, max_distance=MAXD, max_iterations=5)
            cs.icp(ct, T_init=T0, max_distance=MAXD, max_iterations=5, loss=abi.ICP_LOSS_HUBER, scale=0.02, trim=0.8)
            cs.icp(ct, T_init=T0, method=abi.ICP_GENERALIZED, max_distance=MAXD, max_iterations=5)
            cs.evaluate_registration(ct, T0, MAXD)
            open_counts = abi.debug_live_resources()
            g.close()
    N = abi.estimate_normals(tgt, knn=12)
    Fh, _, _ = abi.compute_fpfh(tgt, N, knn=16, return_spfh=True)
    abi.fpfh_from_points(src, normal_knn=12, knn=16)
    abi.match_descriptors(F[NS], F[NT], knn=1, mutual=False)
    abi.icp_robust(src, tgt, T_init=T0, max_distance=MAXD, max_iterations=5, loss=abi.ICP_LOSS_HUBER, scale=0.02, trim=0.8)
    abi.evaluate_registration(src, tgt, T0, MAXD)
    A = abi.distance_based_correspondences(src, tgt, 2, MAXD, True)
    assert len(A) >= 3
    abi.ransac_correspondences(src, tgt, A, max_distance=0.05, max_hypotheses=2000)
    return open_counts


def test_a_cloud_round_leaves_nothing_behind(scene, route):
    _round(scene)   # (per-thread caches such as the search's events exist from here on)
    base = abi.debug_live_resources()
    open_counts = _round(scene)
    after = abi.debug_live_resources()
    print("baseline", base, "\nopen", open_counts, "\nafter", after)
    assert _held(after) == _held(base)
    assert all(open_counts[k] > base[k] for k in HELD), (open_counts, base)   # the counting counts


# ---- present exactly when owned ----------------------------------------------------------------------------------------

ALL = range(10)
INFO = {abi.CLOUD_NORMALS: lambda i: bool(i.has_normals), abi.CLOUD_DESCRIPTORS: lambda i: i.descriptor_dim > 0,
        abi.CLOUD_SPFH: lambda i: bool(i.has_spfh), abi.CLOUD_COVARIANCES: lambda i: bool(i.has_covariances),
        abi.CLOUD_VOXEL_COUNTS: lambda i: bool(i.has_voxel_counts), abi.CLOUD_VOXEL_TRACE: lambda i: i.trace_n > 0}


def _check_present(c, table, step):
    """for each of the ten attachments: the download succeeds iff info() reports it iff `table` names it"""
    L, info = abi.load_library(), c.info()
    buf = np.zeros(64 * max(len(c), int(info.trace_n), 1), dtype=np.float64)   # (room for the widest: 33 doubles a point)
    for what in ALL:
        want = what in table
        rc = L.clipper_hip_cloud_download(c.h, what, buf.ctypes.data_as(C.c_void_p))
        assert (rc == 0) == want, (step, what, rc)
        if not want:
            assert rc == E_STATE and "was never computed" in abi._last_error(), (step, what, rc, abi._last_error())
        if what in INFO:
            assert INFO[what](info) == want, (step, what)


@pytest.mark.parametrize("with_normals", [False, True], ids=["points", "normals"])
def test_present_exactly_when_owned(scene, with_normals):
    _, tgt, _, F = scene
    N0 = abi.estimate_normals(tgt, knn=12) if with_normals else None
    have = {abi.CLOUD_POINTS} | ({abi.CLOUD_NORMALS} if with_normals else set())
    with abi.DeviceCloud(tgt, normals=N0) as raw:
        _check_present(raw, have, "create")
        with raw.voxel_down_sample(VOXEL, return_trace=True) as c:
            _check_present(raw, have, "create, after voxel")
            have = have | {abi.CLOUD_VOXEL_COUNTS, abi.CLOUD_VOXEL_TRACE}
            _check_present(c, have, "voxel")
            c.estimate_normals(knn=12)
            have |= {abi.CLOUD_NORMALS, abi.CLOUD_NORMAL_COUNTS}
            _check_present(c, have, "normals")
            c.compute_fpfh(knn=16)
            have |= {abi.CLOUD_DESCRIPTORS, abi.CLOUD_SPFH, abi.CLOUD_FPFH_COUNTS}
            _check_present(c, have, "fpfh")
            c.estimate_covariances(knn=12)
            have |= {abi.CLOUD_COVARIANCES, abi.CLOUD_COVARIANCE_COUNTS}
            _check_present(c, have, "covariances")
            assert have == set(ALL)
            before = abi.debug_live_resources()["device_buffers"]
            c.set_descriptors(F[NT][:, :len(c)])
            assert abi.debug_live_resources()["device_buffers"] == before - 2   # SPFH and its counts went with the FPFH
            have -= {abi.CLOUD_SPFH, abi.CLOUD_FPFH_COUNTS}
            _check_present(c, have, "set_descriptors")
            assert c.info().descriptor_dim == 8 and c.descriptors().tobytes() == F[NT][:, :len(c)].tobytes()


def test_an_empty_cloud_keeps_its_normals_through_the_voxel_stage():
    with abi.DeviceCloud(np.zeros((3, 0)), normals=np.zeros((3, 0))) as raw, raw.voxel_down_sample(0.25, return_trace=True) as c:
        for cloud in (raw, c):
            assert len(cloud) == 0 and cloud.info().has_normals
            _check_present(cloud, {abi.CLOUD_POINTS, abi.CLOUD_NORMALS}, "empty")
            L = abi.load_library()
            for what in (abi.CLOUD_POINTS, abi.CLOUD_NORMALS):
                buf = np.full(8, 7.0)
                assert L.clipper_hip_cloud_download(cloud.h, what, buf.ctypes.data_as(C.c_void_p)) == 0
                assert (buf == 7.0).all()                                # nothing was written


# ---- the box and the index side by side --------------------------------------------------------------------------------

def _fields(info):
    return [info.iterations, info.status, info.count, info.fitness, info.inlier_rmse, info.route, list(info.dim), info.candidates,
            info.history.tobytes()]


def test_box_and_index_side_by_side(scene):
    """a target first searched by the brute-force route keeps its box; the grid route then builds the index, once; the
    routes alternate after that and nothing is built again. Every result has the bytes of the host-buffer call."""
    src, tgt, T0, _ = scene
    kw = dict(T_init=T0, max_distance=MAXD, max_iterations=8)
    prev = abi.knn_search()
    try:
        host = {}
        for mode in ROUTES:
            abi.knn_set_search(mode)
            host[mode] = (abi.icp(src, tgt, **kw), abi.estimate_normals(tgt, knn=12), abi.evaluate_registration(src, tgt, T0, MAXD))

        def icp_equals_host(mode):
            T, info = cs.icp(ct, **kw)
            hT, hinfo = host[mode][0]
            assert info.route == mode and T.tobytes() == hT.tobytes() and _fields(info) == _fields(hinfo)
            assert hinfo.iterations >= 2 and hinfo.count > NS // 2       # the case does iterate on real inliers

        with abi.DeviceCloud(src) as cs, abi.DeviceCloud(tgt) as ct:
            abi.knn_set_search(abi.KNN_BRUTE)
            icp_equals_host(abi.KNN_BRUTE)
            assert ct.info().grid_builds == 0 and list(ct.info().grid_dim) == [0, 0, 0]
            abi.knn_set_search(abi.KNN_GRID)
            ct.estimate_normals(knn=12)
            assert ct.info().grid_builds == 1 and ct.normals().tobytes() == host[abi.KNN_GRID][1].tobytes()
            icp_equals_host(abi.KNN_GRID)
            assert ct.info().grid_builds == 1
            abi.knn_set_search(abi.KNN_BRUTE)
            icp_equals_host(abi.KNN_BRUTE)
            assert ct.info().grid_builds == 1 and min(ct.info().grid_dim) >= 1
            abi.knn_set_search(abi.KNN_GRID)
            assert cs.evaluate_registration(ct, T0, MAXD) == host[abi.KNN_GRID][2]
            assert ct.info().grid_builds == 1 and cs.info().grid_builds == 0
    finally:
        abi.knn_set_search(prev)
