"""GPU test of the front end's stages on clouds that live on the device (host_cloud.hpp) against their host-buffer calls
on the same inputs: voxel down-sampling, normals, FPFH, covariances. Each stage on a handle runs the body its
host-buffer call runs, on the cloud's buffers instead of on copies made for the call, so every comparison is an
equality of bytes, on both routes of the nearest-neighbour search.

Sizes: voxel n = 0 (no voxel), 1, 513 (one past a chunk of 512 of the sums, in one voxel and in many); the
neighbourhood stages n = 3 (fewer points than most neighbourhoods ask for), 64 (one wave), 300 (two workgroups) at
knn = 3, 16, 32 (the smallest, a list of 16, the longest), with and without a radius."""
import numpy as np
import pytest

from clipper_amd import _abi as abi

pytestmark = pytest.mark.gpu

ROUTES = [abi.KNN_BRUTE, abi.KNN_GRID]


@pytest.fixture(params=ROUTES, ids=["brute", "grid"])
def route(request):
    prev = abi.knn_set_search(request.param)
    yield request.param
    abi.knn_set_search(prev)


def _points(n, seed=0):
    return np.asfortranarray(np.random.default_rng(100 + n + seed).random((3, n)))


def _unit(n, seed=0):
    v = np.random.default_rng(200 + n + seed).normal(size=(3, n))
    return np.asfortranarray(v / np.linalg.norm(v, axis=0))


@pytest.mark.parametrize("with_normals", [False, True], ids=["points", "normals"])
@pytest.mark.parametrize("n,voxel_size", [(0, 0.25), (1, 0.25), (513, 0.25), (513, 2.0)])
def test_voxel(n, voxel_size, with_normals):
    P, N = _points(n), (_unit(n) if with_normals else None)
    host = abi.voxel_down_sample(P, voxel_size, N=N, return_counts=True, return_trace=True, return_info=True)
    hP, hN = host[0], (host[1] if with_normals else None)
    hcnt, htrace, hinfo = host[-3], host[-2], host[-1]
    with abi.DeviceCloud(P, normals=N) as c:
        out, info = c.voxel_down_sample(voxel_size, return_trace=True, return_info=True)
        with out:
            assert len(out) == hP.shape[1] and (n == 0 or 1 <= len(out) <= n)
            assert out.points().tobytes() == hP.tobytes()
            ci = out.info()
            assert bool(ci.has_normals) == with_normals and ci.trace_n == n
            if with_normals:
                assert out.normals().tobytes() == hN.tobytes()
            else:
                with pytest.raises(abi.ClipperError, match="error -5: .*never computed"):
                    out.normals()
            if n > 0:
                assert out.counts(abi.CLOUD_VOXEL_COUNTS).tobytes() == hcnt.tobytes()
                assert out.counts(abi.CLOUD_VOXEL_TRACE).tobytes() == htrace.tobytes()
            assert (list(info.dim), info.passes, info.sort_tile, info.chunk, info.max_count) == \
                (list(hinfo.dim), hinfo.passes, hinfo.sort_tile, hinfo.chunk, hinfo.max_count)
            if voxel_size == 2.0:
                assert len(out) == 1 and info.max_count == 513       # one voxel, two chunks of the sum
        # the input cloud is untouched, and a second run gives the same bytes
        assert c.points().tobytes() == P.tobytes()
        with c.voxel_down_sample(voxel_size) as again:
            assert again.points().tobytes() == hP.tobytes()
            if n > 0:
                with pytest.raises(abi.ClipperError, match="error -5: .*never computed"):
                    again.counts(abi.CLOUD_VOXEL_TRACE)                # (no trace was asked for)


def test_voxel_refusals():
    with abi.DeviceCloud(_points(10)) as c:
        for bad in (0.0, -1.0, np.inf, np.nan):
            with pytest.raises(abi.ClipperError, match="error -1: voxel_size must be finite and greater than 0"):
                c.voxel_down_sample(bad)
        with pytest.raises(abi.ClipperError, match="error -1: .*more than 2\\^21 voxels"):
            c.voxel_down_sample(1e-9)


@pytest.mark.parametrize("radius", [0.0, 0.35], ids=["knn", "radius"])
@pytest.mark.parametrize("knn", [3, 16, 32])
@pytest.mark.parametrize("n", [3, 64, 300])
def test_normals_fpfh_covariances(route, n, knn, radius):
    P = _points(n)
    view = np.array([0.5, 0.5, 5.0])
    hN, hncnt = abi.estimate_normals(P, knn=knn, radius=radius, viewpoint=view, return_counts=True)
    hF, hS, hfcnt = abi.compute_fpfh(P, hN, knn=knn, radius=radius, return_spfh=True)
    hC, hccnt = abi.estimate_covariances(P, knn=knn, radius=radius, epsilon=1e-3, return_counts=True)
    with abi.DeviceCloud(P) as c:
        for what in (c.normals, c.descriptors, c.spfh, c.covariances, lambda: c.counts(abi.CLOUD_NORMAL_COUNTS),
                     lambda: c.counts(abi.CLOUD_FPFH_COUNTS), lambda: c.counts(abi.CLOUD_COVARIANCE_COUNTS)):
            with pytest.raises(abi.ClipperError, match="error -5: .*never computed"):
                what()
        with pytest.raises(abi.ClipperError, match="error -5: .*the cloud has no normals"):
            c.compute_fpfh(knn=knn, radius=radius)
        c.estimate_normals(knn=knn, radius=radius, viewpoint=view)
        assert c.normals().tobytes() == hN.tobytes()
        assert c.counts(abi.CLOUD_NORMAL_COUNTS).tobytes() == hncnt.tobytes()
        c.compute_fpfh(knn=knn, radius=radius)
        assert c.info().descriptor_dim == abi.FPFH_DIM
        assert c.descriptors().tobytes() == hF.tobytes() and c.spfh().tobytes() == hS.tobytes()
        assert c.counts(abi.CLOUD_FPFH_COUNTS).tobytes() == hfcnt.tobytes()
        c.estimate_covariances(knn=knn, radius=radius, epsilon=1e-3)
        assert c.covariances().tobytes() == hC.tobytes()
        assert c.counts(abi.CLOUD_COVARIANCE_COUNTS).tobytes() == hccnt.tobytes()
        assert c.points().tobytes() == P.tobytes()
    # normals handed in at create serve compute_fpfh as the host call's N does
    with abi.DeviceCloud(P, normals=hN) as c:
        assert c.compute_fpfh(knn=knn, radius=radius).descriptors().tobytes() == hF.tobytes()


@pytest.mark.parametrize("n,normal_knn,knn", [(3, 3, 3), (64, 16, 32), (300, 32, 16), (300, 16, 16)])
def test_fpfh_from_points_equals_the_two_calls(route, n, normal_knn, knn):
    P = _points(n, seed=7)
    hN = abi.estimate_normals(P, knn=normal_knn)
    hF = abi.compute_fpfh(P, hN, knn=knn)
    oF, oN = abi.fpfh_from_points(P, normal_knn=normal_knn, knn=knn)
    assert oF.tobytes() == hF.tobytes() and oN.tobytes() == hN.tobytes()       # (what the host-buffer call promises)
    with abi.DeviceCloud(P) as c:
        c.fpfh_from_points(normal_knn=normal_knn, knn=knn)
        assert c.descriptors().tobytes() == hF.tobytes() and c.normals().tobytes() == hN.tobytes()
    with abi.DeviceCloud(P) as c:
        c.estimate_normals(knn=normal_knn).compute_fpfh(knn=knn)
        assert c.descriptors().tobytes() == hF.tobytes()


def test_a_voxel_made_cloud_feeds_the_next_stage(route):
    P = _points(2000, seed=3)
    with abi.DeviceCloud(P) as raw, raw.voxel_down_sample(0.11) as c:
        centroids = c.points()
        assert 300 < len(c) < 2000
        hN = abi.estimate_normals(centroids, knn=16)
        hF = abi.compute_fpfh(centroids, hN, knn=32)
        c.estimate_normals(knn=16).compute_fpfh(knn=32)
        assert c.normals().tobytes() == hN.tobytes() and c.descriptors().tobytes() == hF.tobytes()
        # and its descriptors match as the downloaded ones do
        hA, hsqd = abi.match_descriptors(hF, hF, knn=2, mutual=True)
        with c.match(c, knn=2, mutual=True) as pairs:
            A, sqd = pairs.download()
        assert A.tobytes() == hA.tobytes() and sqd.tobytes() == hsqd.tobytes()
        # a voxel-made cloud can be down-sampled again (its corners come from the device's fold)
        hP2 = abi.voxel_down_sample(centroids, 0.3)
        with c.voxel_down_sample(0.3) as c2:
            assert c2.points().tobytes() == hP2.tobytes()


def test_the_stages_search_the_kept_grid():
    """under the grid route every search against a cloud — the self-search of the normals, FPFH and covariance stages,
    ICP, the evaluation — queries ONE index, built at the first of them: grid_builds stays 1, and every result is the
    host-buffer call's, which builds a grid of its own per call"""
    P, Q = _points(300, seed=11), _points(200, seed=12)
    prev = abi.knn_set_search(abi.KNN_GRID)
    try:
        hN = abi.estimate_normals(P, knn=16)
        hF = abi.compute_fpfh(P, hN, knn=32)
        hC = abi.estimate_covariances(P, knn=20)
        with abi.DeviceCloud(P) as c, abi.DeviceCloud(Q) as q:
            assert c.info().grid_builds == 0
            c.estimate_normals(knn=16)
            assert c.info().grid_builds == 1 and min(c.info().grid_dim) >= 1
            dim = list(c.info().grid_dim)
            c.compute_fpfh(knn=32)
            c.estimate_covariances(knn=20)
            c.fpfh_from_points(normal_knn=16, knn=32)
            T, info = q.icp(c, method=abi.ICP_POINT_TO_PLANE, max_distance=0.3, max_iterations=5)
            ev = q.evaluate_registration(c, T, 0.3)
            assert c.info().grid_builds == 1 and list(c.info().grid_dim) == dim == list(info.dim)
            assert q.info().grid_builds == 0                         # (nothing searched the source)
            assert c.normals().tobytes() == hN.tobytes() and c.descriptors().tobytes() == hF.tobytes()
            assert c.covariances().tobytes() == hC.tobytes()
            hT, hinfo = abi.icp(Q, P, method=abi.ICP_POINT_TO_PLANE, N_tgt=hN, max_distance=0.3, max_iterations=5)
            assert T.tobytes() == hT.tobytes() and info.history.tobytes() == hinfo.history.tobytes()
            assert info.candidates == hinfo.candidates and ev == abi.evaluate_registration(Q, P, T, 0.3)
            # the brute-force route in between keeps the index, and builds none
            abi.knn_set_search(abi.KNN_BRUTE)
            c.estimate_normals(knn=16)
            assert c.info().grid_builds == 1 and c.normals().tobytes() == hN.tobytes()
    finally:
        abi.knn_set_search(prev)


def test_stage_refusals_leave_the_cloud_as_it_was():
    P = _points(50)
    with abi.DeviceCloud(P) as c:
        c.estimate_normals(knn=8)
        before = c.normals().tobytes()
        for call, msg in ((lambda: c.estimate_normals(knn=2), "knn must be in 3..32"),
                          (lambda: c.estimate_normals(knn=8, radius=np.inf), "radius must be finite"),
                          (lambda: c.estimate_normals(knn=8, viewpoint=[0.0, np.nan, 0.0]), "viewpoint: non-finite"),
                          (lambda: c.compute_fpfh(knn=33), "knn must be in 3..32"),
                          (lambda: c.estimate_covariances(knn=8, epsilon=0.0), "epsilon must be in")):
            with pytest.raises(abi.ClipperError, match="error -1: .*" + msg):
                call()
        assert c.normals().tobytes() == before and c.info().descriptor_dim == 0 and not c.info().has_covariances
    with abi.DeviceCloud(np.zeros((3, 0))) as empty:
        with pytest.raises(abi.ClipperError, match="error -1: .*a cloud needs at least one point"):
            empty.estimate_normals()
