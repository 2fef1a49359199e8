"""GPU test of the facades over the clouds that live on the device: clipper_amd.registration.DeviceCloud / DevicePairs
(ctypes, clipper_amd/_abi.py) and clipperpy.utils.DeviceCloud / DevicePairs (pybind11 over
include/clipper/device_cloud.h), with CLIPPER.score_pairwise_consistency on them. Every facade returns the bytes of the
host-buffer calls; close() twice is harmless; a handle used after close() raises and does not crash."""
import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration as reg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(11)
    xy = rng.random((2, 400))
    P0 = np.asfortranarray(np.vstack([xy, 0.3 * np.sin(4.0 * xy[0]) + 0.2 * xy[1] ** 2]))
    a = 0.04
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    P1 = np.asfortranarray(R @ P0[:, :350] + np.array([[0.01], [0.02], [-0.01]]))
    return P0, P1


def _host_chain(P0, P1):
    N0, N1 = abi.estimate_normals(P0, knn=16), abi.estimate_normals(P1, knn=16)
    F0, F1 = abi.compute_fpfh(P0, N0, knn=32), abi.compute_fpfh(P1, N1, knn=32)
    A, sqd = abi.match_descriptors(F1, F0, knn=2, mutual=True)
    return N0, N1, F0, F1, A, sqd


def test_ctypes_round_trip(clouds):
    P0, P1 = clouds
    N0, N1, F0, F1, A, sqd = _host_chain(P0, P1)
    assert reg.DeviceCloud is abi.DeviceCloud and reg.DevicePairs is abi.DevicePairs
    with reg.DeviceCloud(P0) as c0, reg.DeviceCloud(P1) as c1:
        assert len(c0) == 400 and len(c1) == 350 and c0.points().tobytes() == P0.tobytes()
        c0.estimate_normals(knn=16).compute_fpfh(knn=32)
        c1.fpfh_from_points(normal_knn=16, knn=32)
        assert c0.normals().tobytes() == N0.tobytes() and c1.normals().tobytes() == N1.tobytes()
        assert c0.descriptors().tobytes() == F0.tobytes() and c1.descriptors().tobytes() == F1.tobytes()
        with c1.match(c0, knn=2, mutual=True) as pairs:
            gA, gs = pairs.download()
            assert len(A) > 50 and gA.tobytes() == A.tobytes() and gs.tobytes() == sqd.tobytes()
            # descriptors -> pairs -> staged solve -> gathered points -> closed-form transform -> plane ICP, all on handles
            g = abi.HipClipper(storage=abi.STORE_F32_CSC)
            g.stage_inputs_clouds(c1, c0, pairs)
            g.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
            h = abi.HipClipper(storage=abi.STORE_F32_CSC)
            h.stage_inputs(P1, P0, A)
            h.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
            u0 = np.random.default_rng(1).random(len(A))
            g.stage_u0(u0)
            h.stage_u0(u0)
            sg, sh = g.solve_staged(), h.solve_staged()
            assert sg.u.tobytes() == sh.u.tobytes() and np.array_equal(sg.nodes, sh.nodes) and len(sg.nodes) >= 3
            sel = g.get_selected_associations()
            k = len(sel)
            T = abi.estimate_rigid_transform(c1.gather_points(sel[:, 0]), c0.gather_points(sel[:, 1]),
                                             np.stack([np.arange(k)] * 2, axis=1))
            assert T.tobytes() == abi.estimate_rigid_transform(P1, P0, sel).tobytes()
            Ti, info = c1.icp(c0, T_init=T, method=abi.ICP_POINT_TO_PLANE, max_distance=0.1)
            Th, hinfo = abi.icp(P1, P0, T_init=T, method=abi.ICP_POINT_TO_PLANE, N_tgt=N0, max_distance=0.1)
            assert Ti.tobytes() == Th.tobytes() and info.history.tobytes() == hinfo.history.tobytes()
            assert info.fitness > 0.9
            g.close()
            h.close()


def test_ctypes_close_twice_and_use_after_close(clouds):
    P0, _ = clouds
    c = reg.DeviceCloud(P0)
    p = reg.DevicePairs(np.array([[0, 1], [2, 3]]))
    other = reg.DeviceCloud(P0)
    c.close()
    c.close()
    p.close()
    p.close()
    for call in (lambda: len(c), c.points, c.info, c.estimate_normals, lambda: c.match(other), lambda: other.match(c),
                 lambda: c.icp(other, max_distance=1.0), lambda: other.icp(c, max_distance=1.0), lambda: c.voxel_down_sample(0.1),
                 lambda: len(p), p.download):
        with pytest.raises(abi.ClipperError, match="is closed"):
            call()
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    with pytest.raises(abi.ClipperError, match="is closed"):
        g.stage_inputs_clouds(other, other, p)
    g.close()
    assert other.points().tobytes() == P0.tobytes()                  # the library is as usable as before
    other.close()
    live = abi.debug_live_resources()
    del c, p, other
    assert abi.debug_live_resources() == live                        # (nothing was left to free)


def test_clipperpy_round_trip(clouds):
    P0, P1 = clouds
    N0, N1, F0, F1, A, sqd = _host_chain(P0, P1)
    cp = clipper_amd.load_clipperpy()
    with cp.utils.DeviceCloud(P0) as c0, cp.utils.DeviceCloud(P1, normals=N1) as c1:
        assert len(c0) == 400 and np.asarray(c0.points()).tobytes(order="F") == P0.tobytes(order="F")
        c0.estimate_normals(knn=16)
        c0.compute_fpfh(knn=32)
        c1.compute_fpfh(knn=32)
        assert np.asarray(c0.normals()).tobytes(order="F") == N0.tobytes(order="F")
        assert np.asarray(c0.descriptors()).tobytes(order="F") == F0.tobytes(order="F")
        assert np.asarray(c1.descriptors()).tobytes(order="F") == F1.tobytes(order="F")
        with c1.match(c0, knn=2, mutual=True) as pairs:
            assert len(pairs) == len(A)
            gA, gs = pairs.download_with_sqd()
            assert np.array_equal(np.asarray(gA), A) and np.asarray(gs).tobytes() == sqd.tobytes()
            # CLIPPER scores from the handles what it scores from the arrays
            iparams = cp.invariants.EuclideanDistanceParams()
            iparams.sigma, iparams.epsilon = 0.015, 0.05
            u0 = np.random.default_rng(1).random(len(A))
            sols = []
            for from_clouds in (True, False):
                solver = cp.CLIPPER(cp.invariants.EuclideanDistance(iparams), cp.Params())
                if from_clouds:
                    solver.score_pairwise_consistency(c1, c0, pairs)
                else:
                    solver.score_pairwise_consistency(P1, P0, A)
                solver.solve(u0)
                sols.append((np.asarray(solver.get_solution().u).tobytes(), np.asarray(solver.get_selected_associations()).tobytes(),
                             np.asarray(solver.get_initial_associations()).tobytes()))
            assert sols[0] == sols[1]
        T, info = c1.icp(c0, method="plane", max_distance=0.1, max_iterations=10)
        Th, hinfo = abi.icp(P1, P0, method=abi.ICP_POINT_TO_PLANE, N_tgt=N0, max_distance=0.1, max_iterations=10)
        assert np.asarray(T).tobytes(order="F") == Th.tobytes(order="F")
        assert np.asarray(info["history"]).tobytes(order="C") == hinfo.history.tobytes(order="C")
        assert c0.grid_builds() in (0, 1) and c0.info()["grid_builds"] == c0.grid_builds()
        assert c0.info()["n"] == 400 and c0.info()["descriptor_dim"] == 33 and c0.info()["has_normals"]
        assert np.asarray(c0.counts("normals")).tobytes() == abi.estimate_normals(P0, knn=16, return_counts=True)[1].tobytes()
        with pytest.raises(ValueError, match="what must be"):
            c0.counts("nothing")
        with pytest.raises(ValueError, match="method must be"):
            c1.icp(c0, method="planar", max_distance=0.1)
        Tr, ir = c1.icp(c0, method="plane", max_distance=0.1, max_iterations=10, loss="huber", scale=0.02, trim=0.9)
        Thr, hr = abi.icp_robust(P1, P0, method=abi.ICP_POINT_TO_PLANE, N_tgt=N0, max_distance=0.1, max_iterations=10,
                                 loss=abi.ICP_LOSS_HUBER, scale=0.02, trim=0.9)
        assert np.asarray(Tr).tobytes(order="F") == Thr.tobytes(order="F") and ir["within"] == hr.within
        assert c1.evaluate_registration(c0, T, 0.1) == abi.evaluate_registration(P1, P0, np.asarray(T), 0.1)
        with cp.utils.DeviceCloud(P1) as c2:
            c2.fpfh_from_points(normal_knn=16, knn=32)
            assert np.asarray(c2.descriptors()).tobytes(order="F") == F1.tobytes(order="F")
        with cp.utils.DevicePairs(A, sqd=sqd) as p2, cp.utils.DevicePairs(A) as p3:
            assert p2.has_sqd and not p3.has_sqd and len(p2) == len(A)
            assert np.asarray(p2.download_with_sqd()[1]).tobytes() == sqd.tobytes()
        G = np.asarray(c0.gather_points([3, 1, 3]))
        assert G.tobytes(order="F") == P0[:, [3, 1, 3]].tobytes(order="F")
        with c0.voxel_down_sample(0.2, return_trace=True) as v:
            hP, hcnt, htrace = abi.voxel_down_sample(P0, 0.2, return_counts=True, return_trace=True)
            assert np.asarray(v.points()).tobytes(order="F") == hP.tobytes(order="F")
            assert np.asarray(v.counts("voxel")).tobytes() == hcnt.tobytes()
            assert np.asarray(v.counts("voxel_trace")).tobytes() == htrace.tobytes()


def test_clipperpy_close_twice_and_use_after_close(clouds):
    P0, _ = clouds
    cp = clipper_amd.load_clipperpy()
    c, other = cp.utils.DeviceCloud(P0), cp.utils.DeviceCloud(P0)
    p = cp.utils.DevicePairs(np.array([[0, 1], [2, 3]], dtype=np.int32))
    c.close()
    c.close()
    p.close()
    p.close()
    for call in (lambda: len(c), c.points, c.estimate_normals, lambda: c.match(other), lambda: other.match(c),
                 lambda: other.icp(c, max_distance=1.0), lambda: len(p), p.download):
        with pytest.raises(RuntimeError, match="closed or empty handle"):
            call()
    with pytest.raises(ValueError, match="not of unit length"):     # CLIPPER_HIP_E_INVALID -> std::invalid_argument
        cp.utils.DeviceCloud(P0, normals=2.0 * np.ones((3, 400)))
    with pytest.raises(RuntimeError, match="has no descriptors"):   # CLIPPER_HIP_E_STATE
        other.match(other)
    assert np.asarray(other.points()).tobytes(order="F") == P0.tobytes(order="F")
    other.close()
