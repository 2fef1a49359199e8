"""GPU test of ICP and evaluate_registration on clouds that live on the device (clipper_hip_cloud_icp,
clipper_hip_cloud_evaluate_registration: host_cloud.hpp over host_icp.hpp's icp_body) against the host-buffer calls on
the same inputs, on both routes of the search: T_out, the history and every info field but the device time, byte for
byte. And what the handles add: the target's grid is built at the first call against a cloud and KEPT.

Sizes: a source of 200 points against a target of 300 (two workgroups of sources, a target of several grid cells)."""
import numpy as np
import pytest

from clipper_amd import _abi as abi

pytestmark = pytest.mark.gpu

NS, NT = 200, 300
MAXD = 0.25


@pytest.fixture(scope="module")
def scene():
    """a wavy sheet sampled twice: the target, and a source that is a moved, jittered part of it"""
    rng = np.random.default_rng(42)
    xy = rng.random((2, NT))
    tgt = np.asfortranarray(np.vstack([xy, 0.2 * np.sin(3.0 * xy[0]) * np.cos(2.0 * xy[1])]))
    a = 0.05
    R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    src = np.asfortranarray(R @ tgt[:, :NS] + np.array([[0.02], [-0.01], [0.015]]) + 1e-3 * rng.normal(size=(3, NS)))
    prev = abi.knn_set_search(abi.KNN_BRUTE)
    Nt = abi.estimate_normals(tgt, knn=12)
    Cs, Ct = abi.estimate_covariances(src, knn=12), abi.estimate_covariances(tgt, knn=12)
    abi.knn_set_search(prev)
    T0 = np.eye(4)
    T0[:3, 3] = [0.01, 0.0, -0.01]
    return src, tgt, Nt, Cs, Ct, T0


@pytest.fixture(params=[abi.KNN_BRUTE, abi.KNN_GRID], ids=["brute", "grid"])
def route(request):
    prev = abi.knn_set_search(request.param)
    yield request.param
    abi.knn_set_search(prev)


def _clouds(scene, normals=True, covariances=True):
    """the scene on the device; the covariances are estimated there, by the stage whose bytes the host's Cs / Ct are"""
    src, tgt, Nt, _, _, _ = scene
    cs, ct = abi.DeviceCloud(src), abi.DeviceCloud(tgt, normals=Nt if normals else None)
    if covariances:
        prev = abi.knn_set_search(abi.KNN_BRUTE)
        cs.estimate_covariances(knn=12)
        ct.estimate_covariances(knn=12)
        abi.knn_set_search(prev)
    return cs, ct


def _fields(info):
    out = [info.iterations, info.status, info.count, info.fitness, info.inlier_rmse, info.route, list(info.dim), info.candidates,
           info.history.tobytes()]
    for name in ("within", "weight_sum", "trim_sqd"):
        if hasattr(info, name):
            out.append(getattr(info, name))
    return out


CONFIGS = {
    "point": dict(method=abi.ICP_POINT_TO_POINT),
    "plane": dict(method=abi.ICP_POINT_TO_PLANE),
    "generalized": dict(method=abi.ICP_GENERALIZED),
    "robust_trimmed_plane": dict(method=abi.ICP_POINT_TO_PLANE, loss=abi.ICP_LOSS_HUBER, scale=0.02, trim=0.8),
    "robust_trimmed_generalized": dict(method=abi.ICP_GENERALIZED, loss=abi.ICP_LOSS_CAUCHY, scale=0.05, trim=0.9),
}


def _host(scene, method, loss=None, scale=0.0, trim=1.0, max_iterations=12):
    src, tgt, Nt, Cs, Ct, T0 = scene
    kw = dict(T_init=T0, max_distance=MAXD, max_iterations=max_iterations)
    if method == abi.ICP_GENERALIZED:
        if loss is None:
            return abi.icp_generalized(src, Cs, tgt, Ct, **kw)
        return abi.icp_generalized_robust(src, Cs, tgt, Ct, loss=loss, scale=scale, trim=trim, **kw)
    if loss is None:
        return abi.icp(src, tgt, method=method, N_tgt=Nt, **kw)
    return abi.icp_robust(src, tgt, method=method, N_tgt=Nt, loss=loss, scale=scale, trim=trim, **kw)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_icp_equals_the_host_route(scene, route, name):
    cfg = CONFIGS[name]
    hT, hinfo = _host(scene, **cfg)
    assert hinfo.iterations >= 2 and hinfo.count > NS // 2               # the case does iterate on real inliers
    cs, ct = _clouds(scene)
    with cs, ct:
        T, info = cs.icp(ct, T_init=scene[5], max_distance=MAXD, max_iterations=12, **cfg)
        assert T.tobytes() == hT.tobytes()
        assert _fields(info) == _fields(hinfo)
        assert info.route == route
        assert ct.info().grid_builds == (1 if route == abi.KNN_GRID else 0)


def test_evaluation_equals_the_host_route(scene, route):
    src, tgt, _, _, _, T0 = scene
    want = abi.evaluate_registration(src, tgt, T0, MAXD, return_correspondences=True)
    cs, ct = _clouds(scene, covariances=False)
    with cs, ct:
        got = cs.evaluate_registration(ct, T0, MAXD, return_correspondences=True)
        assert got[:3] == want[:3] and got[3].tobytes() == want[3].tobytes()
        assert want[2] > NS // 2


def test_the_grid_is_built_once_and_kept(scene):
    src, tgt, Nt, _, _, T0 = scene
    prev = abi.knn_set_search(abi.KNN_GRID)
    try:
        hT, hinfo = _host(scene, abi.ICP_POINT_TO_PLANE)
        cs, ct = _clouds(scene, covariances=False)
        with cs, ct:
            assert ct.info().grid_builds == 0 and list(ct.info().grid_dim) == [0, 0, 0]
            T1, i1 = cs.icp(ct, T_init=T0, method=abi.ICP_POINT_TO_PLANE, max_distance=MAXD, max_iterations=12)
            assert ct.info().grid_builds == 1 and list(ct.info().grid_dim) == list(i1.dim) and min(i1.dim) >= 1
            T2, i2 = cs.icp(ct, T_init=T0, method=abi.ICP_POINT_TO_PLANE, max_distance=MAXD, max_iterations=12)
            ev = cs.evaluate_registration(ct, T1, MAXD)
            assert ct.info().grid_builds == 1                            # two ICP calls and an evaluation: one build
            assert cs.info().grid_builds == 0                            # (nothing was searched against the source)
            assert T2.tobytes() == T1.tobytes() == hT.tobytes() and _fields(i2) == _fields(i1) == _fields(hinfo)
            assert ev == abi.evaluate_registration(src, tgt, T1, MAXD)
            # the other way round builds the source's grid, once
            cs.evaluate_registration(cs, None, MAXD)
            ct.evaluate_registration(cs, None, MAXD)
            assert cs.info().grid_builds == 1 and ct.info().grid_builds == 1
    finally:
        abi.knn_set_search(prev)


def test_switching_the_route_between_calls_keeps_the_bytes(scene):
    T0 = scene[5]
    prev = abi.knn_set_search(abi.KNN_BRUTE)
    try:
        cs, ct = _clouds(scene)
        with cs, ct:
            runs = []
            for mode in (abi.KNN_BRUTE, abi.KNN_GRID, abi.KNN_BRUTE, abi.KNN_GRID):
                abi.knn_set_search(mode)
                T, info = cs.icp(ct, T_init=T0, method=abi.ICP_GENERALIZED, max_distance=MAXD, max_iterations=12)
                assert info.route == mode
                hT, hinfo = _host(scene, abi.ICP_GENERALIZED)
                assert T.tobytes() == hT.tobytes() and _fields(info) == _fields(hinfo)
                runs.append((T.tobytes(), info.history.tobytes(), info.count))
            assert all(r == runs[0] for r in runs) and ct.info().grid_builds == 1
    finally:
        abi.knn_set_search(prev)


def test_missing_attachments_and_bad_arguments(scene):
    src, tgt, Nt, _, _, T0 = scene
    with abi.DeviceCloud(src) as cs, abi.DeviceCloud(tgt) as ct:
        with pytest.raises(abi.ClipperError, match="error -5: .*point-to-plane needs the target's normals"):    # E_STATE
            cs.icp(ct, method=abi.ICP_POINT_TO_PLANE, max_distance=MAXD)
        with pytest.raises(abi.ClipperError, match="error -5: .*needs the covariances of both clouds"):
            cs.icp(ct, method=abi.ICP_GENERALIZED, max_distance=MAXD)
        ct.estimate_covariances(knn=12)
        with pytest.raises(abi.ClipperError, match="error -5: .*needs the covariances of both clouds"):           # the source's
            cs.icp(ct, method=abi.ICP_GENERALIZED, max_distance=MAXD)
        for kw, msg in ((dict(max_distance=0.0), "max_distance must be positive"), (dict(method=7, max_distance=1.0), "unknown method 7"),
                        (dict(max_distance=1.0, max_iterations=-1), "max_iterations must be in"),
                        (dict(max_distance=1.0, loss=9), "unknown loss 9"), (dict(max_distance=1.0, loss=0, trim=0.0), "trim must be in")):
            with pytest.raises(abi.ClipperError, match="error -1: cloud_icp: " + msg):
                cs.icp(ct, **kw)
        bad = np.eye(4)
        bad[3, 0] = 0.5
        with pytest.raises(abi.ClipperError, match="error -1: cloud_icp: T_init: the bottom row"):
            cs.icp(ct, T_init=bad, max_distance=1.0)
        with pytest.raises(abi.ClipperError, match="error -1: cloud_evaluate_registration: max_distance must be positive"):
            cs.evaluate_registration(ct, None, -1.0)
        with abi.DeviceCloud(np.zeros((3, 0))) as empty:
            with pytest.raises(abi.ClipperError, match="error -1: .*a cloud needs at least one point"):
                cs.icp(empty, max_distance=1.0)
        T, info = cs.icp(ct, T_init=T0, max_distance=MAXD)           # and the clouds are still usable
        assert info.count > 0
