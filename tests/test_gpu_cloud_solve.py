"""GPU test of staging a solve from clouds that live on the device (clipper_hip_stage_inputs_clouds: host_cloud.hpp, the
max-abs fold and the point-then-normal table of k_cloud.hip.h) against clipper_hip_stage_inputs on the same arrays:
after the same _staged fill and solve_staged the two contexts hold the same u bytes, the same selected set and the
same clipper_solve_info_t (all of it but the wall time). And of clipper_hip_cloud_gather_points, whose selected points
give clipper_hip_estimate_rigid_transform the fit the host arrays give it.

Sizes: m = 1, 64, 65 (the point tables' stride rounds m up to 64) and 500, from the synthetic registration data set of
clipper_amd.registration."""
import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import registration as reg

pytestmark = pytest.mark.gpu

MS = [1, 64, 65, 500]


def _dataset(m, seed=0):
    rng = np.random.default_rng(77 + seed)
    model = rng.random((4000, 3))
    T = np.eye(4)
    T[:3, :3] = reg.random_rotation(rng)
    T[:3, 3] = [0.3, -0.2, 0.1]
    D1, D2, A, Agt = reg.make_registration_dataset(model, m, 600, 40, 0.3 if m > 1 else 0.0, 0.01, T, seed=seed)
    return np.asfortranarray(D1), np.asfortranarray(D2), A, Agt


def _unit(n, seed):
    v = np.random.default_rng(seed).normal(size=(3, n))
    return np.asfortranarray(v / np.linalg.norm(v, axis=0))


def _solution(g, u0):
    g.stage_u0(u0)
    s = g.solve_staged()
    return (s.u.tobytes(), s.nodes.tobytes(), s.score, s.ifinal, s.d, s.n_passes, s.n_trials,
            g.get_selected_associations().tobytes(), g.get_initial_associations().tobytes())


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64], ids=["f32_csc", "f64"])
@pytest.mark.parametrize("m", MS)
def test_euclidean_solve_from_clouds(m, storage):
    D1, D2, A, _ = _dataset(m)
    u0 = np.random.default_rng(m).random(m)
    host = abi.HipClipper(storage=storage)
    host.stage_inputs(D1, D2, A)
    host.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
    want = _solution(host, u0)
    with abi.DeviceCloud(D1) as c1, abi.DeviceCloud(D2) as c2, abi.DevicePairs(A) as pairs:
        dev = abi.HipClipper(storage=storage)
        dev.stage_inputs_clouds(c1, c2, pairs)
    # (the clouds and the pairs are gone: what was staged is the context's own)
    assert dev.m == m
    dev.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
    got = _solution(dev, u0)
    assert got == want
    if m >= 64:
        assert len(host.soln.nodes) >= 3                                 # a real clique, not an empty answer
    host.close()
    dev.close()


@pytest.mark.parametrize("m", MS)
def test_pointnormal_solve_from_clouds(m):
    D1, D2, A, _ = _dataset(m, seed=1)
    N1, N2 = _unit(D1.shape[1], 5), _unit(D2.shape[1], 6)
    u0 = np.random.default_rng(m).random(m)
    host = abi.HipClipper(storage=abi.STORE_F32_CSC)
    host.stage_inputs(np.vstack([D1, N1]), np.vstack([D2, N2]), A)
    host.affinity_pointnormal_staged()
    want = _solution(host, u0)
    dev = abi.HipClipper(storage=abi.STORE_F32_CSC)
    with abi.DeviceCloud(D1, normals=N1) as c1, abi.DeviceCloud(D2, normals=N2) as c2, abi.DevicePairs(A) as pairs:
        dev.stage_inputs_clouds(c1, c2, pairs, with_normals=True)
        dev.affinity_pointnormal_staged()
        assert _solution(dev, u0) == want
        # the same context staged again, now without normals: the Euclidean fill of the host arrays
        dev.stage_inputs_clouds(c1, c2, pairs)
        dev.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
        host.stage_inputs(D1, D2, A)
        host.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
        assert _solution(dev, u0) == _solution(host, u0)
    host.close()
    dev.close()


def test_the_prefilter_guard_sees_the_host_value():
    """max |coordinate| decides the fp32 prefilter's threshold: the largest magnitude sits in the LAST point of the
    second cloud, negative, far from every workgroup's first element; the solutions agree only if the device's fold
    found it"""
    D1, D2, A, _ = _dataset(500, seed=2)
    D2[2, -1] = -3.0e3
    u0 = np.random.default_rng(9).random(len(A))
    host = abi.HipClipper(storage=abi.STORE_F32_CSC)
    host.stage_inputs(D1, D2, A)
    host.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
    dev = abi.HipClipper(storage=abi.STORE_F32_CSC)
    with abi.DeviceCloud(D1) as c1, abi.DeviceCloud(D2) as c2, abi.DevicePairs(A) as pairs:
        dev.stage_inputs_clouds(c1, c2, pairs)
    dev.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
    assert _solution(dev, u0) == _solution(host, u0)
    assert dev.get_affinity_matrix().tobytes() == host.get_affinity_matrix().tobytes()
    assert dev.get_constraint_matrix().tobytes() == host.get_constraint_matrix().tobytes()
    host.close()
    dev.close()


def test_gathered_points_give_the_host_fit():
    D1, D2, A, Agt = _dataset(500, seed=3)
    sel = A[:len(Agt)][::3]                                              # some of the correct pairs, in list order
    want = abi.estimate_rigid_transform(D1, D2, sel)
    with abi.DeviceCloud(D1) as c1, abi.DeviceCloud(D2) as c2:
        G1, G2 = c1.gather_points(sel[:, 0]), c2.gather_points(sel[:, 1])
        assert G1.tobytes() == np.asfortranarray(D1[:, sel[:, 0]]).tobytes()
        assert G2.tobytes() == np.asfortranarray(D2[:, sel[:, 1]]).tobytes()
        k = len(sel)
        got = abi.estimate_rigid_transform(G1, G2, np.stack([np.arange(k)] * 2, axis=1))
        assert got.tobytes() == want.tobytes()
        assert c1.gather_points([]).shape == (3, 0)
        assert c1.gather_points([5, 5, 0]).tobytes() == np.asfortranarray(D1[:, [5, 5, 0]]).tobytes()   # repeats, any order
        for bad in ([-1], [D1.shape[1]]):
            with pytest.raises(abi.ClipperError, match="error -1: .*outside the cloud's"):
                c1.gather_points(bad)


def test_refusals():
    D1, D2, A, _ = _dataset(64, seed=4)
    with abi.DeviceCloud(D1) as c1, abi.DeviceCloud(D2) as c2, abi.DevicePairs(A) as pairs:
        grp = abi.HipClipper(storage=abi.STORE_F32_CSC, group=[0, 0])    # column shards
        with pytest.raises(abi.ClipperError, match="error -7: .*one-shard contexts only"):   # CLIPPER_HIP_E_SCOPE
            grp.stage_inputs_clouds(c1, c2, pairs)
        grp.close()
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        with pytest.raises(abi.ClipperError, match="error -5: .*needs the normals of both clouds"):
            g.stage_inputs_clouds(c1, c2, pairs, with_normals=True)
        with abi.DevicePairs() as none:
            with pytest.raises(abi.ClipperError, match="error -1: .*no associations"):
                g.stage_inputs_clouds(c1, c2, none)
        far = A.copy()
        far[3, 1] = D2.shape[1]                                          # one past the second cloud
        with abi.DevicePairs(far) as p:
            with pytest.raises(abi.ClipperError, match="error -1: association 3 = .* out of range"):
                g.stage_inputs_clouds(c1, c2, p)
        g.stage_inputs_clouds(c1, c2, pairs)                            # and the context is still usable
        g.affinity_euclidean_staged(sigma=0.015, epsilon=0.05)
        assert g.m == 64
        g.close()
