"""CPU-side checks of the ICP entry points (clipper_hip_icp, clipper_hip_evaluate_registration): the struct layouts
against a C program, the refusals (every check runs on the host before any device work, so they answer with no device
present, each naming its value), and clipper_hip_estimate_rigid_transform, whose rotation fit moved into
clipper_amd/csrc/icp_rules.hpp: its bits are the ones it gave before the move."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from tests import icp_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_match_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu '
                   '%d %d %d %d %d %d\\n", sizeof(clipper_icp_params_t), offsetof(clipper_icp_params_t, max_distance),'
                   'offsetof(clipper_icp_params_t, rel_rmse), sizeof(clipper_icp_info_t), offsetof(clipper_icp_info_t, route),'
                   'offsetof(clipper_icp_info_t, candidates), offsetof(clipper_icp_info_t, device_ms),'
                   'CLIPPER_ICP_POINT_TO_POINT, CLIPPER_ICP_POINT_TO_PLANE, CLIPPER_ICP_CONVERGED, CLIPPER_ICP_MAX_ITERATIONS,'
                   'CLIPPER_ICP_TOO_FEW, CLIPPER_ICP_DEGENERATE);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:7] == [C.sizeof(abi.IcpParams), abi.IcpParams.max_distance.offset, abi.IcpParams.rel_rmse.offset,
                       C.sizeof(abi.IcpInfo), abi.IcpInfo.route.offset, abi.IcpInfo.candidates.offset,
                       abi.IcpInfo.device_ms.offset] == [32, 8, 24, 64, 32, 48, 56]
    assert got[7:] == [abi.ICP_POINT_TO_POINT, abi.ICP_POINT_TO_PLANE, abi.ICP_CONVERGED, abi.ICP_MAX_ITERATIONS,
                       abi.ICP_TOO_FEW, abi.ICP_DEGENERATE] == [im.POINT, im.PLANE, im.CONVERGED, im.MAX_ITERATIONS,
                                                                im.TOO_FEW, im.DEGENERATE]
    p = abi.IcpParams(max_distance=0.1)
    assert (p.method, p.max_iterations, p.rel_fitness, p.rel_rmse) == (0, 30, 1e-6, 1e-6)


def _refusals():
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    P = np.ascontiguousarray(np.arange(12, dtype=np.float64).reshape(4, 3) / 7.0)
    bad = P.copy()
    bad[2, 1] = np.inf
    N = np.tile((0.0, 0.0, 1.0), (4, 1))
    long_n = N * 1.5
    I = np.eye(4).T.reshape(-1).copy()
    row, nan = I.copy(), I.copy()
    row[11] = 2.0            # column-major: entry (3, 2)
    nan[12] = np.nan         # entry (0, 3)
    T = np.zeros(16)
    ok = abi.IcpParams(abi.ICP_POINT_TO_POINT, 0.1)
    plane = abi.IcpParams(abi.ICP_POINT_TO_PLANE, 0.1)
    icp = lambda *a: ("icp", a)    # noqa: E731
    ev = lambda *a: ("ev", a)      # noqa: E731
    r = C.byref
    return [
        (icp(0, None, 4, dp(P), None, 4, None, r(ok), dp(T), None, None), "null source point array"),
        (icp(0, dp(P), 4, None, None, 4, None, r(ok), dp(T), None, None), "null target point array"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(ok), None, None, None), "null T_out"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, None, dp(T), None, None), "null params"),
        (icp(0, dp(P), 0, dp(P), None, 4, None, r(ok), dp(T), None, None), "source: a cloud needs at least one point (n = 0)"),
        (icp(0, dp(P), 4, dp(P), None, -3, None, r(ok), dp(T), None, None), "target: a cloud needs at least one point (n = -3)"),
        (icp(0, dp(P), 4, dp(P), None, 2 ** 31, None, r(ok), dp(T), None, None), "target: more than 2^31 - 1 points in a cloud (n = 2147483648)"),
        (icp(0, dp(bad), 4, dp(P), None, 4, None, r(ok), dp(T), None, None), "source: non-finite value at coordinate 1 of point 2"),
        (icp(0, dp(P), 4, dp(bad), None, 4, None, r(ok), dp(T), None, None), "target: non-finite value at coordinate 1 of point 2"),
        (icp(0, dp(P), 4, dp(P), None, 4, dp(nan), r(ok), dp(T), None, None), "T_init: non-finite value at entry (0, 3)"),
        (icp(0, dp(P), 4, dp(P), None, 4, dp(row), r(ok), dp(T), None, None), "T_init: the bottom row must be 0 0 0 1 (entry (3, 2) = 2)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(plane), dp(T), None, None), "point-to-plane needs the target's normals (N_tgt is null)"),
        (icp(0, dp(P), 4, dp(P), dp(long_n), 4, None, r(plane), dp(T), None, None), "normal 0 is not of unit length (squared length = 2.25)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(7, 0.1)), dp(T), None, None), "unknown method 7"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(0, -1.0)), dp(T), None, None), "max_distance must be positive and finite (max_distance = -1)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(0, np.inf)), dp(T), None, None), "max_distance must be positive and finite (max_distance = inf)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(0, 0.1, 1001)), dp(T), None, None), "max_iterations must be in 0..1000 (max_iterations = 1001)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(0, 0.1, -1)), dp(T), None, None), "max_iterations must be in 0..1000 (max_iterations = -1)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(0, 0.1, 30, -1e-3)), dp(T), None, None), "rel_fitness must be at least 0 (rel_fitness = -0.001)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(0, 0.1, 30, 0.0, np.nan)), dp(T), None, None), "rel_rmse must be at least 0 (rel_rmse = nan)"),
        (ev(0, None, 4, dp(P), 4, None, 0.1, None, None, None, None), "null source point array"),
        (ev(0, dp(P), 4, dp(P), 0, None, 0.1, None, None, None, None), "target: a cloud needs at least one point (n = 0)"),
        (ev(0, dp(P), 4, dp(bad), 4, None, 0.1, None, None, None, None), "target: non-finite value at coordinate 1 of point 2"),
        (ev(0, dp(P), 4, dp(P), 4, dp(row), 0.1, None, None, None, None), "T: the bottom row must be 0 0 0 1 (entry (3, 2) = 2)"),
        (ev(0, dp(P), 4, dp(P), 4, None, 0.0, None, None, None, None), "max_distance must be positive and finite (max_distance = 0)"),
    ], (P, bad, N, long_n, I, row, nan, T, ok, plane)


def test_refusals_name_their_values_without_a_device():
    L = abi.load_library()
    cases, keep = _refusals()
    for (which, args), text in cases:
        fn = L.clipper_hip_icp if which == "icp" else L.clipper_hip_evaluate_registration
        rc = fn(*args)
        msg = abi._last_error()
        assert rc == -1 and text in msg, (rc, msg, text)      # CLIPPER_HIP_E_INVALID
    assert keep


def test_python_facade_refuses_before_the_library():
    from clipper_amd import registration as reg
    P = np.zeros((4, 3))
    with pytest.raises(ValueError):
        reg.icp(P, P, method="colour", max_distance=0.1)
    with pytest.raises(ValueError):
        reg.icp(P, P, T_init=np.eye(3), max_distance=0.1)
    with pytest.raises(ValueError):
        reg.icp(P, P, max_distance=0.1, search="tree")
    with pytest.raises(abi.ClipperError, match="max_distance must be positive"):
        reg.evaluate_registration(P, P)


# T (column-major) of clipper_hip_estimate_rigid_transform on the fixture below, as the library gave it before
# rotation_from_cross_covariance moved into icp_rules.hpp
RIGID_BITS = """bf2521baae107ca0 3fefffffbc7922dc 3f3f201ae024bac0 0000000000000000 bfefffffad8ebc68 bf25194738c35560
bf41606b19081400 0000000000000000 bf415fc6c71d0400 bf3f2189c2d70740 3fefffff77f6b3db 0000000000000000 3feffbf334de2183
400002aeed49e9dd 4008009518713ff5 3ff0000000000000"""


def test_estimate_rigid_transform_bits_unchanged():
    P = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_points_4096.f32"), dtype="<f4").reshape(-1, 3).astype(np.float64)
    k = 60
    D1, E = P[:k], P[100:100 + k] * 0.01
    perm = (np.arange(k) * 7) % k
    Q = np.stack([-D1[:, 1] + 1.0, D1[:, 0] + 2.0, D1[:, 2] + 3.0], axis=1) + E      # a quarter turn about z, a shift, a perturbation
    D2 = np.zeros_like(Q)
    D2[perm] = Q
    A = np.stack([np.arange(k), perm], axis=1).astype(np.int32)
    T = abi.estimate_rigid_transform(D1.T, D2.T, A)
    want = np.array([int(x, 16) for x in RIGID_BITS.split()], np.uint64).view(np.float64).reshape(4, 4).T
    assert T.tobytes() == want.tobytes()
    # and the model's restatement of the rotation fit gives the same rotation from the same cross-covariance
    cp, cq = np.zeros(3), np.zeros(3)
    for i in range(k):
        cp, cq = cp + D1[A[i, 0]], cq + D2[A[i, 1]]
    cp, cq = cp / float(k), cq / float(k)
    H = np.zeros((3, 3))
    for i in range(k):
        H = H + np.outer(D2[A[i, 1]] - cq, D1[A[i, 0]] - cp)
    R = np.array(im.rotation_from_cross_covariance([float(x) for x in H.reshape(-1)])).reshape(3, 3)
    assert R.tobytes() == np.ascontiguousarray(T[:3, :3]).tobytes()
