"""CPU test of the boundary of the clouds that live on the device (include/clipper_hip.h, clipper_amd/csrc/host_cloud.hpp):
the new symbols are exported, the ctypes structures have the sizes a C program prints, everything that enters from the
host is refused with CLIPPER_HIP_E_INVALID before any device work, and without a device create says so
(CLIPPER_HIP_E_NODEVICE: there is no CPU fallback). No compute call: needs no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import build, registration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NODEVICE = -1, -4

NEW = ["clipper_hip_cloud_create", "clipper_hip_cloud_destroy", "clipper_hip_cloud_count", "clipper_hip_cloud_download",
       "clipper_hip_cloud_info", "clipper_hip_cloud_set_descriptors", "clipper_hip_pairs_create", "clipper_hip_pairs_destroy",
       "clipper_hip_pairs_count", "clipper_hip_pairs_has_sqd", "clipper_hip_pairs_download", "clipper_hip_cloud_voxel_downsample",
       "clipper_hip_cloud_estimate_normals", "clipper_hip_cloud_compute_fpfh", "clipper_hip_cloud_fpfh_from_points",
       "clipper_hip_cloud_estimate_covariances", "clipper_hip_cloud_match", "clipper_hip_stage_inputs_clouds",
       "clipper_hip_cloud_gather_points", "clipper_hip_cloud_icp", "clipper_hip_cloud_evaluate_registration"]


def _no_gpu():
    try:
        return abi.device_count() <= 0
    except Exception:
        return True


def _err():
    return (abi.load_library().clipper_hip_last_error() or b"").decode()


def test_new_symbols_are_exported():
    lib = C.CDLL(build.build_hip())
    for name in NEW:
        assert name in abi.EXPORTED_SYMBOLS and hasattr(lib, name), name


def test_struct_sizes_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf("%zu %zu %zu %d %d\\n",'
                   'sizeof(clipper_hip_cloud_info_t), offsetof(clipper_hip_cloud_info_t, device),'
                   'offsetof(clipper_hip_cloud_info_t, grid_dim), CLIPPER_HIP_CLOUD_POINTS, CLIPPER_HIP_CLOUD_VOXEL_TRACE);'
                   'return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(abi.CloudInfo), abi.CloudInfo.device.offset, abi.CloudInfo.grid_dim.offset,
                   abi.CLOUD_POINTS, abi.CLOUD_VOXEL_TRACE]
    assert got[0] == 56


def test_everything_from_the_host_is_checked_before_any_device_work():
    L = abi.load_library()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))   # noqa: E731
    P = np.asfortranarray(np.random.default_rng(0).random((3, 10)))
    N = np.zeros((3, 10), order="F")
    N[2] = 1.0
    h = C.c_void_p()
    create = L.clipper_hip_cloud_create

    assert create(0, dp(P), None, 10, None) == E_INVALID and "null output handle" in _err()
    assert create(0, dp(P), None, -1, C.byref(h)) == E_INVALID and "negative number of points (n = -1)" in _err()
    assert create(0, dp(P), None, 2 ** 31, C.byref(h)) == E_INVALID and "more than 2^31 - 1 points" in _err()   # (P is not read)
    assert create(0, None, None, 10, C.byref(h)) == E_INVALID and "null point array" in _err()
    for bad in (np.nan, np.inf, -np.inf):
        Q = P.copy(order="F")
        Q[1, 7] = bad
        assert create(0, dp(Q), None, 10, C.byref(h)) == E_INVALID
        assert "P: non-finite value at coordinate 1 of point 7" in _err()
    for scale in (0.9, 1.1):                       # squared lengths 0.81 and 1.21: outside [0.99, 1.01]
        M = N.copy(order="F")
        M[:, 4] *= scale
        assert create(0, dp(P), dp(M), 10, C.byref(h)) == E_INVALID and "N: normal 4 is not of unit length" in _err()
    M = N.copy(order="F")
    M[0, 3] = np.nan
    assert create(0, dp(P), dp(M), 10, C.byref(h)) == E_INVALID and "N: non-finite value at coordinate 0 of normal 3" in _err()
    assert not h.value                             # a refused create hands out NULL

    A = np.asfortranarray(np.array([[0, 1], [2, 3]], dtype=np.int32))
    pc = L.clipper_hip_pairs_create
    assert pc(0, ip(A), None, 2, None) == E_INVALID and "null output handle" in _err()
    assert pc(0, ip(A), None, -1, C.byref(h)) == E_INVALID and "m = -1" in _err()
    assert pc(0, None, None, 2, C.byref(h)) == E_INVALID and "null association array" in _err()
    B = A.copy(order="F")
    B[1, 1] = -1
    assert pc(0, ip(B), None, 2, C.byref(h)) == E_INVALID and "negative index -1 in row 1" in _err()
    assert not h.value

    # null handles: every call on a handle refuses them, the destroyers take them
    out = np.zeros(30)
    nb, prm, ipr = abi.Neighborhood(16, 0.0), abi.MatchParams(1, 1, 0.0, 0.0), abi.IcpParams(max_distance=1.0)
    info, vinfo, T = abi.CloudInfo(), abi.VoxelInfo(), np.eye(4).reshape(-1)
    assert L.clipper_hip_cloud_count(None) == E_INVALID and L.clipper_hip_pairs_count(None) == E_INVALID
    assert L.clipper_hip_pairs_has_sqd(None) == E_INVALID
    for rc in (L.clipper_hip_cloud_download(None, abi.CLOUD_POINTS, out.ctypes.data_as(C.c_void_p)),
               L.clipper_hip_cloud_info(None, C.byref(info)),
               L.clipper_hip_cloud_set_descriptors(None, dp(out), 3),
               L.clipper_hip_pairs_download(None, ip(A), None),
               L.clipper_hip_cloud_voxel_downsample(None, 0.1, 0, C.byref(h), C.byref(vinfo)),
               L.clipper_hip_cloud_estimate_normals(None, C.byref(nb), None),
               L.clipper_hip_cloud_compute_fpfh(None, C.byref(nb)),
               L.clipper_hip_cloud_fpfh_from_points(None, C.byref(nb), None, C.byref(nb)),
               L.clipper_hip_cloud_estimate_covariances(None, C.byref(nb), 1e-3),
               L.clipper_hip_cloud_match(None, None, C.byref(prm), C.byref(h), None, None),
               L.clipper_hip_stage_inputs_clouds(None, None, None, None, 0),
               L.clipper_hip_cloud_gather_points(None, ip(A), 1, dp(out)),
               L.clipper_hip_cloud_icp(None, None, None, C.byref(ipr), None, dp(T), None, None, None),
               L.clipper_hip_cloud_evaluate_registration(None, None, None, 1.0, None, None, None, None)):
        assert rc == E_INVALID and "null" in _err(), _err()
    L.clipper_hip_cloud_destroy(None)
    L.clipper_hip_pairs_destroy(None)


@pytest.mark.skipif(not _no_gpu(), reason="a HIP device is visible")
def test_without_a_device_create_says_so():
    L = abi.load_library()
    P = np.asfortranarray(np.random.default_rng(0).random((3, 10)))
    h = C.c_void_p()
    assert L.clipper_hip_cloud_create(0, P.ctypes.data_as(C.POINTER(C.c_double)), None, 10, C.byref(h)) == E_NODEVICE
    assert "no HIP device" in _err() and not h.value
    A = np.zeros((2, 2), dtype=np.int32, order="F")
    assert L.clipper_hip_pairs_create(0, A.ctypes.data_as(C.POINTER(C.c_int32)), None, 2, C.byref(h)) == E_NODEVICE
    with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
        abi.DeviceCloud(P)
    with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
        registration.DeviceCloud(P)                # the same class, reached through the registration module
    with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
        abi.DevicePairs(np.array([[0, 1]]))


def test_python_checks_and_closed_handles_raise():
    with pytest.raises(ValueError, match="must be 3 x n"):
        abi.DeviceCloud(np.zeros((4, 5)))
    with pytest.raises(ValueError, match="same number of points"):
        abi.DeviceCloud(np.zeros((3, 5)), normals=np.zeros((3, 4)))
    c = abi.DeviceCloud(_h=None)                   # a handle that was never opened behaves like a closed one
    c.close()
    c.close()
    for call in (lambda: len(c), c.points, c.info, lambda: c.estimate_normals(), lambda: c.gather_points([0])):
        with pytest.raises(abi.ClipperError, match="this DeviceCloud is closed"):
            call()
    p = abi.DevicePairs(_h=None)
    p.close()
    with pytest.raises(abi.ClipperError, match="this DevicePairs is closed"):
        p.download()
