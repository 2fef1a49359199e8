"""CPU checks of clipper_hip_voxel_downsample's boundary: its own argument checks come first and name the offending
argument, then the device (a valid call without one says so: there is no CPU fallback), the layout of
clipper_voxel_info_t against a C program, the symbol in the binding's table."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import registration

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NODEVICE = -1, -4


def _call(P, voxel_size, N=None, n=None, n_out=True, N_out=False):
    """(status, message) of the entry point on the cloud P (n x 3), through ctypes as a C caller would"""
    L = abi.load_library()
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    n = len(P) if n is None else n
    room = max(n, 1)
    Po, No = np.zeros((room, 3)), np.zeros((room, 3))
    cnt, trace = np.zeros(room, np.int32), np.zeros(room, np.int32)
    m, info = C.c_int64(-7), abi.VoxelInfo()
    rc = L.clipper_hip_voxel_downsample(0, dp(P), dp(N), n, C.c_double(voxel_size), dp(Po), dp(No) if (N is not None or N_out) else None,
                                        abi._ip(cnt), abi._ip(trace), C.byref(m) if n_out else None, C.byref(info))
    return rc, (L.clipper_hip_last_error() or b"").decode()


def test_bad_arguments_are_refused_before_the_device_and_named():
    P = np.ascontiguousarray(np.random.default_rng(0).random((8, 3)))
    N = np.tile(np.array([0.0, 0.6, 0.8]), (8, 1))
    nan_p, inf_p, bad_n = P.copy(), P.copy(), N.copy()
    nan_p[3, 1] = np.nan
    inf_p[7, 2] = np.inf
    bad_n[2, 0] = np.nan
    wide = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, float(2 ** 21)]])             # 2^21 + 1 voxels of edge 1 along z
    cases = [
        ((P, 0.0), {}, "voxel_size must be finite and greater than 0 (voxel_size = 0)"),
        ((P, -0.5), {}, "voxel_size must be finite and greater than 0 (voxel_size = -0.5)"),
        ((P, np.nan), {}, "voxel_size must be finite and greater than 0 (voxel_size = nan)"),
        ((P, np.inf), {}, "voxel_size must be finite and greater than 0 (voxel_size = inf)"),
        ((nan_p, 0.1), {}, "P: non-finite value at coordinate 1 of point 3"),
        ((inf_p, 0.1), {}, "P: non-finite value at coordinate 2 of point 7"),
        ((P, 0.1), dict(N=bad_n), "N: non-finite value at coordinate 0 of normal 2"),
        ((wide, 1.0), {}, "voxel_size = 1 gives more than 2^21 voxels along axis 2 (extent 2.09715e+06)"),
        ((P, 1e-9), {}, "voxel_size = 1e-09 gives more than 2^21 voxels along axis 0"),
        ((P, 0.1), dict(n=-1), "a cloud cannot hold a negative number of points (n = -1)"),
        ((None, 0.1), dict(n=8), "null point array"),
        ((P, 0.1), dict(n_out=False), "null n_out"),
        ((P, 0.1), dict(N_out=True), "a normal output array needs the normals N"),
    ]
    for args, kw, msg in cases:
        rc, got = _call(*args, **kw)
        assert rc == E_INVALID and got.startswith(msg), (rc, got, msg)
    # the Python surfaces carry the message
    with pytest.raises(abi.ClipperError, match=r"error -1: voxel_size must be finite and greater than 0 \(voxel_size = 0\)"):
        abi.voxel_down_sample(P.T, 0.0)
    with pytest.raises(abi.ClipperError, match="P: non-finite value at coordinate 1 of point 3"):
        registration.voxel_down_sample(nan_p, 0.1)
    with pytest.raises(abi.ClipperError, match="more than 2\\^21 voxels along axis 2"):
        registration.voxel_down_sample(wide, 1.0)
    with pytest.raises(ValueError, match="P must be 3 x n"):
        abi.voxel_down_sample(np.zeros((2, 5)), 0.1)


def test_good_arguments_reach_the_device_check():
    if abi.device_count() > 0:                                     # (with a device the GPU tests cover the entry point)
        return
    P = np.ascontiguousarray(np.random.default_rng(1).random((8, 3)))
    N = np.tile(np.array([0.0, 0.0, 1.0]), (8, 1))
    fits = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, float(2 ** 21 - 1)]])          # exactly 2^21 voxels: accepted
    for args, kw in (((P, 0.1), {}), ((P, 0.1), dict(N=N)), ((fits, 1.0), {}), ((P, 0.1), dict(n=0))):
        rc, msg = _call(*args, **kw)
        assert rc == E_NODEVICE and "no HIP device visible" in msg, (rc, msg)
    with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
        registration.voxel_down_sample(P, 0.1)


def test_info_layout_matches_the_header(tmp_path):
    src = tmp_path / "vx.c"
    fields = ("dim", "passes", "sort_tile", "chunk", "max_count", "reserved", "kernels_ms", "sort_ms")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(clipper_voxel_info_t)'
                   + "".join(f", offsetof(clipper_voxel_info_t, {f})" for f in fields) + ");return 0;}\n")
    exe = tmp_path / "vx"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    vi = abi.VoxelInfo
    assert got == [C.sizeof(vi)] + [getattr(vi, f).offset for f in fields] == [48, 0, 12, 16, 20, 24, 28, 32, 40]
    assert "clipper_hip_voxel_downsample" in abi.EXPORTED_SYMBOLS
    assert hasattr(abi.load_library(), "clipper_hip_voxel_downsample")
