"""GPU tests of voxel down-sampling (clipper_hip_voxel_downsample: k_sort.hip.h, k_voxel.hip.h, host_voxel.hpp) against
the numpy model tests/voxel_model.py. No tolerance anywhere: points, normals, counts, trace and n_out are compared for
equality of bytes or integers, and every case also asserts counts.sum() == n and that the rows' cell numbers ascend
strictly. The clouds are tests/voxel_model.py's table (each the smallest that reaches its edge of the kernels: the
tile of the sort, the chunk of the sums, each number of passes); the model of a cloud is computed once and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration
from tests import voxel_model as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def device(P, vs, N=None):
    """the call on the cloud P (n x 3): dict like the model's, with the info"""
    out = abi.voxel_down_sample(P.T, vs, N=None if N is None else N.T, return_counts=True, return_trace=True, return_info=True)
    d = dict(points=out[0].T, normals=None if N is None else out[1].T, counts=out[-3], trace=out[-2], info=out[-1])
    return d


def assert_equals_model(got, want, P, vs):
    n, m = len(P), len(want["counts"])
    info = got["info"]
    print(f"n {n} -> {m} rows, dim {list(info.dim)}, passes {info.passes}, max_count {info.max_count}, "
          f"kernels {info.kernels_ms:.3f} ms")
    assert got["points"].shape == (m, 3)                                            # n_out
    assert same_bits(got["points"], want["points"])
    if want["normals"] is not None:
        assert same_bits(got["normals"], want["normals"])
    assert np.array_equal(got["counts"], want["counts"]) and got["counts"].dtype == np.int32
    assert np.array_equal(got["trace"], want["trace"])
    assert int(got["counts"].sum()) == n
    # the cell number of every row, from the points that went to it: one per row, strictly ascending
    k = vm.keys(P, vs)
    rowkey = np.zeros(m, np.uint64)
    rowkey[got["trace"]] = k
    assert np.array_equal(rowkey[got["trace"]], k) and np.all(rowkey[1:] > rowkey[:-1])
    assert list(info.dim) == want["dim"].tolist() and info.passes == want["passes"]
    assert info.max_count == want["max_count"] and info.chunk == vm.CHUNK and info.sort_tile == vm.SORT_TILE
    assert 0.0 <= info.sort_ms <= info.kernels_ms and (info.passes > 0 or info.sort_ms == 0.0)


@pytest.mark.parametrize("name", list(vm.CASES))
def test_every_case_equals_the_model(name):
    P, vs, N, want = vm.case_model(name)
    assert_equals_model(device(P, vs, N), want, P, vs)


def test_the_tile_cases_sit_at_the_librarys_tile():
    """the table is built around vm.SORT_TILE: it must be the tile the library sorts by"""
    P, vs, _, _ = vm.case_model("n1")
    assert device(P, vs)["info"].sort_tile == vm.SORT_TILE
    for n in (vm.SORT_TILE - 1, vm.SORT_TILE, vm.SORT_TILE + 1, 2 * vm.SORT_TILE + 1):
        for form in vm.TILE_FORMS:
            assert len(vm.case_model(f"tile_{n}_{form}")[0]) == n


def test_two_calls_give_identical_bytes():
    P, vs, N, _ = vm.case_model("normals5000")
    a, b = device(P, vs, N), device(P, vs, N)
    for key in ("points", "normals", "counts", "trace"):
        assert same_bits(a[key], b[key]), key
    P, vs, N, _ = vm.case_model("chunk_edges")
    assert same_bits(device(P, vs)["points"], device(P, vs)["points"])


def _raw(P, vs, N=None, outs=("P", "N", "count", "trace"), info=True, n=None):
    L = abi.load_library()
    n = len(P) if n is None else n
    room = max(n, 1)
    bufs = dict(P=np.full((room, 3), -7.0), N=np.full((room, 3), -7.0), count=np.full(room, -7, np.int32),
                trace=np.full(room, -7, np.int32))
    ptr = lambda k: None if k not in outs else (abi._dp(bufs[k]) if k in ("P", "N") else abi._ip(bufs[k]))  # noqa: E731
    m, vi = C.c_int64(-7), abi.VoxelInfo()
    rc = L.clipper_hip_voxel_downsample(0, abi._dp(P), None if N is None else abi._dp(N), n, C.c_double(vs), ptr("P"), ptr("N"),
                                        ptr("count"), ptr("trace"), C.byref(m), C.byref(vi) if info else None)
    return rc, int(m.value), bufs, vi


def test_null_outputs_are_accepted_and_rows_past_n_out_stay_untouched():
    P, vs, N, want = vm.case_model("normals5000")
    P, N = np.ascontiguousarray(P), np.ascontiguousarray(N)
    m = len(want["counts"])
    rc, n_out, _, _ = _raw(P, vs, N, outs=(), info=False)                            # n_out alone
    assert (rc, n_out) == (0, m)
    rc, n_out, _, _ = _raw(P, vs, None, outs=(), info=False)
    assert (rc, n_out) == (0, m)
    for only in ("P", "N", "count", "trace"):
        rc, n_out, bufs, _ = _raw(P, vs, N, outs=(only,))
        assert (rc, n_out) == (0, m)
        want_of = dict(P=want["points"], N=want["normals"], count=want["counts"], trace=want["trace"])[only]
        assert same_bits(bufs[only][:len(want_of)], want_of)
        if only != "trace":
            assert np.all(bufs[only][m:] == -7)                                       # only the first n_out rows are written
        for other in set(bufs) - {only}:
            assert np.all(bufs[other] == -7)
    # an empty cloud has no voxels
    rc, n_out, bufs, vi = _raw(P, vs, None, outs=("P", "count", "trace"), n=0)
    assert (rc, n_out) == (0, 0) and np.all(bufs["P"] == -7) and list(vi.dim) == [0, 0, 0] and vi.passes == 0


def test_refusals_leave_the_library_usable():
    P, vs, _, want = vm.case_model("two_in_one")
    with pytest.raises(abi.ClipperError, match="voxel_size must be finite and greater than 0"):
        abi.voxel_down_sample(P.T, -1.0)
    with pytest.raises(abi.ClipperError, match="more than 2\\^21 voxels along axis 1"):
        abi.voxel_down_sample(np.array([[0.0, 0.0], [0.0, float(2 ** 21)], [0.0, 0.0]]), 1.0)
    with pytest.raises(abi.ClipperError, match="device 99 out of range"):
        abi.voxel_down_sample(P.T, vs, device=99)
    assert same_bits(device(P, vs)["points"], want["points"])


def test_python_surfaces_return_the_abi_bits():
    P, vs, N, want = vm.case_model("normals5000")
    pts, nrm, cnt, trace = registration.voxel_down_sample(P, vs, normals=N, return_counts=True, return_trace=True)
    assert pts.shape == (len(want["counts"]), 3) and pts.flags.c_contiguous
    assert same_bits(pts, want["points"]) and same_bits(nrm, want["normals"])
    assert np.array_equal(cnt, want["counts"]) and np.array_equal(trace, want["trace"])
    assert same_bits(registration.voxel_down_sample(P, vs), want["points"])           # the defaults: the points alone
    pts2, cnt2 = registration.voxel_down_sample(P, vs, return_counts=True)
    assert same_bits(pts2, want["points"]) and np.array_equal(cnt2, want["counts"])
    assert same_bits(abi.voxel_down_sample(P.T, vs), want["points"].T.copy(order="F"))
    cp = clipper_amd.load_clipperpy()
    Pf, Nf = np.asfortranarray(P.T), np.asfortranarray(N.T)
    out = cp.utils.voxel_down_sample(Pf, vs, normals=Nf, return_counts=True, return_trace=True)
    assert same_bits(np.asarray(out[0]).T, want["points"]) and same_bits(np.asarray(out[1]).T, want["normals"])
    assert np.array_equal(np.asarray(out[2]), want["counts"]) and np.array_equal(np.asarray(out[3]), want["trace"])
    assert same_bits(np.asarray(cp.utils.voxel_down_sample(Pf, vs)).T, want["points"])
    with pytest.raises(ValueError, match="voxel_size must be finite and greater than 0"):  # std::invalid_argument
        cp.utils.voxel_down_sample(Pf, 0.0)


def test_cpp_facade_voxel(tmp_path):
    P, vs, N, want = vm.case_model("normals5000")
    exe = str(tmp_path / "test_voxel_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_voxel_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    files = [str(tmp_path / f) for f in ("P.f64", "N.f64", "Po.f64", "No.f64", "cnt.i32", "trace.i32")]
    np.ascontiguousarray(P).tofile(files[0])                     # row-major n x 3 = column-major 3 x n
    np.ascontiguousarray(N).tofile(files[1])
    out = subprocess.run([exe, str(len(P)), repr(float(vs))] + files, capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "ALL VOXEL FACADE TESTS PASSED" in out.stdout
    assert same_bits(np.fromfile(files[2]).reshape(-1, 3), want["points"])
    assert same_bits(np.fromfile(files[3]).reshape(-1, 3), want["normals"])
    assert np.array_equal(np.fromfile(files[4], np.int32), want["counts"])
    assert np.array_equal(np.fromfile(files[5], np.int32), want["trace"])


def test_downsampled_bunny_goes_through_normals_and_fpfh():
    P, vs, _, want = vm.case_model("bunny4096")
    pts = registration.voxel_down_sample(P, vs)
    assert same_bits(pts, want["points"]) and 64 <= len(pts) < len(P)
    nrm = registration.estimate_normals(pts, knn=16)
    F = registration.compute_fpfh(pts, nrm, knn=32)
    assert nrm.shape == (len(pts), 3) and F.shape == (len(pts), 33) and np.all(np.isfinite(F))
    # and with the cloud's own normals carried through the voxels: unit vectors, acceptable to compute_fpfh as they are
    pts2, vn = registration.voxel_down_sample(P, vs, normals=registration.estimate_normals(P, knn=16))
    assert same_bits(pts2, pts)
    assert np.all(np.isfinite(registration.compute_fpfh(pts2, vn, knn=32)))
