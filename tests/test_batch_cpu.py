"""CPU checks of the batched solves: the launch packer and the build-until-it-fits driver (g++ only),
the ctypes layout of clipper_batch_problem_t, and the Python surfaces. The GPU side is tests/test_gpu_batch.py."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_packer(tmp_path):
    exe = str(tmp_path / "test_batch_pack")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_batch_pack.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "batch pack ok" in out


def test_until_fits_driver(tmp_path):
    exe = str(tmp_path / "test_until_fits")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_until_fits.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "until fits ok" in out


def test_batch_problem_layout():
    from clipper_amd import _abi as abi
    P = abi.BatchProblem
    assert C.sizeof(P) == 56
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [
        ("D1", 0), ("n1", 8), ("D2", 16), ("n2", 24), ("A", 32), ("m", 40), ("u0", 48)]


def test_batch_header_declares_the_problem_struct():
    with open(os.path.join(ROOT, "include", "clipper_hip.h")) as f:
        h = f.read()
    for decl in ("const double* D1; int64_t n1;", "const double* D2; int64_t n2;", "const int32_t* A; int64_t m;",
                 "const double* u0;", "} clipper_batch_problem_t;"):
        assert decl in h


def test_hipbatch_surface():
    from clipper_amd import _abi as abi
    for name in ("solve_euclidean", "solve_pointnormal", "route", "selected_associations", "stats", "split", "close"):
        assert callable(getattr(abi.HipBatch, name))
    for sym in ("clipper_hip_batch_create", "clipper_hip_batch_solve_euclidean", "clipper_hip_batch_route",
                "clipper_hip_batch_get_stats"):
        assert sym in abi.EXPORTED_SYMBOLS


def test_clipperpy_batch_surface():
    import clipper_amd
    clipperpy = clipper_amd.load_clipperpy()
    cls = clipperpy.CLIPPERBatch
    for name in ("solve", "get_selected_associations", "set_device", "set_storage", "solved_batched"):
        assert hasattr(cls, name), name
