"""CPU checks of batched solves scored by a user-defined invariant: the entry point is declared and
exported, the Python and clipperpy surfaces exist, invalid invariant arguments are refused before the batch handle is
looked at, the epilogue with its batched fill kernels compiles at every dimension (hiprtc needs no device), and a C++
program using CLIPPERBatch::withDeviceInvariant compiles against include/. The GPU side is
tests/test_gpu_batch_custom.py."""
import os
import subprocess

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) s += (ai[k] - aj[k]) * (ai[k] - aj[k]) - (bi[k] - bj[k]) * (bi[k] - bj[k]);
  return exp(-fabs(s) / params[0]);
}
"""


def test_entry_point_is_declared_and_exported():
    with open(os.path.join(ROOT, "include", "clipper_hip.h")) as f:
        h = f.read()
    assert "int clipper_hip_batch_solve_custom(clipper_hip_batch_t* b, const clipper_hip_invariant_t* inv," in h
    assert "clipper_hip_batch_solve_custom" in abi.EXPORTED_SYMBOLS
    L = abi.load_library()
    assert L.clipper_hip_batch_solve_custom.argtypes is not None


def test_python_surfaces():
    assert callable(abi.HipBatch.solve_custom)
    cp = clipper_amd.load_clipperpy()
    assert callable(cp.CLIPPERBatch.with_device_invariant)


def test_invalid_invariant_arguments_are_refused_without_a_batch():
    L = abi.load_library()
    p = np.zeros(17)
    prm = abi.Params()
    with abi.HipInvariant(SRC, 3) as inv:
        for n in (17, -1):
            rc = L.clipper_hip_batch_solve_custom(None, inv.h, None, 0, abi._dp(p), n, abi.C.byref(prm))
            assert rc == -1 and "nparams" in L.clipper_hip_last_error().decode()
        # valid parameters: the missing batch is what is refused
        rc = L.clipper_hip_batch_solve_custom(None, inv.h, None, 0, abi._dp(p), 16, abi.C.byref(prm))
        assert rc == -1 and "nparams" not in L.clipper_hip_last_error().decode()
    rc = L.clipper_hip_batch_solve_custom(None, None, None, 0, None, 0, abi.C.byref(prm))
    assert rc == -1 and "no invariant" in L.clipper_hip_last_error().decode()


@pytest.mark.parametrize("d", [1, 3, 6, 16, 32])
def test_epilogue_with_the_batched_kernels_compiles(d):
    with abi.HipInvariant(SRC, d) as inv:
        assert inv.h and inv.d == d


def test_epilogue_holds_both_batched_kernels():
    with open(os.path.join(ROOT, "clipper_amd", "csrc", "k_custom_invariant_src.h")) as f:
        s = f.read()
    for name in ("clipper_custom_fill_batch_f32", "clipper_custom_fill_batch_f64", "clipper_custom_fill_f32",
                 "clipper_custom_fill_f64"):
        assert f"void {name}(" in s, name
    assert s.count("__launch_bounds__(256)") == 4


def test_cpp_facade_compiles(tmp_path):
    obj = str(tmp_path / "test_batch_custom_facade.o")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-fopenmp", "-c", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "test_batch_custom_facade.cpp"), "-o", obj])
    assert os.path.getsize(obj) > 0
