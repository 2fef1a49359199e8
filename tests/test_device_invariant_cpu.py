"""CPU checks of user-defined invariants: clipper_hip_invariant_create compiles device source for gfx950
with hiprtc and needs no device; compile errors, a missing or misdeclared clipper_invariant, and out-of-range d or
nparams are refused with a message before any device work."""
import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi

VALID = r"""
#include <hip/hip_runtime.h>
__device__ double sq(double x) { return x * x; }
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) s += sq(ai[k] - aj[k]) - sq(bi[k] - bj[k]);
  return exp(-fabs(s) / params[0]);
}
"""


@pytest.mark.parametrize("d", [1, 3, 6, 16, 32])
def test_a_valid_source_compiles(d):
    with abi.HipInvariant(VALID, d) as inv:
        assert inv.h and inv.d == d


def test_a_syntax_error_comes_back_with_the_compilers_message():
    src = "__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi,\n" \
          "                                    const double* bj, const double* params) {\n  return 1.0 +;\n}\n"
    with pytest.raises(RuntimeError) as e:
        abi.HipInvariant(src, 3)
    msg = str(e.value)
    assert "clipper_hip error -1" in msg           # CLIPPER_HIP_E_INVALID
    assert "invariant:3:" in msg and "error" in msg  # line numbers relative to the user's text


@pytest.mark.parametrize("src", [
    "__device__ double f(const double* a) { return a[0]; }",                                # no clipper_invariant
    "__device__ double clipper_invariant(const double* ai, const double* aj) { return 0.0; }",  # wrong signature
    "__device__ float clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,"
    " const double* p) { return 0.f; }",                                                   # wrong return type
    "double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,"
    " const double* p) { return 0.0; }",                                                   # a host function
])
def test_a_source_without_the_device_function_is_refused(src):
    with pytest.raises(abi.ClipperError, match="clipper_invariant"):
        abi.HipInvariant(src, 3)


@pytest.mark.parametrize("d", [0, 33, -1])
def test_dimension_out_of_range_is_refused(d):
    with pytest.raises(abi.ClipperError, match="dimension"):
        abi.HipInvariant(VALID, d)


def test_nparams_out_of_range_is_refused_before_any_device_work():
    L = abi.load_library()
    with abi.HipInvariant(VALID, 3) as inv:
        p = np.zeros(17)
        D = np.zeros((3, 4))
        for n in (17, -1):
            rc = L.clipper_hip_affinity_custom(None, inv.h, abi._dp(D), 3, 4, abi._dp(D), 4, None, 0, abi._dp(p), n, 1e-4)
            assert rc == -1 and "nparams" in L.clipper_hip_last_error().decode()
        # a context-less call with valid parameters fails on the context, not the parameters
        rc = L.clipper_hip_affinity_custom_staged(None, inv.h, abi._dp(p), 16, 1e-4)
        assert rc == -1 and "nparams" not in L.clipper_hip_last_error().decode()
        # d must be the invariant's
        rc = L.clipper_hip_affinity_custom(None, inv.h, abi._dp(D), 2, 4, abi._dp(D), 4, None, 0, abi._dp(p), 3, 1e-4)
        assert rc == -1 and "d = 3" in L.clipper_hip_last_error().decode()
    assert L.clipper_hip_invariant_destroy(None) == 0


def test_clipperpy_device_invariant_surface():
    cp = clipper_amd.load_clipperpy()
    inv = cp.invariants.DeviceInvariant(VALID, [0.5])
    assert isinstance(inv, cp.invariants.PairwiseInvariant)
    assert inv.source == VALID and list(inv.params) == [0.5]
    with pytest.raises(AttributeError):
        inv.source = "x"
    with pytest.raises(RuntimeError):
        inv(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        cp.CLIPPERBatch(inv, cp.Params())
    with pytest.raises(ValueError):
        cp.invariants.DeviceInvariant(VALID, [0.0] * 17)
