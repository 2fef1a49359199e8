"""CPU-side checks of the generalized ICP entry points (clipper_hip_estimate_covariances, clipper_hip_icp_generalized):
the structs they share with clipper_hip_icp are unchanged and the method's enumerator is 2; every refusal answers on the
host before any device work, so with no device present, each naming its value; clipper_hip_icp refuses method 2 with the
name of the call that takes it; the Python facade's own refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from tests import gicp_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structs_unchanged_and_the_enumerator(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf("%zu %zu %zu %d %d %d\\n",'
                   'sizeof(clipper_icp_params_t), sizeof(clipper_icp_info_t), sizeof(clipper_neighborhood_t),'
                   'CLIPPER_ICP_POINT_TO_POINT, CLIPPER_ICP_POINT_TO_PLANE, CLIPPER_ICP_GENERALIZED);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [C.sizeof(abi.IcpParams), C.sizeof(abi.IcpInfo), C.sizeof(abi.Neighborhood)] == [32, 64, 16]
    assert got[3:] == [abi.ICP_POINT_TO_POINT, abi.ICP_POINT_TO_PLANE, abi.ICP_GENERALIZED] == [0, 1, gm.GENERALIZED]
    facade = open(os.path.join(ROOT, "include", "clipper", "registration.h")).read()
    assert "enum class IcpMethod { PointToPoint = 0, PointToPlane = 1, Generalized = 2 }" in facade


def _refusals():
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    P = np.ascontiguousarray(np.arange(12, dtype=np.float64).reshape(4, 3) / 7.0)
    bad = P.copy()
    bad[2, 1] = np.inf
    I6 = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (4, 1))
    inf6, neg6, flat6, zero6 = I6.copy(), I6.copy(), I6.copy(), I6.copy()
    inf6[1, 4] = np.nan
    neg6[3, 0] = -1.0                       # the first minor
    flat6[2] = (1.0, 1.0, 0.0, 1.0, 0.0, 1.0)   # xx yy - xy^2 == 0: the second
    zero6[1, 5] = 0.0                       # zz == 0: the determinant
    nan_T = np.eye(4).reshape(-1).copy()
    nan_T[12] = np.nan
    T = np.zeros(16)
    out6 = np.zeros((4, 6))
    ok = abi.IcpParams(abi.ICP_GENERALIZED, 0.1)
    g = lambda *a: ("gicp", a)     # noqa: E731
    c = lambda *a: ("cov", a)      # noqa: E731
    icp = lambda *a: ("icp", a)    # noqa: E731
    r = C.byref
    nb = abi.Neighborhood(20)
    return [
        (g(0, None, dp(I6), 4, dp(P), dp(I6), 4, None, r(ok), dp(T), None, None), "icp_generalized: null source point array"),
        (g(0, dp(P), dp(I6), 4, None, dp(I6), 4, None, r(ok), dp(T), None, None), "icp_generalized: null target point array"),
        (g(0, dp(P), None, 4, dp(P), dp(I6), 4, None, r(ok), dp(T), None, None), "icp_generalized: null source covariance array"),
        (g(0, dp(P), dp(I6), 4, dp(P), None, 4, None, r(ok), dp(T), None, None), "icp_generalized: null target covariance array"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, r(ok), None, None, None), "icp_generalized: null T_out"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, None, dp(T), None, None), "icp_generalized: null params"),
        (g(0, dp(P), dp(I6), 0, dp(P), dp(I6), 4, None, r(ok), dp(T), None, None), "source: a cloud needs at least one point (n = 0)"),
        (g(0, dp(bad), dp(I6), 4, dp(P), dp(I6), 4, None, r(ok), dp(T), None, None), "source: non-finite value at coordinate 1 of point 2"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, dp(nan_T), r(ok), dp(T), None, None), "T_init: non-finite value at entry (0, 3)"),
        (g(0, dp(P), dp(inf6), 4, dp(P), dp(I6), 4, None, r(ok), dp(T), None, None), "source covariances: non-finite value at entry 4 of point 1"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(inf6), 4, None, r(ok), dp(T), None, None), "target covariances: non-finite value at entry 4 of point 1"),
        (g(0, dp(P), dp(neg6), 4, dp(P), dp(I6), 4, None, r(ok), dp(T), None, None),
         "source covariances: the matrix of point 3 is not positive definite (leading minor 1 = -1)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(flat6), 4, None, r(ok), dp(T), None, None),
         "target covariances: the matrix of point 2 is not positive definite (leading minor 2 = 0)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(zero6), 4, None, r(ok), dp(T), None, None),
         "target covariances: the matrix of point 1 is not positive definite (leading minor 3 = 0)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, r(abi.IcpParams(0, 0.1)), dp(T), None, None),
         "icp_generalized: method must be CLIPPER_ICP_GENERALIZED (2) (method = 0)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, r(abi.IcpParams(1, 0.1)), dp(T), None, None), "(method = 1)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, r(abi.IcpParams(7, 0.1)), dp(T), None, None), "(method = 7)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, r(abi.IcpParams(2, 0.0)), dp(T), None, None), "max_distance must be positive and finite (max_distance = 0)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, r(abi.IcpParams(2, 0.1, 1001)), dp(T), None, None), "max_iterations must be in 0..1000 (max_iterations = 1001)"),
        (g(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, r(abi.IcpParams(2, 0.1, 30, -1.0)), dp(T), None, None), "rel_fitness must be at least 0 (rel_fitness = -1)"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(ok), dp(T), None, None),
         "icp: method 2 (generalized) takes per-point covariances: call clipper_hip_icp_generalized"),
        (icp(0, dp(P), 4, dp(P), None, 4, None, r(abi.IcpParams(7, 0.1)), dp(T), None, None), "icp: unknown method 7"),
        (c(0, None, 4, r(nb), 1e-3, dp(out6), None), "estimate_covariances: null point array"),
        (c(0, dp(P), 4, r(nb), 1e-3, None, None), "estimate_covariances: null covariance output array"),
        (c(0, dp(P), 4, None, 1e-3, dp(out6), None), "estimate_covariances: null neighbourhood"),
        (c(0, dp(P), 4, r(abi.Neighborhood(2)), 1e-3, dp(out6), None), "neighbourhood: knn must be in 3..32 (knn = 2)"),
        (c(0, dp(P), 4, r(abi.Neighborhood(33)), 1e-3, dp(out6), None), "neighbourhood: knn must be in 3..32 (knn = 33)"),
        (c(0, dp(P), 4, r(abi.Neighborhood(20, np.inf)), 1e-3, dp(out6), None), "neighbourhood: radius must be finite"),
        (c(0, dp(P), 4, r(nb), 0.0, dp(out6), None), "epsilon must be in (0, 1] (epsilon = 0)"),
        (c(0, dp(P), 4, r(nb), 1.5, dp(out6), None), "epsilon must be in (0, 1] (epsilon = 1.5)"),
        (c(0, dp(P), 4, r(nb), np.nan, dp(out6), None), "epsilon must be in (0, 1] (epsilon = nan)"),
        (c(0, dp(P), 4, r(nb), -1e-3, dp(out6), None), "epsilon must be in (0, 1] (epsilon = -0.001)"),
        (c(0, dp(P), 0, r(nb), 1e-3, dp(out6), None), "a cloud needs at least one point (n = 0)"),
        (c(0, dp(bad), 4, r(nb), 1e-3, dp(out6), None), "P: non-finite value at coordinate 1 of point 2"),
    ], (P, bad, I6, inf6, neg6, flat6, zero6, nan_T, T, out6, ok, nb)


def test_refusals_name_their_values_without_a_device():
    L = abi.load_library()
    fns = {"gicp": L.clipper_hip_icp_generalized, "cov": L.clipper_hip_estimate_covariances, "icp": L.clipper_hip_icp}
    cases, keep = _refusals()
    for (which, args), text in cases:
        rc = fns[which](*args)
        msg = abi._last_error()
        assert rc == -1 and text in msg, (rc, msg, text)      # CLIPPER_HIP_E_INVALID
    assert keep


def test_python_facade_refuses_before_the_library():
    from clipper_amd import registration as reg
    P = np.zeros((4, 3))
    I6 = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (4, 1))
    for eps in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="epsilon must be in"):
            reg.estimate_covariances(P, epsilon=eps)
    with pytest.raises(ValueError, match="search must be one of"):
        reg.estimate_covariances(P, search="tree")
    with pytest.raises(ValueError, match="source_covariances must be n x 6"):
        reg.icp_generalized(P, P, source_covariances=I6[:3], target_covariances=I6, max_distance=0.1)
    with pytest.raises(ValueError, match="target_covariances must be n x 6"):
        reg.icp_generalized(P, P, source_covariances=I6, target_covariances=I6.T, max_distance=0.1)
    with pytest.raises(ValueError, match="T_init must be 4 x 4"):
        reg.icp_generalized(P, P, np.eye(3), I6, I6, max_distance=0.1)
    with pytest.raises(ValueError, match="search must be one of"):
        reg.icp_generalized(P, P, None, I6, I6, max_distance=0.1, search="tree")
    with pytest.raises(abi.ClipperError, match="max_distance must be positive"):
        reg.icp_generalized(P, P, None, I6, I6)
    with pytest.raises(abi.ClipperError, match="not positive definite"):
        reg.icp_generalized(P, P, None, I6 * 0.0, I6, max_distance=0.1)
    with pytest.raises(ValueError):                      # the existing call keeps its refusals: it knows two methods
        reg.icp(P, P, method="generalized", max_distance=0.1)
    with pytest.raises(ValueError, match="C_src must be 6 x n"):
        abi.icp_generalized(P.T, I6, P.T, I6.T, max_distance=0.1)
    with pytest.raises(abi.ClipperError, match="call clipper_hip_icp_generalized"):
        abi.icp(P.T, P.T, method=abi.ICP_GENERALIZED, max_distance=0.1)
