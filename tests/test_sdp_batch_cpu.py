"""CPU checks of the batched semidefinite relaxation ("Batches"): the exported entry points and
their bindings, the refusals that return before the device is looked for, the ctypes layout of clipper_sdp_problem_t,
and the plan header (g++ only). The GPU side is tests/test_gpu_sdp_batch.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("clipper_hip_sdp_solve_batch", "clipper_hip_batch_sdp", "clipper_hip_batch_get_sdp")


def test_library_exports_and_bindings():
    lib = C.CDLL(build.build_hip())  # cross-compiles for gfx950 if stale; no GPU needed
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.EXPORTED_SYMBOLS
    L = abi.load_library()
    assert L.clipper_hip_sdp_solve_batch.argtypes[1] == C.POINTER(abi.SdpProblem)
    assert L.clipper_hip_batch_sdp.argtypes is not None and L.clipper_hip_batch_get_sdp.argtypes is not None
    assert callable(abi.sdp_solve_batch) and callable(abi.HipBatch.sdp)


def test_problem_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    offs = "".join(f'printf(" %zu", offsetof(clipper_sdp_problem_t, {n}));' for n, _ in abi.SdpProblem._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\n'
                   f'int main(void){{printf("%zu", sizeof(clipper_sdp_problem_t));{offs}printf("\\n");return 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[0] == C.sizeof(abi.SdpProblem) == 64
    assert got[1:] == [getattr(abi.SdpProblem, n).offset for n, _ in abi.SdpProblem._fields_]


def test_refusals_before_the_device():
    eye = np.eye(4)
    big = np.eye(abi.SDP_MAX_N + 1)
    with pytest.raises(abi.ClipperError, match=r"error -7: problem 2:.*limit of 128"):
        abi.sdp_solve_batch([(eye, eye), (eye, eye), (big, big), (eye, eye)])
    with pytest.raises(abi.ClipperError, match=r"error -1: .*max_iters"):
        abi.sdp_solve_batch([(eye, eye)], abi.SdpParams(max_iters=0))
    with pytest.raises(abi.ClipperError, match=r"error -1: .*eps_abs"):
        abi.sdp_solve_batch([(eye, eye)], abi.SdpParams(eps_abs=-1.0))
    assert abi.sdp_solve_batch([]) == []  # count = 0: a successful no-op
    # the raw entry point: a NULL matrix, n = 0, a negative count, a NULL list
    L = abi.load_library()
    prm, info = abi.SdpParams(), (abi.SdpInfo * 2)()
    M = np.asfortranarray(eye)
    dp = M.ctypes.data_as(C.POINTER(C.c_double))
    ok = abi.SdpProblem(dp, dp, 4, None, None, None, None, None)
    for bad, what in ((abi.SdpProblem(None, dp, 4, None, None, None, None, None), r"problem 1:.*M and C"),
                      (abi.SdpProblem(dp, None, 4, None, None, None, None, None), r"problem 1:.*M and C"),
                      (abi.SdpProblem(dp, dp, 0, None, None, None, None, None), r"problem 1:.*empty")):
        arr = (abi.SdpProblem * 2)(ok, bad)
        assert L.clipper_hip_sdp_solve_batch(0, arr, 2, C.byref(prm), info) == -1
        import re
        assert re.search(what, abi._last_error()), abi._last_error()
    arr = (abi.SdpProblem * 2)(ok, ok)
    assert L.clipper_hip_sdp_solve_batch(0, arr, -1, C.byref(prm), info) == -1
    assert L.clipper_hip_sdp_solve_batch(0, None, 2, C.byref(prm), info) == -1
    assert L.clipper_hip_sdp_solve_batch(0, arr, 2, None, info) == -1
    assert L.clipper_hip_sdp_solve_batch(0, arr, 0, C.byref(prm), info) == 0
    assert L.clipper_hip_sdp_solve_batch(0, None, 0, C.byref(prm), None) == 0
    assert L.clipper_hip_batch_sdp(None, C.byref(prm), info) == -1
    assert L.clipper_hip_batch_get_sdp(None, 0, None, None, None, None) < 0


def test_plan_header(tmp_path):
    exe = str(tmp_path / "test_sdp_batch_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_sdp_batch_plan.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "sdp batch plan ok" in out


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "clipper_amd", "csrc", "host_sdpplan.hpp")).read()
    assert "#include <hip" not in text and "hipMalloc" not in text


def test_facade_surfaces():
    import clipper_amd
    cp = clipper_amd.load_clipperpy()
    assert callable(cp.sdp.solve_batch)
    for name in ("solve_as_msrc_sdr", "sdp_solutions"):
        assert hasattr(cp.CLIPPERBatch, name), name
    h = open(os.path.join(ROOT, "include", "clipper", "sdp.h")).read()
    assert "std::vector<Solution> solve(const std::vector<MatrixXd>& M, const std::vector<MatrixXd>& C" in h
    b = open(os.path.join(ROOT, "include", "clipper", "batch.h")).read()
    assert "std::vector<Solution> solveAsMSRCSDR(const sdp::Params& params" in b
    assert "const std::vector<sdp::Solution>& sdpSolutions() const" in b
