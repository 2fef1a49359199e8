"""CPU checks of the wide route of the semidefinite relaxation ("The wide route"): the route
switch of the C ABI and its bindings, the constants and the layout of clipper_sdp_info_t against the header, the
refusals that return before the device is looked for, and the plan header (g++ only). The GPU side is
tests/test_gpu_sdp_wide.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _default_route():
    """every test of this file leaves the process on the default route (the suite shares one process)"""
    try:
        yield
    finally:
        abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP)


def test_library_exports_and_bindings():
    lib = C.CDLL(build.build_hip())  # cross-compiles for gfx950 if stale; no GPU needed
    for name in ("clipper_hip_sdp_set_route", "clipper_hip_sdp_route"):
        assert hasattr(lib, name), name
        assert name in abi.EXPORTED_SYMBOLS
    assert callable(abi.sdp_set_route) and callable(abi.sdp_route)


def test_constants_and_info_layout_match_header(tmp_path):
    src = tmp_path / "wide.c"
    offs = "".join(f'printf(" %zu", offsetof(clipper_sdp_info_t, {n}));' for n, _ in abi.SdpInfo._fields_)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\n'
                   'int main(void){printf("%d %d %d %d %d", CLIPPER_HIP_SDP_WIDE_MAX_N, CLIPPER_HIP_SDP_ROUTE_WORKGROUP,'
                   ' CLIPPER_HIP_SDP_ROUTE_AUTO, CLIPPER_HIP_SDP_ROUTE_WIDE, CLIPPER_HIP_SDP_MAX_N);'
                   f'printf(" %zu", sizeof(clipper_sdp_info_t));{offs}printf("\\n");return 0;}}\n')
    exe = tmp_path / "wide"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:5] == [abi.SDP_WIDE_MAX_N, abi.SDP_ROUTE_WORKGROUP, abi.SDP_ROUTE_AUTO, abi.SDP_ROUTE_WIDE, abi.SDP_MAX_N]
    assert got[:5] == [1024, 0, 1, 2, 128]
    # `route` sits where `pad` sat: the sixth int32, before the first double; the size is what it was
    assert got[5] == C.sizeof(abi.SdpInfo) == 6 * 4 + 10 * 8
    assert got[6:] == [getattr(abi.SdpInfo, n).offset for n, _ in abi.SdpInfo._fields_]
    assert abi.SdpInfo.route.offset == 20 and abi.SdpInfo.route.size == 4 and abi.SdpInfo.pobj.offset == 24


def test_set_route():
    assert abi.sdp_route() == abi.SDP_ROUTE_WORKGROUP  # the default
    assert abi.sdp_set_route(abi.SDP_ROUTE_AUTO) == abi.SDP_ROUTE_WORKGROUP  # returns the previous setting
    assert abi.sdp_route() == abi.SDP_ROUTE_AUTO
    assert abi.sdp_set_route(abi.SDP_ROUTE_WIDE) == abi.SDP_ROUTE_AUTO
    for bad in (7, -1, 3):
        with pytest.raises(abi.ClipperError, match=r"error -1: .*route"):
            abi.sdp_set_route(bad)
        assert abi.load_library().clipper_hip_sdp_set_route(bad) == -1
        assert abi.sdp_route() == abi.SDP_ROUTE_WIDE  # unchanged
    assert abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP) == abi.SDP_ROUTE_WIDE
    assert abi.sdp_route() == abi.SDP_ROUTE_WORKGROUP


def test_refusals_before_the_device():
    eye = np.eye(4)
    huge = np.eye(abi.SDP_WIDE_MAX_N + 1)
    big = np.eye(abi.SDP_MAX_N + 1)
    for route in (abi.SDP_ROUTE_AUTO, abi.SDP_ROUTE_WIDE):
        abi.sdp_set_route(route)
        with pytest.raises(abi.ClipperError, match=r"error -7: .*n = 1025.*limit of 1024"):
            abi.sdp_solve(huge, huge)
        with pytest.raises(abi.ClipperError, match=r"error -7: problem 2:.*limit of 1024"):
            abi.sdp_solve_batch([(eye, eye), (big, big), (huge, huge), (eye, eye)])
        with pytest.raises(abi.ClipperError, match=r"error -1: .*max_iters"):
            abi.sdp_solve(big, big, abi.SdpParams(max_iters=0))
    abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP)
    with pytest.raises(abi.ClipperError, match=r"error -7: .*limit of 128"):
        abi.sdp_solve(big, big)
    with pytest.raises(abi.ClipperError, match=r"error -7: problem 1:.*limit of 128"):
        abi.sdp_solve_batch([(eye, eye), (big, big)])


def test_plan_header(tmp_path):
    exe = str(tmp_path / "test_sdp_wide_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_sdp_wide_plan.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "sdp wide plan ok" in out


def test_rules_header(tmp_path):
    """the scalar rules of the iteration (sdp_rules.hpp) on the host, and their constants against the model's"""
    from tests import sdp_model as sm
    exe = str(tmp_path / "test_sdp_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_sdp_rules.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "sdp rules ok" in out
    line = [ln for ln in out.splitlines() if ln.startswith("constants:")]
    assert len(line) == 1
    words = line[0].split()[1:]
    got = dict(zip(words[0::2], words[1::2]))
    assert float(got["RHO0"]) == sm.RHO0 and int(got["ADAPT_EVERY"]) == sm.ADAPT_EVERY
    assert float(got["ADAPT_MU"]) == sm.ADAPT_MU and float(got["ADAPT_TAU"]) == sm.ADAPT_TAU
    text = open(os.path.join(ROOT, "clipper_amd", "csrc", "sdp_rules.hpp")).read()
    assert "#include <hip" not in text and "__global__" not in text


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "clipper_amd", "csrc", "host_sdpwide_plan.hpp")).read()
    assert "#include <hip" not in text and "hipMalloc" not in text


def test_facade_surfaces():
    import clipper_amd
    cp = clipper_amd.load_clipperpy()
    assert [int(cp.sdp.Route.Workgroup), int(cp.sdp.Route.Auto), int(cp.sdp.Route.Wide)] == [0, 1, 2]
    assert cp.sdp.route() == cp.sdp.Route.Workgroup
    cp.sdp.set_route(cp.sdp.Route.Auto)
    assert cp.sdp.route() == cp.sdp.Route.Auto and abi.sdp_route() == abi.SDP_ROUTE_AUTO  # one setting per process
    cp.sdp.set_route(cp.sdp.Route.Workgroup)
    assert abi.sdp_route() == abi.SDP_ROUTE_WORKGROUP
    h = open(os.path.join(ROOT, "include", "clipper", "sdp.h")).read()
    assert "enum class Route { Workgroup = 0, Auto = 1, Wide = 2 };" in h
    assert "void setRoute(Route route);" in h and "Route route();" in h
