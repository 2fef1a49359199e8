"""CPU checks of the semidefinite relaxation's interfaces (no GPU): the ctypes structs against the C header (a gcc
program prints sizes and offsets), the ABI constants, and the clipperpy names."""
import ctypes
import os
import subprocess

import pytest

from clipper_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _c_layout(tmp_path, struct, fields):
    src = tmp_path / "layout.c"
    offs = "".join(f'printf(" %zu", offsetof({struct}, {f}));' for f in fields)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\n'
                   f'int main(void){{printf("%zu", sizeof({struct}));{offs}printf(" %d\\n", CLIPPER_HIP_SDP_MAX_N);return 0;}}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]


@pytest.mark.parametrize("cls,struct", [(abi.SdpParams, "clipper_sdp_params_t"), (abi.SdpInfo, "clipper_sdp_info_t")])
def test_struct_layouts_match_header(tmp_path, cls, struct):
    names = [f[0] for f in cls._fields_]
    got = _c_layout(tmp_path, struct, names)
    assert got[0] == ctypes.sizeof(cls)
    assert got[1:-1] == [getattr(cls, f).offset for f in names]
    assert got[-1] == abi.SDP_MAX_N == 128


def test_params_defaults_are_the_reference_defaults():
    p = abi.SdpParams()  # sdp.h:40-52
    assert (p.verbose, p.max_iters, p.acceleration_interval, p.acceleration_lookback) == (0, 2000, 10, 10)
    assert p.eps_abs == pytest.approx(1e-3) and p.eps_rel == pytest.approx(1e-3)
    assert p.eps_infeas == pytest.approx(1e-7) and p.time_limit_secs == 0.0


def test_entry_points_are_exported_names():
    assert "clipper_hip_sdp" in abi.EXPORTED_SYMBOLS and "clipper_hip_sdp_solve" in abi.EXPORTED_SYMBOLS
    assert callable(abi.sdp_solve) and callable(abi.HipClipper.sdp)


def test_clipperpy_names():
    import clipper_amd
    cp = clipper_amd.load_clipperpy()
    assert hasattr(cp, "sdp") and callable(cp.sdp.solve)
    s = cp.SDPSolution()
    for f in ("X", "lambdas", "evec1", "thr", "nodes", "iters", "pobj", "dobj", "t", "t_parse", "t_scs",
              "t_scs_setup", "t_scs_solve", "t_scs_linsys", "t_scs_cone", "t_scs_accel", "t_extract"):
        assert hasattr(s, f), f
    assert callable(cp.CLIPPER.set_device_sdp) and callable(cp.CLIPPER.solve_as_msrc_sdr)


def test_facade_header_declares_the_solver():
    h = open(os.path.join(ROOT, "include", "clipper", "sdp.h")).read()
    assert "Solution solve(const MatrixXd& M, const MatrixXd& C, const Params& params = Params{});" in h
    c = open(os.path.join(ROOT, "include", "clipper", "clipper.h")).read()
    assert "void setDeviceSdp(bool on)" in c and "bool device_sdp_ = false;" in c
