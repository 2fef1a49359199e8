"""CPU-side checks of the robust ICP entry points (clipper_hip_icp_robust, clipper_hip_icp_generalized_robust): the
layouts of clipper_icp_robust_t and clipper_icp_robust_info_t against a C program that includes the header; every refusal
of the robust settings through the real library with no device (the argument check comes first, then "no HIP device
visible"), each naming its value; the Python facade sends the default keywords to the plain entry points."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import registration as reg
from tests import icp_robust_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_and_enumerators(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf('
                   '"%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", sizeof(clipper_icp_robust_t),'
                   'offsetof(clipper_icp_robust_t, loss), offsetof(clipper_icp_robust_t, reserved),'
                   'offsetof(clipper_icp_robust_t, scale), offsetof(clipper_icp_robust_t, trim),'
                   'sizeof(clipper_icp_robust_info_t), offsetof(clipper_icp_robust_info_t, within),'
                   'offsetof(clipper_icp_robust_info_t, weight_sum), offsetof(clipper_icp_robust_info_t, trim_sqd),'
                   'CLIPPER_ICP_LOSS_NONE, CLIPPER_ICP_LOSS_HUBER, CLIPPER_ICP_LOSS_CAUCHY, CLIPPER_ICP_LOSS_TUKEY,'
                   'CLIPPER_ICP_LOSS_GEMAN_MCCLURE);return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    R, I = abi.IcpRobust, abi.IcpRobustInfo
    assert got[:5] == [C.sizeof(R), R.loss.offset, R.reserved.offset, R.scale.offset, R.trim.offset] == [24, 0, 4, 8, 16]
    assert got[5:9] == [C.sizeof(I), I.within.offset, I.weight_sum.offset, I.trim_sqd.offset] == [24, 0, 8, 16]
    assert got[9:] == [abi.ICP_LOSS_NONE, abi.ICP_LOSS_HUBER, abi.ICP_LOSS_CAUCHY, abi.ICP_LOSS_TUKEY,
                       abi.ICP_LOSS_GEMAN_MCCLURE] == [rm.NONE, rm.HUBER, rm.CAUCHY, rm.TUKEY, rm.GEMAN_MCCLURE]
    for name in ("clipper_hip_icp_robust", "clipper_hip_icp_generalized_robust"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(abi.load_library(), name)
    facade = open(os.path.join(ROOT, "include", "clipper", "registration.h")).read()
    assert "enum class IcpLoss { None = 0, Huber = 1, Cauchy = 2, Tukey = 3, GemanMcClure = 4 }" in facade


def _robust(loss=0, scale=0.0, trim=1.0, reserved=0):
    r = abi.IcpRobust(loss, scale, trim)
    r.reserved = reserved
    return r


# (the robust settings, what the refusal says)
REFUSALS = [
    (None, "null robust"),
    (_robust(loss=5), "unknown loss 5 (the losses are 0..4)"),
    (_robust(loss=-1), "unknown loss -1 (the losses are 0..4)"),
    (_robust(reserved=3), "robust: reserved must be 0 (reserved = 3)"),
    (_robust(abi.ICP_LOSS_HUBER, 0.0), "scale must be positive and finite with a loss (scale = 0)"),
    (_robust(abi.ICP_LOSS_CAUCHY, -0.25), "scale must be positive and finite with a loss (scale = -0.25)"),
    (_robust(abi.ICP_LOSS_TUKEY, np.inf), "scale must be positive and finite with a loss (scale = inf)"),
    (_robust(abi.ICP_LOSS_GEMAN_MCCLURE, np.nan), "scale must be positive and finite with a loss (scale = "),
    (_robust(trim=0.0), "trim must be in (0, 1] (trim = 0)"),
    (_robust(trim=-0.5), "trim must be in (0, 1] (trim = -0.5)"),
    (_robust(trim=1.5), "trim must be in (0, 1] (trim = 1.5)"),
    (_robust(trim=np.nan), "trim must be in (0, 1] (trim = "),
]


def _call(L, which, rb, prm=None, T_out=True):
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    P = np.ascontiguousarray(np.arange(12, dtype=np.float64).reshape(4, 3) / 7.0)
    I6 = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (4, 1))
    T = np.zeros(16)
    rbp = None if rb is None else C.byref(rb)
    if which == "icp":
        prm = prm or abi.IcpParams(abi.ICP_POINT_TO_POINT, 0.1)
        rc = L.clipper_hip_icp_robust(0, dp(P), 4, dp(P), None, 4, None, C.byref(prm), rbp, dp(T) if T_out else None, None,
                                      None, None)
    else:
        prm = prm or abi.IcpParams(abi.ICP_GENERALIZED, 0.1)
        rc = L.clipper_hip_icp_generalized_robust(0, dp(P), dp(I6), 4, dp(P), dp(I6), 4, None, C.byref(prm), rbp,
                                                  dp(T) if T_out else None, None, None, None)
    return rc, abi._last_error()


@pytest.mark.parametrize("which", ["icp", "gicp"])
def test_refusals_name_their_values_without_a_device(which):
    L = abi.load_library()
    name = "icp_robust: " if which == "icp" else "icp_generalized_robust: "
    for rb, text in REFUSALS:
        rc, msg = _call(L, which, rb)
        assert rc == -1 and name + text in msg, (rc, msg, text)      # CLIPPER_HIP_E_INVALID
    # the checks the plain calls make are made here too
    rc, msg = _call(L, which, _robust(), T_out=False)
    assert rc == -1 and name + "null T_out" in msg
    rc, msg = _call(L, which, _robust(), prm=abi.IcpParams(abi.ICP_GENERALIZED if which == "icp" else 0, 0.1))
    assert rc == -1 and ("call clipper_hip_icp_generalized" in msg if which == "icp" else "(method = 0)" in msg)
    rc, msg = _call(L, which, _robust(), prm=abi.IcpParams(0 if which == "icp" else 2, 0.0))
    assert rc == -1 and "max_distance must be positive and finite (max_distance = 0)" in msg
    # without a loss the scale is not read: accepted, and only then the device is asked for
    if abi.device_count() == 0:
        for rb in (_robust(), _robust(scale=-1.0), _robust(abi.ICP_LOSS_HUBER, 0.01, 0.5)):
            rc, msg = _call(L, which, rb)
            assert rc == -4 and "no HIP device visible" in msg, (rc, msg)     # CLIPPER_HIP_E_NODEVICE


def test_python_facade_keywords(monkeypatch):
    P = np.zeros((4, 3))
    I6 = np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (4, 1))
    with pytest.raises(ValueError, match="loss must be one of"):
        reg.icp(P, P, max_distance=0.1, loss="welsch")
    with pytest.raises(ValueError, match="loss must be one of"):
        reg.icp_generalized(P, P, None, I6, I6, max_distance=0.1, loss="l2")
    with pytest.raises(abi.ClipperError, match=r"icp_robust: trim must be in \(0, 1\] \(trim = 2\)"):
        reg.icp(P, P, max_distance=0.1, trim=2.0)
    with pytest.raises(abi.ClipperError, match=r"icp_generalized_robust: scale must be positive and finite with a loss \(scale = 0\)"):
        reg.icp_generalized(P, P, None, I6, I6, max_distance=0.1, loss="huber")
    # the defaults take the existing path, anything else the new one
    seen = []
    monkeypatch.setattr(abi, "icp", lambda *a, **k: seen.append(("icp", k)) or "plain")
    monkeypatch.setattr(abi, "icp_robust", lambda *a, **k: seen.append(("icp_robust", k)) or "robust")
    monkeypatch.setattr(abi, "icp_generalized", lambda *a, **k: seen.append(("gicp", k)) or "plain")
    monkeypatch.setattr(abi, "icp_generalized_robust", lambda *a, **k: seen.append(("gicp_robust", k)) or "robust")
    assert reg.icp(P, P, max_distance=0.1) == "plain" and reg.icp(P, P, max_distance=0.1, loss="none", scale=0.0, trim=1.0) == "plain"
    assert reg.icp(P, P, max_distance=0.1, loss="cauchy", scale=0.02) == "robust"
    assert reg.icp(P, P, max_distance=0.1, trim=0.7) == "robust"
    assert reg.icp_generalized(P, P, None, I6, I6, max_distance=0.1) == "plain"
    assert reg.icp_generalized(P, P, None, I6, I6, max_distance=0.1, loss="tukey", scale=0.03, trim=0.8) == "robust"
    assert [s[0] for s in seen] == ["icp", "icp", "icp_robust", "icp_robust", "gicp", "gicp_robust"]
    assert "loss" not in seen[0][1] and (seen[2][1]["loss"], seen[2][1]["scale"], seen[2][1]["trim"]) == (abi.ICP_LOSS_CAUCHY, 0.02, 1.0)
    assert (seen[5][1]["loss"], seen[5][1]["scale"], seen[5][1]["trim"]) == (abi.ICP_LOSS_TUKEY, 0.03, 0.8)
