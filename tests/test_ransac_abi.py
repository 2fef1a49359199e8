"""CPU-side checks of clipper_hip_ransac_correspondences and clipper_hip_ransac_needed: the struct layouts against a C
program, the refusals (every check runs on the host before the device is asked, so they answer with no device present,
each naming its value), the device after them, and the stop rule against the model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import registration as reg
from tests import ransac_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_NODEVICE = -1, -4


def test_struct_layouts_match_header(tmp_path):
    fields_p = ["max_distance", "edge_similarity", "confidence", "max_hypotheses", "hypotheses_per_round", "n_sample",
                "refine_iterations", "reserved", "seed"]
    fields_i = ["status", "refined", "evaluated", "checked", "best_hypothesis", "best_count", "count", "fitness",
                "inlier_rmse", "sample", "device_ms"]
    args = ["sizeof(clipper_ransac_params_t)"] + [f"offsetof(clipper_ransac_params_t, {f})" for f in fields_p]
    args += ["sizeof(clipper_ransac_info_t)"] + [f"offsetof(clipper_ransac_info_t, {f})" for f in fields_i]
    enums = ["CLIPPER_RANSAC_CONVERGED", "CLIPPER_RANSAC_MAX_HYPOTHESES", "CLIPPER_RANSAC_NO_MODEL", "CLIPPER_HIP_E_INVALID",
             "CLIPPER_HIP_E_NODEVICE"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf("'
                   + "%zu " * len(args) + "%d " * len(enums) + '\\n", ' + ", ".join(args + enums) + ');return 0;}\n')
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [C.sizeof(abi.RansacParams)] + [getattr(abi.RansacParams, f).offset for f in fields_p]
    want += [C.sizeof(abi.RansacInfo)] + [getattr(abi.RansacInfo, f).offset for f in fields_i]
    assert got[:len(args)] == want
    assert want[0] == 56 and want[len(fields_p) + 1] == 104
    assert got[len(args):] == [abi.RANSAC_CONVERGED, abi.RANSAC_MAX_HYPOTHESES, abi.RANSAC_NO_MODEL, E_INVALID, E_NODEVICE]
    assert [abi.RANSAC_CONVERGED, abi.RANSAC_MAX_HYPOTHESES, abi.RANSAC_NO_MODEL] == [rm.CONVERGED, rm.MAX_HYPOTHESES, rm.NO_MODEL]
    p = abi.RansacParams(0.02)
    assert (p.edge_similarity, p.confidence, p.max_hypotheses, p.hypotheses_per_round, p.n_sample, p.refine_iterations,
            p.reserved, p.seed) == (0.9, 0.999, 100000, 4096, 3, 1, 0, 0)


def _inputs():
    D1 = np.asfortranarray(np.array([[0.0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]))          # 3 x 4
    D2 = np.asfortranarray(np.array([[0.0, 1, 0, 0, 5], [0, 0, 1, 0, 6], [0, 0, 0, 1, 7]]))  # 3 x 5
    A = np.array([0, 1, 2, 3, 0, 1, 2, 4], np.int32)                                         # column-major 4 x 2
    return D1, D2, A


def _call(D1=None, D2=None, A=None, m=4, n1=4, n2=5, prm="default", T="default", device=0, **kw):
    L = abi.load_library()
    d1, d2, a = _inputs()
    D1 = d1 if D1 is None else D1
    D2 = d2 if D2 is None else D2
    A = a if A is None else A
    dp = lambda x: None if x is False else x.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    p = abi.RansacParams(**dict(dict(max_distance=0.02), **kw)) if prm == "default" else prm
    Tbuf = np.zeros(16) if T == "default" else T
    rc = L.clipper_hip_ransac_correspondences(device, dp(D1), n1, dp(D2), n2,
                                              None if A is False else A.ctypes.data_as(C.POINTER(C.c_int32)), m,
                                              None if p is None else C.byref(p), dp(Tbuf), None, None)
    return rc, abi._last_error()


def _refusals():
    d1, d2, a = _inputs()
    nan1, inf2 = d1.copy(order="F"), d2.copy(order="F")
    nan1[1, 2] = np.nan
    inf2[0, 4] = np.inf
    neg, far = a.copy(), a.copy()
    neg[1] = -1
    far[6] = 5
    bad_reserved = abi.RansacParams(0.02)
    bad_reserved.reserved = 7
    return [
        (dict(T=False), "null T_out"),
        (dict(prm=None), "null params"),
        (dict(D1=False), "null D1 point array"),
        (dict(D2=False), "null D2 point array"),
        (dict(A=False), "null association array"),
        (dict(n1=0), "D1: a cloud needs at least one point (n = 0)"),
        (dict(n2=2 ** 31), "D2: more than 2^31 - 1 points in a cloud (n = 2147483648)"),
        (dict(m=2), "fewer associations than a sample holds (m = 2, n_sample = 3)"),
        (dict(n_sample=5), "fewer associations than a sample holds (m = 4, n_sample = 5)"),
        (dict(m=2 ** 31), "more than 2^31 - 1 associations (m = 2147483648)"),
        (dict(A=neg), "association row 1 out of range (-1, 1)"),
        (dict(A=far), "association row 2 out of range (2, 5)"),
        (dict(n2=4), "association row 3 out of range (3, 4)"),
        (dict(D1=nan1), "D1: non-finite value at coordinate 1 of point 2 (association row 2)"),
        (dict(D2=inf2), "D2: non-finite value at coordinate 0 of point 4 (association row 3)"),
        (dict(max_distance=0.0), "max_distance must be positive and finite (max_distance = 0)"),
        (dict(max_distance=np.inf), "max_distance must be positive and finite (max_distance = inf)"),
        (dict(edge_similarity=1.0), "edge_similarity must be in [0, 1) (edge_similarity = 1)"),
        (dict(edge_similarity=-0.1), "edge_similarity must be in [0, 1) (edge_similarity = -0.1)"),
        (dict(confidence=0.0), "confidence must be in (0, 1) (confidence = 0)"),
        (dict(confidence=1.0), "confidence must be in (0, 1) (confidence = 1)"),
        (dict(max_hypotheses=0), "max_hypotheses must be in 1..2^31 - 1 (max_hypotheses = 0)"),
        (dict(max_hypotheses=2 ** 31), "max_hypotheses must be in 1..2^31 - 1 (max_hypotheses = 2147483648)"),
        (dict(hypotheses_per_round=128), "hypotheses_per_round must be a multiple of 256 in 256..65536 (hypotheses_per_round = 128)"),
        (dict(hypotheses_per_round=300), "(hypotheses_per_round = 300)"),
        (dict(hypotheses_per_round=65792), "(hypotheses_per_round = 65792)"),
        (dict(n_sample=2), "n_sample must be in 3..8 (n_sample = 2)"),
        (dict(n_sample=9), "n_sample must be in 3..8 (n_sample = 9)"),
        (dict(refine_iterations=-1), "refine_iterations must be in 0..10 (refine_iterations = -1)"),
        (dict(refine_iterations=11), "refine_iterations must be in 0..10 (refine_iterations = 11)"),
        (dict(prm=bad_reserved), "reserved must be 0 (reserved = 7)"),
    ]


@pytest.mark.parametrize("kw,text", _refusals(), ids=lambda x: x if isinstance(x, str) else None)
def test_refusals_name_their_values_before_the_device(kw, text):
    # device 12345 does not exist anywhere: a refusal that names the argument shows the check came first
    rc, msg = _call(device=12345, **kw)
    assert rc == E_INVALID and "ransac_correspondences: " in msg and text in msg, (rc, msg)


def test_valid_arguments_reach_the_device():
    rc, msg = _call()
    if abi.device_count() > 0:
        assert rc == 0, msg
        rc, msg = _call(device=12345)
        assert rc == E_INVALID and "device 12345 out of range" in msg, (rc, msg)
    else:
        assert rc == E_NODEVICE and "no HIP device visible" in msg, (rc, msg)


def test_needed_is_the_models():
    for count, m, n, conf in [(10, 10, 3, 0.999), (40, 200, 3, 0.999), (3, 1000, 3, 0.999), (3, 2 ** 31 - 1, 3, 0.999),
                              (50, 1000, 4, 0.99), (0, 10, 3, 0.5), (7, 9, 8, 0.999999)]:
        assert abi.ransac_needed(count, m, n, conf) == rm.needed(count, m, n, conf)
    assert abi.ransac_needed(10, 10, 3, 0.999) == 1 and abi.ransac_needed(3, 2 ** 31 - 1, 3, 0.999) == 2 ** 63 - 1
    for bad in [(11, 10, 3, 0.999), (-1, 10, 3, 0.999), (1, 0, 3, 0.999), (1, 10, 2, 0.999), (1, 10, 3, 1.0)]:
        with pytest.raises(abi.ClipperError, match="ransac_needed"):
            abi.ransac_needed(*bad)


def test_python_facades_share_one_signature():
    import inspect
    a = inspect.signature(abi.ransac_correspondences)
    b = inspect.signature(reg.ransac_correspondences)
    names = ["D1", "D2", "A", "max_distance", "n_sample", "edge_similarity", "max_hypotheses", "confidence", "seed",
             "refine_iterations", "hypotheses_per_round", "device"]
    assert list(a.parameters) == names == list(b.parameters)
    defaults = [p.default for p in a.parameters.values()][4:]
    assert defaults == [3, 0.9, 100000, 0.999, 0, 1, 4096, 0] == [p.default for p in b.parameters.values()][4:]
    with pytest.raises(abi.ClipperError, match="n_sample must be in 3..8"):
        reg.ransac_correspondences(np.zeros((3, 4)), np.zeros((3, 4)), np.zeros((4, 2), np.int32), 0.02, n_sample=2)
