"""CPU test of the host side of descriptor matching (clipper_amd/csrc/host_match_select.hpp): the argument checks, the
zero padding and the filters (mutual check, ratio test, distance bound) are pure host code;
tests/cpp/test_match_select.cpp (g++ only) checks the filters on lists written by hand — each alone and all together,
the boundary cases of every comparison, the row order — and each refusal with its message."""
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_match_filters_and_refusals(tmp_path):
    exe = str(tmp_path / "test_match_select")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_match_select.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "match select ok" in out


def test_entry_point_refuses_bad_arguments_before_any_device_work():
    F = np.random.default_rng(0).random((33, 10))
    for kw, msg in ((dict(knn=9), "knn must be in 1..8 (knn = 9)"), (dict(ratio=1.5), "ratio must be 0 (off) or in (0, 1)"),
                    (dict(knn=2, ratio=0.8), "the ratio test needs knn == 1")):
        with pytest.raises(abi.ClipperError) as e:
            abi.match_descriptors(F, F, **kw)
        assert "error -1:" in str(e.value) and msg in str(e.value)
    with pytest.raises(abi.ClipperError, match="descriptors must have 1..64 coordinates"):
        abi.match_descriptors(np.zeros((65, 4)), np.zeros((65, 4)))
    bad = F.copy()
    bad[5, 7] = np.inf
    with pytest.raises(abi.ClipperError, match="F1: non-finite value at coordinate 5 of descriptor 7"):
        abi.match_descriptors(F, bad)
    if abi.device_count() <= 0:                    # no CPU fallback: a valid call without a device says so
        with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
            abi.match_descriptors(F, F)
