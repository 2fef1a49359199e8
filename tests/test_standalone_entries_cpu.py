"""CPU checks of what the stand-alone calls share: host_knn_k.hpp's list-length rule and K dispatch (a g++ program),
and the order every stand-alone entry point keeps: its own argument checks first, then the device (host_call.hpp's
use_device). The table is tests/standalone_entries.py's."""
import os
import subprocess

import pytest

from clipper_amd import _abi as abi
from tests import standalone_entries as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_length_rule_and_k_dispatch(tmp_path):
    """knn_list_k against a plain loop for every clamp pair in use; dispatch_k over every list a launch site names"""
    exe = str(tmp_path / "test_knn_k")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_knn_k.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=60).decode()
    assert "knn k ok" in out, out[-2000:]


@pytest.mark.parametrize("entry", se.ENTRIES, ids=lambda e: e[0])
def test_argument_checks_come_first_then_the_device(entry):
    if abi.device_count() > 0:                                     # (with a device the GPU tests cover the entry points)
        return
    rc, msg = se.call(entry, 0)
    assert rc == se.E_NODEVICE and "no HIP device visible" in msg, (rc, msg)
    rc, msg = se.call(entry, 0, bad=True)
    assert rc == se.E_INVALID and entry[2] in msg, (rc, msg)
