"""CPU test of the matcher's shared filter rules (clipper_amd/csrc/match_rules.hpp): tests/cpp/test_match_rules.cpp
(g++ only) drives the predicate the device's k_match_select uses with a plain loop in the kernel's order of work
(count, scan, write) and compares it with clipper_match::select row for row; once more as a stand-alone program under
the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "sanitized"])
def test_rules_reproduce_select(tmp_path, flags):
    exe = str(tmp_path / "test_match_rules")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_match_rules.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "match rules ok" in out.stdout, out.stdout + out.stderr
