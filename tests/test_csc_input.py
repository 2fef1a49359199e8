"""CPU test of the sparse input checks of clipper_hip_set_sparse (clipper_amd/csrc/host_csc_input.hpp): the
structure checks, the upper-triangle filter, the C == pattern(M) test and the symmetric lists are pure host code;
tests/cpp/test_csc_input.cpp (g++ only) checks each refusal with its message, the dropped-entry count and the lists of
small matrices against answers written by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_csc_input_checks_and_lists(tmp_path):
    exe = str(tmp_path / "test_csc_input")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_csc_input.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "csc input ok" in out
