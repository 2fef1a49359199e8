"""CPU test of the order in which an ICP call's refusals are tried (clipper_amd/csrc/host_icp_check.hpp's check_call):
tests/cpp/test_icp_call_checks.cpp (g++ alone, no device) builds, for each of the five entry points, a call that is
wrong in every rung at once, repairs the rungs one at a time and compares every message."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_refusals_come_in_the_entry_points_order(tmp_path):
    exe = str(tmp_path / "test_icp_call_checks")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_icp_call_checks.cpp"), "-o", exe])
    run = subprocess.run([exe], timeout=60, capture_output=True, text=True)
    assert run.returncode == 0 and "icp call checks ok" in run.stdout and "FAILED" not in run.stdout, run.stdout
