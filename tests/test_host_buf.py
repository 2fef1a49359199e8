"""CPU test of the host side's owning types (clipper_amd/csrc/host_buf.hpp: DevBuf, PinnedBuf, Event):
tests/cpp/test_host_buf.cpp (g++ only) includes the header over counting stubs of the runtime calls it makes and checks
that an array is kept while it is large enough and replaced by exactly the size asked for otherwise; that a growth
that fails leaves {null, 0} so that a later, smaller request allocates (the stale capacity of the resident solver's
exchange buffer); that a moved-from owner frees nothing and a move-assignment frees the target's array once; that
every free runs with the buffer's own device current; that two buffers which shared a capacity field are
independent; that the live counters return to zero and the allocation count counts every success; that a mapped
pinned buffer asks for its device alias once per allocation. Run twice: plain, and under the address and
undefined-behaviour sanitizers (a stand-alone program)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_owners_over_counting_stubs(tmp_path, flags):
    exe = str(tmp_path / "test_host_buf")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-self-move", *flags, "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_host_buf.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = run.stdout.decode()
    assert run.returncode == 0 and "host buf ok" in out and "FAILED" not in out, out[-4000:]
