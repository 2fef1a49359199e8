"""k_wave.hip.h on the device: wave_sum, wave_max, wave_scan_incl, block_scan_excl, block_scan_array at every
instantiation the kernels use, and the project's scan kernels (k_row_scan, k_slice_scan_*, k_rv_scan, k_kg_slabs,
k_kg_sum) launched as the host code launches them, each against a plain host loop, bit for bit, with guard words
round every output. The program is tests/hip/wave_check.hip, built by clipper_amd/build.py with the library; it runs
ONCE here, as a child process, and every case asserts its own line of that run."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_bin", "wave_check")
RUN_LIMIT_S = 120


def _case_names():
    try:
        return subprocess.run([EXE, "--list"], capture_output=True, text=True, timeout=60, check=True).stdout.split()
    except (OSError, subprocess.SubprocessError):
        return ["(wave_check --list did not run)"]  # the one case fails below: a missing executable is no skip


@pytest.fixture(scope="module")
def run():
    """the one run of the program: its exit status (None: not started, or ended at the time limit) and its output"""
    if not os.path.isfile(EXE):
        return None, f"{EXE} is missing: clipper_amd/build.py's build_all() builds it"
    try:
        p = subprocess.run([EXE], capture_output=True, text=True, timeout=RUN_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        return None, f"no end after {RUN_LIMIT_S} s\n{e.stdout or ''}\n{e.stderr or ''}"
    return p.returncode, p.stdout + p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("case", _case_names())
def test_wave_check(run, case):
    status, output = run
    # 0: all passed, 1: mismatches, each on its case's line. Anything else (2: a HIP error, a signal, the time limit)
    # ends every case with the whole output; nothing is run again.
    assert status in (0, 1), f"wave_check ended with status {status}:\n{output}"
    lines = [ln for ln in output.splitlines() if ln.split(":")[0].split(" ", 1)[-1] == case]
    assert lines == [f"PASS {case}"], "\n".join(lines) or f"no line for {case} in:\n{output}"
