"""CPU checks of the selector of the nearest-neighbour search's route (clipper_hip_knn_set_search, DESIGN.md section 9,
"The grid route of the search"): the setter and the getter, the refusal of an unknown mode, the layout of the
statistics record, what a grid-mode search answers without a device, and the plan function's promises (dim = 1 on
zero-extent axes, never more cells than points)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def search_mode():
    """hands the test the setter and puts the process-wide mode back as it was found"""
    before = abi.knn_search()
    try:
        yield abi.knn_set_search
    finally:
        abi.knn_set_search(before)


def test_symbols_and_constants_match_the_header(tmp_path):
    for name in ("clipper_hip_knn_set_search", "clipper_hip_knn_search", "clipper_hip_knn_last_search"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(abi.load_library(), name)
    src = tmp_path / "knn.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf("%d %d %d %d %d %d %d %d %d\\n",'
                   'CLIPPER_HIP_KNN_BRUTE, CLIPPER_HIP_KNN_GRID, CLIPPER_HIP_KNN_AUTO, (int)sizeof(clipper_hip_knn_stats_t),'
                   '(int)offsetof(clipper_hip_knn_stats_t, dim), (int)offsetof(clipper_hip_knn_stats_t, queries),'
                   '(int)offsetof(clipper_hip_knn_stats_t, candidates), (int)offsetof(clipper_hip_knn_stats_t, auto_min_n),'
                   '(int)CLIPPER_HIP_KNN_AUTO_MIN_N);return 0;}\n')
    exe = tmp_path / "knn"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got[:3] == [abi.KNN_BRUTE, abi.KNN_GRID, abi.KNN_AUTO] == [0, 1, 2]
    assert got[3] == C.sizeof(abi.KnnStats)
    assert got[4:8] == [abi.KnnStats.dim.offset, abi.KnnStats.queries.offset, abi.KnnStats.candidates.offset,
                        abi.KnnStats.auto_min_n.offset]
    assert abi.knn_last_search().auto_min_n == got[8] >= 1       # the library reports the threshold it was built with


def test_setter_returns_the_previous_mode_and_the_getter_follows(search_mode):
    assert abi.knn_search() == abi.KNN_BRUTE                       # the default (every test puts it back)
    assert search_mode(abi.KNN_GRID) == abi.KNN_BRUTE
    assert abi.knn_search() == abi.KNN_GRID
    assert search_mode(abi.KNN_AUTO) == abi.KNN_GRID
    assert abi.knn_search() == abi.KNN_AUTO
    assert search_mode(abi.KNN_BRUTE) == abi.KNN_AUTO
    assert abi.knn_search() == abi.KNN_BRUTE


def test_setter_refuses_an_unknown_mode(search_mode):
    search_mode(abi.KNN_GRID)
    for bad in (-1, 3, 99):
        with pytest.raises(abi.ClipperError, match=f"unknown search mode {bad}"):
            abi.knn_set_search(bad)
        assert abi.load_library().clipper_hip_knn_set_search(bad) == -1
        assert f"unknown search mode {bad}" in abi.load_library().clipper_hip_last_error().decode()
        assert abi.knn_search() == abi.KNN_GRID                    # unchanged
    assert abi.load_library().clipper_hip_knn_last_search(None) == -1


def test_grid_mode_without_a_device_says_so(search_mode):
    if abi.device_count() > 0:                                     # (with a device the GPU tests cover the grid route)
        return
    search_mode(abi.KNN_GRID)
    P = np.random.default_rng(0).random((3, 50))
    idx, sqd = np.zeros((50, 2), np.int32), np.zeros((50, 2))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    rc = abi.load_library().clipper_hip_knn(0, P.ctypes.data_as(dp), 50, P.ctypes.data_as(dp), 50, 3, 2,
                                            idx.ctypes.data_as(ip), sqd.ctypes.data_as(dp))
    assert rc == -4 and "no HIP device" in abi.load_library().clipper_hip_last_error().decode()
    # the argument checks come first, as under brute force
    rc = abi.load_library().clipper_hip_knn(0, P.ctypes.data_as(dp), 50, P.ctypes.data_as(dp), 50, 3, 17,
                                            idx.ctypes.data_as(ip), sqd.ctypes.data_as(dp))
    assert rc == -1 and "knn must be in 1..16" in abi.load_library().clipper_hip_last_error().decode()


def test_plan_function(tmp_path):
    """dim = 1 on zero-extent axes (planar, collinear, identical points); cells <= max(1, n1) for n1 from 1 to 10^7
    over boxes of every shape; finite non-negative factors; the cell of a coordinate is monotone."""
    exe = str(tmp_path / "test_knn_grid_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_knn_grid_rules.cpp"), "-o", exe])
    out = subprocess.check_output([exe, "plan"], timeout=300).decode()
    assert "knn grid plan ok" in out, out[-2000:]


def test_python_facade_restores_the_mode_and_refuses_unknown_names(search_mode):
    from clipper_amd import registration
    search_mode(abi.KNN_AUTO)
    with pytest.raises(ValueError, match="search must be one of"):
        registration.ground_truth_associations(np.zeros((4, 3)), np.zeros((4, 3)), 0.1, search="kdtree")
    assert abi.knn_search() == abi.KNN_AUTO
    with registration._knn_search("grid"):
        assert abi.knn_search() == abi.KNN_GRID
    assert abi.knn_search() == abi.KNN_AUTO
