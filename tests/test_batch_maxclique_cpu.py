"""CPU checks of the batched maximum-clique call ("Batches"): the exported entry points and their
bindings, the refusals that return before the device is looked for, the facades' surfaces, and the plan header (g++
only). The GPU side is tests/test_gpu_batch_maxclique.py."""
import ctypes as C
import os
import subprocess

from clipper_amd import _abi as abi
from clipper_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("clipper_hip_batch_max_clique", "clipper_hip_batch_max_clique_stats")


def test_library_exports_and_bindings():
    lib = C.CDLL(build.build_hip())  # cross-compiles for gfx950 if stale; no GPU needed
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in abi.EXPORTED_SYMBOLS
    L = abi.load_library()
    assert L.clipper_hip_batch_max_clique.argtypes[3] == C.POINTER(abi.MaxCliqueInfo)
    assert len(L.clipper_hip_batch_max_clique_stats.argtypes) == 4
    assert callable(abi.HipBatch.max_clique) and callable(abi.HipBatch.max_clique_stats)
    assert callable(abi.HipBatch.get_nodes)


def test_header_declares_the_entry_points():
    h = open(os.path.join(ROOT, "include", "clipper_hip.h")).read()
    assert "int clipper_hip_batch_max_clique(clipper_hip_batch_t* b, int method, double time_limit_s," in h
    assert "int clipper_hip_batch_max_clique_stats(const clipper_hip_batch_t* b, int32_t* launches, int32_t* n_batched," in h


def test_refusals_before_the_device():
    L = abi.load_library()
    info = (abi.MaxCliqueInfo * 1)()
    assert L.clipper_hip_batch_max_clique(None, abi.MC_EXACT, 0.0, info) == -1
    assert L.clipper_hip_batch_max_clique(None, abi.MC_EXACT, 0.0, None) == -1
    assert L.clipper_hip_batch_max_clique_stats(None, None, None, None) == -1


def test_plan_header(tmp_path):
    exe = str(tmp_path / "test_mc_batch_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_mc_batch_plan.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "mc batch plan ok" in out


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "clipper_amd", "csrc", "host_mcplan.hpp")).read()
    assert "#include <hip" not in text and "hipMalloc" not in text


def test_new_sources_are_in_the_build_lists():
    """the library is rebuilt when one of them changes: the staleness check takes its sources from the tree"""
    from clipper_amd import build
    srcs = build.hip_sources()
    for f in ("k_maxclique.hip.h", "host_maxclique.hpp", "host_mcplan.hpp", "clipper_hip.hip"):
        assert os.path.join(ROOT, "clipper_amd", "csrc", f) in srcs, f
        assert os.path.exists(os.path.join(ROOT, "clipper_amd", "csrc", f)), f
    assert os.path.join(ROOT, "include", "clipper_hip.h") in srcs


def test_facade_surfaces():
    import clipper_amd
    cp = clipper_amd.load_clipperpy()
    assert hasattr(cp.CLIPPERBatch, "solve_as_maximum_clique")
    b = open(os.path.join(ROOT, "include", "clipper", "batch.h")).read()
    assert "std::vector<Solution> solveAsMaximumClique(const maxclique::Params& params" in b
