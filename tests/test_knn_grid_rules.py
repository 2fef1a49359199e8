"""CPU test of the rules of the nearest-neighbour search's grid route (clipper_amd/csrc/knn_grid_rules.hpp, DESIGN.md
section 9, "The grid route of the search"): tests/cpp/test_knn_grid_rules.cpp (g++ only) restates build + query on the
host over the rules header and the plan function and compares the lists with a direct brute force, entry for entry
and bit for bit, for K in {1, 4, 32} on uniform clouds, a self-search, the same shifted by 1e6, a shuffled integer
lattice, repeated points, planar and collinear clouds, identical points, queries outside the box, fewer points than K,
and two tight clusters a unit apart (which degenerates to visiting most of the cloud: slow there, never wrong)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_grid_lists_equal_brute_force_on_the_host(tmp_path):
    exe = str(tmp_path / "test_knn_grid_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_knn_grid_rules.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "knn grid rules ok" in out and "knn grid plan ok" in out, out[-4000:]
    assert "DIFFERENT" not in out
