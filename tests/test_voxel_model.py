"""CPU tests of voxel down-sampling (clipper_hip_voxel_downsample): the rules header voxel_rules.hpp with the host
checks host_voxel_check.hpp, compiled with g++ alone by tests/cpp/test_voxel_rules.cpp into a restatement of the whole
call (its order found twice: std::stable_sort, and an LSD radix sort over the header's digits), against the numpy
model tests/voxel_model.py on the table of clouds the GPU tests use. Every comparison is an equality of bytes or
integers. The model asserts its own sharpness: adding a voxel's members in the reversed order changes bits."""
import os
import subprocess

import numpy as np
import pytest

from tests import voxel_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("voxel") / "test_voxel_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_voxel_rules.cpp"), "-o", out])
    return out


def run_host(exe, tmp_path, P, voxel_size, N=None):
    """the g++ program's result as a dict like the model's, or its refusal as a string"""
    n = len(P)
    pf, nf, of = (str(tmp_path / f) for f in ("P.f64", "N.f64", "out.bin"))
    np.ascontiguousarray(P, np.float64).tofile(pf)
    if N is not None:
        np.ascontiguousarray(N, np.float64).tofile(nf)
    r = subprocess.run([exe, str(n), pf, nf if N is not None else "-", repr(float(voxel_size)), of], capture_output=True,
                       text=True, timeout=300)
    if r.returncode == 2:
        return r.stdout.strip()
    assert r.returncode == 0 and "voxel rules ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    raw = open(of, "rb").read()
    head = np.frombuffer(raw, np.int64, 5)
    m, at = int(head[0]), 40
    out = dict(dim=head[1:4].copy(), passes=int(head[4]))
    out["points"] = np.frombuffer(raw, np.float64, 3 * m, at).reshape(m, 3)
    at += 24 * m
    out["normals"] = None
    if N is not None:
        out["normals"] = np.frombuffer(raw, np.float64, 3 * m, at).reshape(m, 3)
        at += 24 * m
    out["counts"] = np.frombuffer(raw, np.int32, m, at)
    at += 4 * m
    out["trace"] = np.frombuffer(raw, np.int32, n, at)
    at += 4 * n
    out["keys"] = np.frombuffer(raw, np.uint64, m, at)
    assert at + 8 * m == len(raw)
    return out


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_equals_model(got, want):
    assert same_bits(np.ascontiguousarray(got["points"]), want["points"])
    assert (got["normals"] is None) == (want["normals"] is None)
    if want["normals"] is not None:
        assert same_bits(np.ascontiguousarray(got["normals"]), want["normals"])
    assert np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["trace"], want["trace"])
    assert np.array_equal(got["keys"], want["keys"])
    assert np.array_equal(got["dim"], want["dim"]) and got["passes"] == want["passes"]


@pytest.mark.parametrize("name", list(vm.CASES))
def test_rules_header_gives_the_models_bits(exe, tmp_path, name):
    P, vs, N, want = vm.case_model(name)
    got = run_host(exe, tmp_path, P, vs, N)
    assert_equals_model(got, want)
    assert want["counts"].sum() == len(P) and np.all(np.diff(want["keys"].astype(np.int64)) > 0)


def test_the_table_reaches_what_it_is_there_for():
    """the properties the cases are named after, asserted on the model: a change of a cloud shows what it did to it"""
    m = lambda name: vm.case_model(name)[3]                                     # noqa: E731
    assert m("identical64")["dim"].tolist() == [1, 1, 1] and m("identical64")["passes"] == 0
    assert m("identical64")["counts"].tolist() == [64] and m("one_voxel_700")["counts"].tolist() == [700]
    assert m("chunk_edges")["counts"].tolist() == [511, 512, 513, 1024, 1025]
    for p, corner in vm.PASS_CORNERS.items():
        assert m(f"passes{p}")["passes"] == p and m(f"passes{p}")["dim"].tolist() == [c + 1 for c in corner]
    assert vm.PASS_CORNERS[8] == (2 ** 20 - 1,) * 3 and int(m("passes8")["keys"].max()) == 2 ** 60 - 1
    td = m("top_digit")
    assert td["passes"] == 3 and len(td["keys"]) == 16
    assert np.all(td["keys"] & np.uint64(0xFFFF) == 0) and len(set((td["keys"] >> np.uint64(16)).tolist())) == 16
    f = m("faces")
    assert f["dim"].tolist() == [5, 5, 5] and len(f["counts"]) == 125 and int(f["keys"].max()) == 124
    assert np.all(f["counts"] >= 2)
    assert m("planar")["dim"][2] == 1 and m("planar")["dim"][0] > 1
    assert np.array_equal(m("shifted_1e6")["counts"], m("uniform5000")["counts"])
    assert np.array_equal(m("shifted_1e6")["trace"], m("uniform5000")["trace"])
    assert m("opposite_normals")["normals"].tolist()[0] == [0.0, 0.0, 1.0]
    assert m("opposite_normals")["normals"].tolist()[1] != [0.0, 0.0, 1.0]
    T = vm.SORT_TILE
    for n in (T - 1, T, T + 1, 2 * T + 1):
        assert m(f"tile_{n}_equal")["passes"] == 0 and m(f"tile_{n}_equal")["counts"].tolist() == [n]
        assert m(f"tile_{n}_equal_far")["passes"] == 2 and m(f"tile_{n}_equal_far")["counts"].tolist() == [n - 1, 1]
        d = m(f"tile_{n}_descending")
        assert np.array_equal(d["trace"], np.arange(n - 1, -1, -1)) and d["passes"] == 2
        r = m(f"tile_{n}_random")
        assert r["passes"] == 2 and len(r["counts"]) <= 555 and r["counts"].max() >= 3


def test_model_is_sharp_about_the_order_of_addition():
    """adding a voxel's members in descending index is a different function: the bits must show it (the share of rows is
    printed), or a wrong order would pass every comparison"""
    for name in ("one_voxel_700", "uniform5000"):
        P, vs, N, want = vm.case_model(name)
        rev = vm.voxel_down_sample(P, vs, N, reverse=True)
        assert np.array_equal(rev["counts"], want["counts"]) and np.array_equal(rev["trace"], want["trace"])
        changed = np.any(rev["points"] != want["points"], axis=1)
        print(f"{name}: {changed.sum()} of {len(changed)} rows change when the members are added in reversed order")
        assert changed.any()
    P, vs, N, want = vm.case_model("one_voxel_700_normals")
    assert np.any(vm.voxel_down_sample(P, vs, N, reverse=True)["normals"] != want["normals"])


def test_host_checks_refuse_what_the_entry_point_refuses(exe, tmp_path):
    P = np.random.default_rng(0).random((5, 3))
    bad = P.copy()
    bad[3, 1] = np.nan
    wide = np.array([[0.0, 0.0, 0.0], [0.0, float(2 ** 21), 0.0]])            # 2^21 + 1 voxels of edge 1 along y
    fits = np.array([[0.0, 0.0, 0.0], [0.0, float(2 ** 21 - 1), 0.0]])
    N = np.tile([0.0, 0.0, 1.0], (5, 1))
    badn = N.copy()
    badn[2, 0] = np.inf
    assert run_host(exe, tmp_path, P, 0.0) == "refused: voxel_size must be finite and greater than 0 (voxel_size = 0)"
    assert run_host(exe, tmp_path, P, -1.0) == "refused: voxel_size must be finite and greater than 0 (voxel_size = -1)"
    assert run_host(exe, tmp_path, P, np.nan).startswith("refused: voxel_size must be finite and greater than 0")
    assert run_host(exe, tmp_path, P, np.inf) == "refused: voxel_size must be finite and greater than 0 (voxel_size = inf)"
    assert run_host(exe, tmp_path, bad, 0.1) == "refused: P: non-finite value at coordinate 1 of point 3"
    assert run_host(exe, tmp_path, P, 0.1, badn) == "refused: N: non-finite value at coordinate 0 of normal 2"
    assert run_host(exe, tmp_path, wide, 1.0) == \
        "refused: voxel_size = 1 gives more than 2^21 voxels along axis 1 (extent 2.09715e+06)"
    assert run_host(exe, tmp_path, P, 1e-320).startswith("refused: voxel_size = ")   # (1 / voxel_size is infinite)
    got = run_host(exe, tmp_path, fits, 1.0)
    assert got["dim"].tolist() == [1, 2 ** 21, 1] and got["passes"] == 3
    with pytest.raises(ValueError):
        vm.voxel_down_sample(wide, 1.0)
    empty = run_host(exe, tmp_path, np.zeros((0, 3)), 0.1)
    assert len(empty["points"]) == 0 and len(empty["trace"]) == 0
