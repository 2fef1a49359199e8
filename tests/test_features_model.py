"""CPU tests of the point-cloud features (clipper_hip_estimate_normals / clipper_hip_compute_fpfh): the numpy model
tests/features_model.py against the contract's own properties, the rules header features_rules.hpp (compiled with g++
alone by tests/cpp/test_features_rules.cpp) against the model, the inputs of the GPU tests against the preconditions
those tests rely on (eigenvalue gap, bin margin), every refusal of the entry points with its message (they are raised
before any device work, so no device is needed), and the struct layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import registration
from tests import features_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def inputs():
    """(name, P, knn, radius) of the three clouds the GPU tests compare bit for bit, with the model's results"""
    out = []
    for name, P, knn, radius in (("uniform", fm.uniform_cloud(), 16, 0.0), ("bunny16", fm.bunny(), 16, 0.0),
                                 ("bunny32r", fm.bunny(), 32, 0.02)):
        N, cnt, gap = fm.normals(P, knn, radius)
        F, S, fcnt, margin = fm.fpfh(P, N, knn, radius)
        out.append(dict(name=name, P=P, knn=knn, radius=radius, N=N, cnt=cnt, gap=gap, F=F, S=S, margin=margin))
    return out


def test_group_sums_are_200_where_a_point_has_a_real_neighbour(inputs):
    for d in inputs:
        idx, sqd, kept, cnt = fm.neighborhoods(d["P"], d["knn"], d["radius"])
        real = np.array([np.any(kept[i] & (idx[i] != i) & (sqd[i] != 0)) for i in range(len(d["P"]))])
        assert real.sum() > 0.9 * len(real)
        sums = d["F"].reshape(-1, 3, 11).sum(axis=2)
        assert np.all(np.abs(sums[real] - 200.0) <= 1e-9), d["name"]
        # SPFH alone: every pair adds one count to each group, scaled by 100 / (cnt - 1)
        assert np.all(np.abs(d["S"].reshape(-1, 3, 11).sum(axis=2)[d["cnt"] >= 2] - 100.0) <= 1e-9)


def test_inputs_meet_the_gpu_tests_preconditions(inputs):
    """the share of points whose normal the data do not determine (gap < 1e-3) is capped at 5 %, and no bin coordinate
    lies within 1e-9 of a bin edge: printed, so that a change of the inputs shows what it did to them"""
    for d in inputs:
        print(f"{d['name']}: min gap {d['gap'].min():.3g}, min margin {d['margin'].min():.3g}, "
              f"cnt {d['cnt'].min()}..{d['cnt'].max()}")
        assert np.mean(d["gap"] < 1e-3) <= 0.05
        assert d["margin"].min() >= 1e-9
        assert np.all(np.abs(np.linalg.norm(d["N"], axis=1) - 1.0) <= 1e-12)


@pytest.mark.parametrize("name", [k for k, v in fm.GPU_CASES.items() if v[4]])
def test_every_generic_gpu_case_meets_the_preconditions(name):
    """what tests/test_gpu_features.py asserts about its own inputs before it compares, checked where no device is
    needed: at most 5 % of the points left out by the gap condition, no bin coordinate within 1e-9 of an integer"""
    m = fm.case_model(name)
    few = m["cnt"] < 3
    assert (~few & (m["gap"] < 1e-3)).sum() <= 0.05 * len(m["P"])
    assert np.all(np.isinf(m["margin"]) | (m["margin"] >= 1e-9))
    if name == "radius":
        assert (m["cnt"] == 1).any() and (m["cnt"] == 2).any() and (m["cnt"] >= 3).any()


def test_model_on_clouds_with_known_answers():
    # 4 coplanar points: the normal is the plane's, exactly up to sign; the largest component made positive
    P = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    N, cnt, _ = fm.normals(P, 4)
    assert np.all(cnt == 4) and np.all(np.abs(N - (0.0, 0.0, 1.0)) <= 1e-15)
    N, _, _ = fm.normals(P, 4, viewpoint=(0.5, 0.5, -2.0))
    assert np.all(np.abs(N - (0.0, 0.0, -1.0)) <= 1e-15)
    # a point exactly on the radius is kept: power-of-two coordinates, 0.5^2 == 0.25 == radius * radius exactly
    G = fm.grid_cloud()
    idx, sqd, kept, cnt = fm.neighborhoods(G, 8, 0.5)
    assert np.all(sqd[kept] <= 0.25) and np.any(sqd[kept] == 0.25) and np.all(sqd[~kept] >= 0.5)
    assert cnt.min() == 4 and cnt.max() == 6            # a corner: itself and 3 axis neighbours; an edge centre: 5
    # fewer than three neighbours: the fixed normal; one neighbour: an SPFH of one pair, times 100
    P = np.array([[0.0, 0.0, 0.0], [1.0, 2.0, 3.0]])
    N, cnt, gap = fm.normals(P, 3)
    assert cnt.tolist() == [2, 2] and np.all(N == (0.0, 0.0, 1.0)) and np.all(gap == 0)
    F, S, _, _ = fm.fpfh(P, N, 3)
    assert np.all(S.reshape(2, 3, 11).sum(axis=2) == 100.0) and np.all(np.sort(S, axis=1)[:, -3:] == 100.0)
    assert np.all(np.abs(F.reshape(2, 3, 11).sum(axis=2) - 200.0) <= 1e-9)


def test_rules_header_gives_the_models_bins_and_normals(tmp_path):
    exe = str(tmp_path / "test_features_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-I",
                           os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_features_rules.cpp"), "-o", exe])
    p1, n1, p2, n2 = fm.random_pairs(2000)
    pairs, nbrs = str(tmp_path / "pairs.f64"), str(tmp_path / "nbrs.f64")
    np.concatenate([p1, n1, p2, n2], axis=1).tofile(pairs)
    # the neighbourhoods of the bunny at knn = 16, each with its own point first (list order is (distance, index))
    P = fm.bunny()
    idx, _, _, cnt = fm.neighborhoods(P, 16)
    assert np.all(cnt == 16) and np.all(idx[:, 0] == np.arange(len(P)))
    P[idx].tofile(nbrs)
    out = subprocess.check_output([exe, pairs, "2000", nbrs, str(len(P)), "16"], timeout=300).decode().split("\n")
    assert "features rules ok" in out
    got = np.array([[int(x) for x in ln.split()] for ln in out[:2000]])
    f = fm.pair_features(p1, n1, p2, n2)
    c = fm.bin_coords(f)
    assert np.abs(c - np.round(c)).min() >= 1e-9            # no pair sits on a bin edge: atan2's last bits cannot matter
    assert np.all(f[:10] == 0)                              # the degenerate pairs
    assert np.array_equal(got, fm.bins(f))
    # normals: sin(angle) <= 1e-9 where the gap is >= 1e-3 (eigenvector perturbation <= 2 ||E|| / gap with ||E|| about
    # (K + c) 2^-52 l2 for a centred sum of K <= 32 terms plus the solver: 2e-11 at a gap of 1e-3)
    rows = np.array([[float(x) for x in ln.split()] for ln in out[2000:2000 + len(P)]])
    for got_n, view in ((rows[:, :3], None), (rows[:, 3:], (0.5, 0.5, 3.0))):
        N, _, gap = fm.normals(P, 16, viewpoint=view)
        sure = gap >= 1e-3
        assert np.mean(~sure) <= 0.05
        assert np.all(np.abs(np.linalg.norm(got_n, axis=1) - 1.0) <= 1e-14)
        assert fm.sin_angle(got_n, N)[sure].max() <= 1e-9
        # the sign, wherever the rule decides it by more than rounding
        if view is None:
            clear = sure & (np.sort(np.abs(N), axis=1)[:, 2] - np.sort(np.abs(N), axis=1)[:, 1] > 1e-6)
        else:
            d = np.asarray(view) - P
            clear = sure & (np.abs(fm.dot(N, d)) / np.linalg.norm(d, axis=1) > 1e-6)
        assert clear.sum() > 0.9 * len(P) and np.all(fm.dot(got_n, N)[clear] > 0)


def _raw(name, *args):
    L = abi.load_library()
    rc = getattr(L, name)(*args)
    return rc, (L.clipper_hip_last_error() or b"").decode()


def test_entry_points_refuse_bad_arguments_before_any_device_work():
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    n = 5
    P = np.ascontiguousarray(np.random.default_rng(0).random((n, 3)))
    N = np.tile(np.array([0.0, 0.6, 0.8]), (n, 1))
    Nout, F = np.zeros((n, 3)), np.zeros((n, 33))
    nb = abi.Neighborhood(3, 0.0)
    ok = C.byref(nb)
    nan_p, inf_p = P.copy(), P.copy()
    nan_p[3, 1] = np.nan
    inf_p[4, 2] = -np.inf
    bad_n, long_n, short_n = N.copy(), N.copy(), N.copy()
    bad_n[2, 0] = np.inf
    long_n[1] = (0.0, 0.0, 1.01)
    short_n[4] = (0.0, 0.0, 0.0)
    view = np.array([0.0, np.nan, 0.0])
    cases = [
        ("clipper_hip_estimate_normals", (0, None, n, ok, None, dp(Nout), None), "null point array"),
        ("clipper_hip_estimate_normals", (0, dp(P), n, ok, None, None, None), "null normal output array"),
        ("clipper_hip_estimate_normals", (0, dp(P), n, None, None, dp(Nout), None), "null neighbourhood"),
        ("clipper_hip_estimate_normals", (0, dp(P), 0, ok, None, dp(Nout), None), "a cloud needs at least one point (n = 0)"),
        ("clipper_hip_estimate_normals", (0, dp(P), n, C.byref(abi.Neighborhood(2, 0.0)), None, dp(Nout), None),
         "neighbourhood: knn must be in 3..32 (knn = 2)"),
        ("clipper_hip_estimate_normals", (0, dp(P), n, C.byref(abi.Neighborhood(33, 0.0)), None, dp(Nout), None),
         "neighbourhood: knn must be in 3..32 (knn = 33)"),
        ("clipper_hip_estimate_normals", (0, dp(P), n, C.byref(abi.Neighborhood(3, np.inf)), None, dp(Nout), None),
         "neighbourhood: radius must be finite (radius = inf)"),
        ("clipper_hip_estimate_normals", (0, dp(P), n, C.byref(abi.Neighborhood(3, np.nan)), None, dp(Nout), None),
         "neighbourhood: radius must be finite (radius = nan)"),
        ("clipper_hip_estimate_normals", (0, dp(nan_p), n, ok, None, dp(Nout), None),
         "P: non-finite value at coordinate 1 of point 3"),
        ("clipper_hip_estimate_normals", (0, dp(P), n, ok, dp(view), dp(Nout), None),
         "viewpoint: non-finite value at coordinate 1"),
        ("clipper_hip_compute_fpfh", (0, None, dp(N), n, ok, dp(F), None, None), "null point array"),
        ("clipper_hip_compute_fpfh", (0, dp(P), None, n, ok, dp(F), None, None), "null normal array"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(N), n, ok, None, None, None), "null descriptor output array"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(N), n, None, dp(F), None, None), "null neighbourhood"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(N), -1, ok, dp(F), None, None), "a cloud needs at least one point (n = -1)"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(N), n, C.byref(abi.Neighborhood(40, 0.0)), dp(F), None, None),
         "neighbourhood: knn must be in 3..32 (knn = 40)"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(N), n, C.byref(abi.Neighborhood(8, -np.inf)), dp(F), None, None),
         "neighbourhood: radius must be finite (radius = -inf)"),
        ("clipper_hip_compute_fpfh", (0, dp(inf_p), dp(N), n, ok, dp(F), None, None),
         "P: non-finite value at coordinate 2 of point 4"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(bad_n), n, ok, dp(F), None, None),
         "N: non-finite value at coordinate 0 of normal 2"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(long_n), n, ok, dp(F), None, None),
         "N: normal 1 is not of unit length (squared length = 1.0201)"),
        ("clipper_hip_compute_fpfh", (0, dp(P), dp(short_n), n, ok, dp(F), None, None),
         "N: normal 4 is not of unit length (squared length = 0)"),
        ("clipper_hip_fpfh_from_points", (0, None, n, ok, None, ok, dp(F), None), "null point array"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), n, ok, None, ok, None, None), "null descriptor output array"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), n, None, None, ok, dp(F), None), "null normal neighbourhood"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), n, ok, None, None, dp(F), None), "null feature neighbourhood"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), n, C.byref(abi.Neighborhood(2, 0.0)), None, ok, dp(F), None),
         "normal neighbourhood: knn must be in 3..32 (knn = 2)"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), n, ok, None, C.byref(abi.Neighborhood(33, 0.0)), dp(F), None),
         "feature neighbourhood: knn must be in 3..32 (knn = 33)"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), n, ok, None, C.byref(abi.Neighborhood(4, np.nan)), dp(F), None),
         "feature neighbourhood: radius must be finite (radius = nan)"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), 0, ok, None, ok, dp(F), None), "a cloud needs at least one point (n = 0)"),
        ("clipper_hip_fpfh_from_points", (0, dp(nan_p), n, ok, None, ok, dp(F), None),
         "P: non-finite value at coordinate 1 of point 3"),
        ("clipper_hip_fpfh_from_points", (0, dp(P), n, ok, dp(view), ok, dp(F), None),
         "viewpoint: non-finite value at coordinate 1"),
    ]
    for name, args, msg in cases:
        assert _raw(name, *args) == (-1, msg), (name, msg)          # CLIPPER_HIP_E_INVALID
    # the Python surfaces carry the message
    with pytest.raises(abi.ClipperError, match=r"error -1: neighbourhood: knn must be in 3..32 \(knn = 2\)"):
        abi.estimate_normals(P.T, knn=2)
    with pytest.raises(abi.ClipperError, match="N: normal 1 is not of unit length"):
        registration.compute_fpfh(P, long_n, knn=3)
    with pytest.raises(abi.ClipperError, match=r"feature neighbourhood: knn must be in 3..32 \(knn = 64\)"):
        registration.compute_fpfh(P, knn=64)
    if abi.device_count() <= 0:                    # no CPU fallback: a valid call without a device says so
        with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
            registration.estimate_normals(P, knn=3)
        with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
            registration.compute_fpfh(P, N, knn=3)
        with pytest.raises(abi.ClipperError, match="error -4: no HIP device"):
            registration.compute_fpfh(P)


def test_neighborhood_layout_matches_the_header(tmp_path):
    src = tmp_path / "nb.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){printf("%zu %zu %zu %zu\\n",'
                   'sizeof(clipper_neighborhood_t), offsetof(clipper_neighborhood_t, knn),'
                   'offsetof(clipper_neighborhood_t, reserved), offsetof(clipper_neighborhood_t, radius));return 0;}\n')
    exe = tmp_path / "nb"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    nb = abi.Neighborhood
    assert got == [C.sizeof(nb), nb.knn.offset, nb.reserved.offset, nb.radius.offset] == [16, 0, 4, 8]
    assert (abi.Neighborhood().knn, abi.Neighborhood().radius) == (16, 0.0)
    for name in ("clipper_hip_estimate_normals", "clipper_hip_compute_fpfh", "clipper_hip_fpfh_from_points"):
        assert name in abi.EXPORTED_SYMBOLS and hasattr(abi.load_library(), name)
