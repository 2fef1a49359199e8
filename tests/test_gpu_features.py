"""GPU tests of the point-cloud features (clipper_hip_estimate_normals, clipper_hip_compute_fpfh,
clipper_hip_fpfh_from_points: k_features.hip.h, host_features.hpp) against the numpy model tests/features_model.py.

Counts: exactly. Normals: sin(angle to numpy's eigh) <= 1e-9 wherever the eigenvalue gap (l1 - l0) / l2 is >= 1e-3
(eigenvector perturbation <= 2 ||E|| / gap; ||E|| is about (K + c) 2^-52 l2 for a centred sum of K <= 32 terms plus the
solver: 2e-11 at a gap of 1e-3, so 1e-9 leaves a factor of 50), with the share of points the gap condition leaves out
capped at 5 %; the sign wherever the rule decides it by more than 1e-6. SPFH and FPFH from the model's normals: bit for
bit, after the test has asserted that no bin coordinate of its input lies within 1e-9 of a bin edge (only atan2 may
differ from libm, by ulps). The one-call route: the two-call route's bits. Each cloud is the smallest that reaches its
edge of the kernels; the model of a cloud is computed once and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration
from tests import features_model as fm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


CASES, model = fm.GPU_CASES, fm.case_model


@pytest.mark.parametrize("name", list(CASES))
def test_counts_and_normals(name):
    m = model(name)
    P, view = m["P"], m["view"]
    N, cnt = abi.estimate_normals(P.T, knn=m["knn"], radius=m["radius"], viewpoint=view, return_counts=True)
    N = N.T
    assert np.array_equal(cnt, m["cnt"])
    assert np.all(np.isfinite(N)) and np.all(np.abs(np.linalg.norm(N, axis=1) - 1.0) <= 1e-14)
    few = m["cnt"] < 3
    assert np.all(N[few] == (0.0, 0.0, 1.0))
    sure = ~few & (m["gap"] >= 1e-3)
    left_out = ~few & ~sure
    sin = fm.sin_angle(N, m["N"])
    print(f"{name}: cnt {cnt.min()}..{cnt.max()}, {few.sum()} fixed, {left_out.sum()} left out, "
          f"max sin {sin[sure].max() if sure.any() else 0.0:.3g}, min gap {m['gap'][~few].min() if (~few).any() else 0:.3g}")
    if m["generic"]:
        assert left_out.sum() <= 0.05 * len(P)
    if sure.any():
        assert sin[sure].max() <= 1e-9
    if view is None:
        a = np.sort(np.abs(m["N"]), axis=1)
        clear = sure & (a[:, 2] - a[:, 1] > 1e-6)
    else:
        d = np.asarray(view) - P
        clear = sure & (np.abs(fm.dot(m["N"], d)) / np.linalg.norm(d, axis=1) > 1e-6)
    assert np.all(fm.dot(N, m["N"])[clear] > 0)
    if name == "radius":
        assert (m["cnt"] == 1).any() and (m["cnt"] == 2).any() and (m["cnt"] >= 3).any()
    if name == "on_radius":
        assert m["cnt"].min() == 4 and m["cnt"].max() == 6
    if name == "line3":                                # any unit vector orthogonal to the line
        assert np.all(np.abs(N @ np.array([0.3, -0.7, 0.45])) / np.linalg.norm([0.3, -0.7, 0.45]) <= 1e-9)
    if name == "plane4":                               # exactly, and the largest component positive
        assert np.all(N == (0.0, 0.0, 1.0))
        assert np.all(abi.estimate_normals(P.T, knn=4, viewpoint=(0.5, 0.5, -2.0)).T == (0.0, 0.0, -1.0))


@pytest.mark.parametrize("name", [k for k, v in CASES.items() if v[4]])
def test_spfh_and_fpfh_bit_for_bit_from_given_normals(name):
    m = model(name)
    assert np.all(np.isinf(m["margin"]) | (m["margin"] >= 1e-9)), "the input sits on a bin edge: choose another"
    F, S, cnt = abi.compute_fpfh(m["P"].T, m["N"].T, knn=m["knn"], radius=m["radius"], return_spfh=True)
    print(f"{name}: min margin {m['margin'].min():.3g}, SPFH rows differing {np.any(S.T != m['S'], axis=1).sum()}, "
          f"FPFH rows differing {np.any(F.T != m['F'], axis=1).sum()}, max |dF| {np.abs(F.T - m['F']).max():.3g}")
    assert np.array_equal(cnt, m["cnt"])
    assert np.array_equal(S.T, m["S"])
    assert np.array_equal(F.T, m["F"])
    if name == "doubled_k8":                           # the twin is a neighbour at sqd == 0: counted in SPFH, no weight
        idx, sqd, kept, _ = fm.neighborhoods(m["P"], m["knn"])
        assert np.all((sqd[:, 1] == 0) & (idx[:, :2].min(axis=1) == np.arange(len(m["P"])) % 150))


@pytest.mark.parametrize("name,nk,nr,fk,fr", [("bunny_k16", 16, 0.0, 32, 0.0), ("bunny_k16", 32, 0.03, 16, 0.02),
                                              ("n1025_k16", 8, 0.0, 8, 0.0), ("n2", 3, 0.0, 5, 0.0),
                                              ("radius", 10, 0.2, 20, 0.25), ("n2100_k32", 5, 0.0, 30, 0.0)])
def test_one_call_route_gives_the_two_call_routes_bits(name, nk, nr, fk, fr):
    P = model(name)["P"]
    view = (0.3, 0.2, 5.0)
    N2 = abi.estimate_normals(P.T, knn=nk, radius=nr, viewpoint=view)
    F2 = abi.compute_fpfh(P.T, N2, knn=fk, radius=fr)
    F1, N1 = abi.fpfh_from_points(P.T, normal_knn=nk, normal_radius=nr, viewpoint=view, knn=fk, radius=fr)
    assert np.array_equal(N1, N2) and np.array_equal(F1, F2)
    assert F1.shape == (33, len(P)) and np.all(np.isfinite(F1))


def test_refusals_leave_the_library_usable():
    m = model("n10_k16")
    P = np.ascontiguousarray(m["P"])
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    L = abi.load_library()
    n = len(P)
    out, F = np.zeros((n, 3)), np.zeros((n, 33))
    ok = C.byref(abi.Neighborhood(16, 0.0))
    bad = P.copy()
    bad[7, 2] = np.nan
    zero = np.zeros((n, 3))
    cases = [
        (L.clipper_hip_estimate_normals, (0, dp(P), n, C.byref(abi.Neighborhood(2, 0.0)), None, dp(out), None),
         "neighbourhood: knn must be in 3..32 (knn = 2)"),
        (L.clipper_hip_estimate_normals, (0, dp(bad), n, ok, None, dp(out), None),
         "P: non-finite value at coordinate 2 of point 7"),
        (L.clipper_hip_compute_fpfh, (0, dp(P), dp(zero), n, ok, dp(F), None, None),
         "N: normal 0 is not of unit length (squared length = 0)"),
        (L.clipper_hip_compute_fpfh, (0, dp(P), None, n, ok, dp(F), None, None), "null normal array"),
        (L.clipper_hip_fpfh_from_points, (0, dp(P), n, ok, None, C.byref(abi.Neighborhood(3, np.inf)), dp(F), None),
         "feature neighbourhood: radius must be finite (radius = inf)"),
        (L.clipper_hip_fpfh_from_points, (0, dp(P), 0, ok, None, ok, dp(F), None), "a cloud needs at least one point (n = 0)"),
        (L.clipper_hip_estimate_normals, (99, dp(P), n, ok, None, dp(out), None),
             f"device 99 out of range ({abi.device_count()} visible)"),
    ]
    for fn, args, msg in cases:
        rc = fn(*args)
        assert (rc, (L.clipper_hip_last_error() or b"").decode()) == (-1, msg)
        F2, S2, cnt = abi.compute_fpfh(P.T, m["N"].T, knn=16, return_spfh=True)     # the next valid call succeeds
        assert np.array_equal(F2.T, m["F"]) and np.array_equal(cnt, m["cnt"])


def test_python_surfaces_return_the_abi_bits():
    m = model("bunny_k16")
    P = m["P"]
    view = (0.0, 0.1, 1.0)
    N = abi.estimate_normals(P.T, knn=12, viewpoint=view)
    F = abi.compute_fpfh(P.T, N, knn=20, radius=0.03)
    Nr = registration.estimate_normals(P, knn=12, viewpoint=view)                     # rows = points
    assert Nr.shape == (len(P), 3) and np.array_equal(Nr, N.T)
    assert np.array_equal(registration.compute_fpfh(P, Nr, knn=20, radius=0.03), F.T)
    Fr = registration.compute_fpfh(P, knn=20, radius=0.03, normal_knn=12, viewpoint=view)
    assert Fr.shape == (len(P), 33) and np.array_equal(Fr, F.T)
    assert np.array_equal(registration.estimate_normals(P), abi.estimate_normals(P.T, knn=16).T)   # the defaults
    assert np.array_equal(registration.compute_fpfh(P), abi.fpfh_from_points(P.T, 16, 0.0, None, 32, 0.0)[0].T)
    cp = clipper_amd.load_clipperpy()
    Pf = np.asfortranarray(P.T)
    Np = np.asarray(cp.utils.estimate_normals(Pf, knn=12, viewpoint=list(view)))
    assert np.array_equal(Np, N)
    assert np.array_equal(np.asarray(cp.utils.compute_fpfh(Pf, np.asfortranarray(Np), knn=20, radius=0.03)), F)
    assert np.array_equal(np.asarray(cp.utils.estimate_normals(Pf)), abi.estimate_normals(P.T))
    with pytest.raises(ValueError, match="knn must be in 3..32"):                     # std::invalid_argument
        cp.utils.estimate_normals(Pf, knn=2)


def test_cpp_facade_features(tmp_path):
    P = model("bunny_k16")["P"]
    exe = str(tmp_path / "test_features_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_features_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    files = [str(tmp_path / f) for f in ("P.f64", "N.f64", "F.f64", "F1.f64")]
    P.tofile(files[0])                              # row-major n x 3 = column-major 3 x n
    out = subprocess.run([exe, str(len(P))] + files, capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "ALL FEATURES FACADE TESTS PASSED" in out.stdout
    view = (0.0, 0.1, 1.0)
    N = abi.estimate_normals(P.T, knn=12, viewpoint=view)
    F = abi.compute_fpfh(P.T, N, knn=20, radius=0.03)
    assert np.array_equal(np.fromfile(files[1]).reshape(-1, 3), N.T)
    assert np.array_equal(np.fromfile(files[2]).reshape(-1, 33), F.T)
    assert np.array_equal(np.fromfile(files[3]).reshape(-1, 33), F.T)


def test_end_to_end():
    """raw clouds -> normals -> FPFH -> mutual matches -> Euclidean fill -> solve -> rigid transform, with nothing but
    this library: the bunny and a rotated, translated, permuted copy of it (noise-free: the errors are rounding). The
    numpy model gives 593 mutual matches on this input, 590 of them correct. The rotation error is read off the
    antisymmetric part of R^T Rhat (its sine): an arccos of the trace cannot resolve an angle below 1e-8. The fill's
    epsilon sits between what the two kinds of pairs show: two correct associations differ in their distances by
    rounding (4e-16 here), while the wrong ones land on a point 0.7 to 1.4 mm beside the right one (the sample has such
    near-twins) and differ from most others by about that much."""
    P = fm.bunny()
    Q, perm, T = fm.transformed_copy(P)
    F0 = registration.compute_fpfh(P, knn=16, viewpoint=P.mean(axis=0))
    F1 = registration.compute_fpfh(Q, knn=16, viewpoint=Q.mean(axis=0))
    A, _ = registration.match_descriptors(F0, F1, knn=1, mutual=True)
    right = perm[A[:, 0]] == A[:, 1]
    print(f"{len(A)} mutual matches, {right.sum()} correct")
    assert len(A) >= 500 and right.mean() >= 0.95
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(P.T, Q.T, A, sigma=5e-6, epsilon=1e-5)
    s = g.solve(np.random.default_rng(4).random(len(A)))
    sel = A[s.nodes]
    print(f"{len(sel)} selected")
    assert len(sel) >= 400 and np.all(perm[sel[:, 0]] == sel[:, 1])         # every selected association is correct
    That = abi.estimate_rigid_transform(P.T, Q.T, sel)
    E = T[:3, :3].T @ That[:3, :3]
    assert np.trace(E) > 2.9
    rot = float(np.arcsin(min(1.0, 0.5 * np.linalg.norm([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]))))
    trans = float(np.linalg.norm(That[:3, 3] - T[:3, 3]))
    print(f"rotation error {rot:.3g} rad, translation error {trans:.3g}")
    assert rot <= 1e-9 and trans <= 1e-9
