"""GPU tests of the descriptor matcher (clipper_hip_match_descriptors: k_match.hip.h, host_match.hpp) against the numpy
model tests/match_model.py on top of oracle/bm_utils_ref.knn_bruteforce: the forward lists bit for bit (same fp64
operations in the same order, ties by index), the filters' rows and distances exactly, every refusal with its message,
the Python / C++ surfaces, and the path descriptors -> associations -> affinity -> solve end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration
from oracle import bm_utils_ref as ref
from tests import match_model as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# every edge of the kernel at the smallest size that reaches it: one point; fewer points than K with a padded d; a
# second query block, one tile short, no padding; one coordinate into the second group with a second chunk of one
# point; three chunks through the merge; the widest instantiation; a lone query block over several chunks
@pytest.mark.parametrize("n0,n1,d,knn", [(1, 1, 1, 1), (5, 3, 33, 4), (257, 1023, 8, 1), (300, 1025, 9, 2),
                                          (130, 2049, 33, 4), (513, 700, 64, 8), (64, 3000, 32, 1)])
def test_lists_bit_for_bit(n0, n1, d, knn):
    rng = np.random.default_rng(n0 + n1 + d)
    F0, F1 = rng.random((n0, d)), rng.random((n1, d))
    A, sqd, idx, lsq = abi.match_descriptors(F0.T, F1.T, knn=knn, mutual=False, return_lists=True)
    ridx, rsqd = ref.knn_bruteforce(F0, F1, knn)
    assert idx.shape == (n0, knn) and np.array_equal(idx, ridx.astype(np.int32))
    have = ridx >= 0
    assert np.array_equal(lsq[have], rsqd[have])              # identical fp64 operations: equal to the last bit
    assert np.all(lsq[~have] == 1e300) and np.all(idx[~have] == -1)
    assert have.sum() == n0 * min(knn, n1)
    # without a filter the rows are the lists, read row by row
    assert np.array_equal(A, np.stack([np.nonzero(have)[0], ridx[have]], axis=1)) and np.array_equal(sqd, rsqd[have])


def test_ties_keep_the_lower_index():
    rng = np.random.default_rng(1)
    base = rng.random((40, 16))
    F1 = np.concatenate([base, base, base])       # every descriptor three times: indices j, j + 40, j + 80
    F0 = base[:10] + 1e-3
    _, _, idx, _ = abi.match_descriptors(F0.T, F1.T, knn=3, mutual=False, return_lists=True)
    for i in range(10):
        assert idx[i].tolist() == [i, i + 40, i + 80]
    # the same duplicates among the queries: the backward lists break their ties by the lower index of F0
    F0 = np.concatenate([F0, F0, F0])
    for knn, rows in ((3, 90), (2, 40)):          # knn = 2: the third copy of a query loses the tie in the backward list
        A, sqd = abi.match_descriptors(F0.T, F1.T, knn=knn, mutual=True)
        Am, sqdm, _, _ = mm.match_model(F0, F1, knn=knn, mutual=True)
        assert len(Am) == rows and np.array_equal(A, Am) and np.array_equal(sqd, sqdm)
    assert A[:, 0].max() == 19 and sorted(set(A[:, 1] // 40)) == [0, 1]


@pytest.fixture(scope="module")
def recipe():
    return mm.filter_recipe()


@pytest.mark.parametrize("swap", [False, True])
@pytest.mark.parametrize("knn,mutual,ratio,max_sqdist", mm.CONFIGS)
def test_filters(recipe, knn, mutual, ratio, max_sqdist, swap):
    F0, F1, _ = recipe
    if swap:                                       # n0 > n1: the backward search is not the forward one's mirror
        F0, F1 = F1, F0
    A, sqd = abi.match_descriptors(F0.T, F1.T, knn=knn, mutual=bool(mutual), ratio=ratio, max_sqdist=max_sqdist)
    Am, sqdm, _, _ = mm.match_model(F0, F1, knn, bool(mutual), ratio, max_sqdist)
    assert 0 < len(Am) < len(F0) * knn
    assert A.dtype == np.int32 and np.array_equal(A, Am) and np.array_equal(sqd, sqdm)


def _raw(F0, n0, F1, n1, d, prm, cap, A=True):
    """the C entry point itself: (status, message)"""
    L = abi.load_library()
    buf = np.zeros(2 * max(cap, 1), dtype=np.int32)
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    rc = L.clipper_hip_match_descriptors(0, dp(F0), n0, dp(F1), n1, d, None if prm is None else C.byref(prm),
                                         buf.ctypes.data_as(C.POINTER(C.c_int32)) if A else None, None, cap, None, None)
    return rc, (L.clipper_hip_last_error() or b"").decode()


def test_refusals_leave_the_library_usable():
    rng = np.random.default_rng(5)
    n0, n1, d = 6, 5, 4
    F0, F1 = np.ascontiguousarray(rng.random((n0, d))), np.ascontiguousarray(rng.random((n1, d)))
    P = abi.MatchParams
    ok = P(1, 1, 0.0, 0.0)
    bad = F0.copy()
    bad[2, 3] = np.nan
    inf = F1.copy()
    inf[4, 0] = np.inf
    cases = [
        ((None, n0, F1, n1, d, ok, n0), "null descriptor array"),
        ((F0, n0, None, n1, d, ok, n0), "null descriptor array"),
        ((F0, n0, F1, n1, d, None, n0), "null match parameters"),
        ((F0, 0, F1, n1, d, ok, n0), "both descriptor sets need at least one point (n0 = 0, n1 = 5)"),
        ((F0, n0, F1, 0, d, ok, n0), "both descriptor sets need at least one point (n0 = 6, n1 = 0)"),
        ((F0, n0, F1, n1, 0, ok, n0), "descriptors must have 1..64 coordinates (d = 0)"),
        ((F0, n0, F1, n1, 65, ok, n0), "descriptors must have 1..64 coordinates (d = 65)"),
        ((F0, n0, F1, n1, d, P(0, 1, 0.0, 0.0), n0), "knn must be in 1..8 (knn = 0)"),
        ((F0, n0, F1, n1, d, P(9, 1, 0.0, 0.0), 9 * n0), "knn must be in 1..8 (knn = 9)"),
        ((F0, n0, F1, n1, d, P(1, 1, -0.5, 0.0), n0), "ratio must be 0 (off) or in (0, 1) (ratio = -0.5)"),
        ((F0, n0, F1, n1, d, P(1, 1, 1.0, 0.0), n0), "ratio must be 0 (off) or in (0, 1) (ratio = 1)"),
        ((F0, n0, F1, n1, d, P(2, 1, 0.8, 0.0), 2 * n0), "the ratio test needs knn == 1 (knn = 2)"),
        ((bad, n0, F1, n1, d, ok, n0), "F0: non-finite value at coordinate 3 of descriptor 2"),
        ((F0, n0, inf, n1, d, ok, n0), "F1: non-finite value at coordinate 0 of descriptor 4"),
    ]
    want = mm.match_model(F0, F1, 1, True)[0]
    for args, msg in cases:
        rc, got = _raw(*args)
        assert (rc, got) == (-1, msg), (msg, rc, got)        # CLIPPER_HIP_E_INVALID
        A, _ = abi.match_descriptors(F0.T, F1.T)      # the next valid call succeeds
        assert np.array_equal(A, want)
    # a capacity one row short names the needed count; the exact capacity is enough
    full = mm.match_model(F0, F1, 2, False)[0]
    assert len(full) == 2 * n0
    assert _raw(F0, n0, F1, n1, d, P(2, 0, 0.0, 0.0), 2 * n0 - 1) == (-1, f"capacity {2 * n0 - 1} < {2 * n0} associations")
    assert _raw(F0, n0, F1, n1, d, P(2, 0, 0.0, 0.0), 2 * n0)[0] == 2 * n0
    assert _raw(F0, n0, F1, n1, d, P(2, 0, 0.0, 0.0), 2 * n0, A=False) == (-1, "null association buffer")
    with pytest.raises(abi.ClipperError, match="knn must be in 1..8"):
        abi.match_descriptors(F0.T, F1.T, knn=9)


def test_python_surfaces_return_the_abi_rows(recipe):
    F0, F1, _ = recipe
    cp = clipper_amd.load_clipperpy()
    for kw in (dict(), dict(knn=1, mutual=False, ratio=0.8), dict(knn=2, mutual=True, max_sqdist=0.12)):
        A, sqd = abi.match_descriptors(F0.T, F1.T, **kw)
        assert len(A) > 0
        Ar, sqdr = registration.match_descriptors(F0, F1, **kw)             # row-major n x d, as extractors give it
        assert np.array_equal(Ar, A) and np.array_equal(sqdr, sqd)
        Ap = cp.utils.match_descriptors(np.asfortranarray(F0.T), np.asfortranarray(F1.T), **kw)
        assert Ap.dtype == np.int32 and np.array_equal(np.asarray(Ap), A)
    with pytest.raises(ValueError, match="knn must be in 1..8"):             # std::invalid_argument
        cp.utils.match_descriptors(np.asfortranarray(F0.T), np.asfortranarray(F1.T), knn=9)


def test_cpp_facade_match_descriptors(recipe, tmp_path):
    F0, F1, _ = recipe
    exe = str(tmp_path / "test_match_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_match_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    f0, f1 = str(tmp_path / "F0.f64"), str(tmp_path / "F1.f64")
    F0.tofile(f0)                                  # row-major n x d = column-major d x n
    F1.tofile(f1)
    out = subprocess.run([exe, str(F0.shape[1]), str(len(F0)), str(len(F1)), f0, f1], capture_output=True, text=True,
                         timeout=300)
    sys.stdout.write(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr
    assert "ALL MATCH FACADE TESTS PASSED" in out.stdout
    lines = out.stdout.split("\n")
    pos = 0
    for name, kw in (("default", dict()), ("ratio", dict(mutual=False, ratio=0.8)), ("knn2", dict(knn=2, max_sqdist=0.12))):
        head = lines[pos].split()
        assert head[0] == name
        n = int(head[1])
        got = np.array([[int(x) for x in ln.split()] for ln in lines[pos + 1:pos + 1 + n]], dtype=np.int32).reshape(-1, 2)
        pos += 1 + n
        A, _ = abi.match_descriptors(F0.T, F1.T, **kw)
        assert n > 0 and np.array_equal(got, A)


def test_end_to_end():
    """descriptors -> associations -> Euclidean fill -> solve, with nothing but this library; the CPU twin is
    tests/test_match_model.py::test_end_to_end_on_the_cpu_oracle (precision 0.994, recall 0.743 there)."""
    pts, noisy, F0, F1, Agt = mm.bunny_recipe()
    A, _ = abi.match_descriptors(F0.T, F1.T, knn=1, mutual=False)
    assert np.array_equal(A, mm.match_model(F0, F1, knn=1, mutual=False)[0])
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(pts.T, noisy.T, A, sigma=0.015, epsilon=0.05)
    s = g.solve(np.random.default_rng(4).random(len(A)))
    p, r = ref.get_precision_recall(A[s.nodes], Agt)
    print(f"precision {p:.3f} recall {r:.3f} of {len(Agt)} true pairs, {len(s.nodes)} selected")
    assert p >= 0.9 and r >= 0.5
