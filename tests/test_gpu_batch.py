"""Batched solves (clipper_hip_batch_*, HipBatch): every problem of a batch gives, bit for bit, what a
lone HipClipper of the same storage gives with the same inputs, u0 and params whenever both took the same route;
problems the resident solver does not take, or whose batched launch gave up, are solved alone and still match."""
import dataclasses
import os
import subprocess

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = synth.EUCLID_BENCH_PARAMS
PN = dict(sigp=0.5, epsp=0.5, sign=0.10, epsn=0.35)


def _lone(storage, p, params=None, kind="euclidean", g=None):
    g = g or abi.HipClipper(params=params or abi.Params(), device=0, storage=storage)
    if kind == "euclidean":
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    else:
        g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, **PN)
    s = g.solve(p.u0)
    return g, s, g.last_solver, g.get_selected_associations()


def _assert_bits(sb, sl, what):
    assert np.array_equal(sb.u, sl.u), f"{what}: u differs"
    assert sb.nodes.tolist() == sl.nodes.tolist(), f"{what}: nodes differ"
    assert sb.score == sl.score and sb.ifinal == sl.ifinal, f"{what}: score / ifinal differ"
    assert sb.n_passes == sl.n_passes and sb.n_trials == sl.n_trials, f"{what}: passes / trials differ"


def _check_against_lone(batch, sols, probs, storage, params=None, kind="euclidean", allow_route_change=False):
    g = abi.HipClipper(params=params or abi.Params(), device=0, storage=storage)
    routes = []
    for i, (p, sb) in enumerate(zip(probs, sols)):
        _, sl, last, sel = _lone(storage, p, params, kind, g)
        r = batch.route(i)
        routes.append((r, last))
        what = f"problem {i} (m={len(p.u0)}, storage {storage}, route {r}, lone {last})"
        if r == last:
            _assert_bits(sb, sl, what)
            assert np.array_equal(batch.selected_associations(i), sel), f"{what}: selected associations differ"
        else:
            # a batched launch that gave up while the lone solve stayed resident: the routes' equivalence
            assert allow_route_change and r == 0 and last == 1, what
            assert sb.nodes.tolist() == sl.nodes.tolist() and sb.ifinal == sl.ifinal, what
            assert sb.n_trials == sl.n_trials and abs(sb.score - sl.score) <= 1e-9 * max(1.0, abs(sl.score)), what
    g.close()
    return routes


MIXED_M = [1, 2, 63, 64, 65, 300, 512, 513, 1000, 1500, 2047, 2048]


def _mixed(maker, n=30, seed0=100):
    rhos = [0.0, 0.4, 0.9]
    return [maker(MIXED_M[k % len(MIXED_M)], rhos[k % 3], seed=seed0 + k) for k in range(n)]


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_batch_bit_identity_euclidean(storage):
    probs = _mixed(synth.make_euclidean_problem)
    b = abi.HipBatch(storage=storage)
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    routes = _check_against_lone(b, sols, probs, storage)
    assert sum(r for r, _ in routes) >= 20, routes  # (the resident route is the common one here)
    assert all(r == last for r, last in routes), routes
    launches, nb, na = b.stats()
    assert launches >= 1 and nb + na == len(probs)
    b.close()


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_batch_bit_identity_pointnormal(storage):
    probs = _mixed(synth.make_pointnormal_problem, n=16, seed0=300)
    b = abi.HipBatch(storage=storage)
    sols = b.solve_pointnormal([(p.D1, p.D2, p.A, p.u0) for p in probs], **PN)
    routes = _check_against_lone(b, sols, probs, storage, kind="pointnormal")
    assert all(r == last for r, last in routes), routes
    b.close()


def test_batch_against_oracle():
    from oracle import clipper_ref as ref
    probs = [synth.make_euclidean_problem(m, rho, seed=500 + k)
             for k, (m, rho) in enumerate([(64, 0.0), (300, 0.4), (513, 0.9), (1000, 0.9), (2048, 0.4)])]
    b = abi.HipBatch()
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    for i, (p, s) in enumerate(zip(probs, sols)):
        r = ref.RefClipper()
        r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        sr = r.solve(p.u0)
        assert sorted(s.nodes.tolist()) == sorted(sr.nodes.tolist()), f"problem {i}: node set differs from the oracle"
        assert abs(s.score - sr.score) <= 1e-6 * abs(sr.score), f"problem {i}: score differs from the oracle"
    b.close()


def test_batch_not_resident_solved_alone():
    alone_seen = 0
    cases = [(abi.STORE_F32, [synth.make_euclidean_problem(m, 0.9, seed=700 + m) for m in (64, 600)]),
             (abi.STORE_F64, [synth.make_euclidean_problem(300, 0.4, seed=710)]),
             (abi.STORE_F32_CSC, [synth.make_euclidean_problem(3000, 0.9, seed=720),
                                  synth.make_euclidean_problem(256, 0.9, seed=721)]),
             (abi.STORE_F64_CSC, [synth.make_euclidean_problem(2048, 0.0, seed=730),
                                  synth.make_euclidean_problem(512, 0.4, seed=731)])]
    for storage, probs in cases:
        b = abi.HipBatch(storage=storage)
        sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
        routes = _check_against_lone(b, sols, probs, storage)
        for r, last in routes:
            assert r == last
            alone_seen += last == 0
        b.close()
    assert alone_seen >= 3, "dense storages and m = 3000 are solved alone"


def test_batch_more_units_than_one_launch():
    b = abi.HipBatch()
    probs = [synth.make_euclidean_problem(64, 0.9, seed=1000 + k) for k in range(300)]
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    launches, nb, na = b.stats()
    assert launches > 1 and nb == 300 and na == 0, (launches, nb, na)
    g = abi.HipClipper(device=0, storage=abi.STORE_F32_CSC)
    for i in range(0, 300, 7):  # (a sample: the lone solves cost more than the batch)
        _, sl, last, _ = _lone(abi.STORE_F32_CSC, probs[i], g=g)
        assert last == 1
        _assert_bits(sols[i], sl, f"problem {i}")
    g.close()
    probs = [synth.make_euclidean_problem(1024, 0.9, seed=2000 + k) for k in range(20)]
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)  # (the same batch object, reused)
    launches, nb, na = b.stats()
    assert launches > 1 and nb + na == 20, (launches, nb, na)
    _check_against_lone(b, sols, probs, abi.STORE_F32_CSC, allow_route_change=True)
    b.close()


def test_batch_forced_giveup(monkeypatch):
    probs = [synth.make_euclidean_problem(m, 0.9, seed=3000 + m) for m in (600, 1000, 1500)]
    probs.append(synth.make_euclidean_problem(100, 0.9, seed=3100))  # one unit: exchanges nothing, cannot time out
    b = abi.HipBatch()
    monkeypatch.setenv("CLIPPER_HIP_RESIDENT_TIMEOUT_TICKS", "-1")  # every wait is "late"
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    routes = _check_against_lone(b, sols, probs, abi.STORE_F32_CSC)  # the lone solves under the same knob
    assert [r for r, _ in routes] == [0, 0, 0, 1], routes
    monkeypatch.delenv("CLIPPER_HIP_RESIDENT_TIMEOUT_TICKS")
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    assert [b.route(i) for i in range(4)] == [1, 1, 1, 1]
    _check_against_lone(b, sols, probs, abi.STORE_F32_CSC)
    b.close()


def test_batch_reuse_and_edges():
    b = abi.HipBatch()
    assert b.solve_euclidean([], **INV) == []
    assert b.stats() == (0, 0, 0)
    # m = 1, and an empty A (all-to-all of 4 x 5 points), next to ordinary problems
    p1 = synth.make_euclidean_problem(1, 0.0, seed=11)
    rng = np.random.default_rng(5)
    D1, D2 = rng.random((3, 4)), rng.random((3, 5))
    pa = synth.Problem(D1=D1, D2=D2, A=np.zeros((0, 2), np.int32), Agt=None, u0=rng.random(20), meta={})
    p3 = synth.make_euclidean_problem(400, 0.4, seed=12)
    probs = [p1, pa, p3]
    for rounding in (abi.ROUNDING_NONZERO, abi.ROUNDING_DSD_HEU, abi.ROUNDING_DSD):
        prm = abi.Params(rounding=rounding)
        sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], params=prm, **INV)
        _check_against_lone(b, sols, probs, abi.STORE_F32_CSC, params=prm)
    # an invalid problem fails the whole call, names its index, and the batch goes on working
    bad = synth.make_euclidean_problem(100, 0.4, seed=13)
    Abad = bad.A.copy()
    Abad[7, 1] = 10 ** 6
    with pytest.raises(abi.ClipperError, match="problem 1"):
        b.solve_euclidean([(p3.D1, p3.D2, p3.A, p3.u0), (bad.D1, bad.D2, Abad, bad.u0)], **INV)
    assert b.L.clipper_hip_batch_solve_euclidean(b.b, None, 1, 3, 0.01, 0.06, 0.0, abi.C.byref(abi.Params())) == -1
    with pytest.raises(abi.ClipperError):  # a missing u0
        b.solve_euclidean([(p3.D1, p3.D2, p3.A)], **INV)
    probs2 = [synth.make_euclidean_problem(m, 0.9, seed=14 + m) for m in (90, 700)]
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs2], **INV)
    _check_against_lone(b, sols, probs2, abi.STORE_F32_CSC)
    b.close()


def _check_against_fresh_lone(batch, sols, probs, storage):
    """every problem against a lone context of its own: every route must agree, and every bit"""
    for i, (p, sb) in enumerate(zip(probs, sols)):
        g, sl, last, sel = _lone(storage, p)
        what = f"problem {i} (m={len(p.u0)}, d={p.D1.shape[0]}, storage {storage}, route {batch.route(i)}, lone {last})"
        assert batch.route(i) == last, what
        _assert_bits(sb, sl, what)
        assert np.array_equal(batch.selected_associations(i), sel), f"{what}: selected associations differ"
        g.close()


def _sized(sizes, seed0):
    # m = 130: two 128-row chunks, three 64-column groups; m = 700 next to it
    return [synth.make_euclidean_problem(m, 0.9, seed=seed0 + k) for k, m in enumerate(sizes)]


def test_batch_fill_that_cannot_be_queued_d4():
    # d = 4 on slices: the fill cannot emit (dense store -> groups -> slices), so it runs to its end inside the
    # child's turn and the batch has nothing left to complete for it. A fourth coordinate of zeros: the 3-D distances.
    probs = [dataclasses.replace(p, D1=np.vstack([p.D1, np.zeros((1, p.D1.shape[1]))]),
                                 D2=np.vstack([p.D2, np.zeros((1, p.D2.shape[1]))])) for p in _sized((130, 700), 5000)]
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    _check_against_fresh_lone(b, sols, probs, abi.STORE_F32_CSC)
    b.close()


def test_batch_fill_that_cannot_be_queued_rect():
    # d = 3 with fp64 values in the slices: the rectangular fill, which runs to its end inside the child's turn too
    probs = _sized((130, 700), 5100)
    b = abi.HipBatch(storage=abi.STORE_F64_CSC)
    sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    _check_against_fresh_lone(b, sols, probs, abi.STORE_F64_CSC)
    b.close()


def test_batch_three_calls_grow_then_reuse():
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    # fresh children: every arena overflows once; the same sizes again: nothing does; the sizes swapped: each child
    # meets the other size, one grows and one reuses
    for call, sizes in enumerate([(130, 700), (130, 700), (700, 130)]):
        probs = _sized(sizes, 5200 + 10 * call)
        sols = b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
        _check_against_fresh_lone(b, sols, probs, abi.STORE_F32_CSC)
    b.close()


def test_clipperpy_batch_matches_lone():
    import clipper_amd
    clipperpy = clipper_amd.load_clipperpy()
    probs = [synth.make_euclidean_problem(m, 0.9, seed=4000 + m) for m in (64, 500, 1200)]
    iparams = clipperpy.invariants.EuclideanDistanceParams()
    iparams.sigma, iparams.epsilon, iparams.mindist = INV["sigma"], INV["epsilon"], INV["mindist"]
    inv = clipperpy.invariants.EuclideanDistance(iparams)
    params = clipperpy.Params()
    cb = clipperpy.CLIPPERBatch(inv, params)
    sols = cb.solve([(p.D1, p.D2, p.A.astype(np.int32), p.u0) for p in probs])
    for i, p in enumerate(probs):
        c = clipperpy.CLIPPER(inv, params)
        c.score_pairwise_consistency(p.D1, p.D2, p.A.astype(np.int32))
        c.solve(p.u0)
        sl = c.get_solution()
        assert list(sols[i].nodes) == list(sl.nodes) and sols[i].score == sl.score and sols[i].ifinal == sl.ifinal
        assert np.array_equal(np.asarray(sols[i].u), np.asarray(sl.u))
        assert np.array_equal(np.asarray(cb.get_selected_associations(i)), np.asarray(c.get_selected_associations()))


def test_batch_facade_cpp(tmp_path):
    exe = str(tmp_path / "test_batch_facade")
    lib = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_batch_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "batch.cpp"),
        "-L", lib, "-lclipper_hip", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "batch facade ok" in out.stdout
