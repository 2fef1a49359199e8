"""Batched solves scored by a user-defined invariant (clipper_hip_batch_solve_custom, HipBatch.solve_custom,
CLIPPERBatch::withDeviceInvariant): one launch of the invariant's batched fill kernel scores every
problem, and every problem then gives, bit for bit, what a lone HipClipper of the same storage gives with
affinity_custom + solve on the same inputs, u0 and params, whenever both took the same route."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import synth
from tests.test_gpu_batch import MIXED_M, _assert_bits
from tests.test_gpu_device_invariant import EUCLID_SRC, EXP_SRC, POINTNORMAL_SRC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGES = [abi.STORE_F32, abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC]
INV = synth.EUCLID_BENCH_PARAMS
EPRM = [INV["sigma"], INV["epsilon"], INV["mindist"]]
PN = dict(sigp=0.5, epsp=0.5, sign=0.10, epsn=0.35)
PPRM = [PN["sigp"], PN["epsp"], PN["sign"], PN["epsn"]]


@pytest.fixture(scope="module")
def euclid_inv():
    with abi.HipInvariant(EUCLID_SRC, 3) as inv:
        yield inv


def _tuples(probs):
    return [(p.D1, p.D2, p.A, p.u0) for p in probs]


def _check_against_lone(batch, sols, probs, storage, inv, iprm, params=None, allow_route_change=False):
    """every problem against a lone affinity_custom + solve (one lone context, reused, as tests/test_gpu_batch.py)"""
    g = abi.HipClipper(params=params or abi.Params(), device=0, storage=storage)
    routes = []
    for i, (p, sb) in enumerate(zip(probs, sols)):
        g.affinity_custom(inv, p.D1, p.D2, p.A, iprm)
        sl = g.solve(p.u0)
        last, sel = g.last_solver, g.get_selected_associations()
        r = batch.route(i)
        routes.append((r, last))
        what = f"problem {i} (m={len(p.u0)}, storage {storage}, route {r}, lone {last})"
        if r == last:
            _assert_bits(sb, sl, what)
            assert np.array_equal(batch.selected_associations(i), sel), f"{what}: selected associations differ"
        else:  # a batched launch that gave up while the lone solve stayed resident: the routes' equivalence
            assert allow_route_change and r == 0 and last == 1, what
            assert sb.nodes.tolist() == sl.nodes.tolist() and sb.ifinal == sl.ifinal, what
            assert sb.n_trials == sl.n_trials and abs(sb.score - sl.score) <= 1e-9 * max(1.0, abs(sl.score)), what
    g.close()
    return routes


def _mixed(maker, n=30, seed0=100, big=True):
    rhos = [0.0, 0.4, 0.9]
    probs = [maker(MIXED_M[k % len(MIXED_M)], rhos[k % 3], seed=seed0 + k) for k in range(n)]
    if big:
        probs.append(maker(3000, 0.9, seed=seed0 + n))  # no resident plan: solved alone
    return probs


@pytest.mark.parametrize("storage", STORAGES)
def test_euclidean_restated_against_lone_custom(euclid_inv, storage):
    probs = _mixed(synth.make_euclidean_problem)
    b = abi.HipBatch(storage=storage)
    sols = b.solve_custom(euclid_inv, _tuples(probs), EPRM)
    routes = _check_against_lone(b, sols, probs, storage, euclid_inv, EPRM)
    assert all(r == last for r, last in routes), routes
    if storage in (abi.STORE_F32_CSC, abi.STORE_F64_CSC):
        assert sum(r for r, _ in routes) >= 20, routes
        assert routes[-1] == (0, 0)  # m = 3000
    else:
        assert all(r == 0 for r, _ in routes)  # dense storages: solved alone
    launches, nb, na = b.stats()
    assert nb + na == len(probs)
    assert b.split()["fill_ms"] > 0
    b.close()


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_against_the_builtin_batch(euclid_inv, storage):
    probs = _mixed(synth.make_euclidean_problem, seed0=900, big=False)
    bc, bb = abi.HipBatch(storage=storage), abi.HipBatch(storage=storage)
    sc = bc.solve_custom(euclid_inv, _tuples(probs), EPRM)
    sb = bb.solve_euclidean(_tuples(probs), **INV)
    agree = 0
    for i, p in enumerate(probs):
        if bc.route(i) == bb.route(i):
            _assert_bits(sc[i], sb[i], f"problem {i} (m={len(p.u0)})")
            assert np.array_equal(bc.selected_associations(i), bb.selected_associations(i))
            agree += 1
    assert agree >= len(probs) - 2
    bc.close(), bb.close()


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64])
def test_pointnormal_restated(storage):
    probs = _mixed(synth.make_pointnormal_problem, n=16, seed0=300, big=False)
    with abi.HipInvariant(POINTNORMAL_SRC, 6) as inv:
        b = abi.HipBatch(storage=storage)
        sols = b.solve_custom(inv, _tuples(probs), PPRM)
        routes = _check_against_lone(b, sols, probs, storage, inv, PPRM)
        assert all(r == last for r, last in routes), routes
        b.close()


def test_dense_storage_has_no_build_rounds(euclid_inv, capfd, monkeypatch):
    # dense fp32 storage: no compressed child, so the build rounds run over an empty list — the batch still waits for
    # the fill before it reads the fill's events. One problem, m = 130 (more than one 128-row chunk).
    monkeypatch.setenv("CLIPPER_HIP_HOST_TIMING", "1")
    p = synth.make_euclidean_problem(130, 0.9, seed=1300)
    b = abi.HipBatch(storage=abi.STORE_F32)
    sols = b.solve_custom(euclid_inv, _tuples([p]), EPRM)
    err = capfd.readouterr().err
    routes = _check_against_lone(b, sols, [p], abi.STORE_F32, euclid_inv, EPRM)
    assert routes == [(0, 0)]
    # the children's affinity_kernel_ms: the event time of one small launch, not a pair read before it was through
    mt = re.search(r"\[batch-custom\] n = 1:.* (\d+) tiles ([0-9.]+) ms \(events\)", err)
    assert mt and int(mt.group(1)) >= 1 and 0.0 < float(mt.group(2)) < 1000.0, err
    assert b.split()["fill_ms"] > 0
    b.close()


@pytest.mark.parametrize("nan", [False, True])
def test_formula_with_exp_and_nan(nan):
    d = 3
    prm = [0.05 * d, 0.02, 0.3 if nan else 0.0]
    probs = [synth.make_euclidean_problem(m, 0.4, seed=1200 + m) for m in (50, 300, 700, 1500)]
    with abi.HipInvariant(EXP_SRC, d) as inv:
        for storage in (abi.STORE_F32_CSC, abi.STORE_F64_CSC, abi.STORE_F32):
            b = abi.HipBatch(storage=storage)
            sols = b.solve_custom(inv, _tuples(probs), prm)
            routes = _check_against_lone(b, sols, probs, storage, inv, prm)
            assert all(r == last for r, last in routes), routes
            b.close()


def test_against_oracle(euclid_inv):
    from oracle import clipper_ref as ref
    probs = [synth.make_euclidean_problem(m, rho, seed=500 + k)
             for k, (m, rho) in enumerate([(64, 0.0), (300, 0.4), (513, 0.9), (1000, 0.9), (2048, 0.4)])]
    b = abi.HipBatch()
    sols = b.solve_custom(euclid_inv, _tuples(probs), EPRM)
    for i, (p, s) in enumerate(zip(probs, sols)):
        r = ref.RefClipper()
        r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        sr = r.solve(p.u0)
        assert sorted(s.nodes.tolist()) == sorted(sr.nodes.tolist()), f"problem {i}: node set differs from the oracle"
        assert abs(s.score - sr.score) <= 1e-6 * abs(sr.score), f"problem {i}: score differs from the oracle"
    b.close()


def test_reuse_and_edges(euclid_inv, capfd, monkeypatch):
    monkeypatch.setenv("CLIPPER_HIP_HOST_TIMING", "1")
    b = abi.HipBatch()
    assert b.solve_custom(euclid_inv, [], EPRM) == []
    assert b.stats() == (0, 0, 0)
    probs = [synth.make_euclidean_problem(m, 0.9, seed=1400 + m) for m in (100, 600, 1500)]
    s1 = b.solve_custom(euclid_inv, _tuples(probs), EPRM)
    capfd.readouterr()
    # the same shapes again: the same bits, and one round of builds (no slice arena grown)
    s2 = b.solve_custom(euclid_inv, _tuples(probs), EPRM)
    err = capfd.readouterr().err
    assert "[batch-custom] n = 3:" in err and "1 build round" in err, err
    for i in range(len(probs)):
        _assert_bits(s2[i], s1[i], f"problem {i}, second call")
    # larger shapes after smaller ones
    big = [synth.make_euclidean_problem(m, 0.4, seed=1500 + m) for m in (2048, 2000, 64, 1800)]
    sols = b.solve_custom(euclid_inv, _tuples(big), EPRM)
    _check_against_lone(b, sols, big, abi.STORE_F32_CSC, euclid_inv, EPRM)
    # an invalid problem fails the call (rows != the invariant's d; invalid point data at the C ABI), the batch goes on
    with pytest.raises(ValueError, match="problem 1"):
        b.solve_custom(euclid_inv, [_tuples(probs)[0], (probs[1].D1[:2], probs[1].D2[:2], probs[1].A, probs[1].u0)],
                       EPRM)
    bad = abi.BatchProblem(abi._dp(probs[0].D1), 0, abi._dp(probs[0].D2), 0, None, 0, abi._dp(probs[0].u0))
    arr = (abi.BatchProblem * 1)(bad)
    assert b.L.clipper_hip_batch_solve_custom(b.b, euclid_inv.h, arr, 1, None, 0, abi.C.byref(abi.Params())) == -1
    assert "problem 0" in abi._last_error()
    sols = b.solve_custom(euclid_inv, _tuples(probs), EPRM)
    _check_against_lone(b, sols, probs, abi.STORE_F32_CSC, euclid_inv, EPRM)
    b.close()


def test_forced_giveup(euclid_inv, monkeypatch):
    probs = [synth.make_euclidean_problem(m, 0.9, seed=3000 + m) for m in (600, 1000, 1500)]
    probs.append(synth.make_euclidean_problem(100, 0.9, seed=3100))  # one unit: exchanges nothing, cannot time out
    b = abi.HipBatch()
    monkeypatch.setenv("CLIPPER_HIP_RESIDENT_TIMEOUT_TICKS", "-1")  # every wait is "late"
    sols = b.solve_custom(euclid_inv, _tuples(probs), EPRM)
    routes = _check_against_lone(b, sols, probs, abi.STORE_F32_CSC, euclid_inv, EPRM)  # the same knob
    assert [r for r, _ in routes] == [0, 0, 0, 1], routes
    monkeypatch.delenv("CLIPPER_HIP_RESIDENT_TIMEOUT_TICKS")
    sols = b.solve_custom(euclid_inv, _tuples(probs), EPRM)
    assert [b.route(i) for i in range(4)] == [1, 1, 1, 1]
    _check_against_lone(b, sols, probs, abi.STORE_F32_CSC, euclid_inv, EPRM)
    b.close()


def test_clipperpy_with_device_invariant_matches_lone():
    cp = clipper_amd.load_clipperpy()
    probs = [synth.make_euclidean_problem(m, 0.9, seed=4000 + m) for m in (64, 500, 1200)]
    inv = cp.invariants.DeviceInvariant(EUCLID_SRC, EPRM)
    params = cp.Params()
    cb = cp.CLIPPERBatch.with_device_invariant(inv, params)
    del inv  # the batch keeps it alive
    sols = cb.solve([(p.D1, p.D2, p.A.astype(np.int32), p.u0) for p in probs])
    inv = cp.invariants.DeviceInvariant(EUCLID_SRC, EPRM)
    for i, p in enumerate(probs):
        c = cp.CLIPPER(inv, params)
        c.score_pairwise_consistency(p.D1, p.D2, p.A.astype(np.int32))
        c.solve(p.u0)
        sl = c.get_solution()
        assert cb.solved_batched(i) == c.last_solve_was_resident()
        assert list(sols[i].nodes) == list(sl.nodes) and sols[i].score == sl.score and sols[i].ifinal == sl.ifinal
        assert np.array_equal(np.asarray(sols[i].u), np.asarray(sl.u))
        assert np.array_equal(np.asarray(cb.get_selected_associations(i)), np.asarray(c.get_selected_associations()))
    with pytest.raises(ValueError):
        cp.CLIPPERBatch(inv, params)  # the constructor still takes the built-ins only


def test_cpp_facade(tmp_path):
    exe = str(tmp_path / "test_batch_custom_facade")
    lib = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-std=c++17", "-O1", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_batch_custom_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "batch.cpp"),
        "-L", lib, "-lclipper_hip", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "batch custom facade ok" in out.stdout
