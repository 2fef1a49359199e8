"""GPU tests of the batched maximum-clique call (clipper_hip_batch_max_clique, HipBatch.max_clique; DESIGN.md section
9, "Batches"): per problem the batched call returns the node list, max_core, heuristic_size, edges and num_nodes of
HipClipper.max_clique on a lone context scored from the same inputs on the same storage — whatever else the batch
holds, wherever the problem stands in it and however the launches were cut — and the sequential model of
tests/maxclique_model.py says what that list must be, so that both cannot be wrong in the same way.

The batch's solve accepts m = 1, so the edgeless row of the table stays."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import synth
from tests import maxclique_model as mm
from tests.test_gpu_device_invariant import EUCLID_SRC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGES = (abi.STORE_F32_CSC, abi.STORE_F64_CSC, abi.STORE_F32, abi.STORE_F64)
METHODS = (abi.MC_EXACT, abi.MC_HEU, abi.MC_KCORE)
INV = synth.EUCLID_BENCH_PARAMS
EPRM = [INV["sigma"], INV["epsilon"], INV["mindist"]]
EQUAL_FIELDS = ("num_nodes", "max_core", "heuristic_size", "edges")

# (m, rho, seed): K, HEU, omega and what the row covers are tabulated in DESIGN.md 9 "Batches"
ROWS = [(1, 0.0, 13), (2, 0.0, 14), (40, 0.5, 1), (64, 0.7, 2), (65, 0.9, 3), (96, 0.95, 103), (128, 0.9, 4),
        (129, 0.8, 5), (200, 0.95, 6), (700, 0.95, 9), (1000, 0.95, 11), (300, 0.9, 7), (513, 0.9, 8), (1000, 0.9, 10),
        (2048, 0.95, 12), (2100, 0.95, 15)]
SMALL = [r for r in ROWS if r[0] <= 513]

# The throughput test's bound: four times the ratio (one batched EXACT call) / (the loop of 64 lone calls) measured on
# an MI355X by tools/batch_maxclique_probe.py when the batched call was added (the loop 125.5 ms, the batched call
# 7.07 ms), capped at 1. Since the lone call runs through the batch's driver the loop takes 100.2 ms and the ratio is
# 0.0698 ("ratio" in profiles/batch_maxclique_probe.json); the bound stays.
MEASURED_RATIO = 0.0564
RATIO_BOUND = min(1.0, 4 * MEASURED_RATIO)

# The time-limit test: the unlimited batched EXACT call on its 8 problems, measured by tools/batch_maxclique_probe.py
# (profiles/batch_maxclique_probe.json "time_limit_batch"), in seconds: 187 times the limit of the test, so epsilon stays as the issue gives it and a time-out is asserted.
TL_EPSILON = 0.15
TL_UNLIMITED_S = 9.35
TL_LIMIT_S = 0.05

_problems, _lone, _model = {}, {}, {}


def _problem(row):
    if row not in _problems:
        _problems[row] = synth.make_euclidean_problem(row[0], row[1], seed=row[2])
    return _problems[row]


def _tuples(rows):
    return [(p.D1, p.D2, p.A, p.u0) for p in map(_problem, rows)]


def _lone_context(row, storage):
    p = _problem(row)
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    return g


def _fields(info):
    return tuple(getattr(info, f) for f in EQUAL_FIELDS)


def lone(row, storage, method):
    """(nodes, the equal fields, timed_out, selected associations) of HipClipper.max_clique; computed once"""
    key = (row, storage)
    if key not in _lone:
        g = _lone_context(row, storage)
        out = {}
        for meth in METHODS:
            nodes, info = g.max_clique(meth)
            out[meth] = (nodes.tolist(), _fields(info), info.timed_out, g.get_selected_associations())
        if storage == abi.STORE_F32_CSC and row not in _model:
            _model[row] = mm.adjacency_from_matrix(g.get_constraint_matrix())
        g.close()
        _lone[key] = out
    return _lone[key][method]


def model(row):
    """(adjacency, KCORE's list, HEU's list, omega) of the sequential model; computed once"""
    if row not in _model or not isinstance(_model[row], tuple):
        lone(row, abi.STORE_F32_CSC, abi.MC_EXACT)
        adj = _model[row]
        if adj.sum() == 0:
            _model[row] = (adj, list(range(adj.shape[0])), [], 0)
        else:
            core = mm.core_numbers(adj)
            heu = mm.heu(adj, core)
            _model[row] = (adj, mm.kcore(adj, core), heu, mm.omega(adj, lower=len(heu)))
    return _model[row]


def model_of(g, key, cache):
    """the model's tuple for the graph of a lone context (for the problems that are no row of the table); once per key"""
    if key not in cache:
        adj = mm.adjacency_from_matrix(g.get_constraint_matrix())
        core = mm.core_numbers(adj)
        heu = mm.heu(adj, core)
        cache[key] = (adj, mm.kcore(adj, core), heu, mm.omega(adj, lower=len(heu)))
    return cache[key]


def assert_model(row, meth, nodes, info, mdl=None):
    """the model's list (KCORE, HEU) or size (EXACT: omega, and a clique), its edges and HEU's size"""
    adj, kc, heu, omega = mdl or model(row)
    what = f"row {row}, method {meth}"
    assert info.edges == int(adj.sum()) // 2, what
    if meth == abi.MC_KCORE:
        assert list(nodes) == kc, what
    elif meth == abi.MC_HEU:
        assert list(nodes) == heu and info.heuristic_size == len(heu), what
    else:
        assert len(nodes) == omega and mm.is_clique(adj, nodes), (what, len(nodes), omega)
        assert info.heuristic_size == len(heu), what


def _batch(rows, storage=abi.STORE_F32_CSC):
    b = abi.HipBatch(storage=storage)
    b.solve_euclidean(_tuples(rows), **INV)
    return b


# ---- 1. equal to the lone call and to the model -------------------------------------------------------------------

def test_equal_to_the_lone_call_and_to_the_model():
    b = _batch(ROWS)
    for meth in METHODS:
        res = b.max_clique(meth)
        assert len(res) == len(ROWS)
        launches, nb, na = b.max_clique_stats()
        assert (nb, na) == (15, 1) and launches >= 3, (launches, nb, na)
        for i, (row, (nodes, info)) in enumerate(zip(ROWS, res)):
            what = f"row {row}, method {meth}"
            ln, lf, lto, lsel = lone(row, abi.STORE_F32_CSC, meth)
            assert nodes.tolist() == ln, what
            assert _fields(info) == lf, (what, _fields(info), lf)
            assert info.timed_out == 0 and lto == 0 and info.seconds > 0, what
            assert_model(row, meth, nodes.tolist(), info)
            assert b.get_nodes(i).tolist() == nodes.tolist(), what
            sel = b.selected_associations(i)
            assert np.array_equal(sel, np.asarray(_problem(row).A)[nodes].reshape(-1, 2)), what
            assert np.array_equal(sel, lsel.reshape(-1, 2)), what
    # the table's figures for the rows a glance can check
    assert model((1, 0.0, 13))[3] == 0 and model((2, 0.0, 14))[3] == 2
    assert len(model((65, 0.9, 3))[2]) == 5 and model((65, 0.9, 3))[3] == 6  # EXACT finds a larger clique
    assert len(model((2048, 0.95, 12))[2]) == 10 and model((2048, 0.95, 12))[3] == 101
    b.close()


# ---- 2. storages ------------------------------------------------------------------------------------------------------

def test_storages_give_identical_lists():
    lists = {}
    for storage in STORAGES:
        b = _batch(SMALL, storage)
        for meth in METHODS:
            res = b.max_clique(meth)
            lists[(storage, meth)] = [(n.tolist(), _fields(i)) for n, i in res]
            for row, (n, i) in zip(SMALL, res):
                assert_model(row, meth, n.tolist(), i)
        assert b.max_clique_stats()[1:] == (len(SMALL), 0)
        b.close()
    for meth in METHODS:
        first = lists[(STORAGES[0], meth)]
        for k, row in enumerate(SMALL):
            assert first[k] == (lone(row, abi.STORE_F32_CSC, meth)[0], lone(row, abi.STORE_F32_CSC, meth)[1]), (row, meth)
        for storage in STORAGES[1:]:
            assert lists[(storage, meth)] == first, (storage, meth)
    # and a lone context of each storage agrees on a row with a real search
    row = (200, 0.95, 6)
    for storage in STORAGES[1:]:
        assert lone(row, storage, abi.MC_EXACT)[:2] == lone(row, STORAGES[0], abi.MC_EXACT)[:2], storage
    assert len(lone(row, STORAGES[0], abi.MC_EXACT)[0]) == model(row)[3]


def test_both_storage_kinds_in_one_driver():
    """(65, 0.9, 3), whose omega = K + 1 fills a stack to its last level, and (129, 0.8, 5), two words per row and one
    bit, on a slice storage and on a dense one of the other value type."""
    rows = [(65, 0.9, 3), (129, 0.8, 5)]
    lists = {}
    for storage in (abi.STORE_F32_CSC, abi.STORE_F64):
        b = _batch(rows, storage)
        for meth in METHODS:
            res = b.max_clique(meth)
            for row, (n, i) in zip(rows, res):
                assert_model(row, meth, n.tolist(), i)
            lists[(storage, meth)] = [(n.tolist(), _fields(i)) for n, i in res]
        b.close()
    for meth in METHODS:
        assert lists[(abi.STORE_F32_CSC, meth)] == lists[(abi.STORE_F64, meth)], meth


def test_largest_and_smallest_problem_in_one_adjacency_launch():
    """m = 1, 2048 and 2 side by side: most workgroups of the adjacency and degree launches lie past the rows and
    slices of their problem."""
    rows = [(1, 0.0, 13), (2048, 0.95, 12), (2, 0.0, 14)]
    for storage in (abi.STORE_F32_CSC, abi.STORE_F32):
        b = _batch(rows, storage)
        for meth in (abi.MC_KCORE, abi.MC_HEU):
            res = b.max_clique(meth)
            assert b.max_clique_stats()[1:] == (3, 0)
            for row, (n, i) in zip(rows, res):
                assert_model(row, meth, n.tolist(), i)
        b.close()


# ---- 3. composition ---------------------------------------------------------------------------------------------------

def test_composition_order_and_repetition():
    for meth in (abi.MC_EXACT, abi.MC_HEU):
        b = _batch(ROWS)
        a = [(n.tolist(), _fields(i)) for n, i in b.max_clique(meth)]
        res = b.max_clique(meth)
        again = [(n.tolist(), _fields(i)) for n, i in res]
        assert again == a, meth
        for row, (n, i) in zip(ROWS, res):
            assert_model(row, meth, n.tolist(), i)
        b.close()
        r = _batch(ROWS[::-1])
        rev = [(n.tolist(), _fields(i)) for n, i in r.max_clique(meth)][::-1]
        assert rev == a, meth
        r.close()
        one = abi.HipBatch(storage=abi.STORE_F32_CSC)
        for k, row in enumerate(ROWS):
            one.solve_euclidean(_tuples([row]), **INV)
            (n, i), = one.max_clique(meth)
            assert (n.tolist(), _fields(i)) == a[k], (row, meth)
            assert one.max_clique_stats()[1:] == ((1, 0) if row[0] <= 2048 else (0, 1)), row
        one.close()


# ---- 4. other invariants ----------------------------------------------------------------------------------------------

def test_pointnormal_and_custom_invariants():
    probs = [synth.make_pointnormal_problem(m, 0.9, seed=7) for m in (100, 300)]
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_pointnormal([(p.D1, p.D2, p.A, p.u0) for p in probs])
    models = {}
    for meth in METHODS:
        res = b.max_clique(meth)
        for p, (nodes, info) in zip(probs, res):
            g = abi.HipClipper(storage=abi.STORE_F32_CSC)
            g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A)
            ln, li = g.max_clique(meth)
            assert nodes.tolist() == ln.tolist() and _fields(info) == _fields(li), (len(p.u0), meth)
            assert_model(len(p.u0), meth, nodes.tolist(), info, model_of(g, len(p.u0), models))
            g.close()
    b.close()
    rows = [(65, 0.9, 3), (200, 0.95, 6), (300, 0.9, 7)]
    with abi.HipInvariant(EUCLID_SRC, 3) as inv:
        b = abi.HipBatch(storage=abi.STORE_F32_CSC)
        b.solve_custom(inv, _tuples(rows), EPRM)
        for meth in METHODS:
            res = b.max_clique(meth)
            for row, (nodes, info) in zip(rows, res):
                p = _problem(row)
                g = abi.HipClipper(storage=abi.STORE_F32_CSC)
                g.affinity_custom(inv, p.D1, p.D2, p.A, EPRM)
                ln, li = g.max_clique(meth)
                assert nodes.tolist() == ln.tolist() and _fields(info) == _fields(li), (row, meth)
                assert_model(row, meth, nodes.tolist(), info, model_of(g, row, models))
                g.close()
                if meth == abi.MC_EXACT:
                    assert len(nodes) == model(row)[3], row
        b.close()


# ---- 5. no side effects ----------------------------------------------------------------------------------------------

def test_no_side_effects_on_solve_and_sdp():
    rows = [r for r in ROWS if r[0] <= 1000]
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    first = b.solve_euclidean(_tuples(rows), **INV)
    for meth in METHODS:
        b.max_clique(meth)
    second = b.solve_euclidean(_tuples(rows), **INV)
    for row, s0, s1 in zip(rows, first, second):
        assert np.array_equal(s0.u, s1.u) and s0.nodes.tolist() == s1.nodes.tolist(), row
    b.close()
    rows = [r for r in ROWS if r[0] <= 128]
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_euclidean(_tuples(rows), **INV)
    prm = dict(eps_abs=1e-4, eps_rel=1e-4, max_iters=2000)
    before = b.sdp(abi.SdpParams(**prm))
    cl = b.max_clique(abi.MC_EXACT)
    for k, (nodes, _) in enumerate(cl):
        assert b.get_nodes(k).tolist() == nodes.tolist()
    after = b.sdp(abi.SdpParams(**prm))
    for row, r0, r1 in zip(rows, before, after):
        assert np.array_equal(r0.X, r1.X) and np.array_equal(r0.evec1, r1.evec1), row
        assert r0.nodes.tolist() == r1.nodes.tolist() and r0.iters == r1.iters and r0.pobj == r1.pobj, row
    for k, r1 in enumerate(after):
        assert b.get_nodes(k).tolist() == r1.nodes.tolist()
    b.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------

def test_refusals():
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    with pytest.raises(abi.ClipperError, match=r"error -5"):
        b.max_clique()
    assert b.max_clique_stats() == (0, 0, 0)
    b.solve_euclidean([], **INV)
    assert b.max_clique() == []  # an empty batch
    rows = [(40, 0.5, 1), (65, 0.9, 3)]
    sols = b.solve_euclidean(_tuples(rows), **INV)
    with pytest.raises(abi.ClipperError, match=r"error -1: .*method 7"):
        b.max_clique(7)
    # still usable, and the solve's lists are still there
    for k, s in enumerate(sols):
        assert b.get_nodes(k).tolist() == s.nodes.tolist()
    assert b.L.clipper_hip_batch_max_clique(b.b, abi.MC_EXACT, 0.0, None) == 0  # infos = NULL
    for k, row in enumerate(rows):
        assert b.get_nodes(k).tolist() == lone(row, abi.STORE_F32_CSC, abi.MC_EXACT)[0]
        assert len(b.get_nodes(k)) == model(row)[3] and mm.is_clique(model(row)[0], b.get_nodes(k)), row
    b.close()


# ---- 7. the time limit ---------------------------------------------------------------------------------------------------

def test_time_limit():
    """8 problems of m = 2048 at density ~ 0.32 (K = 518, HEU 32, omega = 58 for seed 77). The unlimited batched call
    on them takes TL_UNLIMITED_S (profiles/batch_maxclique_probe.json); only when that is at least four times the limit
    is a time-out asserted."""
    probs = [synth.make_euclidean_problem(2048, 0.98, seed=s) for s in range(77, 85)]
    inv = dict(sigma=0.1, epsilon=TL_EPSILON, mindist=0.0)
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **inv)
    t0 = time.time()
    res = b.max_clique(abi.MC_EXACT, time_limit=TL_LIMIT_S)
    wall = time.time() - t0
    print(f"time limit {TL_LIMIT_S} s on 8 problems of m = 2048: {wall:.3f} s, timed out "
          f"{[i.timed_out for _, i in res]}, sizes {[len(n) for n, _ in res]}, heuristic {[i.heuristic_size for _, i in res]}")
    assert wall < 5.0, wall
    for p, (nodes, info) in zip(probs, res):
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **inv)
        adj = mm.adjacency_from_matrix(g.get_constraint_matrix())
        assert mm.is_clique(adj, nodes) and len(nodes) >= info.heuristic_size
        assert info.edges == int(adj.sum()) // 2 and info.max_core == int(mm.core_numbers_levels(adj).max())
        if info.timed_out == 0:
            ln, li = g.max_clique(abi.MC_EXACT)
            assert nodes.tolist() == ln.tolist() and _fields(info) == _fields(li)
        g.close()
    assert TL_UNLIMITED_S >= 4 * TL_LIMIT_S  # (else epsilon has to be widened: see the issue's rule in the docstring)
    assert any(i.timed_out == 1 for _, i in res)
    b.close()


# ---- 8. throughput --------------------------------------------------------------------------------------------------------

def test_batched_call_beats_the_loop_of_lone_calls():
    """64 problems, m cycling through 200 / 500 / 1000 at 95 % outliers: one batched EXACT call against the loop of 64
    lone max_clique calls on contexts scored beforehand, both the best of three in this process. The batched call must
    be faster; asserted is four times the ratio measured on an MI355X (MEASURED_RATIO), capped at 1."""
    ms = [200, 500, 1000]
    probs = [synth.make_euclidean_problem(ms[k % 3], 0.95, seed=5000 + k) for k in range(64)]
    ctxs = []
    for p in probs:
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        ctxs.append(g)
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)

    def loop():
        return [g.max_clique(abi.MC_EXACT) for g in ctxs]

    def batch():
        return b.max_clique(abi.MC_EXACT)

    def best(f):
        f()  # warm-up
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = f()
            ts.append(time.perf_counter() - t0)
        return min(ts), r

    ta, ra = best(loop)
    tb, rb = best(batch)
    print(f"64 problems of m = 200 / 500 / 1000: loop of lone calls {ta * 1e3:.1f} ms, one batched call {tb * 1e3:.1f} ms, "
          f"ratio {tb / ta:.4f}, launches {b.max_clique_stats()[0]}")
    for k in range(len(probs)):
        assert rb[k][0].tolist() == ra[k][0].tolist() and _fields(rb[k][1]) == _fields(ra[k][1]), k
    for k in range(len(probs)):  # (edges, K and a clique no smaller than the model's HEU for all; m = 200: the whole model)
        adj = mm.adjacency_from_matrix(ctxs[k].get_constraint_matrix())
        core = mm.core_numbers(adj)
        nodes, info = rb[k]
        assert info.edges == int(adj.sum()) // 2 and info.max_core == int(core.max()), k
        assert info.heuristic_size == len(mm.heu(adj, core)) <= len(nodes) and mm.is_clique(adj, nodes), k
    for k in range(0, len(probs), 3):
        assert_model(k, abi.MC_EXACT, rb[k][0].tolist(), rb[k][1], model_of(ctxs[k], k, {}))
    for g in ctxs:
        g.close()
    b.close()
    assert tb / ta < RATIO_BOUND, (ta, tb, RATIO_BOUND)


# ---- 9. facades -------------------------------------------------------------------------------------------------------------

def test_clipperpy_solve_as_maximum_clique(golden):
    cp = clipper_amd.load_clipperpy()
    g = golden["affinity_test"]
    ip = cp.invariants.EuclideanDistanceParams()
    cb = cp.CLIPPERBatch(cp.invariants.EuclideanDistance(ip), cp.Params())
    with pytest.raises(Exception):
        cb.solve_as_maximum_clique(cp.MCParams())  # before any solve
    rows = [(65, 0.9, 3), (200, 0.95, 6)]
    A0 = np.asarray(cp.utils.create_all_to_all(4, 3)).astype(np.int32)
    probs = [(np.array(g["model"]), np.array(g["data"]), A0, np.full(12, 0.5))]
    # (the default invariant parameters score the golden problem; the table's rows under them are compared with HipBatch)
    probs += [(p.D1, p.D2, np.asarray(p.A).astype(np.int32), p.u0) for p in map(_problem, rows)]
    first = cb.solve(probs)
    hb = abi.HipBatch(storage=abi.STORE_F32_CSC)
    hb.solve_euclidean([(q[0], q[1], q[2], q[3]) for q in probs], sigma=ip.sigma, epsilon=ip.epsilon, mindist=ip.mindist)
    for meth, ameth in ((cp.MCMethod.EXACT, abi.MC_EXACT), (cp.MCMethod.HEU, abi.MC_HEU), (cp.MCMethod.KCORE, abi.MC_KCORE)):
        prm = cp.MCParams()
        prm.method = meth
        out = cb.solve_as_maximum_clique(prm)
        ref = hb.max_clique(ameth)
        assert len(out) == 3
        assert sorted(out[0].nodes) == [0, 4, 8]
        for i, (o, (nodes, _)) in enumerate(zip(out, ref)):
            assert list(o.nodes) == nodes.tolist() and o.score == -1 and o.ifinal == 0 and o.t > 0
            assert np.all(np.asarray(o.u) == 0) and np.asarray(o.u).shape == (len(probs[i][3]),)
            sel = np.asarray(cb.get_selected_associations(i))
            assert np.array_equal(sel.reshape(-1, 2), probs[i][2][nodes].reshape(-1, 2))
        Ain = np.asarray(cb.get_selected_associations(0))
        assert Ain.shape == (3, 2) and np.all(Ain[:, 0] == Ain[:, 1])
    again = cb.solve(probs)
    for a, f in zip(again, first):
        assert np.array_equal(np.asarray(a.u), np.asarray(f.u))
    hb.close()


def test_cpp_facade_batch_maximum_clique(tmp_path, golden):
    exe = str(tmp_path / "test_batch_maxclique_facade")
    pfile = str(tmp_path / "points.txt")
    g = golden["affinity_test"]
    np.savetxt(pfile, np.concatenate([np.array(g["model"]).T.ravel(), np.array(g["data"]).T.ravel()]), fmt="%.17g")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_batch_maxclique_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "batch.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe, pfile], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL BATCH MAXCLIQUE FACADE TESTS PASSED" in out.stdout
