"""GPU tests of the batched semidefinite relaxation (clipper_hip_sdp_solve_batch, clipper_hip_batch_sdp; DESIGN.md
section 11, "Batches"): per problem the batched call returns, bit for bit, what the lone entry point returns for that
problem on the same device — whatever else the batch holds, wherever the problem stands in it and however the launches
were cut — and where an answer is known it is asserted too, so that both cannot be wrong in the same way."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import synth
from tests.test_gpu_sdp import TIGHT, _certificate, _clique_union

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORAGES = (abi.STORE_F32_CSC, abi.STORE_F64_CSC, abi.STORE_F32, abi.STORE_F64)
INV = synth.EUCLID_BENCH_PARAMS
CLIQUES = [(1, 1), (7, 3), (33, 6), (64, 9), (100, 12), (128, 12)]
INFO_FIELDS = ("iters", "sweeps", "converged", "timed_out", "num_nodes", "pobj", "dobj", "r_prim", "r_dual", "rho", "thr")


def _params(**kw):
    return abi.SdpParams(**kw)


def _assert_bits(rb, rl, what):
    for f in ("X", "Y", "lambdas", "evec1"):
        assert np.array_equal(getattr(rb, f), getattr(rl, f)), f"{what}: {f} differs"
    assert rb.nodes.tolist() == rl.nodes.tolist(), f"{what}: nodes differ"
    for f in INFO_FIELDS:
        assert getattr(rb.info, f) == getattr(rl.info, f), f"{what}: {f}: {getattr(rb.info, f)} != {getattr(rl.info, f)}"
    assert rb.thr == rl.thr and rb.iters == rl.iters and rb.pobj == rl.pobj and rb.dobj == rl.dobj, what


def _euclid_matrices(m, rho, seed):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    g = abi.HipClipper(storage=abi.STORE_F64)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    M, Cm = g.get_affinity_matrix(), g.get_constraint_matrix()
    g.close()
    return M, Cm


# ---- known answers ------------------------------------------------------------------------------------------------

def test_clique_unions_in_one_batch():
    probs, Ks = [], []
    for n, k in CLIQUES:
        A, K = _clique_union(n, k, seed=n)
        probs.append((A, A))
        Ks.append(K)
    res = abi.sdp_solve_batch(probs, _params(**TIGHT))
    assert len(res) == len(CLIQUES)
    for (n, k), K, (A, _), r in zip(CLIQUES, Ks, probs, res):
        assert r.info.converged == 1, (n, k)
        assert r.nodes.tolist() == K, (n, k)
        assert abs(r.pobj + k) <= 1e-4 * k, (n, k, r.pobj)
        _certificate(A, A, r, 1e-6, 1e-6)


# ---- bit for bit against the lone call ----------------------------------------------------------------------------

def _assorted(golden):
    probs = []
    for n, k in CLIQUES:
        A, _ = _clique_union(n, k, seed=n)
        probs.append((A, A))
    M = np.array(golden["dsd_test_20x20"]["M"])
    probs.append((M, (M > 0).astype(float)))
    rng = np.random.default_rng(5)  # tests/test_gpu_sdp.py::test_explicit_constraint_matrix
    n = 50
    up = np.triu(rng.random((n, n)) < 0.4, 1)
    M = np.where(up, rng.uniform(0.1, 1.0, (n, n)), 0.0)
    M = M + M.T + np.eye(n)
    cu = np.triu(rng.random((n, n)) < 0.5, 1)
    probs.append((M, (cu | cu.T).astype(float) + np.eye(n)))
    A, K = _clique_union(30, 5, seed=4)  # tests/test_gpu_sdp.py::test_lower_triangle_and_zero_diagonal
    Mg, Cg = A.copy(), A.copy()
    iu = np.triu_indices(30, 1)
    rng = np.random.default_rng(9)
    Mg[iu] = rng.uniform(-5, 5, len(iu[0]))
    Cg[iu] = rng.integers(0, 2, len(iu[0]))
    Cg[K[0], K[0]] = 0.0
    probs.append((Mg, Cg))
    return probs


def test_bits_against_the_lone_call(golden):
    probs = _assorted(golden)
    res = abi.sdp_solve_batch(probs, _params(**TIGHT))
    for i, ((M, Cm), rb) in enumerate(zip(probs, res)):
        rl = abi.sdp_solve(M, Cm, _params(**TIGHT))
        _assert_bits(rb, rl, f"problem {i} (n = {M.shape[0]})")
        _certificate(M, Cm, rb, 1e-6, 1e-6)
    # without X and Y: the same small results
    lean = abi.sdp_solve_batch(probs, _params(**TIGHT), want_xy=False)
    for rb, rn in zip(res, lean):
        assert rn.X.size == 0 and rn.Y.size == 0
        assert np.array_equal(rn.evec1, rb.evec1) and np.array_equal(rn.lambdas, rb.lambdas)
        assert rn.nodes.tolist() == rb.nodes.tolist() and rn.pobj == rb.pobj and rn.dobj == rb.dobj


# ---- composition does not matter ----------------------------------------------------------------------------------

def test_composition_order_and_determinism():
    rng = np.random.default_rng(77)
    sizes = rng.integers(2, 49, 300)
    probs = [_euclid_matrices(int(m), float(rng.choice([0.3, 0.6, 0.8])), seed=9000 + k) for k, m in enumerate(sizes)]
    eps = dict(eps_abs=1e-4, eps_rel=1e-4)
    a = abi.sdp_solve_batch(probs, _params(**eps))
    iters = sorted({r.iters for r in a})
    print(f"300 problems: {len(iters)} distinct iteration counts, {iters[0]}..{iters[-1]}")
    assert len(iters) >= 5, iters  # (or nothing here says anything about compaction)
    b = abi.sdp_solve_batch(probs, _params(**eps))
    rev = abi.sdp_solve_batch(probs[::-1], _params(**eps))[::-1]
    for i in range(len(probs)):
        _assert_bits(b[i], a[i], f"second call, problem {i}")
        _assert_bits(rev[i], a[i], f"reversed batch, problem {i}")
    for i in rng.choice(len(probs), 12, replace=False):
        rl = abi.sdp_solve(probs[i][0], probs[i][1], _params(**eps))
        _assert_bits(a[i], rl, f"alone, problem {i} (n = {sizes[i]})")


# ---- the CLIPPERBatch route ----------------------------------------------------------------------------------------

def _weak_duality(r, u, M, eps_abs, eps_rel):
    """-dobj bounds the optimum of the problem solve() attacks: u >= 0 of unit norm makes u u^T feasible."""
    tol = eps_abs + eps_rel * abs(r.dobj) + 1e-6
    val = float(u @ M @ u)
    assert -r.dobj >= val - tol, (-r.dobj, val, tol)


@pytest.mark.parametrize("storage", STORAGES)
def test_hipbatch_sdp_matches_lone_contexts(storage):
    rng = np.random.default_rng(31)
    ms = [30, 128] + rng.integers(30, 129, 18).tolist()
    probs = [synth.make_euclidean_problem(int(m), [0.5, 0.7, 0.9][k % 3], seed=7000 + k) for k, m in enumerate(ms)]
    eps = dict(eps_abs=1e-4, eps_rel=1e-4, max_iters=5000)
    b = abi.HipBatch(storage=storage)
    inputs = [(p.D1, p.D2, p.A, p.u0) for p in probs]
    sols = b.solve_euclidean(inputs, **INV)
    res = b.sdp(_params(**eps))
    assert len(res) == len(probs)
    for i, p in enumerate(probs):
        g = abi.HipClipper(storage=storage)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        nodes, rl = g.sdp(_params(**eps))
        what = f"problem {i} (m = {ms[i]}, storage {storage})"
        _assert_bits(res[i], rl, what)
        assert res[i].nodes.tolist() == nodes.tolist(), what
        assert np.array_equal(b.selected_associations(i), g.get_selected_associations()), what
        M = g.get_affinity_matrix()
        _certificate(M, g.get_constraint_matrix(), res[i], 1e-4, 1e-4)
        _weak_duality(res[i], sols[i].u, M, 1e-4, 1e-4)
        g.close()
    # the children's solver state is untouched
    again = b.solve_euclidean(inputs, **INV)
    for i in range(len(probs)):
        assert np.array_equal(again[i].u, sols[i].u) and again[i].nodes.tolist() == sols[i].nodes.tolist(), i
    b.close()


def test_hipbatch_sdp_pointnormal():
    p = synth.make_pointnormal_problem(80, 0.8, seed=7)
    eps = dict(eps_abs=1e-5, eps_rel=1e-5, max_iters=20000)
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    sols = b.solve_pointnormal([(p.D1, p.D2, p.A, p.u0)] * 2)
    res = b.sdp(_params(**eps))
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A)
    nodes, rl = g.sdp(_params(**eps))
    for i in range(2):
        _assert_bits(res[i], rl, f"problem {i}")
        assert np.array_equal(b.selected_associations(i), g.get_selected_associations())
        _weak_duality(res[i], sols[i].u, g.get_affinity_matrix(), 1e-5, 1e-5)
    _certificate(g.get_affinity_matrix(), g.get_constraint_matrix(), res[0], 1e-5, 1e-5)
    b.close()


def test_hipbatch_sdp_refusals():
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    with pytest.raises(abi.ClipperError, match=r"error -5"):
        b.sdp()
    probs = [synth.make_euclidean_problem(m, 0.8, seed=60 + m) for m in (40, 90, 200, 50)]
    inputs = [(p.D1, p.D2, p.A, p.u0) for p in probs]
    sols = b.solve_euclidean(inputs, **INV)
    with pytest.raises(abi.ClipperError, match=r"error -7: problem 2:.*limit of 128"):
        b.sdp()
    # still usable: the same solve, then a relaxation of a batch that fits
    again = b.solve_euclidean(inputs, **INV)
    for s0, s1 in zip(sols, again):
        assert np.array_equal(s0.u, s1.u)
    b.solve_euclidean(inputs[:2], **INV)
    res = b.sdp()
    assert len(res) == 2 and all(len(r.nodes) > 0 for r in res)
    b.close()


# ---- stop rules, refusals on the device ---------------------------------------------------------------------------

def test_max_iters_and_time_limit():
    probs = [_euclid_matrices(128, 0.6, seed=2 + k) for k in range(4)]
    tight = abi.sdp_solve_batch(probs, _params(**TIGHT))
    res = abi.sdp_solve_batch(probs, _params(max_iters=5, eps_abs=1e-9, eps_rel=1e-9))
    for (M, Cm), r, t in zip(probs, res, tight):
        assert r.iters == 5 and r.info.converged == 0 and r.info.timed_out == 0 and len(r.nodes) > 0
        _, d5 = _certificate(M, Cm, r, 1e-9, 1e-9)
        assert d5 >= -t.pobj - 1e-4 * abs(t.pobj)  # still a bound on the optimum
    many = [probs[k % 4] for k in range(64)]
    t0 = time.time()
    res = abi.sdp_solve_batch(many, _params(max_iters=10 ** 6, eps_abs=1e-12, eps_rel=1e-12, time_limit_secs=0.3))
    wall = time.time() - t0
    print(f"time limit 0.3 s on 64 problems of n = 128: {wall:.3f} s, iterations {sorted({r.iters for r in res})}")
    assert wall < 5.0, wall
    for k, r in enumerate(res):
        assert r.info.timed_out == 1 and r.info.converged == 0, (k, r.iters)
        M, Cm = many[k]
        _, d = _certificate(M, Cm, r, 1e-12, 1e-12)
        t = tight[k % 4]
        assert d >= -t.pobj - 1e-4 * abs(t.pobj)


def test_infeasible_problem_is_named():
    eye = np.eye(6)
    Cz = np.ones((6, 6))
    np.fill_diagonal(Cz, 0.0)
    with pytest.raises(abi.ClipperError, match=r"error -1: problem 3:.*diagonal"):
        abi.sdp_solve_batch([(eye, eye), (eye, eye), (eye, eye), (eye, Cz), (eye, eye)])


# ---- the reference-facing surfaces ----------------------------------------------------------------------------------

def test_clipperpy_batch_surfaces(golden):
    cp = clipper_amd.load_clipperpy()
    probs = _assorted(golden)[4:]
    prm = cp.SDPParams()
    prm.eps_abs, prm.eps_rel, prm.max_iters = 1e-6, 1e-6, 20000
    sols = cp.sdp.solve_batch([np.asfortranarray(M) for M, _ in probs], [np.asfortranarray(Cm) for _, Cm in probs], prm)
    ref = abi.sdp_solve_batch(probs, _params(**TIGHT))
    assert len(sols) == len(ref)
    for s, r in zip(sols, ref):
        assert isinstance(s, cp.SDPSolution)
        assert list(s.nodes) == r.nodes.tolist() and np.array_equal(np.asarray(s.X), r.X)
        assert np.array_equal(np.asarray(s.evec1), r.evec1) and np.array_equal(np.asarray(s.lambdas), r.lambdas)
        assert s.iters == r.iters and s.thr == r.thr and s.t > 0
        assert s.pobj == pytest.approx(r.pobj, rel=1e-6) and s.dobj == pytest.approx(r.dobj, rel=1e-6)
    # CLIPPERBatch.solve_as_msrc_sdr against HipBatch.sdp
    ps = [synth.make_euclidean_problem(m, 0.7, seed=300 + m) for m in (40, 77, 128)]
    ip = cp.invariants.EuclideanDistanceParams()
    ip.sigma, ip.epsilon, ip.mindist = INV["sigma"], INV["epsilon"], INV["mindist"]
    cb = cp.CLIPPERBatch(cp.invariants.EuclideanDistance(ip), cp.Params())
    with pytest.raises(Exception):
        cb.solve_as_msrc_sdr(prm)  # before any solve
    first = cb.solve([(p.D1, p.D2, p.A.astype(np.int32), p.u0) for p in ps])
    out = cb.solve_as_msrc_sdr(prm)
    hb = abi.HipBatch(storage=abi.STORE_F32_CSC)
    hb.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in ps], **INV)
    ref = hb.sdp(_params(**TIGHT))
    full = cb.sdp_solutions()
    assert len(out) == len(full) == len(ps)
    for i, (o, s, r) in enumerate(zip(out, full, ref)):
        assert sorted(o.nodes) == r.nodes.tolist() and o.score == -1 and o.ifinal == 0 and o.t > 0
        assert np.all(np.asarray(o.u) == 0) and np.asarray(o.u).shape == (len(ps[i].u0),)
        assert list(s.nodes) == r.nodes.tolist() and np.array_equal(np.asarray(s.X), r.X)
        assert np.array_equal(np.asarray(s.evec1), r.evec1) and s.iters == r.iters
        assert s.dobj == pytest.approx(r.dobj, rel=1e-6)
        assert np.array_equal(np.asarray(cb.get_selected_associations(i)), hb.selected_associations(i))
    again = cb.solve([(p.D1, p.D2, p.A.astype(np.int32), p.u0) for p in ps])
    for a, f in zip(again, first):
        assert np.array_equal(np.asarray(a.u), np.asarray(f.u))
    hb.close()


def test_cpp_facade_sdp_batch(tmp_path, golden):
    exe = str(tmp_path / "test_sdp_batch_facade")
    mfile = str(tmp_path / "M.txt")
    np.savetxt(mfile, np.array(golden["dsd_test_20x20"]["M"]), fmt="%.17g")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_sdp_batch_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "batch.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe, mfile], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL SDP BATCH FACADE TESTS PASSED" in out.stdout


# ---- it is actually batched ----------------------------------------------------------------------------------------

def test_batched_call_beats_the_loop_of_lone_calls():
    """64 problems of m = 64, max_iters = 100 (the numpy model: 48..100 iterations each, 4 475 in all): with every
    problem on a compute unit of its own the ideal ratio is 100 / 4 475 = 1 / 45; asserted: one batched call takes at
    most a quarter of the loop of lone calls, which serialised launches cannot meet."""
    probs = [_euclid_matrices(64, 0.7, seed=1000 + k) for k in range(64)]
    prm = dict(eps_abs=1e-4, eps_rel=1e-4, max_iters=100)

    def loop():
        return [abi.sdp_solve(M, Cm, _params(**prm)) for M, Cm in probs]

    def batch():
        return abi.sdp_solve_batch(probs, _params(**prm))

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
    total = sum(r.iters for r in ra)
    print(f"64 problems of n = 64: loop of lone calls {ta * 1e3:.1f} ms, one batched call {tb * 1e3:.1f} ms, "
          f"ratio {tb / ta:.4f} (iterations {min(r.iters for r in ra)}..{max(r.iters for r in ra)}, {total} in all)")
    for i in range(len(probs)):
        _assert_bits(rb[i], ra[i], f"problem {i}")
    assert tb <= ta / 4, (ta, tb)
