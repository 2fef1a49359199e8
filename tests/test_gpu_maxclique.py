"""GPU tests of the maximum-clique solver (clipper_hip_max_clique, CLIPPER::solveAsMaximumClique)
against the sequential model of tests/maxclique_model.py."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import clipper_amd
from clipper_amd import _abi as abi
from clipper_amd import registration as reg
from clipper_amd import synth
from tests import maxclique_model as mm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
STORAGES = (abi.STORE_F32_CSC, abi.STORE_F64_CSC, abi.STORE_F32, abi.STORE_F64)
METHODS = (abi.MC_EXACT, abi.MC_HEU, abi.MC_KCORE)


def _adj_of(g):
    return mm.adjacency_from_matrix(g.get_constraint_matrix())


def _euclid(m, rho, seed, storage=abi.STORE_F32_CSC):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    return g


def _pointnormal(m, storage=abi.STORE_F32_CSC):
    p = synth.make_pointnormal_problem(m, 0.9, seed=7)
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A)
    return g


def _bunny(storage=abi.STORE_F32_CSC):
    d = json.load(open(os.path.join(HERE, "golden", "bunny_points.json")))
    pts = np.array(d["points"], dtype=np.float64)
    rng = np.random.default_rng(1000)
    T = np.eye(4)
    T[:3, :3] = reg.random_rotation(rng)
    T[:3, 3] = rng.uniform(-5, 5, 3)
    D1, D2, A, _ = reg.make_registration_dataset(pts, seed=0, T_21=T, m=100, n1=100, n2o=25, outrat=0.9, sigma=0.01)
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(D1, D2, A, sigma=0.01, epsilon=0.02, mindist=0.0)
    return g


def _random_pair(m, p, seed):
    """A symmetric M with an explicit C != pattern(M): C drops some of M's entries and adds its own."""
    rng = np.random.default_rng(seed)
    up = np.triu(rng.random((m, m)) < p, 1)
    M = np.where(up, rng.uniform(0.1, 1.0, (m, m)), 0.0)
    M = M + M.T + np.eye(m)
    cu = np.triu((rng.random((m, m)) < p) ^ (up & (rng.random((m, m)) < 0.3)), 1)
    Cm = (cu | cu.T).astype(float) + np.eye(m)
    return M, Cm


def _csc_upper(X):
    """strictly-upper CSC of a dense symmetric matrix (what clipper_hip_set_sparse reads)"""
    m = X.shape[0]
    colptr, rows, vals = [0], [], []
    for j in range(m):
        i = np.flatnonzero(X[:j, j])
        rows += i.tolist()
        vals += X[i, j].tolist()
        colptr.append(len(rows))
    return np.array(colptr, np.int64), np.array(rows, np.int32), np.array(vals, np.float64)


def _check_all_methods(g, adj, core=None):
    core = mm.core_numbers(adj) if core is None else core
    assert g.core_numbers().tolist() == core.tolist()
    kc, info = g.max_clique(abi.MC_KCORE)
    assert kc.tolist() == mm.kcore(adj, core) and info.max_core == int(core.max())
    heu = mm.heu(adj, core)
    h, info = g.max_clique(abi.MC_HEU)
    assert h.tolist() == heu and info.heuristic_size == len(heu)
    w = mm.omega(adj, lower=len(heu))
    e, info = g.max_clique(abi.MC_EXACT)
    assert len(e) == w and mm.is_clique(adj, e) and info.timed_out == 0
    assert info.edges == int(adj.sum()) // 2
    return e.tolist()


# ---- the reference's golden cases --------------------------------------------------------------------------------

def test_golden_affinity_test(golden):
    g = golden["affinity_test"]
    c = abi.HipClipper(storage=abi.STORE_F32_CSC)
    c.score_pairwise_consistency_euclidean(np.array(g["model"]), np.array(g["data"]))  # all-to-all
    A = c.get_initial_associations()
    Mtrue = np.array(g["Mtrue"])
    assert np.array_equal(c.get_constraint_matrix(), (Mtrue != 0).astype(float))
    want = [2 if v in (0, 4, 8) else (0 if v == 11 else 1) for v in range(12)]
    import networkx as nx
    assert [nx.core_number(nx.from_numpy_array((Mtrue != 0) & ~np.eye(12, dtype=bool)))[v] for v in range(12)] == want
    assert c.core_numbers().tolist() == want
    for meth in METHODS:
        nodes, info = c.max_clique(meth)
        assert nodes.tolist() == [0, 4, 8], meth
    assert np.array_equal(c.get_selected_associations(), A[[0, 4, 8]])


def test_golden_dsd_20x20_nine_maximum_cliques(golden):
    M = np.array(golden["dsd_test_20x20"]["M"])
    Cm = (M != 0).astype(float)
    adj = mm.adjacency_from_matrix(Cm)
    core = mm.core_numbers(adj)
    assert int(core.max()) == 3 and mm.omega(adj) == 3
    lists = []
    for storage in STORAGES:
        c = abi.HipClipper(storage=storage)
        c.set_matrix_data(M, Cm)
        assert c.core_numbers().tolist() == core.tolist()
        kc, _ = c.max_clique(abi.MC_KCORE)
        assert kc.tolist() == [3, 4, 5, 8, 9, 13, 15, 16, 17]
        for _ in range(2):
            e, info = c.max_clique(abi.MC_EXACT)
            assert len(e) == 3 and mm.is_clique(adj, e) and info.max_core == 3
            lists.append(e.tolist())
    assert all(x == lists[0] for x in lists), lists


# ---- core numbers and methods against the model -------------------------------------------------------------------

@pytest.mark.parametrize("m", [100, 1000, 2048])
def test_euclidean_problems(m):
    g = _euclid(m, 0.9, seed=31 + m)
    adj = _adj_of(g)
    lists = {tuple(_check_all_methods(g, adj))}
    for storage in (abi.STORE_F64_CSC, abi.STORE_F32, abi.STORE_F64):
        g2 = _euclid(m, 0.9, seed=31 + m, storage=storage)
        assert np.array_equal(_adj_of(g2), adj)
        lists.add(tuple(_check_all_methods(g2, adj)))
    assert len(lists) == 1, lists


def test_pointnormal_problem():
    g = _pointnormal(1000)
    _check_all_methods(g, _adj_of(g))


def test_bunny_configuration():
    g = _bunny()
    _check_all_methods(g, _adj_of(g))


@pytest.mark.parametrize("m,p,seed", [(150, 0.3, 1), (300, 0.5, 2), (500, 0.1, 3)])
def test_explicit_constraint_matrix_dense_and_sparse(m, p, seed):
    M, Cm = _random_pair(m, p, seed)
    adj = mm.adjacency_from_matrix(Cm)
    assert not np.array_equal(adj, mm.adjacency_from_matrix(M))
    core = mm.core_numbers(adj)
    lists = set()
    for storage in STORAGES:
        g = abi.HipClipper(storage=storage)
        g.set_matrix_data(M, Cm)
        lists.add(tuple(_check_all_methods(g, adj, core)))
        g2 = abi.HipClipper(storage=storage)
        g2.set_sparse_matrix_data(m, *_csc_upper(M), *_csc_upper(Cm))
        lists.add(tuple(_check_all_methods(g2, adj, core)))
    assert len(lists) == 1, lists


def test_staging_kept_by_a_context():
    """One context, matrices of m = 300, 65 and 300 again: its staging buffer is reused with other offsets and a
    smaller need; every call equals the model, and the third round the first, list for list."""
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    rounds = []
    for m, seed in ((300, 1), (65, 2), (300, 1)):
        M, Cm = _random_pair(m, 0.3, seed)
        g.set_matrix_data(M, Cm)
        adj = mm.adjacency_from_matrix(Cm)
        _check_all_methods(g, adj)
        rounds.append([g.core_numbers().tolist()] + [g.max_clique(meth)[0].tolist() for meth in METHODS])
    g.close()
    assert rounds[2] == rounds[0] and len(rounds[1][0]) == 65


def test_explicit_c_on_slices_and_on_a_dense_store():
    """m = 129 (two words per row and one bit): with an explicit C of another pattern than M's the graph is C's, on a
    slice storage (where the slices hold M) as on a dense one."""
    M, Cm = _random_pair(129, 0.3, 4)
    adj = mm.adjacency_from_matrix(Cm)
    assert not np.array_equal(adj, mm.adjacency_from_matrix(M))
    core = mm.core_numbers(adj)
    lists = set()
    for storage in (abi.STORE_F32_CSC, abi.STORE_F64):
        g = abi.HipClipper(storage=storage)
        g.set_matrix_data(M, Cm)
        lists.add(tuple(_check_all_methods(g, adj, core)))
        g.close()
    assert len(lists) == 1, lists


def test_bench_problem_exact():
    p = synth.make_euclidean_problem(10000, 0.95, seed=12345)
    gs = abi.HipClipper(storage=abi.STORE_F32_CSC)
    gs.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    adj = _adj_of(gs)
    core = mm.core_numbers(adj)
    assert gs.core_numbers().tolist() == core.tolist()
    heu = mm.heu(adj, core)
    w = mm.omega(adj, lower=len(heu))
    e1, i1 = gs.max_clique(abi.MC_EXACT)
    e2, _ = gs.max_clique(abi.MC_EXACT)
    assert len(e1) == w and mm.is_clique(adj, e1) and i1.heuristic_size == len(heu)
    gd = abi.HipClipper(storage=abi.STORE_F64)
    gd.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    e3, _ = gd.max_clique(abi.MC_EXACT)
    assert e1.tolist() == e2.tolist() == e3.tolist()
    print(f"m=10000: K={i1.max_core} heu={i1.heuristic_size} omega={len(e1)} searched={i1.roots_searched} "
          f"pruned={i1.roots_pruned} nodes={i1.bb_nodes} {i1.seconds * 1e3:.1f} ms")


# ---- edge cases ---------------------------------------------------------------------------------------------------

def test_edgeless_and_complete_graphs():
    m = 70
    for storage in STORAGES:
        g = abi.HipClipper(storage=storage)
        g.set_matrix_data(np.eye(m), np.eye(m))
        assert g.core_numbers().tolist() == [0] * m
        assert g.max_clique(abi.MC_EXACT)[0].tolist() == []
        assert g.max_clique(abi.MC_HEU)[0].tolist() == []
        assert g.max_clique(abi.MC_KCORE)[0].tolist() == list(range(m))
        full = np.ones((m, m))
        g.set_matrix_data(full * 0.5 + np.eye(m) * 0.5, full)
        assert g.core_numbers().tolist() == [m - 1] * m
        for meth in METHODS:
            nodes, info = g.max_clique(meth)
            assert nodes.tolist() == list(range(m)) and info.max_core == m - 1


def test_no_matrix_and_column_shards():
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    with pytest.raises(abi.ClipperError, match="error -5"):
        g.max_clique(abi.MC_EXACT)
    with pytest.raises(abi.ClipperError, match="error -5"):
        g.core_numbers()
    p = synth.make_euclidean_problem(300, 0.9, seed=3)
    grp = abi.HipClipper(storage=abi.STORE_F32_CSC, group=[0, 0])
    grp.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    with pytest.raises(abi.ClipperError, match="error -7"):
        grp.max_clique(abi.MC_KCORE)
    with pytest.raises(abi.ClipperError, match="error -7"):
        grp.core_numbers()


def test_time_limit():
    m = 2000
    rng = np.random.default_rng(11)
    up = np.triu(rng.random((m, m)) < 0.5, 1)
    Cm = (up | up.T).astype(float) + np.eye(m)
    g = abi.HipClipper(storage=abi.STORE_F32)
    g.set_matrix_data(Cm, Cm)
    heu, _ = g.max_clique(abi.MC_HEU)
    t0 = time.time()
    e, info = g.max_clique(abi.MC_EXACT, time_limit=0.5)
    wall = time.time() - t0
    assert wall < 5.0 and info.timed_out == 1, (wall, info.timed_out)
    adj = mm.adjacency_from_matrix(Cm)
    assert mm.is_clique(adj, e) and len(e) >= len(heu)


def test_no_side_effects_on_solve():
    p = synth.make_euclidean_problem(1000, 0.9, seed=21)
    fresh = abi.HipClipper(storage=abi.STORE_F32_CSC)
    fresh.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    s0 = fresh.solve(p.u0)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    for meth in METHODS:
        nodes, _ = g.max_clique(meth)
        sel = g.get_selected_associations()
        assert np.array_equal(sel, np.asarray(p.A)[nodes])
    s1 = g.solve(p.u0)
    assert np.array_equal(s1.u, s0.u) and s1.nodes.tolist() == s0.nodes.tolist()


# ---- the reference-facing surfaces ------------------------------------------------------------------------------

def test_clipperpy_solve_as_maximum_clique(golden):
    cp = clipper_amd.load_clipperpy()
    g = golden["affinity_test"]
    inv = cp.invariants.EuclideanDistance(cp.invariants.EuclideanDistanceParams())
    c = cp.CLIPPER(inv, cp.Params())
    c.score_pairwise_consistency(np.array(g["model"]), np.array(g["data"]), cp.utils.create_all_to_all(4, 3))
    for meth in (cp.MCMethod.EXACT, cp.MCMethod.HEU, cp.MCMethod.KCORE):
        prm = cp.MCParams()
        prm.method = meth
        c.solve_as_maximum_clique(prm)
        s = c.get_solution()
        assert sorted(s.nodes) == [0, 4, 8] and s.score == -1 and s.ifinal == 0 and s.t > 0
        assert np.all(np.asarray(s.u) == 0) and np.asarray(s.u).shape == (12,)
        Ain = c.get_selected_associations()
        assert Ain.shape == (3, 2) and np.all(Ain[:, 0] == Ain[:, 1])


def test_cpp_facade_maximum_clique(tmp_path):
    exe = str(tmp_path / "test_maxclique_facade")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "test_maxclique_facade.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL MAXCLIQUE FACADE TESTS PASSED" in out.stdout
    assert "PMC is not built" not in out.stdout
