"""GPU tests of the compressed storage (CLIPPER_HIP_STORE_F32_CSC / _F64_CSC): M kept as slices
(k_slices.hip.h), written by k_affinity_sym itself or packed from groups / CSC lists
(k_slice_count / scan / k_slice_pack), read by k_gemv_slices, expanded on demand by
k_slice_expand. Everything the parity suite runs per storage mode (tests/test_gpu_parity.py,
STORAGES) covers it too; here are the cases specific to the format: slice edges, empty and fully
dense slices, growth of the buffers, fp64 values, setSparseMatrixData without a dense
intermediate, the fall-back to the dense store."""
import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth
from oracle import clipper_ref as ref

pytestmark = pytest.mark.gpu

INV = synth.EUCLID_BENCH_PARAMS


def _affinity(storage, p, **inv):
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **(inv or INV))
    return g


# slices are 128 rows x 64 columns (tiles of the fill kernel 128 x 128): sizes on and around
# their edges, and a ragged last tile
@pytest.mark.parametrize("m", [2, 63, 64, 65, 127, 128, 129, 191, 193, 257, 640, 1000, 2049])
def test_matrix_round_trip_bitwise(m):
    p = synth.make_euclidean_problem(m, 0.7, seed=m)
    gd, gc = _affinity(abi.STORE_F32, p), _affinity(abi.STORE_F32_CSC, p)
    assert gc.storage_in_use == abi.STORE_F32_CSC and gd.storage_in_use == abi.STORE_F32
    Md, Mc = gd.get_affinity_matrix(), gc.get_affinity_matrix()   # k_csc_expand behind the second
    assert np.array_equal(Md, Mc)
    assert np.array_equal(gd.get_constraint_matrix(), gc.get_constraint_matrix())
    x = np.random.default_rng(m).random(m)
    yd, yc = gd.matvec(x), gc.matvec(x)   # dense pass vs the pass on the slices: the order of the sums differs
    assert np.allclose(yd[0], yc[0], rtol=1e-13, atol=1e-13) and np.allclose(yd[1], yc[1], rtol=1e-13, atol=1e-13)
    # the solver (passes on the slices) after the dense store was materialised for the getters
    sd, sc = gd.solve(p.u0), gc.solve(p.u0)
    assert sorted(sd.nodes.tolist()) == sorted(sc.nodes.tolist())
    assert abs(sd.score - sc.score) <= 1e-9 * max(1.0, abs(sd.score))


@pytest.mark.parametrize("rho,eps", [(0.0, 0.05), (0.95, 1e-9), (0.5, 10.0)])
def test_dense_and_empty_groups(rho, eps):
    """rho = 0: every association is an inlier — every group is full (64 entries per column);
    epsilon -> 0: no consistent pair at all — every list is empty; epsilon huge: everything
    consistent."""
    m = 700
    p = synth.make_euclidean_problem(m, rho, seed=3)
    inv = dict(sigma=0.015, epsilon=eps, mindist=0.0)
    g = _affinity(abi.STORE_F32_CSC, p, **inv)
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **inv)
    Mg, Mr = g.get_affinity_matrix(), r.get_affinity_matrix()
    assert np.array_equal(Mg != 0, Mr != 0)
    sg, sr = g.solve(p.u0), r.solve(p.u0)
    assert sorted(sg.nodes.tolist()) == sorted(sr.nodes.tolist())
    assert abs(sg.score - sr.score) <= 1e-6 * max(1.0, abs(sr.score))
    assert sg.ifinal == sr.ifinal


def test_buffers_grow_and_are_reused():
    """one context, problems of changing size and density: the lists are re-allocated when they
    do not fit and reused when they do; results equal those of fresh contexts."""
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    for m, rho, seed in [(500, 0.9, 1), (2000, 0.9, 2), (2000, 0.2, 3), (500, 0.9, 1), (2000, 0.95, 4)]:
        p = synth.make_euclidean_problem(m, rho, seed=seed)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        s = g.solve(p.u0)
        f = _affinity(abi.STORE_F32_CSC, p)
        sf = f.solve(p.u0)
        assert s.nodes.tolist() == sf.nodes.tolist() and s.score == sf.score   # bit-identical
        assert np.array_equal(s.u, sf.u)
        r = ref.RefClipper()
        r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        sr = r.solve(p.u0)
        assert sorted(s.nodes.tolist()) == sorted(sr.nodes.tolist())
        f.close()
    g.close()


def _random_symmetric(m, density, seed):
    rng = np.random.default_rng(seed)
    U = np.triu((rng.random((m, m)) < density) * rng.uniform(0.1, 1.0, (m, m)), 1)
    M = U + U.T + np.eye(m)
    return M, (M != 0).astype(np.float64)


@pytest.mark.parametrize("m", [130, 777])
def test_set_matrix_paths(m):
    """setMatrixData with C == pattern(M): k_csc_build from the uploaded dense store; with any
    other C the context falls back to the dense store (and says so)."""
    M, C = _random_symmetric(m, 0.08, seed=m)
    u0 = np.random.default_rng(1).random(m)
    gd, gc = abi.HipClipper(storage=abi.STORE_F32), abi.HipClipper(storage=abi.STORE_F32_CSC)
    gd.set_matrix_data(M, C)
    gc.set_matrix_data(M, C)
    assert gc.storage_in_use == abi.STORE_F32_CSC
    assert np.array_equal(gd.get_affinity_matrix(), gc.get_affinity_matrix())
    sd, sc = gd.solve(u0), gc.solve(u0)
    assert sorted(sd.nodes.tolist()) == sorted(sc.nodes.tolist())
    assert abs(sd.score - sc.score) <= 1e-9 * max(1.0, abs(sd.score))
    # a constraint matrix that is NOT the pattern of M: dense fall-back
    C2 = C.copy()
    i, j = np.argwhere(np.triu(M, 1) != 0)[0]
    C2[i, j] = C2[j, i] = 0.0
    gc.set_matrix_data(M, C2)
    gd.set_matrix_data(M, C2)
    assert gc.storage_in_use == abi.STORE_F32
    sd, sc = gd.solve(u0), gc.solve(u0)
    assert sd.nodes.tolist() == sc.nodes.tolist() and sd.score == sc.score
    # and back to the compressed copy with the next affinity build
    p = synth.make_euclidean_problem(m, 0.8, seed=5)
    gc.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    assert gc.storage_in_use == abi.STORE_F32_CSC


def test_pointnormal_and_other_fill_kernels(monkeypatch):
    """PointNormalDistance through k_affinity_sym<PointNormalInv>; the strip / plain fill kernels
    through k_csc_build (CLIPPER_HIP_AFFINITY)."""
    p = synth.make_pointnormal_problem(900, 0.8, seed=9)
    inv = p.meta["invariant"]
    mats = {}
    for mode in ("", "strip", "plain"):
        if mode:
            monkeypatch.setenv("CLIPPER_HIP_AFFINITY", mode)
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, **inv)
        assert g.storage_in_use == abi.STORE_F32_CSC
        mats[mode] = (g.get_affinity_matrix(), g.solve(p.u0))
        g.close()
        if mode:
            monkeypatch.delenv("CLIPPER_HIP_AFFINITY")
    for mode in ("strip", "plain"):
        assert np.array_equal(mats[""][0], mats[mode][0])
        assert mats[""][1].nodes.tolist() == mats[mode][1].nodes.tolist()
        assert mats[""][1].score == mats[mode][1].score


def test_dsd_rounding_on_compressed_storage():
    p = synth.make_euclidean_problem(400, 0.8, seed=21)
    out = {}
    for st in (abi.STORE_F32, abi.STORE_F32_CSC):
        g = abi.HipClipper(abi.Params(rounding=abi.ROUNDING_DSD), storage=st)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        out[st] = g.solve(p.u0)
    assert sorted(out[abi.STORE_F32].nodes.tolist()) == sorted(out[abi.STORE_F32_CSC].nodes.tolist())


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_dsd_gathers_its_sub_matrix_from_the_slices(storage):
    """dsd::solve(M, S) (dsd.cpp:274-320) with M in slices: the induced sub-matrix is gathered by
    k_slice_gather_sub from the slices themselves (no dense copy of M is made) — several chunks and
    column groups, a node list in arbitrary order, column shards, and a list that names a node twice
    (gathered by index from a dense copy, as before): all against the oracle's procedure on the matrix
    the device holds."""
    from oracle import dsd_ref
    p = synth.make_euclidean_problem(700, 0.85, seed=33)
    g = abi.HipClipper(storage=storage)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    M = g.get_affinity_matrix()
    s = g.solve(p.u0)
    S = np.flatnonzero(s.u > 0).astype(np.int32)
    assert 20 <= S.size <= 400
    want = dsd_ref.densest_subgraph(M, S.tolist())
    assert g.densest_subgraph(S).tolist() == want
    rng = np.random.default_rng(5)
    assert sorted(g.densest_subgraph(rng.permutation(S).astype(np.int32)).tolist()) == want
    # a list reaching over every chunk of rows and a sparse part of the graph
    S2 = np.unique(np.concatenate([S[:40], rng.choice(700, 60, replace=False)])).astype(np.int32)
    assert g.densest_subgraph(S2).tolist() == dsd_ref.densest_subgraph(M, S2.tolist())
    twice = np.concatenate([S[:30], S[:1]]).astype(np.int32)
    assert sorted(g.densest_subgraph(twice).tolist()) == dsd_ref.densest_subgraph(M, twice.tolist())
    for nshards in (2, 3):
        grp = abi.HipClipper(storage=storage, group=[0] * nshards)
        grp.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        assert grp.densest_subgraph(S).tolist() == want
        grp.close()
    g.close()


def test_column_shards_keep_a_compressed_copy_each(monkeypatch):
    """what bench.py --gpus N > 1 does with its default storage: every column shard (here a
    1-rank RCCL world, and in-process groups of 2, 3 and 5 shards on the one GPU) builds a
    compressed copy of its dense slice (k_csc_build) and streams it with k_gemv_csc +
    k_reduce_pass."""
    p = synth.make_euclidean_problem(1200, 0.9, seed=3)
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    sr = r.solve(p.u0)
    monkeypatch.setenv("CLIPPER_HIP_FORCE_RCCL", "1")
    g = abi.HipClipper(storage=abi.STORE_F32_CSC, rank=0, world=1)
    g.comm_init(g.unique_id())
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    assert g.storage_in_use == abi.STORE_F32_CSC
    sg = g.solve(p.u0)
    assert sg.nodes.tolist() == sr.nodes.tolist()
    assert abs(sg.score - sr.score) <= 1e-6 * abs(sr.score)
    monkeypatch.delenv("CLIPPER_HIP_FORCE_RCCL")
    Md = abi.HipClipper(storage=abi.STORE_F32)
    Md.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    Mref = Md.get_affinity_matrix()
    for nshards in (2, 3, 5):
        grp = abi.HipClipper(storage=abi.STORE_F32_CSC, group=[0] * nshards)
        grp.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        assert grp.storage_in_use == abi.STORE_F32_CSC
        assert np.array_equal(grp.get_affinity_matrix(), Mref)
        s3 = grp.solve(p.u0)
        assert s3.nodes.tolist() == sr.nodes.tolist()
        assert abs(s3.score - sg.score) <= 1e-12 * abs(sg.score)   # another summation order
        s3b = grp.solve(p.u0)
        assert np.array_equal(s3.u, s3b.u)                           # run-to-run bit-identical
        grp.close()


@pytest.mark.parametrize("m,rho,seed", [(6500, 0.95, 2)])
def test_column_shards_window_mode(m, rho, seed):
    """The window of 6 candidates per pass (automatic from m = 8500 on the slices) on sharded compressed copies."""
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    one = abi.HipClipper(storage=abi.STORE_F32_CSC)
    one.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    assert one.window == 4   # the automatic choice at this size
    s1 = one.solve(p.u0)
    grp = abi.HipClipper(storage=abi.STORE_F32_CSC, group=[0] * 4)
    grp.set_window(6)
    grp.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    assert grp.window == 6 and grp.storage_in_use == abi.STORE_F32_CSC
    s4 = grp.solve(p.u0)
    assert sorted(s4.nodes.tolist()) == sorted(s1.nodes.tolist())
    assert abs(s4.score - s1.score) <= 1e-9 * abs(s1.score)


def test_full_size_10k_compressed_parity():
    """BASELINE.json's headline problem in the storage bench.py runs: oracle comparison."""
    m = 10000
    p = synth.make_euclidean_problem(m, 0.95, seed=12345)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    sg = g.solve(p.u0)
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    sr = r.solve(p.u0)
    assert sg.nodes.tolist() == sr.nodes.tolist()
    assert abs(sg.score - sr.score) <= 1e-6 * abs(sr.score)
    assert sg.ifinal == sr.ifinal
    # the pass as a linear map (compressed) against the dense store's pass of a second context
    d = abi.HipClipper(storage=abi.STORE_F32)
    d.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    sd = d.solve(p.u0)
    assert sorted(sd.nodes.tolist()) == sorted(sg.nodes.tolist())
    assert abs(sd.score - sg.score) <= 1e-9 * abs(sd.score)


# ------------------------------------------------------------------------------------------
# fp64 values in the slices (CLIPPER_HIP_STORE_F64_CSC): the parity-exact mode at compressed cost
# ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,rho,seed", [(129, 0.7, 1), (1037, 0.8, 7), (2500, 0.9, 11)])
def test_f64_slices_equal_the_dense_f64_store(m, rho, seed):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    gd, gc = _affinity(abi.STORE_F64, p), _affinity(abi.STORE_F64_CSC, p)
    assert gc.storage_in_use == abi.STORE_F64_CSC and gd.storage_in_use == abi.STORE_F64
    assert np.array_equal(gd.get_affinity_matrix(), gc.get_affinity_matrix())   # fp64 values, bit for bit
    x = np.random.default_rng(m).random(m)
    yd, yc = gd.matvec(x), gc.matvec(x)
    assert np.allclose(yd[0], yc[0], rtol=1e-13, atol=1e-13) and np.allclose(yd[1], yc[1], rtol=1e-13, atol=1e-13)
    sd, sc = gd.solve(p.u0), gc.solve(p.u0)
    assert sd.nodes.tolist() == sc.nodes.tolist() and sd.ifinal == sc.ifinal
    assert sd.n_trials == sc.n_trials
    assert abs(sd.score - sc.score) <= 1e-10 * max(1.0, abs(sd.score))   # the order of the additions differs (resident solver)
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    sr = r.solve(p.u0)
    assert sc.nodes.tolist() == sr.nodes.tolist() and sc.n_trials == sr.n_trials
    assert abs(sc.score - sr.score) <= 1e-9 * abs(sr.score)


# ------------------------------------------------------------------------------------------
# setSparseMatrixData (clipper.cpp:162-166): lists -> slices, no dense intermediate
# ------------------------------------------------------------------------------------------

def _upper_csc(M):
    import scipy.sparse as sp
    U = sp.csc_matrix(np.triu(M, 1))
    U.sort_indices()
    return U


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
@pytest.mark.parametrize("m", [77, 640, 1500])
def test_set_sparse_equals_set_matrix(m, storage):
    import scipy.sparse as sp
    M, C = _random_symmetric(m, 0.07, seed=m)
    U = _upper_csc(M)
    P = sp.csc_matrix((np.ones_like(U.data), U.indices, U.indptr), shape=U.shape)
    u0 = np.random.default_rng(3).random(m)
    a, b = abi.HipClipper(storage=storage), abi.HipClipper(storage=storage)
    a.set_matrix_data(M, C)
    b.set_sparse_matrix_data(m, U.indptr, U.indices, U.data, P.indptr, P.indices, P.data)
    assert b.storage_in_use == storage
    assert np.array_equal(a.get_affinity_matrix(), b.get_affinity_matrix())
    assert np.array_equal(a.get_constraint_matrix(), b.get_constraint_matrix())
    sa, sb = a.solve(u0), b.solve(u0)
    assert sa.nodes.tolist() == sb.nodes.tolist() and sa.score == sb.score and np.array_equal(sa.u, sb.u)
    # the LOWER triangle handed over instead (rows > column): selfadjointView<Upper> (clipper.cpp:194-271)
    # never reads it — an empty matrix, in the reference, in the oracle and here
    L = sp.csc_matrix(np.tril(M, -1))
    L.sort_indices()
    PL = sp.csc_matrix((np.ones_like(L.data), L.indices, L.indptr), shape=L.shape)
    c = abi.HipClipper(storage=storage)
    c.set_sparse_matrix_data(m, L.indptr, L.indices, L.data, PL.indptr, PL.indices, PL.data)
    assert "below the diagonal" in c.last_error() and str(2 * L.nnz) in c.last_error()   # (M's and C's: accepted, with a warning — ADVICE r04)
    assert np.array_equal(c.get_affinity_matrix(), np.eye(m))
    assert np.array_equal(c.get_constraint_matrix(), np.eye(m))
    r = ref.RefClipper()
    r.set_sparse_matrix_data(m, L.indptr, L.indices, L.data, PL.indptr, PL.indices, PL.data)
    assert np.array_equal(r.get_affinity_matrix(), np.eye(m))
    yM, yC = r.matvec(u0)
    assert not yM.any() and not yC.any()
    # ... and solved as the graph without edges it is: one node, the oracle's (slices that hold no entry at all)
    se, sr = c.solve(u0), r.solve(u0)
    assert se.nodes.tolist() == sr.nodes.tolist() and len(sr.nodes) == 1 and se.ifinal == sr.ifinal
    assert abs(se.score - sr.score) <= 1e-6 * max(1.0, abs(sr.score)) and np.all(np.isfinite(se.u))
    assert np.max(np.abs(se.u - sr.u)) <= 1e-7 and (storage != abi.STORE_F64_CSC or se.n_trials == sr.n_trials)
    # ... and a stored diagonal, which the reference would count once on top of the identity, is refused
    D = sp.csc_matrix(np.triu(M, 1) + np.diag(np.full(m, 0.25)))
    D.sort_indices()
    PD = sp.csc_matrix((np.ones_like(D.data), D.indices, D.indptr), shape=D.shape)
    with pytest.raises(abi.ClipperError):
        c.set_sparse_matrix_data(m, D.indptr, D.indices, D.data, PD.indptr, PD.indices, PD.data)
    r.set_sparse_matrix_data(m, D.indptr, D.indices, D.data, PD.indptr, PD.indices, PD.data)
    yM, _ = r.matvec(u0)
    assert np.allclose(yM, (np.triu(M, 1) + np.triu(M, 1).T) @ u0 + 0.25 * u0, rtol=1e-13, atol=1e-13)  # the oracle: once


@pytest.mark.parametrize("storage", [abi.STORE_F32, abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC])
def test_set_sparse_full_symmetric_input_counts_every_pair_once(storage):
    """A SpAffinity with BOTH triangles stored — which the reference accepts and reads the upper
    half of (selfadjointView<Upper>, clipper.cpp:194-271) — is the same matrix in every storage mode;
    where the two copies of a pair differ, the upper one counts."""
    import scipy.sparse as sp
    m = 300
    M, C = _random_symmetric(m, 0.1, seed=9)
    U = _upper_csc(M)
    P = sp.csc_matrix((np.ones_like(U.data), U.indices, U.indptr), shape=U.shape)
    a = abi.HipClipper(storage=storage)
    a.set_sparse_matrix_data(m, U.indptr, U.indices, U.data, P.indptr, P.indices, P.data)
    Ma, Ca = a.get_affinity_matrix(), a.get_constraint_matrix()
    F = sp.csc_matrix(M - np.diag(np.diag(M)))          # both triangles
    low = sp.csc_matrix(np.tril(M, -1) * 0.5)            # ... the lower copies carry other values
    F = sp.csc_matrix(sp.triu(F, 1) + low)
    F.sort_indices()
    PF = sp.csc_matrix((np.ones_like(F.data), F.indices, F.indptr), shape=F.shape)
    b = abi.HipClipper(storage=storage)
    b.set_sparse_matrix_data(m, F.indptr, F.indices, F.data, PF.indptr, PF.indices, PF.data)
    assert "below the diagonal" in b.last_error()     # the lower copies were ignored, and the caller is told
    assert b.storage_in_use == storage
    assert np.array_equal(b.get_affinity_matrix(), Ma)
    assert np.array_equal(b.get_constraint_matrix(), Ca)
    u0 = np.random.default_rng(1).random(m)
    sa, sb = a.solve(u0), b.solve(u0)
    assert sa.nodes.tolist() == sb.nodes.tolist() and sa.score == sb.score


def test_set_sparse_rejects_malformed_input():
    m = 50
    M, C = _random_symmetric(m, 0.2, seed=2)
    U = _upper_csc(M)
    ones = np.ones_like(U.data)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    ok = (m, U.indptr, U.indices, U.data, U.indptr, U.indices, ones)
    g.set_sparse_matrix_data(*ok)
    s0 = g.solve(np.ones(m))
    bad_ptr = U.indptr.copy()
    bad_ptr[5] = bad_ptr[6] + 1                      # decreasing
    bad_row = U.indices.copy()
    bad_row[3] = m                                   # out of range
    neg_row = U.indices.copy()
    neg_row[0] = -1
    first = U.indptr.copy()
    first[0] = 1
    for args in [(m, bad_ptr, U.indices, U.data, bad_ptr, U.indices, ones),
                 (m, U.indptr, bad_row, U.data, U.indptr, bad_row, ones),
                 (m, U.indptr, neg_row, U.data, U.indptr, neg_row, ones),
                 (m, first, U.indices, U.data, first, U.indices, ones)]:
        with pytest.raises(abi.ClipperError):
            g.set_sparse_matrix_data(*args)
        s1 = g.solve(np.ones(m))       # rejected before anything was touched: the old matrix is intact
        assert s1.nodes.tolist() == s0.nodes.tolist() and s1.score == s0.score
    # the same (row, column) stored twice (found while the lists are merged: no matrix afterwards)
    import scipy.sparse as sp
    dup_ptr = U.indptr.copy()
    col = int(np.argmax(np.diff(U.indptr) >= 1))
    at = int(U.indptr[col])
    dup_rows = np.insert(U.indices, at, U.indices[at])
    dup_vals = np.insert(U.data, at, U.data[at])
    dup_ptr[col + 1:] += 1
    with pytest.raises(abi.ClipperError):
        g.set_sparse_matrix_data(m, dup_ptr, dup_rows, dup_vals, dup_ptr, dup_rows, np.ones_like(dup_vals))
    with pytest.raises(abi.ClipperError):
        g.solve(np.ones(m))
    g.set_sparse_matrix_data(*ok)                       # and the context is still usable
    s2 = g.solve(np.ones(m))
    assert s2.nodes.tolist() == s0.nodes.tolist() and s2.score == s0.score


def test_set_sparse_large_without_a_dense_store():
    """m = 300 000 (BASELINE's last configuration): a dense fp32 store would be 360 GB — it cannot
    exist on one MI355X. 0.02 % density = 9 M stored entries upload, pack and multiply in
    O(nnz) memory; the product is checked against scipy."""
    import scipy.sparse as sp
    m = 300_000
    rng = np.random.default_rng(8)
    nnz = 9_000_000
    i = rng.integers(0, m, nnz)
    j = rng.integers(0, m, nnz)
    keep = i < j
    U = sp.csc_matrix((rng.uniform(0.1, 1.0, int(keep.sum())), (i[keep], j[keep])), shape=(m, m))
    U.sum_duplicates()
    U.sort_indices()
    ones = np.ones_like(U.data)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.set_sparse_matrix_data(m, U.indptr, U.indices, U.data, U.indptr, U.indices, ones)
    assert g.storage_in_use == abi.STORE_F32_CSC
    x = rng.random(m)
    yM, yC = g.matvec(x)
    S32 = sp.csc_matrix((U.data.astype(np.float32).astype(np.float64), U.indices, U.indptr), shape=(m, m))
    P = sp.csc_matrix((ones, U.indices, U.indptr), shape=(m, m))
    assert np.allclose(yM, S32 @ x + S32.T @ x, rtol=1e-12, atol=1e-12)
    assert np.allclose(yC, P @ x + P.T @ x, rtol=1e-12, atol=1e-12)
    s = g.solve(rng.random(m))
    assert len(s.nodes) >= 2 and np.isfinite(s.score)


_NOMEM_CHILD = r"""
import os, resource, sys
import numpy as np
sys.path.insert(0, {root!r})
from clipper_amd import _abi as abi
m = 11000
g = abi.HipClipper(storage=abi.STORE_F32_CSC)
# the strict upper triangle of a full m x m matrix: 60 M entries; the symmetric lists the library
# builds on the host from them (host vectors proportional to nnz) need > 1.4 GB
indptr = np.concatenate([[0], np.cumsum(np.arange(m, dtype=np.int64))])
indices = np.concatenate([np.arange(j, dtype=np.int32) for j in range(m)])
vals = np.full(indices.size, 0.5)
ones = np.ones(indices.size)
vm = 0
for line in open("/proc/self/status"):
    if line.startswith("VmSize:"):
        vm = int(line.split()[1]) * 1024
resource.setrlimit(resource.RLIMIT_AS, (vm + (256 << 20), vm + (256 << 20)))
lib = g.L
rc = lib.clipper_hip_set_sparse(g.h, m, abi._i64p(indptr), abi._ip(indices), abi._dp(vals),
                                abi._i64p(indptr), abi._ip(indices), abi._dp(ones))
print("RESULT", rc, lib.clipper_hip_last_error().decode(), flush=True)
os._exit(0)
"""


def test_set_sparse_out_of_host_memory_comes_back_as_an_error_code():
    """No exception crosses extern "C" (VERDICT r03 item 7): with the address space capped
    just above what the process already holds, the host vectors clipper_hip_set_sparse sizes by the
    caller's nnz cannot be allocated — std::bad_alloc is caught at the boundary and CLIPPER_HIP_E_NOMEM
    (-2) comes back; the process is alive to print it."""
    import subprocess, sys, os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", _NOMEM_CHILD.format(root=root)], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT")]
    assert lines, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
    assert lines[0].split()[1] == "-2", lines[0]
