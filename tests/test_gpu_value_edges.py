"""Handed-over matrices at fp32's value edges (tests/value_edges.py) on every route of the two setters: what the store
holds, what the getters return and what the products read — against value_edges.held, the stored-value rule of
DESIGN.md 2d in numpy. tests/test_value_edges_cpu.py shows on the CPU what entitles this file to equality.

Every case runs on set_matrix_data and set_sparse_matrix_data x the four storages x 1, 2 and 3 column shards (at m = 65
the third shard owns no column); the "-explicitC" cases are the explicit constraint matrix. Bars:
  routing       storage_in_use: slices only with C == pattern(M), else the dense store of the same width
  matrices      get_affinity_matrix() == held(M, storage) and get_constraint_matrix() == C (the pattern of the fp64 M, or
                the explicit C), np.array_equal: every setter is a single cast
  e_j products  yM == column j of the held off-diagonal matrix, yC == column j of C_off, np.array_equal: one product
                with 1.0 and additions of zeros are exact in any order
  dyadic x      x_j = k_j 2^-10, k_j integer in [1, 1024]: yC exact (sums of such numbers over fewer than 2^40 terms are
                exact in any order); |yM_i - fsum_j(M_ij x_j)| <= (n_i + 2) 2^-53 sum_j |M_ij x_j| + n_i 2^-1074 with n_i the
                stored entries of row i: the any-order summation bound with one rounding per product, plus a floor for
                subnormal results — derived, not measured, no margin on top
  afterwards    an ordinary matrix in the same context solves as the oracle does
The solve case "tinyedge" is compared with the oracle on (held M, pattern of the fp64 M) under the bars of
tests/test_gpu_degenerate.py. The last tests: the setters' refusals of non-finite values and of values that round to
fp32 infinity, and the routes that were reached."""
import collections
import math

import numpy as np
import pytest

from clipper_amd import _abi as abi
from oracle import clipper_ref as ref
from tests import degenerate_cases as dc
from tests import value_edges as ve
from tests.test_gpu_degenerate import _check
from tests.test_gpu_parity import F64S, STORAGES

pytestmark = pytest.mark.gpu
ROUTES = collections.Counter()
RAN = set()
SETTERS = ("dense", "sparse")
_CACHE = {}

assert (abi.STORE_F32, abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC) == \
    (ve.STORE_F32, ve.STORE_F64, ve.STORE_F32_CSC, ve.STORE_F64_CSC) and tuple(F64S) == ve.F64S


def _context(storage, shards):
    return abi.HipClipper(storage=storage) if shards == 1 else abi.HipClipper(storage=storage, group=[0] * shards)


def _load(g, c, setter):
    if setter == "sparse":
        g.set_sparse_matrix_data(*c.upper_csc())
    else:
        g.set_matrix_data(*c.dense())


def _expected_storage(storage, explicit):
    """slices only with C == pattern(M); else the dense store of the same width"""
    if not explicit:
        return storage
    return abi.STORE_F64 if storage in F64S else abi.STORE_F32


def _dyadic_x(m):
    return np.random.default_rng(5 + m).integers(1, 1025, m) * 2.0 ** -10


def _expected(c, storage):
    """per (case, value width), computed once: held matrices, their off-diagonal parts, the dense product's reference
    and bound"""
    key = (c.name, storage in F64S)
    if key not in _CACHE:
        Mh, Ce = ve.expected_matrices(c, storage)
        Moff, Coff = Mh - np.eye(c.m), Ce - np.eye(c.m)
        x = _dyadic_x(c.m)
        yM = np.array([math.fsum((Moff[i] * x).tolist()) for i in range(c.m)])     # (each product: one rounding)
        n = np.count_nonzero(Moff, axis=1)
        bound = (n + 2) * 2.0 ** -53 * (np.abs(Moff) @ x) + n * 2.0 ** -1074
        yC = Coff @ x       # exact: dyadic terms, a few hundred of them
        _CACHE[key] = dict(M=Mh, C=Ce, Moff=Moff, Coff=Coff, x=x, yM=yM, bound=bound, yC=yC, cols=ve.probe_columns(c))
    return _CACHE[key]


def _ordinary_oracle():
    if "ordinary" not in _CACHE:
        o = dc.two_cliques(40, 7, 5)
        r = ref.RefClipper()
        r.set_sparse_matrix_data(*o.upper_csc())
        _CACHE["ordinary"] = (o, r.solve(o.u0))
    return _CACHE["ordinary"]


def _where(bad):
    idx = np.argwhere(bad)
    return f"{len(idx)} entries, the first {idx[:6].tolist()}"


@pytest.mark.parametrize("shards", (1, 2, 3))
@pytest.mark.parametrize("case", ve.cases(), ids=lambda c: c.name)
def test_stored_values_constraints_and_products(case, shards):
    c, local = case, collections.Counter()
    RAN.add("edges")
    W = (((c.m + shards - 1) // shards + 63) // 64) * 64      # a shard's columns: ceil(m / shards) rounded up to 64
    for storage in STORAGES:
        e = _expected(c, storage)
        for setter in SETTERS:
            what = f"{c.name}: {setter} setter, storage {storage}, {shards} shard(s)"
            g = _context(storage, shards)
            _load(g, c, setter)
            in_use = g.storage_in_use
            assert in_use == _expected_storage(storage, c.explicit_c), f"{what}: storage in use {in_use}"
            Mg, Cg = g.get_affinity_matrix(), g.get_constraint_matrix()
            assert np.array_equal(Mg, e["M"]), f"{what}: affinity matrix differs from held: {_where(Mg != e['M'])}"
            assert np.array_equal(Cg, e["C"]), f"{what}: constraint matrix differs: {_where(Cg != e['C'])}"
            for j in e["cols"]:
                x = np.zeros(c.m)
                x[j] = 1.0
                yM, yC = g.matvec(x)
                assert np.array_equal(yM, e["Moff"][:, j]), f"{what}: M e_{j} differs: {_where(yM != e['Moff'][:, j])}"
                assert np.array_equal(yC, e["Coff"][:, j]), f"{what}: C e_{j} differs: {_where(yC != e['Coff'][:, j])}"
            yM, yC = g.matvec(e["x"])
            assert np.array_equal(yC, e["yC"]), f"{what}: C x differs: {_where(yC != e['yC'])}"
            err = np.abs(yM - e["yM"])
            assert np.all(err <= e["bound"]), f"{what}: M x beyond the bound: {_where(err > e['bound'])}, " \
                                              f"worst {np.max(err / e['bound']):.3g} of it"
            # nothing of the edge matrix may stay behind: an ordinary matrix in the same context
            o, so = _ordinary_oracle()
            _load(g, o, setter)
            _check(g.solve(o.u0), so, o, storage, f"an ordinary matrix after {what}", g)
            g.close()
            route = f"{setter} setter -> {'slices' if in_use in (abi.STORE_F32_CSC, abi.STORE_F64_CSC) else 'dense store'}"
            for r in [route] + (["explicit C"] if c.explicit_c else []) + (["a shard without columns"] if (shards - 1) * W >= c.m else []):
                local[r] += 1
                ROUTES[r] += 1
    print(f"{c.name}, {shards} shard(s): routes {dict(local)}")


def _tinyedge_oracle(storage):
    key = ("tinyedge", storage in F64S)
    if key not in _CACHE:
        c = ve.tinyedge(**ve.TINYEDGE)
        h = ve.held_case(c, storage)      # (the lists of C: the pattern of the fp64 M — held keeps every entry)
        assert np.all(h.Mv != 0)
        r = ref.RefClipper()
        r.set_sparse_matrix_data(*h.upper_csc())
        _CACHE[key] = (c, r.solve(c.u0))
    return _CACHE[key]


@pytest.mark.parametrize("shards", (1, 2))
@pytest.mark.parametrize("setter", SETTERS)
@pytest.mark.parametrize("storage", STORAGES)
def test_tinyedge_solves_as_the_oracle_on_the_held_matrix(storage, setter, shards):
    RAN.add("tinyedge")
    c, sr = _tinyedge_oracle(storage)
    g = _context(storage, shards)
    _load(g, c, setter)
    Mh, Ce = ve.expected_matrices(c, storage)
    assert np.array_equal(g.get_affinity_matrix(), Mh) and np.array_equal(g.get_constraint_matrix(), Ce)
    sg = g.solve(c.u0)
    _check(sg, sr, c, storage, f"{setter} setter, storage {storage}, {shards} shard(s)", g)
    ROUTES[f"tinyedge, {setter} setter"] += 1
    print(f"tinyedge storage {storage} {setter} setter {shards} shard(s): trials {sg.n_trials} (oracle {sr.n_trials}) "
          f"nodes {sorted(sg.nodes.tolist())} solver {g.last_solver} storage in use {g.storage_in_use}")
    g.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------

def _with_value(c, pos, v, in_c=False):
    """the dense (M, C) and the CSC lists of the case with the value v at pos (an entry the case holds)"""
    M, C = c.dense()
    (C if in_c else M)[pos] = v       # (the upper triangle alone: the lower one is never read)
    a = list(c.upper_csc())
    k = int(np.nonzero((c.Mi == pos[0]) & (c.Mj == pos[1]))[0][0])
    vals = a[6 if in_c else 3].copy()
    vals[k] = v
    a[6 if in_c else 3] = vals
    return (M, C), tuple(a)


@pytest.mark.parametrize("setter", SETTERS)
@pytest.mark.parametrize("storage", STORAGES)
def test_setters_refuse_values_no_storage_can_hold(storage, setter):
    RAN.add("refusals")
    c = dc.weights_tiefill(65, 0.3)
    k = c.Mv.size // 2
    pos = (int(c.Mi[k]), int(c.Mj[k]))
    f32 = storage not in F64S
    g = _context(storage, 1)
    _load(g, c, setter)
    s0 = g.solve(c.u0)
    M0 = g.get_affinity_matrix()

    def hand_over(v, in_c=False):
        dense, sparse = _with_value(c, pos, v, in_c)
        if setter == "sparse":
            g.set_sparse_matrix_data(*sparse)
        else:
            g.set_matrix_data(*dense)

    refused = [(np.nan, False, "M", "is not finite"), (np.inf, False, "M", "is not finite"), (-np.inf, False, "M", "is not finite"),
               (np.nan, True, "C", "is not finite"), (np.inf, True, "C", "is not finite")]
    first_inf = float.fromhex("0x1.ffffffp+127")      # FLT_MAX plus half its last place: rounds to fp32 infinity
    if f32:
        refused += [(first_inf, False, "M", "rounds to infinity in fp32 storage"), (-1e39, False, "M", "rounds to infinity in fp32 storage")]
    for v, in_c, name, text in refused:
        with pytest.raises(abi.ClipperError) as err:
            hand_over(v, in_c)
        msg = str(err.value)
        assert f"{name}: entry ({pos[0]},{pos[1]})" in msg and text in msg and "clipper_hip error -1:" in msg, msg
        s1 = g.solve(c.u0)      # refused before anything was touched: the matrix held is intact
        assert s1.nodes.tolist() == s0.nodes.tolist() and s1.score == s0.score and np.array_equal(s1.u, s0.u), (v, in_c)
    assert np.array_equal(g.get_affinity_matrix(), M0)
    # accepted: the last double below that tie and FLT_MAX (1 + 2^-25) on every storage; 1e39 where the values are fp64
    for v in [math.nextafter(first_inf, 0.0), -ve.FLT_MAX * (1.0 + 2.0 ** -25)] + ([] if f32 else [first_inf, 1e39]):
        hand_over(v)
        got = g.get_affinity_matrix()[pos]
        assert got == float(ve.held(v, storage)) and np.isfinite(got), (v, got)
    if setter == "dense":       # the diagonal and the lower triangle are never read: whatever they hold
        M, C = c.dense()
        M[np.tril_indices(c.m)] = np.nan
        C[np.tril_indices(c.m, -1)] = np.inf
        g.set_matrix_data(M, C)
        assert np.array_equal(g.get_affinity_matrix(), M0)
    _load(g, c, setter)
    s2 = g.solve(c.u0)
    assert s2.nodes.tolist() == s0.nodes.tolist() and s2.score == s0.score
    ROUTES["refusals"] += 1
    g.close()


def test_every_route_was_reached():
    """(the last test of the file: what the tests above logged; it asks for nothing where only a part of the file ran)"""
    print("routes reached:", dict(sorted(ROUTES.items())))
    if RAN != {"edges", "tinyedge", "refusals"}:
        return
    for route in ("dense setter -> slices", "dense setter -> dense store", "sparse setter -> slices",
                  "sparse setter -> dense store", "explicit C", "a shard without columns"):
        assert ROUTES[route] >= 1, f"route never reached: {route}"
