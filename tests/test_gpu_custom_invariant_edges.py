"""The fills of a user-defined invariant (clipper_custom_fill_{f32,f64} and their batched twins,
k_custom_invariant_src.h; fill_custom, batch_fill_custom) against the plain numpy model of tests/custom_invariant_model.py,
at the value, tile and shard edges the built-in routes are already walked along. Every formula here is exactly rounded
(+ - * / sqrt fabs, -ffp-contract=off), so every comparison is exact: the bits of M in the fp64 storages, the model's
fp32 rule (float32(score), FLT_MIN where that is 0) in the fp32 storages; always C == pattern(M), M == M.T and, since
the getter adds the implicit identity, a diagonal of exactly 1 over a stored diagonal of 0.
tests/test_custom_invariant_model.py checks without a device that every case here holds the pairs and reaches the
geometry it is there for."""
import functools

import numpy as np
import pytest

from clipper_amd import _abi as abi
from oracle import clipper_ref as ref
from tests import custom_invariant_model as cim
from tests.test_gpu_batch import _assert_bits

pytestmark = pytest.mark.gpu

STORAGES = [abi.STORE_F32, abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC]
F64S = (abi.STORE_F64, abi.STORE_F64_CSC)
CSCS = (abi.STORE_F32_CSC, abi.STORE_F64_CSC)
FORMULAS = {"ASYM": cim.asym_np, "PLANT": cim.plant_np}


@pytest.fixture(scope="module")
def invs():
    """every source compiled once"""
    out = {"ASYM": abi.HipInvariant(cim.ASYM_SRC, 2), "PLANT": abi.HipInvariant(cim.PLANT_SRC, 2),
           16: abi.HipInvariant(cim.WIDE_SRC, 16), 32: abi.HipInvariant(cim.WIDE_SRC, 32)}
    yield out
    for inv in out.values():
        inv.close()
    _model.cache_clear()   # (the shared references go with the module's last test)
    _problem.cache_clear()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _problem(m):
    return _frozen(*cim.labelled_problem(m, cim.case_seed(m)))


def _setting(name, which="default"):
    """(params, affinityeps) of a formula's fill"""
    return cim.plant_params(which) if name == "PLANT" else (cim.ASYM_PARAMS, 1e-4)


@functools.lru_cache(maxsize=None)
def _model(name, m, which="default"):
    """the model's M (fp64 and as an fp32 storage holds it) and C, identity on the diagonal as the getters give it;
    computed once per case, shared, never written"""
    D1, D2, A, _ = _problem(m)
    prm, e = _setting(name, which)
    M, Cm = cim.fill(FORMULAS[name], D1, D2, A, prm, e)
    eye = np.eye(m)
    return _frozen(M + eye, cim.store_f32(M) + eye, Cm + eye)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _where(bad):
    idx = np.argwhere(bad)
    return f"{len(idx)} entries, first {idx[:4].tolist()}"


def _assert_matrix(g, want64, want32, wantC, storage, what):
    """the device's M and C against the model: exact, bits included"""
    Mg, Cg = g.get_affinity_matrix(), g.get_constraint_matrix()
    want = want64 if storage in F64S else want32
    assert np.array_equal(_bits(Mg), _bits(want)), f"{what}: M differs from the model at {_where(Mg != want)}"
    assert np.array_equal(Cg, wantC), f"{what}: C differs at {_where(Cg != wantC)}"
    assert np.array_equal(Cg, (Mg != 0).astype(np.float64)), f"{what}: C is not the pattern of M"
    assert np.array_equal(Mg, Mg.T), f"{what}: M is not symmetric"
    assert np.all(np.diag(Mg) == 1.0), f"{what}: the stored diagonal is not 0"
    return Mg


def _filled(inv, m, prm, e, storage, group=None):
    D1, D2, A, _ = _problem(m)
    g = abi.HipClipper(abi.Params(affinityeps=e), storage=storage, group=group)
    g.affinity_custom(inv, D1, D2, A, prm)
    return g


# ---- 1. value edges ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", list(cim.PLANT_SETS))
@pytest.mark.parametrize("storage", STORAGES)
def test_value_edges(invs, storage, which):
    m = cim.VALUE_M
    D1, _, A, _ = _problem(m)
    prm, e = _setting("PLANT", which)
    g = _filled(invs["PLANT"], m, prm, e, storage)
    Mg = _assert_matrix(g, *_model("PLANT", m, which), storage, f"PLANT {which}, storage {storage}")
    g.close()
    kept, values = cim.plant_kept(which), dict(zip(cim.PLANT_KINDS, cim.plant_values(e)))
    got = {}
    for kind, (i, j) in cim.planted_pairs(D1, A).items():
        assert len(i) >= cim.MIN_PLANTED
        v = Mg[i, j]
        assert np.all((v != 0) == kept[kind]), f"{kind}: kept {np.count_nonzero(v)} of {len(v)}, the model keeps " \
                                               f"{'all' if kept[kind] else 'none'}"
        assert np.all(v == v[0]) and np.array_equal(v, Mg[j, i])
        got[kind] = float(v[0])
    assert got["eps_up"] != 0 and got["eps"] == 0 and got["eps_down"] == 0 and got["nan"] == 0
    assert got["zero"] == 0 and got["neg_zero"] == 0 and got["minus_one"] == 0
    assert got["one"] == 1.0 and got["two"] == 2.0
    if e == 0.0:   # everything positive is kept, 2^-1074 included
        if storage in F64S:
            assert got["eps_up"] == 2.0 ** -1074
            for kind in ("1e-46", "2^-150", "1e-40", "flt_min", "sub_max"):
                assert got[kind] == values[kind], kind
        else:
            assert got["eps_up"] == cim.FLT_MIN and got["1e-46"] == cim.FLT_MIN and got["2^-150"] == cim.FLT_MIN
            assert got["1e-40"] == float(np.float32(1e-40)) and got["sub_max"] == cim.SUB_MAX
            assert got["flt_min"] == cim.FLT_MIN
    else:          # 1e-4: the scores below fp32's normals are below affinityeps too
        assert got["eps_up"] == (values["eps_up"] if storage in F64S else float(np.float32(values["eps_up"])))
        for kind in ("1e-46", "2^-150", "1e-40", "flt_min", "sub_max", "eps_half"):
            assert got[kind] == 0, kind


# ---- 2. tile edges, lone fill --------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", list(cim.TILE_CASES))
def test_tile_edges_lone_fill(invs, m):
    storages = STORAGES if m in cim.TILE_ALL_STORAGES else [abi.STORE_F64, abi.STORE_F32_CSC]
    x = np.random.default_rng(m).random(m) + 0.5
    for name in ("ASYM", "PLANT"):
        prm, e = _setting(name)
        M64, M32, Cm = _model(name, m)
        eye = np.eye(m)
        oM, oC = (M64 - eye) @ x, (Cm - eye) @ x
        for storage in storages:
            g = _filled(invs[name], m, prm, e, storage)
            _assert_matrix(g, M64, M32, Cm, storage, f"{name} m={m}, storage {storage}")
            if storage in CSCS:   # the slices built from the dense store (tolerances: tests/test_gpu_fill_boundaries.py)
                yM, yC = g.matvec(x)
                assert np.max(np.abs(yC - oC)) <= 1e-12 * max(1.0, float(np.max(np.abs(oC))))
                tol = 1e-12 if storage == abi.STORE_F64_CSC else 2e-7
                assert np.max(np.abs(yM - oM)) <= tol * max(1.0, float(np.max(np.abs(oM))))
            g.close()


# ---- 3. column shards with an asymmetric formula -------------------------------------------------------------------

@pytest.mark.parametrize("m", sorted({m for m, _ in cim.SHARD_CASES}))
def test_column_shards_with_an_asymmetric_formula(invs, m):
    for name in ("ASYM", "PLANT"):
        prm, e = _setting(name)
        want = _model(name, m)
        for storage in (abi.STORE_F64, abi.STORE_F32_CSC):
            g1 = _filled(invs[name], m, prm, e, storage)
            M1 = _assert_matrix(g1, *want, storage, f"{name} m={m}, storage {storage}, one shard")
            g1.close()
            for shards in (2, 3):
                assert (m, shards) in cim.SHARD_CASES
                g = _filled(invs[name], m, prm, e, storage, group=[0] * shards)
                what = f"{name} m={m}, storage {storage}, {shards} shards"
                Mk = _assert_matrix(g, *want, storage, what)
                assert np.array_equal(_bits(Mk), _bits(M1)), f"{what}: differs from the one-shard fill"
                g.close()


# ---- 4. wide data and all parameters -------------------------------------------------------------------------------

def _wide_want(D1, D2, A, prm):
    M, Cm = cim.fill(cim.wide_np, D1, D2, A, prm, 1e-4)
    eye = np.eye(len(A))
    return M + eye, cim.store_f32(M) + eye, Cm + eye


@pytest.mark.parametrize("d", [16, 32])
def test_wide_data_and_all_parameters(invs, d):
    m = cim.WIDE_M
    D1, D2, A = cim.wide_problem(m, d, cim.case_seed(d))
    prm = list(cim.WIDE_PARAMS)
    first = _wide_want(D1, D2, A, prm)
    assert 0.2 * m * m < np.count_nonzero(first[0]) < 0.9 * m * m
    # one parameter behind params[3] and one coordinate in the second half of a datum that the list uses
    prm2, D1b = list(prm), D1.copy()
    prm2[4 + d % 11] += 0.25
    D1b[d - 3, A[m // 2, 0]] += 0.5
    second = _wide_want(D1b, D2, A, prm2)
    assert np.count_nonzero(second[0] != first[0]) > m
    for storage in (abi.STORE_F64, abi.STORE_F32):
        for group in (None, [0, 0]):
            what = f"WIDE d={d}, storage {storage}, group {group}"
            g = abi.HipClipper(storage=storage, group=group)
            g.affinity_custom(invs[d], D1, D2, A, prm)
            Ma = _assert_matrix(g, *first, storage, what)
            g.affinity_custom(invs[d], D1b, D2, A, prm2)   # the same context and the same compiled handle
            Mb = _assert_matrix(g, *second, storage, what + ", refill")
            assert np.count_nonzero(Ma != Mb) > m
            g.close()


# ---- 5. staged refills across handles ------------------------------------------------------------------------------

@pytest.mark.parametrize("storage", STORAGES)
def test_staged_refills_across_handles(invs, storage):
    """one context, its inputs staged once: every refill is a fresh context's fill. affinityeps travels with each
    call (Params.affinityeps of the context at that moment), so the third step sets it to 0 on the same context; the
    fresh context it is compared with is created with Params(affinityeps=0)."""
    m = cim.VALUE_M
    D1, D2, A, _ = _problem(m)
    g = abi.HipClipper(storage=storage)
    g.stage_inputs(D1, D2, A)
    seen = []
    for step, (name, which) in enumerate((("PLANT", "default"), ("ASYM", "default"), ("PLANT", "eps0"),
                                          ("PLANT", "default"))):
        prm, e = _setting(name, which)
        g.params = abi.Params(affinityeps=e)
        g.affinity_custom_staged(invs[name], prm)
        what = f"step {step}: {name} {which}, storage {storage}"
        Ms = _assert_matrix(g, *_model(name, m, which), storage, what)
        fresh = _filled(invs[name], m, prm, e, storage)
        assert np.array_equal(_bits(Ms), _bits(fresh.get_affinity_matrix())), f"{what}: differs from a fresh context"
        assert np.array_equal(g.get_constraint_matrix(), fresh.get_constraint_matrix()), what
        fresh.close()
        seen.append(Ms)
    assert np.array_equal(_bits(seen[0]), _bits(seen[3]))
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])
    g.close()


# ---- 6. batch ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["PLANT", "ASYM"])
@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64])
def test_batch_against_lone_model_and_oracle(invs, storage, name):
    """one solve_custom call over sizes on the strip, shard-width and column-block edges. A batch exposes no matrix:
    every problem's solution is the lone context's bit for bit (the same route: tests/test_gpu_batch_custom.py), that
    lone context's M is the model's, and on the fp64 storage the oracle solving the model's M selects the same nodes."""
    prm, e = _setting(name)
    probs = [_problem(m) for m in cim.BATCH_MS]
    b = abi.HipBatch(storage=storage)
    sols = b.solve_custom(invs[name], probs, prm, solver_params=abi.Params(affinityeps=e))
    g = abi.HipClipper(abi.Params(affinityeps=e), storage=storage)
    for k, (m, (D1, D2, A, u0), sb) in enumerate(zip(cim.BATCH_MS, probs, sols)):
        g.affinity_custom(invs[name], D1, D2, A, prm)
        M64, M32, Cm = _model(name, m)
        what = f"{name} problem {k} (m={m}), storage {storage}"
        _assert_matrix(g, M64, M32, Cm, storage, what)
        sl = g.solve(u0)
        assert b.route(k) == g.last_solver, f"{what}: batch route {b.route(k)}, lone {g.last_solver}"
        _assert_bits(sb, sl, what)
        assert np.array_equal(b.selected_associations(k), g.get_selected_associations()), what
        if storage == abi.STORE_F32_CSC:
            # the slices are built from the whole pitch of the dense store: they hold M's entries and nothing else
            # only if the fill wrote its padding columns [m, W) as zeros (4 value bytes + 1 row byte per entry)
            entries = g.timings().gemv_useful_bytes / 5.0
            assert entries == np.count_nonzero(M64) - m, f"{what}: the slices hold {entries} entries"
        if storage == abi.STORE_F64:
            r = ref.RefClipper(ref.Params(affinityeps=e))
            r.set_matrix_data(M64, Cm)
            sr = r.solve(u0)
            assert sorted(sb.nodes.tolist()) == sorted(sr.nodes.tolist()), f"{what}: node set differs from the oracle"
    g.close()
    b.close()
