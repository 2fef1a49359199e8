"""CPU checks of the reference that the device's user-defined-invariant fills are held to
(tests/custom_invariant_model.py; the device side is tests/test_gpu_custom_invariant_edges.py): the vectorised formulas
are a scalar transcription's bits, the model's pair rule is the oracle's, every GPU case holds the pairs and reaches the
geometry it claims, and the three sources compile at their dimensions (hiprtc needs no device)."""
import math

import numpy as np
import pytest

from clipper_amd import _abi as abi
from oracle import clipper_ref as ref
from tests import custom_invariant_model as cim


# ---- scalar transcriptions of the three device sources -------------------------------------------------------------

def _plant_py(p):
    def f(ai, aj, bi, bj):
        l = int(ai[0])
        if float(ai[0]) == float(aj[0]) and 1 <= l <= 15:
            return p[l]
        return p[0] / (1.0 + math.sqrt(abs((float(ai[1]) - float(bj[1])) * (float(aj[1]) + 0.25)))) - 0.3
    return f


def _wide_py(d, p):
    def f(ai, aj, bi, bj):
        s = u = 0.0
        for k in range(d):
            s = s + (float(ai[k]) - float(bj[k])) * (float(aj[k]) + p[k % 16])
            u = u + (float(bi[k]) - float(aj[k])) * (float(bj[k]) + p[(k + 5) % 16])
        t = math.sqrt((abs(s) + abs(u)) / d)
        return 1.0 / (1.0 + t) - 0.72
    return f


def _same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array_equal(a.view(np.uint64)[~np.isnan(a)], b.view(np.uint64)[~np.isnan(b)]) and \
        np.array_equal(np.isnan(a), np.isnan(b))


def _sampled(formula_np, formula_py, D1, D2, A, params, n=300, seed=0):
    i, j, s = cim.scores(formula_np, D1, D2, A, params)
    pick = np.random.default_rng(seed).choice(len(i), size=min(n, len(i)), replace=False)
    ai, aj, bi, bj = cim.pair_data(D1, D2, A, i[pick], j[pick])
    sc = [formula_py(ai[:, k], aj[:, k], bi[:, k], bj[:, k]) for k in range(len(pick))]
    assert _same_bits(s[pick], sc)
    return s[pick]


@pytest.mark.parametrize("which", list(cim.PLANT_SETS))
def test_plant_is_its_scalar_transcription(which):
    D1, D2, A, _ = cim.labelled_problem(cim.VALUE_M, cim.case_seed(cim.VALUE_M))
    prm, _ = cim.plant_params(which)
    s = _sampled(cim.plant_np, _plant_py(cim.pad_params(prm).tolist()), D1, D2, A, prm)
    assert np.count_nonzero(np.isnan(s)) > 0          # the sample reaches planted pairs (NaN among them) ...
    assert np.count_nonzero(np.abs(s - 0.1) < 0.2) > 100   # ... and generic ones


def test_plant_generic_value_is_asymmetric():
    D1, D2, A, _ = cim.labelled_problem(65, cim.case_seed(65))
    i, j = cim.distinct_pairs(A)
    prm = cim.pad_params(cim.plant_params("default")[0])
    fwd = cim.plant_np(*cim.pair_data(D1, D2, A, i, j), prm)
    bwd = cim.plant_np(*cim.pair_data(D1, D2, A, j, i), prm)
    generic = D1[0, A[i, 0]] != D1[0, A[j, 0]]
    assert np.count_nonzero(fwd[generic] != bwd[generic]) > 0.9 * np.count_nonzero(generic)


@pytest.mark.parametrize("prm", [cim.ASYM_PARAMS, [1.3, -0.1, 0.0, 0.55]])
def test_asym_is_its_scalar_transcription(prm):
    D1, D2, A, _ = cim.labelled_problem(350, cim.case_seed(350))
    _sampled(cim.asym_np, cim.asym_py(2, prm), D1, D2, A, prm)


@pytest.mark.parametrize("d", [16, 32])
def test_wide_is_its_scalar_transcription_and_reads_every_input(d):
    D1, D2, A = cim.wide_problem(cim.WIDE_M, d, cim.case_seed(d))
    _sampled(cim.wide_np, _wide_py(d, cim.WIDE_PARAMS), D1, D2, A, cim.WIDE_PARAMS)
    # one pair: the value moves with any single coordinate of any of the four data and with any single param
    i, j = (x[:1] for x in cim.distinct_pairs(A))
    data = [x.copy() for x in cim.pair_data(D1, D2, A, i, j)]
    p = cim.pad_params(cim.WIDE_PARAMS)
    base = cim.wide_np(*data, p)[0]
    for which in range(4):
        for k in range(d):
            moved = [x.copy() for x in data]
            moved[which][k] += 0.125
            assert cim.wide_np(*moved, p)[0] != base, (which, k)
    for k in range(16):
        q = p.copy()
        q[k] += 0.125
        assert cim.wide_np(*data, q)[0] != base, k
    fwd = cim.wide_np(*data, p)[0]
    assert cim.wide_np(data[1], data[0], data[3], data[2], p)[0] != fwd   # asymmetric under i <-> j


def test_the_store_rule_on_the_planted_values():
    v = dict(zip(cim.PLANT_KINDS, cim.plant_values(0.0)))
    M = np.array([[v["1e-46"], v["2^-150"], 2.0 ** -1074, v["1e-40"]], [v["sub_max"], v["flt_min"], 0.0, v["two"]]])
    S = cim.store_f32(M)
    assert S[0, 0] == S[0, 1] == S[0, 2] == cim.FLT_MIN       # rounds to 0 in fp32: kept as the smallest normal
    assert S[0, 3] == float(np.float32(1e-40)) and 0 < S[0, 3] < cim.FLT_MIN
    assert S[1, 0] == cim.SUB_MAX and S[1, 1] == cim.FLT_MIN and S[1, 2] == 0.0 and S[1, 3] == 2.0
    assert cim.SUB_MAX == cim.FLT_MIN - 2.0 ** -149


def test_the_pair_rule_is_the_oracles():
    """EuclideanDistance through the model against RefClipper, association indices repeating in both columns"""
    rng = np.random.default_rng(5)
    n1, n2, m = 14, 11, 90
    # coordinates on a grid of 2^-10: squares and their sums are exact, so the oracle's fma chains and numpy's plain
    # sums give the same lengths, and only the two exps can differ
    D1 = rng.integers(0, 1025, (3, n1)) / 1024.0
    D2 = D1[:, rng.permutation(n1)[:n2]] + rng.integers(-12, 13, (3, n2)) / 1024.0
    A = np.stack([rng.integers(0, n1, m), rng.integers(0, n2, m)], axis=1).astype(np.int32)
    assert len(np.unique(A[:, 0])) < m and len(np.unique(A[:, 1])) < m
    i, j = cim.distinct_pairs(A)
    assert 0 < len(i) < m * (m - 1) // 2
    sigma, epsilon = 0.05, 0.2
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(D1, D2, A, sigma=sigma, epsilon=epsilon, mindist=0.0)
    Mr, Cr = r.get_affinity_matrix(), r.get_constraint_matrix()
    off = ~np.eye(m, dtype=bool)
    M, Cm = cim.fill(cim.euclid_np, D1, D2, A, [sigma, epsilon, 0.0], r.params.affinityeps)
    assert np.all(np.diag(M) == 0) and np.array_equal(M, M.T)
    assert 0 < np.count_nonzero(M) < len(i) * 2
    assert np.array_equal((M != 0)[off], (Mr != 0)[off])
    assert np.array_equal(Cm[off], Cr[off])
    nz = (M != 0) & off
    assert np.all(np.abs(M[nz] - Mr[nz]) <= 4 * np.spacing(Mr[nz]))   # the suite's allowance between two exps


@pytest.mark.parametrize("which", list(cim.PLANT_SETS))
def test_value_case_holds_every_planted_kind(which):
    D1, D2, A, _ = cim.labelled_problem(cim.VALUE_M, cim.case_seed(cim.VALUE_M))
    prm, e = cim.plant_params(which)
    M, _ = cim.fill(cim.plant_np, D1, D2, A, prm, e)
    kept, pairs = cim.plant_kept(which), cim.planted_pairs(D1, A)
    counts = {}
    for kind, (i, j) in pairs.items():
        assert len(i) >= cim.MIN_PLANTED, kind
        assert np.all((M[i, j] != 0) == kept[kind]), kind
        counts[kind] = (len(i), "kept" if kept[kind] else "dropped")
    # what the keep rule's edges must do, whatever the set
    assert kept["eps_up"] and not kept["eps"] and not kept["eps_down"] and not kept["nan"] and not kept["neg_zero"]
    assert kept["1e-46"] == kept["sub_max"] == (e == 0.0)
    i, j, s = cim.scores(cim.plant_np, D1, D2, A, prm)
    generic = D1[0, A[i, 0]] != D1[0, A[j, 0]]
    frac = float(np.mean(s[generic] > e))
    assert (0.05 < frac < 0.15) if which == "sparse" else (0.9 < frac < 0.99)
    print(f"PLANT {which} m={cim.VALUE_M}: generic pairs kept {frac:.3f}; planted pairs {counts}")


def test_batch_and_tile_plant_cases_hold_planted_pairs():
    """the sizes large enough to claim planted kinds at all (m >= 1023) hold every one of them"""
    for m in [m for m in list(cim.TILE_CASES) + list(cim.BATCH_MS) if m >= 1023] + [2051]:
        D1, _, A, _ = cim.labelled_problem(m, cim.case_seed(m))
        counts = {k: len(v[0]) for k, v in cim.planted_pairs(D1, A).items()}
        assert min(counts.values()) >= cim.MIN_PLANTED, (m, counts)
        print(f"PLANT m={m}: planted pairs {counts}")


def test_every_case_reaches_the_geometry_it_claims():
    for m, claim in cim.TILE_CASES.items():
        g = cim.shard_geometry(m, 1)
        assert all(g[k] == v for k, v in claim.items()), (m, g)
        print(f"lone m={m}: {g}")
    for (m, shards), claim in cim.SHARD_CASES.items():
        g = cim.shard_geometry(m, shards)
        assert all(g[k] == v for k, v in claim.items()), (m, shards, g)
        print(f"m={m} on {shards} shards: {g}")
    g3 = {m: cim.shard_geometry(m, 3) for m in (127, 129, 1089)}
    assert g3[127]["valid"][-1] == 0 and g3[129]["valid"][-1] == 1          # an empty shard; one valid column
    assert len(set(g3[1089]["valid"])) > 1 and g3[1089]["c0"][1] != 0       # uneven, c0 not 0
    g2 = cim.shard_geometry(2051, 2)
    assert g2["column_blocks"] == 2 and g2["last_block_threads"] == 16      # a second column block inside a shard
    gw = cim.shard_geometry(cim.WIDE_M, 2)
    assert gw["valid"] == [128, 5]
    # the sizes straddle the strip of 32 rows, a shard width of 64 and the block of 1024 columns
    for edge, key in ((32, "row_strips"), (64, "W"), (1024, "column_blocks")):
        below, above = cim.shard_geometry(edge, 1), cim.shard_geometry(edge + 1, 1)
        assert below[key] < above[key] and cim.shard_geometry(edge - 1, 1)[key] == below[key]
        assert {edge - 1, edge, edge + 1} <= set(cim.TILE_CASES)


def test_small_cases_call_the_formula():
    """every size from 2 up holds at least one distinct-association pair, and the asymmetric formulas keep some pairs
    and drop some at the sizes where the pattern is compared as a whole"""
    for m in sorted(set(cim.TILE_CASES) | set(cim.BATCH_MS) | {m for m, _ in cim.SHARD_CASES}):
        D1, D2, A, _ = cim.labelled_problem(m, cim.case_seed(m))
        i, _ = cim.distinct_pairs(A)
        assert (len(i) >= 1) == (m >= 2), m
        if m >= 31:
            for formula, prm, e in ((cim.asym_np, cim.ASYM_PARAMS, 1e-4), (cim.plant_np, *cim.plant_params("default"))):
                M, _ = cim.fill(formula, D1, D2, A, prm, e)
                assert 0 < np.count_nonzero(M) < 2 * len(i), (m, formula.__name__)


@pytest.mark.parametrize("name,src,d", [("PLANT", cim.PLANT_SRC, 2), ("ASYM", cim.ASYM_SRC, 2),
                                        ("WIDE", cim.WIDE_SRC, 16), ("WIDE", cim.WIDE_SRC, 32)])
def test_the_sources_compile(name, src, d):
    with abi.HipInvariant(src, d) as inv:
        assert inv.h and inv.d == d
