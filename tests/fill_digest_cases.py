"""The cases behind tests/golden/fill_route_digests.json: sha256 digests of what every affinity fill route writes, recorded
once (tools/fill_digests.py) and asserted by tests/test_gpu_fill_digests.py, so that a change to the fill kernels that
moves a single bit of a score shows up without an oracle's tolerance in between.

Inputs come from clipper_amd.synth with fixed seeds at m = 300: three 128-tiles per side with a ragged last one, more
than 256 columns (the compacting kernel's second wave is partly outside), 9 row blocks of 32 plus 12 rows (one full and
one ragged group of AFF_RG). The 2-D case keeps the first two coordinates of the 3-D problem, the 4-D case (the
run-time-dimension path) appends the product of the first two as a fourth. 80 % outliers: every case has rejected and
surviving pairs (`digests` asserts 0 < nnz < m (m - 1)).
"""
import hashlib
import os

import numpy as np

from clipper_amd import _abi as abi
from clipper_amd import synth

M = 300
RHO = 0.8
STORAGE_NAMES = {abi.STORE_F32: "F32", abi.STORE_F64: "F64", abi.STORE_F32_CSC: "F32_CSC", abi.STORE_F64_CSC: "F64_CSC"}
VIEW_STORAGES = (abi.STORE_F32_CSC, abi.STORE_F64_CSC)


def cases():
    """name -> (problem, route dimension, pointnormal, invariant parameters)"""
    p3 = synth.make_euclidean_problem(M, RHO, seed=31001)
    p2 = synth.Problem(D1=np.ascontiguousarray(p3.D1[:2]), D2=np.ascontiguousarray(p3.D2[:2]), A=p3.A, Agt=p3.Agt,
                       u0=p3.u0, meta=p3.meta)
    p4 = synth.Problem(D1=np.ascontiguousarray(np.vstack([p3.D1, p3.D1[0] * p3.D1[1]])),
                       D2=np.ascontiguousarray(np.vstack([p3.D2, p3.D2[0] * p3.D2[1]])), A=p3.A, Agt=p3.Agt, u0=p3.u0,
                       meta=p3.meta)
    pn = synth.make_pointnormal_problem(M, RHO, seed=31002)
    e = dict(synth.EUCLID_BENCH_PARAMS)
    return {
        "euclid_d2": (p2, 2, False, e),
        "euclid_d3": (p3, 3, False, e),
        "euclid_d4": (p4, 4, False, e),
        "euclid_d3_mindist": (p3, 3, False, dict(e, mindist=0.25)),
        "pointnormal_d6": (pn, 3, True, dict(sigp=0.5, epsp=0.5, sign=0.10, epsn=0.35)),
    }


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _fill(g, p, pointnormal, prm):
    if pointnormal:
        g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, **prm)
    else:
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **prm)


def _set_mode(mode):
    if mode == "sym":
        os.environ.pop("CLIPPER_HIP_AFFINITY", None)
    else:
        os.environ["CLIPPER_HIP_AFFINITY"] = mode


def digests(routes):
    """{key: sha256}: for every case, M and C of every (storage, shards, mode) route that `routes(d)` lists, and — where
    a rectangular fill exists — clipper_hip_view_matvec on a seeded row subset for two seeded vectors."""
    out = {}
    saved = os.environ.get("CLIPPER_HIP_AFFINITY")
    try:
        for name, (p, d, pointnormal, prm) in cases().items():
            for storage, n, mode in routes(d):
                _set_mode(mode)
                g = abi.HipClipper(storage=storage, group=[0] * n if n > 1 else None)
                _fill(g, p, pointnormal, prm)
                Mg, Cg = g.get_affinity_matrix(), g.get_constraint_matrix()
                g.close()
                nnz = int(np.count_nonzero(Mg))
                assert 0 < nnz < M * (M - 1), (name, nnz)
                key = f"{name}/{STORAGE_NAMES[storage]}/shards{n}/{mode}"
                out[key + "/M"] = _sha(Mg)
                out[key + "/C"] = _sha(Cg)
            _set_mode("sym")
            if d in (2, 3):
                rng = np.random.default_rng(77)
                rows = np.sort(rng.permutation(M)[:97]).astype(np.int32)
                xs = [rng.random(M) + 0.5, rng.standard_normal(M)]
                for storage in VIEW_STORAGES:
                    g = abi.HipClipper(storage=storage)
                    _fill(g, p, pointnormal, prm)
                    for k, x in enumerate(xs):
                        yM, yC = g.view_matvec(rows, x)
                        out[f"{name}/{STORAGE_NAMES[storage]}/view/x{k}"] = _sha(np.concatenate([yM, yC]))
                    g.close()
    finally:
        if saved is None:
            os.environ.pop("CLIPPER_HIP_AFFINITY", None)
        else:
            os.environ["CLIPPER_HIP_AFFINITY"] = saved
    return out
