"""Times the batched maximum-clique call (clipper_hip_batch_max_clique, DESIGN.md section 9 "Batches") against the loop
of lone clipper_hip_max_clique calls it replaces, on synthetic Euclidean problems with the bench parameters at 95 %
outliers (seeds 12345 + k), method EXACT. For every m and every P: one batched call (best of --reps after a warm-up)
with its launch count, and the loop of lone calls measured in the same run on the first min(P, --lone-cap) problems
(one lone context, scored again for each problem; only the clique calls are timed), both per problem in ms. Then the
case tests/test_gpu_batch_maxclique.py asserts a ratio on (64 problems, m cycling through 200 / 500 / 1000, seeds
5000 + k, every lone context scored beforehand, each route the best of 3 after a warm-up), and the unlimited batched
call on the batch of that file's time-limit test (8 problems of m = 2048 at 98 % outliers, sigma 0.1, epsilon
--tl-epsilon; capped by --tl-cap seconds so that a probe cannot run away). One JSON line per case.

  python tools/batch_maxclique_probe.py [--out profiles/batch_maxclique_probe.json] [--sizes 100,500,1000,2048]
                                        [--counts 1,16,64,256] [--reps 2] [--lone-cap 64] [--tl-epsilon 0.15]
                                        [--tl-cap 120]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402

INV = synth.EUCLID_BENCH_PARAMS
FIELDS = ("num_nodes", "max_core", "heuristic_size", "edges")


def same(a, b) -> bool:
    return all(x[0].tolist() == y[0].tolist() and all(getattr(x[1], f) == getattr(y[1], f) for f in FIELDS)
               for x, y in zip(a, b))


def case(m: int, probs, reps: int, lone_cap: int, lone_cache: dict) -> dict:
    P = len(probs)
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)
    b.max_clique(abi.MC_EXACT)  # (warm-up)
    walls, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = b.max_clique(abi.MC_EXACT)
        walls.append((time.perf_counter() - t0) * 1e3)
    launches, nb, na = b.max_clique_stats()
    b.close()
    nl = min(P, lone_cap)
    if nl not in lone_cache:  # (the first nl problems of every batch of this m are the same)
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        lone, ms = [], 0.0
        for k, p in enumerate(probs[:nl]):
            g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
            if k == 0:
                g.max_clique(abi.MC_EXACT)
            t0 = time.perf_counter()
            lone.append(g.max_clique(abi.MC_EXACT))
            ms += (time.perf_counter() - t0) * 1e3
        g.close()
        lone_cache[nl] = (ms, lone)
    lone_ms, lone = lone_cache[nl]
    return {"m": m, "problems": P, "outliers": 0.95, "method": "EXACT",
            "batch_ms_min": min(walls), "batch_ms_all": walls, "batch_ms_per_problem": min(walls) / P,
            "launches": launches, "n_batched": nb, "n_alone": na,
            "clique_min": min(len(n) for n, _ in res), "clique_max": max(len(n) for n, _ in res),
            "bb_nodes_sum": int(sum(i.bb_nodes for _, i in res)),
            "lone_problems": nl, "lone_loop_ms": lone_ms, "lone_ms_per_problem": lone_ms / nl,
            "batch_equals_lone": bool(same(res, lone)),
            "speedup_per_problem": (lone_ms / nl) / (min(walls) / P)}


def ratio_case() -> dict:
    ms = [200, 500, 1000]
    probs = [synth.make_euclidean_problem(ms[k % 3], 0.95, seed=5000 + k) for k in range(64)]
    ctxs = []
    for p in probs:
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
        ctxs.append(g)
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], **INV)

    def best(f):
        f()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts), r

    ta, ra = best(lambda: [g.max_clique(abi.MC_EXACT) for g in ctxs])
    tb, rb = best(lambda: b.max_clique(abi.MC_EXACT))
    launches = b.max_clique_stats()[0]
    for g in ctxs:
        g.close()
    b.close()
    return {"case": "ratio", "problems": 64, "m": ms, "outliers": 0.95, "method": "EXACT", "lone_loop_ms": ta,
            "batch_ms": tb, "ratio": tb / ta, "asserted_ratio": min(1.0, 4 * tb / ta), "launches": launches,
            "batch_equals_lone": bool(same(rb, ra))}


def time_limit_case(epsilon: float, cap: float) -> dict:
    probs = [synth.make_euclidean_problem(2048, 0.98, seed=s) for s in range(77, 85)]
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in probs], sigma=0.1, epsilon=epsilon, mindist=0.0)
    b.max_clique(abi.MC_HEU)  # (warm-up)
    t0 = time.perf_counter()
    res = b.max_clique(abi.MC_EXACT, time_limit=cap)
    wall = time.perf_counter() - t0
    launches = b.max_clique_stats()[0]
    t0 = time.perf_counter()
    lim = b.max_clique(abi.MC_EXACT, time_limit=0.05)
    wall_lim = time.perf_counter() - t0
    b.close()
    return {"case": "time_limit_batch", "problems": 8, "m": 2048, "outliers": 0.98, "sigma": 0.1, "epsilon": epsilon,
            "cap_s": cap, "unlimited_s": wall, "capped": int(sum(i.timed_out for _, i in res)), "launches": launches,
            "max_core": [i.max_core for _, i in res], "heuristic": [i.heuristic_size for _, i in res],
            "clique": [len(n) for n, _ in res], "bb_nodes": [int(i.bb_nodes) for _, i in res],
            "edges": [int(i.edges) for _, i in res],
            "limit_s": 0.05, "limited_wall_s": wall_lim, "limited_timed_out": [i.timed_out for _, i in lim],
            "limited_clique": [len(n) for n, _ in lim]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_maxclique_probe.json"))
    ap.add_argument("--sizes", default="100,500,1000,2048")
    ap.add_argument("--counts", default="1,16,64,256")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--lone-cap", type=int, default=64)
    ap.add_argument("--tl-epsilon", type=float, default=0.15)
    ap.add_argument("--tl-cap", type=float, default=120.0)
    a = ap.parse_args()
    counts = [int(x) for x in a.counts.split(",")]
    rows = []

    def emit(row):
        print(json.dumps(row), flush=True)
        rows.append(row)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:  # (rewritten after every case: a probe that is cut short leaves what it has)
            for r in rows:
                f.write(json.dumps(r) + "\n")

    emit(ratio_case())
    emit(time_limit_case(a.tl_epsilon, a.tl_cap))
    for m in [int(x) for x in a.sizes.split(",") if x]:
        probs = [synth.make_euclidean_problem(m, 0.95, seed=12345 + k) for k in range(max(counts))]
        lone_cache: dict = {}
        for P in counts:
            emit(case(m, probs[:P], a.reps, a.lone_cap, lone_cache))
    return 0


if __name__ == "__main__":
    sys.exit(main())
