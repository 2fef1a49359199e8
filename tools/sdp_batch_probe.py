"""Times the batched semidefinite relaxation (clipper_hip_sdp_solve_batch, DESIGN.md section 11 "Batches") against the
loop of lone calls it replaces, on synthetic Euclidean problems with the bench parameters (70 % outliers, eps 1e-3:
the settings of tools/sdp_probe.py). For every n and every P problems (seeds 12345 + k): one batched call (best of
--reps after a warm-up) with its split setup / iterate / extract, the loop of clipper_hip_sdp_solve calls measured in
the same run, and for P <= 64 the numpy model of tests/sdp_model.py on the host. The loop of lone calls is measured on
the first min(P, --lone-cap) problems of the batch (at n = 128 a lone call takes most of a second) and reported per
problem; `lone_problems` says how many were timed. One JSON line per case.

  python tools/sdp_batch_probe.py [--out profiles/sdp_batch_probe.json] [--sizes 20,64,96,128]
                                  [--counts 1,16,64,256,1024] [--reps 2] [--lone-cap 64]
  python tools/sdp_batch_probe.py --floor-only             only the last line of the file, appended to it: the case
                                                          tests/test_gpu_sdp_batch.py asserts a floor on (64 problems
                                                          of n = 64, seeds 1000 + k, eps 1e-4, at most 100 iterations;
                                                          each route best of 3 after a warm-up)
  python tools/sdp_batch_probe.py --trace-case 64,256     one lone call, then one batched call, nothing timed:
                                                          the program to put behind `rocprofv3 --kernel-trace --stats --`
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402
from tests import sdp_model as sm  # noqa: E402

EPS = 1e-3


def problems(n: int, count: int):
    out = []
    g = abi.HipClipper(storage=abi.STORE_F64)
    for k in range(count):
        p = synth.make_euclidean_problem(n, 0.7, seed=12345 + k)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
        out.append((g.get_affinity_matrix(), g.get_constraint_matrix()))
    g.close()
    return out


def case(n: int, probs, reps: int, lone_cap: int, lone_cache: dict) -> dict:
    P = len(probs)
    prm = abi.SdpParams(eps_abs=EPS, eps_rel=EPS, max_iters=20000)
    abi.sdp_solve_batch(probs, prm, want_xy=False)  # (warm-up: module load, LDS attribute)
    walls, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = abi.sdp_solve_batch(probs, prm, want_xy=False)
        walls.append((time.perf_counter() - t0) * 1e3)
    info = res[0].info
    # the loop of lone calls: the parent route, the same problems, the same process
    nl = min(P, lone_cap)
    if nl not in lone_cache:  # (the first nl problems of every batch of this n are the same)
        abi.sdp_solve(*probs[0], prm)
        t0 = time.perf_counter()
        lone = [abi.sdp_solve(M, C, prm) for M, C in probs[:nl]]
        lone_cache[nl] = ((time.perf_counter() - t0) * 1e3, lone)
    lone_ms, lone = lone_cache[nl]
    same = all(np.array_equal(a.evec1, b.evec1) and a.nodes.tolist() == b.nodes.tolist() and a.iters == b.iters
               and a.pobj == b.pobj and a.dobj == b.dobj for a, b in zip(res, lone))
    iters = [r.iters for r in res]
    row = {"n": n, "problems": P, "outliers": 0.7, "eps": EPS,
           "batch_ms_min": min(walls), "batch_ms_all": walls, "batch_ms_per_problem": min(walls) / P,
           "batch_problems_per_s": P / (min(walls) * 1e-3),
           "batch_setup_ms": info.t_setup * 1e3, "batch_iterate_ms": info.t_solve * 1e3,
           "batch_extract_ms": info.t_extract * 1e3,
           "iters_min": min(iters), "iters_max": max(iters), "iters_sum": sum(iters),
           "converged": int(sum(r.info.converged for r in res)),
           "lone_problems": nl, "lone_loop_ms": lone_ms, "lone_ms_per_problem": lone_ms / nl,
           "lone_problems_per_s": nl / (lone_ms * 1e-3), "batch_equals_lone_bits": bool(same),
           "speedup_per_problem": (lone_ms / nl) / (min(walls) / P)}
    if P <= 64:
        t0 = time.perf_counter()
        refs = [sm.solve(M, C, max_iters=20000, eps_abs=EPS, eps_rel=EPS) for M, C in probs]
        cpu_ms = (time.perf_counter() - t0) * 1e3
        row.update({"cpu_model_ms": cpu_ms, "cpu_model_ms_per_problem": cpu_ms / P,
                    "cpu_model_iters_sum": int(sum(r["iters"] for r in refs)),
                    "batch_beats_cpu_model": bool(min(walls) < cpu_ms)})
    return row


def floor_case() -> dict:
    probs = []
    g = abi.HipClipper(storage=abi.STORE_F64)
    for k in range(64):
        p = synth.make_euclidean_problem(64, 0.7, seed=1000 + k)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
        probs.append((g.get_affinity_matrix(), g.get_constraint_matrix()))
    g.close()
    prm = abi.SdpParams(eps_abs=1e-4, eps_rel=1e-4, max_iters=100)

    def best(f):
        f()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return min(ts), r

    ta, ra = best(lambda: [abi.sdp_solve(M, C, prm) for M, C in probs])
    tb, rb = best(lambda: abi.sdp_solve_batch(probs, prm))
    return {"case": "floor", "n": 64, "problems": 64, "outliers": 0.7, "eps": 1e-4, "max_iters": 100,
            "lone_loop_ms": ta, "batch_ms": tb, "ratio": tb / ta, "asserted_ratio": 0.25,
            "iters_min": min(r.iters for r in ra), "iters_max": max(r.iters for r in ra),
            "iters_sum": sum(r.iters for r in ra),
            "batch_equals_lone_bits": all(np.array_equal(a.X, b.X) and a.nodes.tolist() == b.nodes.tolist()
                                          and a.dobj == b.dobj for a, b in zip(ra, rb))}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdp_batch_probe.json"))
    ap.add_argument("--sizes", default="20,64,96,128")
    ap.add_argument("--counts", default="1,16,64,256,1024")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--lone-cap", type=int, default=64)
    ap.add_argument("--trace-case", default="")
    ap.add_argument("--floor-only", action="store_true")
    a = ap.parse_args()
    if a.floor_only:
        row = floor_case()
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        return 0
    if a.trace_case:
        n, P = [int(x) for x in a.trace_case.split(",")]
        probs = problems(n, P)
        prm = abi.SdpParams(eps_abs=EPS, eps_rel=EPS, max_iters=20000)
        r = abi.sdp_solve(*probs[0], prm)
        res = abi.sdp_solve_batch(probs, prm, want_xy=False)
        print(json.dumps({"n": n, "problems": P, "lone_iters": r.iters, "batch_iters_max": max(x.iters for x in res),
                          "batch_ms": res[0].info.t_total * 1e3, "lone_ms": r.info.t_total * 1e3}))
        return 0
    counts = [int(x) for x in a.counts.split(",")]
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        probs = problems(n, max(counts))
        lone_cache: dict = {}
        for P in counts:
            row = case(n, probs[:P], a.reps, a.lone_cap, lone_cache)
            print(json.dumps(row), flush=True)
            rows.append(row)
    row = floor_case()
    print(json.dumps(row), flush=True)
    rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
