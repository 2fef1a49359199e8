#!/usr/bin/env python3
"""Batched solves against the loop of lone calls, on the grid of the reference's benchmark table
(m in {64, 256, 512, 1024, 2048} x rho in {0, .2, .4, .8, .9}, BASELINE 4), 20 problems per cell, fp32 slices, host
buffers in and results out. Per cell, after a warm-up of both: `--reps` rounds of [one batched call (HipBatch.
solve_euclidean: scoring + solving of all 20), the loop of 20 lone HipClipper calls (score + solve each)] alternated
in this process; medians. Also the split of the batched call (staging + fills + plans, the batched launches, the
problems solved alone, rounding), launches per call and problems per route, and the slowest lone solve of the cell on
the resident route (what the batched launches should take about as long as). Writes profiles/batch_probe.json.
  python tools/batch_probe.py [--problems 20] [--reps 5] [--out profiles/batch_probe.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402

NUM_ASSOCS = [64, 256, 512, 1024, 2048]
OUTRATS = [0.0, 0.2, 0.4, 0.8, 0.9]
INV = dict(sigma=0.015, epsilon=0.05)  # benchmarks/main.cpp:221


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_probe.json"))
    a = ap.parse_args()
    hb = abi.HipBatch(storage=abi.STORE_F32_CSC)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    cells = []
    for rho in OUTRATS:
        for m in NUM_ASSOCS:
            probs = [synth.make_euclidean_problem(m, rho, seed=10000 * int(rho * 10) + 100 * m + k)
                     for k in range(a.problems)]
            plist = [(p.D1, p.D2, p.A, p.u0) for p in probs]

            def lone_loop():
                t_solve, routes = [], []
                for p in probs:
                    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
                    t0 = time.perf_counter()
                    g.solve(p.u0)
                    t_solve.append((time.perf_counter() - t0) * 1e3)
                    routes.append(g.last_solver)
                return t_solve, routes

            hb.solve_euclidean(plist, **INV)  # warm-up of both (first use of the sizes allocates)
            lone_loop()
            tb, tl, splits = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                hb.solve_euclidean(plist, **INV)
                tb.append((time.perf_counter() - t0) * 1e3)
                splits.append(hb.split())
                t0 = time.perf_counter()
                t_solve, lone_routes = lone_loop()
                tl.append((time.perf_counter() - t0) * 1e3)
            launches, nb, na = hb.stats()
            med = lambda v: float(np.median(v))  # noqa: E731
            res_solves = [t for t, r in zip(t_solve, lone_routes) if r == 1]
            cell = dict(m=m, rho=rho, problems=a.problems, batch_ms=med(tb), loop_ms=med(tl),
                        ratio=med(tb) / med(tl), batch_ms_all=tb, loop_ms_all=tl,
                        split_ms={k: med([s[k] for s in splits]) for k in splits[0]},
                        launches=launches, n_batched=nb, n_alone=na, lone_resident=int(sum(lone_routes)),
                        slowest_lone_resident_solve_ms=max(res_solves) if res_solves else None)
            cells.append(cell)
            print(json.dumps({k: v for k, v in cell.items() if not k.endswith("_all")}), flush=True)
    name, cus, _ = g.device_info()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=name, cus=cus, problems_per_cell=a.problems, reps=a.reps, cells=cells), f, indent=1)
    hb.close()
    g.close()


if __name__ == "__main__":
    main()
