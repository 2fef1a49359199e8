#!/usr/bin/env python3
"""The reference's benchmark table (benchmarks/main.cpp:196-300) on the MI355X path: for outlier
ratios rho in {0, .2, .4, .8, .9} and m in {64, 256, 512, 1024, 2048} putative associations,
M Monte-Carlo trials of
    noisy copy of the bunny -> ground-truth associations (GPU nearest neighbours, one-to-one,
    within the noise bound) -> synthetic putative set -> scorePairwiseConsistency -> solve ->
    precision / recall
with affinity and dense-clique times as the reference brackets them (main.cpp:176-188: host
buffers in, result out). `--cpu` runs the oracle on the same inputs beside it. `--batch` solves each
cell's trials as ONE batch (HipBatch, DESIGN.md 10: scoring and solving of all of them in one call;
the table then reports the batch's time per problem in both time columns' place).
  python tools/bm_table.py [--trials 20] [--cpu] [--batch] [--md out.md]
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
from clipper_amd import registration as reg  # noqa: E402

NUM_ASSOCS = [64, 256, 512, 1024, 2048]
OUTRATS = [0.0, 0.2, 0.4, 0.8, 0.9]
SIGMA, BETA = 0.01, 5.54 * 0.01          # BMParams, main.cpp:31-32
INV = dict(sigma=0.015, epsilon=0.05)    # main.cpp:221


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--warm", type=int, default=1, help="unrecorded trials per cell")
    ap.add_argument("--md", default=None)
    ap.add_argument("--batch", action="store_true", help="each cell's trials as one batched call")
    a = ap.parse_args()
    abi.load_library()
    pts = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_points_4096.f32"), "<f4").reshape(-1, 3)
    pcd0 = reg.scale_to_cube(pts.astype(np.float64), 1.0)
    rng = np.random.default_rng(2022)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    hb = abi.HipBatch(storage=abi.STORE_F32_CSC) if a.batch else None
    if a.cpu:
        from oracle import clipper_ref as cref
    rows = []
    t_nn = []
    for rho in OUTRATS:
        for m in NUM_ASSOCS:
            acc = {k: [] for k in ("aff", "sol", "p", "r", "caff", "csol", "same", "batch")}
            cell = []  # --batch: the recorded trials' (A, Agt, pcd1, u0)
            for trial in range(-a.warm, a.trials):   # trial < 0: not recorded (first use of a size
                pcd1 = pcd0 + reg.bounded_normal_noise(rng, len(pcd0), SIGMA, BETA)
                t0 = time.perf_counter()
                Agt0 = reg.ground_truth_associations(pcd0, pcd1, BETA)
                t_nn.append((time.perf_counter() - t0) * 1e3)
                out = reg.generate_synthetic_correspondences(len(pcd0), len(pcd1), Agt0, m, rho, rng)
                if out is None:
                    continue
                A, Agt = out
                u0 = rng.random(m)
                if hb is not None:
                    cell.append((A, Agt, pcd1, u0, trial))
                    continue
                t0 = time.perf_counter()
                g.score_pairwise_consistency_euclidean(pcd0.T, pcd1.T, A, **INV)
                t1 = time.perf_counter()
                s = g.solve(u0)
                t2 = time.perf_counter()
                p, r = reg.precision_recall(A[s.nodes], Agt)
                if trial < 0:                        # allocates device and pinned buffers)
                    continue
                acc["aff"].append((t1 - t0) * 1e3)
                acc["sol"].append((t2 - t1) * 1e3)
                acc["p"].append(p)
                acc["r"].append(r)
                if a.cpu:
                    c = cref.RefClipper()
                    t0 = time.perf_counter()
                    c.score_pairwise_consistency_euclidean(pcd0.T, pcd1.T, A, **INV)
                    t1 = time.perf_counter()
                    sc = c.solve(u0)
                    t2 = time.perf_counter()
                    acc["caff"].append((t1 - t0) * 1e3)
                    acc["csol"].append((t2 - t1) * 1e3)
                    # as SETS: with a thousand near-equal entries of u the ORDER of the heap selection
                    # (utils.cpp:33-55) depends on their last bits
                    acc["same"].append(sorted(sc.nodes.tolist()) == sorted(s.nodes.tolist()))
            if hb is not None and cell:
                probs = [(pcd0.T, c[2].T, c[0], c[3]) for c in cell]
                hb.solve_euclidean(probs, **INV)          # warm-up: the first use of the sizes allocates
                rec = [k for k, c in enumerate(cell) if c[4] >= 0]
                t0 = time.perf_counter()
                sols = hb.solve_euclidean([probs[k] for k in rec], **INV)
                t1 = time.perf_counter()
                acc["batch"].append((t1 - t0) * 1e3)
                for k, s in zip(rec, sols):
                    p, r = reg.precision_recall(cell[k][0][s.nodes], cell[k][1])
                    acc["p"].append(p)
                    acc["r"].append(r)
                    acc["aff"].append(0.0)
                    acc["sol"].append((t1 - t0) * 1e3 / len(rec))
            row = dict(rho=rho, m=m, trials=len(acc["aff"]))
            if acc["batch"]:
                row["batch_ms"] = acc["batch"][0]
                row["launches"], row["n_batched"], row["n_alone"] = hb.stats()
            for k in ("aff", "sol", "p", "r", "caff", "csol"):
                if acc[k]:
                    row[k] = float(np.mean(acc[k]))
                    row[k + "_sd"] = float(np.std(acc[k], ddof=1)) if len(acc[k]) > 1 else 0.0
            if acc["same"]:
                row["sets_identical"] = int(sum(acc["same"]))
            rows.append(row)
            print(json.dumps(row), flush=True)
    lines = ["| ρ [%] | # assoc | affinity [ms] | dense clique [ms] | precision [%] | recall [%] |"
             + (" CPU affinity [ms] | CPU dense clique [ms] | identical sets |" if a.cpu else ""),
             "|---|---|---|---|---|---|" + ("---|---|---|" if a.cpu else "")]
    for r in rows:
        if "aff" not in r:
            continue
        line = (f"| {int(r['rho'] * 100)} | {r['m']} | {r['aff']:.2f} ± {r['aff_sd']:.2f} | "
                f"{r['sol']:.2f} ± {r['sol_sd']:.2f} | {int(r['p'] * 100)} | {int(r['r'] * 100)} |")
        if a.cpu:
            line += (f" {r['caff']:.2f} ± {r['caff_sd']:.2f} | {r['csol']:.2f} ± {r['csol_sd']:.2f} | "
                     f"{r['sets_identical']}/{r['trials']} |")
        lines.append(line)
    lines.append("")
    lines.append(f"ground-truth associations (GPU brute-force 1-NN, 4096 x 4096 points, one-to-one): "
                 f"{np.median(t_nn):.2f} ms per call (median of {len(t_nn)}, host buffers in / out)")
    text = "\n".join(lines)
    print(text)
    if a.md:
        open(a.md, "w").write(text + "\n")


if __name__ == "__main__":
    main()
