#!/usr/bin/env python3
"""tools/icp_robust_probe.py — what a robust loss and what trimming cost per ICP iteration on the device beside plain ICP
("Robust losses and trimmed ICP"), written to profiles/icp_robust_probe.json.

The clouds are tools/icp_probe.py's: n_src = n_tgt in --sizes (default 10 000 and 100 000: a bumpy sphere and a noisy,
slightly moved copy), the grid route, a fixed number of iterations (rel_fitness = rel_rmse = 0: a call never stops
CONVERGED). Per size and method (point, plane, generalized) four variants run in ALTERNATED rounds behind a warm-up:
  plain         clipper_hip_icp / clipper_hip_icp_generalized
  robust_none   the robust entry point with no loss and trim 1: the weighted kernels alone
  huber         Huber at scale 0.01
  trim          trimming at 0.7, no loss
ms_per_iteration is info.device_ms (two events around the loop) over the rounds run: the median, the least and the most
of --reps calls. selection_ms is trim minus robust_none (the same weighted round without the select's launches), both
from those events; selection_share is its part of a trimmed iteration.
Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from clipper_amd import _abi as abi  # noqa: E402
from icp_probe import MODES, clouds  # noqa: E402

METHODS = {"point": abi.ICP_POINT_TO_POINT, "plane": abi.ICP_POINT_TO_PLANE, "generalized": abi.ICP_GENERALIZED}
VARIANTS = {"plain": None, "robust_none": dict(loss=abi.ICP_LOSS_NONE, scale=0.0, trim=1.0),
            "huber": dict(loss=abi.ICP_LOSS_HUBER, scale=0.01, trim=1.0), "trim": dict(loss=abi.ICP_LOSS_NONE, scale=0.0, trim=0.7)}
KW = dict(max_distance=0.05, rel_fitness=0.0, rel_rmse=0.0)


def run(src, tgt, nrm, cs, ct, method, iters, robust):
    if method == "generalized":
        if robust is None:
            return abi.icp_generalized(src, cs, tgt, ct, None, max_iterations=iters, **KW)
        return abi.icp_generalized_robust(src, cs, tgt, ct, None, max_iterations=iters, **KW, **robust)
    N = nrm if method == "plane" else None
    if robust is None:
        return abi.icp(src, tgt, None, METHODS[method], N, max_iterations=iters, **KW)
    return abi.icp_robust(src, tgt, None, METHODS[method], N, max_iterations=iters, **KW, **robust)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_robust_probe.json"))
    a = ap.parse_args()
    abi.knn_set_search(MODES["grid"])
    res = dict(iters=a.iters, reps=a.reps, route="grid", max_distance=KW["max_distance"],
               variants={k: v for k, v in VARIANTS.items()}, sizes={})
    for n in a.sizes:
        src, tgt, nrm = clouds(n)
        cs, ct = abi.estimate_covariances(src, knn=20, epsilon=1e-3), abi.estimate_covariances(tgt, knn=20, epsilon=1e-3)
        cell = {}
        for method in METHODS:
            per = {v: [] for v in VARIANTS}
            last = {}
            for rep in range(a.reps + 1):                     # (round 0: the warm-up)
                for v, robust in VARIANTS.items():
                    _, info = run(src, tgt, nrm, cs, ct, method, a.iters, robust)
                    if rep:
                        per[v].append(info.device_ms / (info.iterations + 1))
                    last[v] = info
            out = {}
            for v in VARIANTS:
                i = last[v]
                out[v] = dict(ms_per_iteration=statistics.median(per[v]), least=min(per[v]), most=max(per[v]),
                              rounds=i.iterations + 1, status=i.status, count=i.count, fitness=i.fitness)
            out["trim"]["within"] = last["trim"].within
            sel = out["trim"]["ms_per_iteration"] - out["robust_none"]["ms_per_iteration"]
            out["selection_ms"] = sel
            out["selection_share"] = sel / out["trim"]["ms_per_iteration"]
            out["huber_over_plain"] = out["huber"]["ms_per_iteration"] / out["plain"]["ms_per_iteration"]
            out["trim_over_plain"] = out["trim"]["ms_per_iteration"] / out["plain"]["ms_per_iteration"]
            # the plain call went through the same bits whichever entry point took it
            assert np.array_equal(last["plain"].history, last["robust_none"].history)
            cell[method] = out
            print(n, method, {v: round(out[v]["ms_per_iteration"], 4) for v in VARIANTS}, "selection", round(sel, 4), flush=True)
        res["sizes"][str(n)] = cell
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
