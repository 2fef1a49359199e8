#!/usr/bin/env python3
"""tools/icp_probe.py — what an ICP iteration costs on the device ("ICP over a kept search
grid"), written to profiles/icp_probe.json.

For n_src = n_tgt in --sizes (default 10 000 and 100 000: a surface sample and a noisy, slightly moved copy of it), both
methods and both search routes, clipper_hip_icp runs a fixed number of iterations (rel_fitness = rel_rmse = 0: it never
stops CONVERGED). Per cell:
  ms_per_iteration   info.device_ms (two events around the loop) over the rounds run, median of --reps calls behind a warm-up
  kernels            the median duration of each kernel of a round, from a rocprofv3 kernel trace of a CHILD process
                     running the same call (a run of its own: tracing slows the host), grouped into search, accumulate,
                     step and transform; kernels_ms their sum
  host_wait_ms       ms_per_iteration - kernels_ms: the device idles while the host reads the status record and
                     queues the next round (launch gaps included)
  rebinned           the same with CLIPPER_HIP_ICP_REBIN=1: the moved source binned anew every iteration (grid route)
  knn_call_ms        a stand-alone clipper_hip_knn K = 1 call on the same clouds, in the same run: whole call and its
                     kernels (clipper_hip_knn_last_search). The condition stated in advance: on the grid route an
                     iteration takes no longer than the call's kernels, which pay the build ICP keeps.
Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402

GROUPS = {"search": ("k_knn_grid", "k_kg_sum", "k_knn_partial", "k_knn_merge", "k_kg_count", "k_row_scan", "k_kg_scatter", "k_kg_init"),
          "accumulate": ("k_icp_accumulate",), "step": ("k_icp_step",), "transform": ("k_icp_transform",)}
MODES = {"brute": abi.KNN_BRUTE, "grid": abi.KNN_GRID}
METHODS = {"point": abi.ICP_POINT_TO_POINT, "plane": abi.ICP_POINT_TO_PLANE}


def clouds(n: int, seed: int = 0):
    """a bumpy sphere sampled n times (a surface, as a scan is), its analytic-sphere normals, and a copy moved by 2
    degrees and 0.01 with noise of 0.001: (src 3 x n, tgt 3 x n, normals 3 x n)"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    tgt = v * (1.0 + 0.1 * np.sin(5.0 * v[:, :1]) * np.cos(4.0 * v[:, 1:2]))
    th = np.deg2rad(2.0)
    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    src = tgt[rng.permutation(n)] @ R.T + 0.01 + rng.uniform(-0.001, 0.001, (n, 3))
    return np.asfortranarray(src.T), np.asfortranarray(tgt.T), np.asfortranarray(v.T)


def run(src, tgt, nrm, method: str, iters: int):
    return abi.icp(src, tgt, None, METHODS[method], nrm if method == "plane" else None, max_distance=0.05,
                   max_iterations=iters, rel_fitness=0.0, rel_rmse=0.0)


def timed(src, tgt, nrm, method, iters, reps):
    run(src, tgt, nrm, method, iters)
    per, wall, info = [], [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        _, info = run(src, tgt, nrm, method, iters)
        wall.append((time.perf_counter() - t0) * 1e3)
        per.append(info.device_ms / (info.iterations + 1))
    return dict(ms_per_iteration=statistics.median(per), call_wall_ms=statistics.median(wall), rounds=info.iterations + 1,
                status=info.status, fitness=info.fitness, inlier_rmse=info.inlier_rmse,
                candidates_per_query=info.candidates / ((info.iterations + 1) * src.shape[1]), dim=list(info.dim))


def child(a):
    """one configuration, twice (a warm-up, then the traced call): run under rocprofv3 by trace()"""
    src, tgt, nrm = clouds(a.n)
    abi.knn_set_search(MODES[a.route])
    run(src, tgt, nrm, a.method, a.iters)
    run(src, tgt, nrm, a.method, a.iters)


def trace(n, method, route, iters, rebin):
    """per-kernel medians (us) of a child's two calls, from the rocpd database of a kernel trace"""
    if not shutil.which("rocprofv3"):
        return None
    out = tempfile.mkdtemp(prefix="icp_probe_")
    env = dict(os.environ, CLIPPER_HIP_ICP_REBIN="1" if rebin else "0")
    cmd = ["rocprofv3", "--kernel-trace", "-d", out, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--child",
           "--n", str(n), "--method", method, "--route", route, "--iters", str(iters)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd=out)
    dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith(".db")]
    if r.returncode != 0 or not dbs:
        shutil.rmtree(out, ignore_errors=True)
        return dict(error=(r.stderr or r.stdout)[-400:])
    rows = sqlite3.connect(dbs[0]).execute("select name, duration from kernels").fetchall()
    shutil.rmtree(out, ignore_errors=True)
    per = {}
    for name, dur in rows:
        short = name.split("(")[0].split("<")[0].split("::")[-1]
        per.setdefault(short, []).append(dur / 1e3)
    rounds = 2 * (iters + 1)
    res = {g: 0.0 for g in GROUPS}
    detail = {}
    for k, v in per.items():
        for g, names in GROUPS.items():
            if k in names:
                # a kernel of every round: its median; one that runs less often (the binning): its total spread over the rounds
                share = statistics.median(v) * (len(v) / rounds if len(v) < rounds else len(v) // rounds)
                res[g] += share / 1e3
                detail[k] = dict(calls=len(v), median_us=statistics.median(v))
    res["kernels_ms"] = sum(res[g] for g in GROUPS)
    res["detail"] = detail
    return res


def knn_call(src, tgt, reps):
    abi.knn(src, tgt, 1)
    wall, dev = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        abi.knn(src, tgt, 1)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(abi.knn_last_search().kernels_ms)
    return dict(call_wall_ms=statistics.median(wall), kernels_ms=statistics.median(dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "icp_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--method", default="point")
    ap.add_argument("--route", default="grid")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if abi.device_count() < 1:
        sys.exit("icp_probe: no GPU visible (there is no fallback)")
    res = dict(label=a.label, library=os.path.basename(abi.LIB_PATH), iters=a.iters, reps=a.reps, cells=[])
    before = abi.knn_search()
    try:
        for n in [int(s) for s in a.sizes.split(",")]:
            src, tgt, nrm = clouds(n)
            for route, mode in MODES.items():
                abi.knn_set_search(mode)
                knn = knn_call(src, tgt, a.reps)
                iters = a.iters if route == "grid" or n <= 20000 else min(a.iters, 4)     # (brute force at 1e10 pairs a round)
                for method in METHODS:
                    os.environ["CLIPPER_HIP_ICP_REBIN"] = "0"
                    cell = dict(n=n, route=route, method=method, knn_call=knn, **timed(src, tgt, nrm, method, iters, a.reps))
                    if not a.no_trace:
                        cell["kernels"] = trace(n, method, route, iters, False)
                        if cell["kernels"] and "kernels_ms" in cell["kernels"]:
                            cell["host_wait_ms"] = cell["ms_per_iteration"] - cell["kernels"]["kernels_ms"]
                    if route == "grid":
                        os.environ["CLIPPER_HIP_ICP_REBIN"] = "1"
                        cell["rebinned"] = timed(src, tgt, nrm, method, iters, a.reps)
                        os.environ["CLIPPER_HIP_ICP_REBIN"] = "0"
                        cell["iteration_within_knn_kernels"] = cell["ms_per_iteration"] <= knn["kernels_ms"]
                    res["cells"].append(cell)
                    print(json.dumps({k: v for k, v in cell.items() if k != "kernels"}), flush=True)
    finally:
        abi.knn_set_search(before)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
