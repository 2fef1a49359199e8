#!/usr/bin/env python3
"""tools/gicp_probe.py — what an iteration of generalized ICP costs on the device beside the other two methods, and what
its covariances cost beside the normals ("Generalized ICP"), written to profiles/gicp_probe.json.

The clouds and the method are tools/icp_probe.py's: n_src = n_tgt in --sizes (default 10 000 and 100 000: a bumpy sphere
and a noisy, slightly moved copy), all three methods and both search routes in the same run, a fixed number of
iterations (rel_fitness = rel_rmse = 0: a call never stops CONVERGED). The covariances of both clouds are
clipper_hip_estimate_covariances' at knn = 20, epsilon = 1e-3. Per cell:
  ms_per_iteration   info.device_ms (two events around the loop) over the rounds run, median of --reps calls behind a warm-up
  kernels            the median duration of each kernel of a round, from a rocprofv3 kernel trace of a CHILD process
                     running the same call (a run of its own: tracing slows the host), grouped into search, accumulate,
                     step and transform; kernels_ms their sum
  accumulate_below_search   the condition stated before the run, for the generalized method on the grid route at the
                     largest size: the accumulate kernel of an iteration takes less time than its search kernels
And per size `covariances`: whole calls of estimate_covariances and estimate_normals at knn = 20 on the grid route and by
brute force (median of --reps behind a warm-up), the kernels k_icp_covariances and k_feat_normals from a trace of a child
that runs both, and their ratios.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from clipper_amd import _abi as abi  # noqa: E402
from icp_probe import GROUPS, MODES, clouds  # noqa: E402

METHODS = {"point": abi.ICP_POINT_TO_POINT, "plane": abi.ICP_POINT_TO_PLANE, "generalized": abi.ICP_GENERALIZED}
KNN, EPSILON = 20, 1e-3


def run(src, tgt, nrm, cs, ct, method: str, iters: int):
    if method == "generalized":
        return abi.icp_generalized(src, cs, tgt, ct, None, max_distance=0.05, max_iterations=iters, rel_fitness=0.0, rel_rmse=0.0)
    return abi.icp(src, tgt, None, METHODS[method], nrm if method == "plane" else None, max_distance=0.05,
                   max_iterations=iters, rel_fitness=0.0, rel_rmse=0.0)


def timed(src, tgt, nrm, cs, ct, method, iters, reps):
    run(src, tgt, nrm, cs, ct, method, iters)
    per, info = [], None
    for _ in range(reps):
        _, info = run(src, tgt, nrm, cs, ct, method, iters)
        per.append(info.device_ms / (info.iterations + 1))
    return dict(ms_per_iteration=statistics.median(per), rounds=info.iterations + 1, status=info.status, fitness=info.fitness,
                inlier_rmse=info.inlier_rmse)


def child(a):
    """one configuration, twice (a warm-up, then the traced call): run under rocprofv3 by trace()"""
    src, tgt, nrm = clouds(a.n)
    abi.knn_set_search(MODES[a.route])
    if a.child == "cov":
        for _ in range(2):
            abi.estimate_covariances(tgt, knn=KNN, epsilon=EPSILON)
            abi.estimate_normals(tgt, knn=KNN)
        return
    cs = ct = None
    if a.method == "generalized":       # (the parent's covariances, from a file: the trace holds the rounds' kernels alone)
        both = np.load(a.cov)
        cs, ct = np.asfortranarray(both[0]), np.asfortranarray(both[1])
    run(src, tgt, nrm, cs, ct, a.method, a.iters)
    run(src, tgt, nrm, cs, ct, a.method, a.iters)


def kernel_durations(what, n, method, route, iters, cov=None):
    """{short kernel name: [durations in us]} of a child, from the rocpd database of a kernel trace; or {"error": ...}.
    cov: the covariances (source, target) the child of a generalized run takes"""
    if not shutil.which("rocprofv3"):
        return None
    out = tempfile.mkdtemp(prefix="gicp_probe_")
    cmd = ["rocprofv3", "--kernel-trace", "-d", out, "-o", "trace", "--", sys.executable, os.path.abspath(__file__), "--child", what,
           "--n", str(n), "--method", method, "--route", route, "--iters", str(iters)]
    if cov is not None:
        np.save(os.path.join(out, "cov.npy"), np.stack(cov))
        cmd += ["--cov", os.path.join(out, "cov.npy")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=out)
    dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith(".db")]
    if r.returncode != 0 or not dbs:
        shutil.rmtree(out, ignore_errors=True)
        return dict(error=(r.stderr or r.stdout)[-400:])
    rows = sqlite3.connect(dbs[0]).execute("select name, duration from kernels").fetchall()
    shutil.rmtree(out, ignore_errors=True)
    per = {}
    for name, dur in rows:
        per.setdefault(name.split("(")[0].split("<")[0].split("::")[-1], []).append(dur / 1e3)
    return per


def trace(n, method, route, iters, cov):
    """per-group kernel time of a round (ms), as tools/icp_probe.py groups it"""
    per = kernel_durations("icp", n, method, route, iters, cov if method == "generalized" else None)
    if per is None or "error" in per:
        return per
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


def covariances(tgt, n, reps, no_trace):
    """estimate_covariances beside estimate_normals at the same knn, in the same run"""
    out = {}
    for route, mode in MODES.items():
        if route == "brute" and n > 20000:
            continue                                        # (1e10 pairs a call: the grid is the route of this size)
        abi.knn_set_search(mode)
        calls = {"covariances": lambda: abi.estimate_covariances(tgt, knn=KNN, epsilon=EPSILON),
                 "normals": lambda: abi.estimate_normals(tgt, knn=KNN)}
        wall = {k: [] for k in calls}
        for f in calls.values():
            f()
        for _ in range(reps):                               # alternating: both see the same machine
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                wall[k].append((time.perf_counter() - t0) * 1e3)
        cell = dict(covariances_call_ms=statistics.median(wall["covariances"]), normals_call_ms=statistics.median(wall["normals"]))
        cell["call_ratio"] = cell["covariances_call_ms"] / cell["normals_call_ms"]
        if not no_trace:
            per = kernel_durations("cov", n, "point", route, 0)
            if per and "error" not in per:
                cell["k_icp_covariances_us"] = statistics.median(per.get("k_icp_covariances", [float("nan")]))
                cell["k_feat_normals_us"] = statistics.median(per.get("k_feat_normals", [float("nan")]))
                cell["kernel_ratio"] = cell["k_icp_covariances_us"] / cell["k_feat_normals_us"]
            else:
                cell["kernels"] = per
        out[route] = cell
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gicp_probe.json"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", default="", choices=["", "icp", "cov"])
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--method", default="generalized")
    ap.add_argument("--route", default="grid")
    ap.add_argument("--cov", default="")
    a = ap.parse_args()
    if a.child:
        return child(a)
    if abi.device_count() < 1:
        sys.exit("gicp_probe: no GPU visible (there is no fallback)")
    sizes = [int(s) for s in a.sizes.split(",")]
    res = dict(label=a.label, library=os.path.basename(abi.LIB_PATH), iters=a.iters, reps=a.reps, knn=KNN, epsilon=EPSILON,
               cells=[], covariances={})
    before = abi.knn_search()
    try:
        for n in sizes:
            src, tgt, nrm = clouds(n)
            abi.knn_set_search(abi.KNN_GRID)
            cs, ct = abi.estimate_covariances(src, knn=KNN, epsilon=EPSILON), abi.estimate_covariances(tgt, knn=KNN, epsilon=EPSILON)
            for route, mode in MODES.items():
                abi.knn_set_search(mode)
                iters = a.iters if route == "grid" or n <= 20000 else min(a.iters, 4)     # (brute force at 1e10 pairs a round)
                for method in METHODS:
                    cell = dict(n=n, route=route, method=method, **timed(src, tgt, nrm, cs, ct, method, iters, a.reps))
                    if not a.no_trace:
                        cell["kernels"] = trace(n, method, route, iters, (cs, ct))
                        if cell["kernels"] and "kernels_ms" in cell["kernels"]:
                            cell["host_wait_ms"] = cell["ms_per_iteration"] - cell["kernels"]["kernels_ms"]
                            if method == "generalized" and route == "grid" and n == max(sizes):
                                cell["accumulate_below_search"] = cell["kernels"]["accumulate"] < cell["kernels"]["search"]
                    res["cells"].append(cell)
                    print(json.dumps({k: (v if k != "kernels" or not v else {g: v.get(g) for g in list(GROUPS) + ["error"] if g in v})
                                      for k, v in cell.items()}), flush=True)
            res["covariances"][str(n)] = covariances(tgt, n, a.reps, a.no_trace)
            print(json.dumps({"n": n, "covariances": res["covariances"][str(n)]}), flush=True)
    finally:
        abi.knn_set_search(before)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
