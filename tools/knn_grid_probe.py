#!/usr/bin/env python3
"""The two routes of the d = 3 nearest-neighbour search side by side ("The grid route of the search"):
brute force (clipper_hip_knn_set_search(CLIPPER_HIP_KNN_BRUTE)) and the uniform grid (CLIPPER_HIP_KNN_GRID), measured
in the same run on the same clouds, with the lists of every cell of the table compared for equality (the run stops at
the first difference).

  clouds   a uniform cube, and a surface: tests/golden/bunny_points.json resampled to the target size with a jitter of
           0.5 % of its extent (points on a 2-D manifold: the realistic case)
  sizes    n in {10 000, 100 000, 1 000 000}; K in {1, 16} through clipper_hip_knn, as a self-search and cloud to cloud;
           K = 32 exists only behind the features, so that row is clipper_hip_estimate_normals(knn = 32): a self-search
  times    the whole call (host buffers in, lists out: wall clock) and the device time between two events around the
           search's kernels (clipper_hip_knn_last_search().kernels_ms): medians of 5 after a warm-up
  1e6      brute force is run on a subset of the queries against the whole cloud and scaled to all of them
           ("extrapolated": true); the grid runs all of them, and the subset's lists are the ones compared. The K = 32
           row is a self-search, which has no subset: brute force runs whole there, once after a warm-up
  fpfh     clipper_hip_fpfh_from_points at 100 000 under both routes
  sweep    self-searches at K = 1, 16 and 32 over small sizes: where the grid starts to win (CLIPPER_HIP_KNN_AUTO_MIN_N)

The grid's target occupancy is a build-time constant (KNN_GRID_POINTS_PER_CELL): to compare values, build the library
once per value and run this tool once per library (CLIPPER_HIP_LIB=..., --label ...).

  python tools/knn_grid_probe.py [--out profiles/knn_grid_probe.json] [--sizes 10000,100000,1000000] [--quick]
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

BRUTE_QUERY_CAP = 20000   # queries of the brute-force route where the searched cloud has 1 000 000 points
ROUTES = (("brute", abi.KNN_BRUTE), ("grid", abi.KNN_GRID))


def uniform(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).random((n, 3))


def surface(n: int, seed: int) -> np.ndarray:
    pts = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "bunny_points.json")))["points"], np.float64)
    rng = np.random.default_rng(seed)
    ext = float((pts.max(axis=0) - pts.min(axis=0)).max())
    # a random point of a random triangle-ish neighbourhood: two fixture points blended, then the jitter
    a, b = pts[rng.integers(0, len(pts), n)], pts[rng.integers(0, len(pts), n)]
    near = np.linalg.norm(a - b, axis=1) < 0.15 * ext
    t = rng.random((n, 1)) * near[:, None]
    return a + t * (b - a) + rng.normal(0.0, 0.005 * ext, (n, 3))


def timed(call, reps: int):
    """median wall ms and median kernels_ms of `call` over reps runs after a warm-up; the last result; the last stats"""
    wall, dev, out, st = [], [], None, None
    for k in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        t1 = time.perf_counter()
        st = abi.knn_last_search()
        if k:
            wall.append((t1 - t0) * 1e3)
            dev.append(st.kernels_ms)
    return float(np.median(wall)), float(np.median(dev)), out, st


def same(a, b) -> bool:
    return all(x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def one_cell(cloud: str, P: np.ndarray, Q: np.ndarray | None, K: int, reps: int) -> dict:
    """P: the searched cloud (n x 3); Q: the queries, or None for a self-search"""
    n = len(P)
    row = dict(cloud=cloud, n=n, K=K, kind="self" if Q is None else "cloud-to-cloud")
    Pt = np.asfortranarray(P.T)
    Qt = Pt if Q is None else np.asfortranarray(Q.T)
    capped = n >= 1000000 and K <= 16
    results = {}
    for name, mode in ROUTES:
        abi.knn_set_search(mode)
        if K == 32:
            call = lambda: abi.estimate_normals(Pt, knn=32, return_counts=True)  # noqa: E731
            # (a self-search cannot be cut down to a subset of its queries: at 1 000 000 brute force runs whole, once)
        elif name == "brute" and capped:
            sub = np.asfortranarray(Qt[:, :BRUTE_QUERY_CAP])
            call = lambda: abi.knn(sub, Pt, K)  # noqa: E731
        else:
            call = lambda: abi.knn(Qt, Pt, K)  # noqa: E731
        once = name == "brute" and K == 32 and n >= 1000000
        wall, dev, out, st = timed(call, 1 if once else reps)
        assert st.route == mode, (name, st.route)
        rec = dict(call_ms=wall, kernels_ms=dev)
        if once:
            rec["single_run"] = True
        if name == "brute" and capped:
            scale = Qt.shape[1] / BRUTE_QUERY_CAP
            rec = dict(call_ms=wall * scale, kernels_ms=dev * scale, extrapolated=True, queries_run=BRUTE_QUERY_CAP)
        if name == "grid":
            rec.update(dim=[int(x) for x in st.dim], candidates_per_query=st.candidates / max(1, st.queries))
        row[name] = rec
        results[name] = out
    if "brute" in results:
        g = results["grid"]
        if capped:
            g = tuple(x[:BRUTE_QUERY_CAP] for x in g)
        assert same(results["brute"], g), f"the routes differ: {row}"
        row["equal"] = True
        row["speedup_kernels"] = row["brute"]["kernels_ms"] / row["grid"]["kernels_ms"]
        row["speedup_call"] = row["brute"]["call_ms"] / row["grid"]["call_ms"]
    print(json.dumps(row), flush=True)
    return row


def fpfh(n: int, reps: int) -> dict:
    P = np.asfortranarray(uniform(n, 5).T)
    row, results = dict(n=n), {}
    for name, mode in ROUTES:
        abi.knn_set_search(mode)
        wall, dev, out, st = timed(lambda: abi.fpfh_from_points(P, normal_knn=16, knn=32), reps)
        assert st.route == mode
        row[name] = dict(call_ms=wall, search_kernels_ms=dev)
        results[name] = out
    assert same(results["brute"], results["grid"]), "fpfh_from_points differs between the routes"
    row["equal"] = True
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_grid_probe.json"))
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--sweep", default="1000,2000,4000,8000,12000,16000,24000,32000,64000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="", help="what distinguishes this library (e.g. its KNN_GRID_POINTS_PER_CELL)")
    ap.add_argument("--quick", action="store_true", help="K = 16 at the two larger sizes only (comparing builds)")
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",") if s]
    before = abi.knn_search()
    res = dict(label=a.label, library=os.path.basename(abi.LIB_PATH), reps=a.reps, table=[], sweep=[], fpfh=[],
               auto_min_n=int(abi.knn_last_search().auto_min_n))
    try:
        for n in sizes:
            if a.quick and n < 100000:
                continue
            for cloud, make in (("uniform", uniform), ("surface", surface)):
                P, Q = make(n, n), make(n, n + 1)
                for K in ((16,) if a.quick else (1, 16, 32)):
                    res["table"].append(one_cell(cloud, P, None, K, a.reps))
                    if K <= 16:
                        res["table"].append(one_cell(cloud, P, Q, K, a.reps))
        if not a.quick:
            for n in [int(s) for s in a.sweep.split(",") if s]:
                for K in (1, 16, 32):
                    r = one_cell("uniform", uniform(n, n), None, K, a.reps)
                    res["sweep"].append(dict(n=n, K=K, brute_kernels_ms=r["brute"]["kernels_ms"],
                                             grid_kernels_ms=r["grid"]["kernels_ms"], brute_call_ms=r["brute"]["call_ms"],
                                             grid_call_ms=r["grid"]["call_ms"]))
            if 100000 in sizes:
                res["fpfh"].append(fpfh(100000, a.reps))
    finally:
        abi.knn_set_search(before)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
