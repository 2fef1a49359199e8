#!/usr/bin/env python3
"""Raw cloud -> normals -> FPFH ("Normals and FPFH") at n in {4096, 10 000, 100 000}, knn = 16 for the
normals and 32 for the features, no radius, uniform random points:

  - one whole call of clipper_hip_fpfh_from_points (host buffers in, F and N out: checks, H2D, search, three kernels,
    D2H), and of the two-call route (estimate_normals, then compute_fpfh: two uploads, two searches), wall time, median
    of 5 after a warm-up;
  - each stage alone, timed with hipEvents by tools/features_probe_kernels.hip (built here if its binary is missing or
    older than its sources): the K = 32 search, the normals, SPFH, the FPFH combination, and the four queued back to
    back;
  - the same stages by brute force on the host cores in the same run: C++ over the same rules header, direct form, 16
    threads (see the helper's head; from n = 100 000 on the search is extrapolated from 10 000 queries).

  python tools/features_probe.py [--out profiles/features_probe.json] [--sizes 4096,10000,100000]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import build as cbuild  # noqa: E402

HELPER_SRC = os.path.join(ROOT, "tools", "features_probe_kernels.hip")
HELPER = os.path.join(ROOT, "tools", "_bin", "features_probe_kernels")


def build_helper() -> str:
    srcs = [HELPER_SRC] + [os.path.join(cbuild.CSRC, f) for f in ("k_features.hip.h", "k_knn.hip.h", "features_rules.hpp",
                                                                   "sdp_rules.hpp")]
    if not os.path.exists(HELPER) or any(os.path.getmtime(s) > os.path.getmtime(HELPER) for s in srcs):
        os.makedirs(os.path.dirname(HELPER), exist_ok=True)
        subprocess.check_call([cbuild.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-I", cbuild.CSRC, HELPER_SRC, "-o", HELPER, "-lpthread"])
    return HELPER


def whole_calls(n: int, reps: int) -> dict:
    P = np.asfortranarray(np.random.default_rng(n).random((3, n)))
    one, two = [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        F1, N1 = abi.fpfh_from_points(P, normal_knn=16, knn=32)
        t1 = time.perf_counter()
        N2 = abi.estimate_normals(P, knn=16)
        F2 = abi.compute_fpfh(P, N2, knn=32)
        t2 = time.perf_counter()
        if k:
            one.append((t1 - t0) * 1e3)
            two.append((t2 - t1) * 1e3)
    return dict(call_ms=float(np.median(one)), call_min_ms=float(min(one)), two_calls_ms=float(np.median(two)),
                routes_equal=bool(np.array_equal(F1, F2) and np.array_equal(N1, N2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "features_probe.json"))
    ap.add_argument("--sizes", default="4096,10000,100000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build-only", action="store_true", help="build the helper and stop (no device needed)")
    a = ap.parse_args()
    exe = build_helper()
    if a.build_only:
        return
    rec = dict(normal_knn=16, feature_knn=32, radius=0.0, reps=a.reps, data="uniform random in [0, 1)^3",
               host="C++ brute force over features_rules.hpp, direct form, 16 threads", cells=[])
    for n in [int(x) for x in a.sizes.split(",")]:
        cell = dict(n=n)
        cell.update(whole_calls(n, a.reps))
        out = subprocess.run([exe, str(n), str(a.reps)], capture_output=True, text=True, timeout=900)
        if out.returncode != 0:
            raise SystemExit(f"{exe} {n}: exit {out.returncode}\n{out.stdout}{out.stderr}")
        k = json.loads(out.stdout.strip().splitlines()[-1])
        cell.update({x: v for x, v in k.items() if x != "n"})
        cell["host_ms"] = k["host_search_ms"] + k["host_normals_ms"] + k["host_spfh_ms"] + k["host_fpfh_ms"]
        cell["call_speedup_vs_host"] = cell["host_ms"] / cell["call_ms"]
        print(json.dumps(cell), flush=True)
        rec["cells"].append(cell)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
