#!/usr/bin/env python3
"""Descriptor matching ("Matching descriptors") at n0 = n1 in {4096, 10 000, 100 000}, d in {3, 33, 64},
knn = 1, mutual = 1, uniform random descriptors:

  - one whole call of clipper_hip_match_descriptors (host buffers in, A out: padding, H2D, both searches, D2H, filters),
    wall time, median of 5 after a warm-up;
  - the search kernels alone, timed with hipEvents by tools/match_probe_kernels.hip (built here if its binary is
    missing or older than its sources): forward, backward, and both queued back to back;
  - at d = 3 the forward search against k_knn_partial<1, 3> (clipper_hip_knn's kernel) on the same clouds: the new
    kernel pads 3 coordinates to 8;
  - the same search by brute force on the host cores in the same run: C++, direct form, 16 threads (see the helper's
    head; from n = 100 000 on extrapolated from 10 000 queries per direction).

  python tools/match_probe.py [--out profiles/match_probe.json] [--sizes 4096,10000,100000] [--dims 3,33,64]
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

HELPER_SRC = os.path.join(ROOT, "tools", "match_probe_kernels.hip")
HELPER = os.path.join(ROOT, "tools", "_bin", "match_probe_kernels")


def build_helper() -> str:
    srcs = [HELPER_SRC] + [os.path.join(cbuild.CSRC, f) for f in ("k_match.hip.h", "k_knn.hip.h")]
    if not os.path.exists(HELPER) or any(os.path.getmtime(s) > os.path.getmtime(HELPER) for s in srcs):
        os.makedirs(os.path.dirname(HELPER), exist_ok=True)
        subprocess.check_call([cbuild.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                               "-I", cbuild.CSRC, HELPER_SRC, "-o", HELPER, "-lpthread"])
    return HELPER


def whole_call(n: int, d: int, reps: int) -> dict:
    rng = np.random.default_rng(n + d)
    F0, F1 = np.asfortranarray(rng.random((d, n))), np.asfortranarray(rng.random((d, n)))
    walls, rows = [], 0
    for k in range(reps + 1):
        t0 = time.perf_counter()
        A, _ = abi.match_descriptors(F0, F1, knn=1, mutual=True)
        if k:
            walls.append((time.perf_counter() - t0) * 1e3)
        rows = len(A)
    return dict(call_ms=float(np.median(walls)), call_min_ms=float(min(walls)), rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_probe.json"))
    ap.add_argument("--sizes", default="4096,10000,100000")
    ap.add_argument("--dims", default="3,33,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--build-only", action="store_true", help="build the helper and stop (no device needed)")
    a = ap.parse_args()
    exe = build_helper()
    if a.build_only:
        return
    rec = dict(knn=1, mutual=1, reps=a.reps, data="uniform random in [0, 1)",
               host="C++ brute force, direct form, 16 threads, both directions", cells=[])
    for n in [int(x) for x in a.sizes.split(",")]:
        for d in [int(x) for x in a.dims.split(",")]:
            cell = dict(n=n, d=d)
            cell.update(whole_call(n, d, a.reps))
            out = subprocess.run([exe, str(n), str(d), str(a.reps)], capture_output=True, text=True, timeout=900)
            if out.returncode != 0:
                raise SystemExit(f"{exe} {n} {d}: exit {out.returncode}\n{out.stdout}{out.stderr}")
            k = json.loads(out.stdout.strip().splitlines()[-1])
            cell.update({x: k[x] for x in ("groups", "chunks", "forward_ms", "backward_ms", "search_ms",
                                           "knn_d3_forward_ms", "host_ms", "host_threads", "host_extrapolated")})
            cell["pairs_per_s"] = 2.0 * n * n / (k["search_ms"] * 1e-3)
            cell["call_speedup_vs_host"] = k["host_ms"] / cell["call_ms"]
            if k["knn_d3_forward_ms"] is not None:
                cell["forward_vs_knn_d3"] = k["forward_ms"] / k["knn_d3_forward_ms"]
            print(json.dumps(cell), flush=True)
            rec["cells"].append(cell)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
