#!/usr/bin/env python3
"""User-defined invariants on the device against the built-in fill and the host loop, on EuclideanDistance
restated as device source (tests/test_gpu_device_invariant.py) with the bench parameters:

  - the cold compile (clipper_hip_invariant_create) and the first fill on a device (module load included) against the
    second;
  - scorePairwiseConsistency with host buffers (wall time of the C ABI call: H2D, gather, fill, slices) and the fill's
    event time (fill kernel + the slices built from the dense store) at m = 1 000, 10 000, 30 000: the device invariant,
    the built-in default route, the built-in with CLIPPER_HIP_AFFINITY=plain;
  - the C++ host loop (a PairwiseInvariant subclass through clipper::CLIPPER, 16 OpenMP threads) at 1 000 and 10 000;
  - the Python subclass (clipperpy, one thread) at 1 000.

The fill kernels' own times come from a separate run under `rocprofv3 --kernel-trace --stats` with --kernels-only
(fills only, no host loops), summarised by tools/rocpd_stats.py.

  python tools/device_invariant_probe.py [--out profiles/device_invariant_probe.json] [--sizes 1000,10000,30000]
  rocprofv3 --kernel-trace --stats -d DIR -o trace -- python tools/device_invariant_probe.py --kernels-only
"""
from __future__ import annotations

import argparse
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import clipper_amd  # noqa: E402
from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402

EUCLID_SRC = r"""
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) {
    const double t1 = ai[k] - aj[k];
    const double t2 = bi[k] - bj[k];
    s1 = fma(t1, t1, s1);
    s2 = fma(t2, t2, s2);
  }
  const double l1 = sqrt(s1), l2 = sqrt(s2);
  if (params[2] > 0 && (l1 < params[2] || l2 < params[2])) return 0.0;
  const double c = fabs(l1 - l2);
  return (c < params[1]) ? exp(-0.5 * c * c / (params[0] * params[0])) : 0.0;
}
"""
KW = synth.EUCLID_BENCH_PARAMS
PRM = [KW["sigma"], KW["epsilon"], KW["mindist"]]


def _median(v):
    return float(np.median(np.asarray(v)))


def _route(route, inv, p, reps):
    """wall time of the host-buffer call and its event time, median over reps (after one warm call)"""
    if route == "builtin_plain":
        os.environ["CLIPPER_HIP_AFFINITY"] = "plain"  # (read when the inputs are staged)
    try:
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        walls, events = [], []
        for k in range(reps + 1):
            t0 = time.perf_counter()
            if route == "device":
                g.affinity_custom(inv, p.D1, p.D2, p.A, PRM)
            else:
                g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **KW)
            w = time.perf_counter() - t0
            if k:
                walls.append(w * 1e3)
                events.append(g.timings().affinity_kernel_ms)
        g.close()
    finally:
        os.environ.pop("CLIPPER_HIP_AFFINITY", None)
    return dict(call_ms=_median(walls), fill_event_ms=_median(events))


def _build_host_loop(td):
    exe = os.path.join(td, "device_invariant_hostloop")
    libdir = os.path.join(ROOT, "clipper_amd", "lib")
    subprocess.check_call([
        "g++", "-O2", "-std=c++17", "-fopenmp", "-I", os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tools", "device_invariant_hostloop.cpp"),
        os.path.join(ROOT, "clipper_amd", "csrc", "host", "clipper.cpp"),
        "-L", libdir, "-lclipper_hip", f"-Wl,-rpath,{libdir}", "-o", exe])
    return exe


def _host_loop(p, exe, td):
    f = [os.path.join(td, n) for n in ("D1.f64", "D2.f64", "A.i32")]
    np.ascontiguousarray(np.asarray(p.D1, dtype=np.float64).T).tofile(f[0])  # column-major 3 x n
    np.ascontiguousarray(np.asarray(p.D2, dtype=np.float64).T).tofile(f[1])
    np.ascontiguousarray(np.asarray(p.A, dtype=np.int32).T).tofile(f[2])     # column-major m x 2
    env = dict(os.environ, OMP_NUM_THREADS="16")
    out = subprocess.run([exe, *f], capture_output=True, text=True, timeout=1800, env=env, check=True)
    return json.loads(out.stdout.strip().splitlines()[-1])["host_loop_s"]


def _python_subclass(p):
    cp = clipper_amd.load_clipperpy()
    sigma, epsilon = KW["sigma"], KW["epsilon"]

    class Custom(cp.invariants.PairwiseInvariant):
        def __init__(self):
            super().__init__()

        def __call__(self, ai, aj, bi, bj):
            c = abs(np.linalg.norm(ai - aj) - np.linalg.norm(bi - bj))
            return math.exp(-0.5 * c * c / (sigma * sigma)) if c < epsilon else 0.0

    c = cp.CLIPPER(Custom(), cp.Params())
    t0 = time.perf_counter()
    c.score_pairwise_consistency(p.D1, p.D2, p.A)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_invariant_probe.json"))
    ap.add_argument("--sizes", default="1000,10000,30000")
    ap.add_argument("--host-sizes", default="1000,10000")
    ap.add_argument("--python-size", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true", help="the fills alone (for the rocprofv3 run); writes nothing")
    a = ap.parse_args()
    sizes = [int(x) for x in a.sizes.split(",")]
    host_sizes = [int(x) for x in a.host_sizes.split(",") if x]
    rec = dict(source="EuclideanDistance restated (d = 3)", params=KW, storage="F32_CSC", rho=0.95)

    t0 = time.perf_counter()
    inv = abi.HipInvariant(EUCLID_SRC, 3)
    rec["compile_s"] = time.perf_counter() - t0
    p = synth.make_euclidean_problem(1000, 0.95, seed=12345)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.stage_inputs(p.D1, p.D2, p.A)
    fills = []
    for _ in range(2):
        t0 = time.perf_counter()
        g.affinity_custom_staged(inv, PRM)
        fills.append((time.perf_counter() - t0) * 1e3)
    g.close()
    rec["first_fill_ms"], rec["second_fill_ms"] = fills
    rec["module_load_ms"] = fills[0] - fills[1]
    print(json.dumps({k: rec[k] for k in ("compile_s", "first_fill_ms", "second_fill_ms")}), flush=True)

    rec["sizes"] = []
    for m in sizes:
        p = synth.make_euclidean_problem(m, 0.95, seed=12345)
        row = dict(m=m)
        for route in ("device", "builtin_default", "builtin_plain"):
            row[route] = _route(route, inv, p, a.reps)
        print(json.dumps(row), flush=True)
        rec["sizes"].append(row)
    inv.close()
    if a.kernels_only:
        return

    with tempfile.TemporaryDirectory() as td:
        exe = _build_host_loop(td)
        for row in rec["sizes"]:
            if row["m"] in host_sizes:
                p = synth.make_euclidean_problem(row["m"], 0.95, seed=12345)
                row["cpp_host_loop_16t_ms"] = _host_loop(p, exe, td) * 1e3
                row["speedup_vs_host_loop"] = row["cpp_host_loop_16t_ms"] / row["device"]["call_ms"]
                print(json.dumps({"m": row["m"], "cpp_host_loop_16t_ms": row["cpp_host_loop_16t_ms"]}), flush=True)
    p = synth.make_euclidean_problem(a.python_size, 0.95, seed=12345)
    rec["python_subclass"] = dict(m=a.python_size, ms=_python_subclass(p) * 1e3)
    print(json.dumps(rec["python_subclass"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
