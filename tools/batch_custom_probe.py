#!/usr/bin/env python3
"""Batched solves scored by a user-defined invariant against the loop of lone calls, on the grid of
tools/batch_probe.py (m in {64, 256, 512, 1024, 2048} x rho in {0, .2, .4, .8, .9}), 20 problems per cell, fp32
slices, host buffers in and results out. The invariant is EuclideanDistance restated as device source. Per cell, after
a warm-up of all three: `--reps` rounds of [one batched custom call (HipBatch.solve_custom), the loop of 20 lone
HipClipper calls (affinity_custom + solve each), one batched built-in call (HipBatch.solve_euclidean) on the same
problems] alternated in this process; medians. Also both batched calls' splits (clipper_hip_batch_get_split), and the
custom call's fill split from one more call with CLIPPER_HIP_HOST_TIMING: staging + the children's dense stores
(hipMalloc), the batched fill kernel (events), the kernel's wait + the slice builds. Writes
profiles/batch_custom_probe.json.
  python tools/batch_custom_probe.py [--problems 20] [--reps 5] [--m 512 ...] [--rho 0.4 ...] [--out FILE]
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402

NUM_ASSOCS = [64, 256, 512, 1024, 2048]
OUTRATS = [0.0, 0.2, 0.4, 0.8, 0.9]
INV = dict(sigma=0.015, epsilon=0.05, mindist=0.0)  # benchmarks/main.cpp:221
IPRM = [INV["sigma"], INV["epsilon"], INV["mindist"]]

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

LINE = re.compile(r"\[batch-custom\] n = \d+: stage \+ begin \(dense stores\) ([\d.]+) ms, (\d+) tiles ([\d.]+) ms "
                  r"\(events\), launch \+ builds ([\d.]+) ms, (\d+) build round")


def fill_split(hb, inv, plist):
    """one batched custom call with CLIPPER_HIP_HOST_TIMING, its stderr line read back from a file"""
    os.environ["CLIPPER_HIP_HOST_TIMING"] = "1"
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+") as f:
        os.dup2(f.fileno(), 2)
        try:
            hb.solve_custom(inv, plist, IPRM)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            del os.environ["CLIPPER_HIP_HOST_TIMING"]
        f.seek(0)
        mt = LINE.search(f.read())
    if not mt:
        return None
    return dict(stage_begin_ms=float(mt.group(1)), tiles=int(mt.group(2)), fill_kernel_ms=float(mt.group(3)),
                launch_and_builds_ms=float(mt.group(4)), build_rounds=int(mt.group(5)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--m", type=int, nargs="*", default=NUM_ASSOCS)
    ap.add_argument("--rho", type=float, nargs="*", default=OUTRATS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_custom_probe.json"))
    a = ap.parse_args()
    inv = abi.HipInvariant(EUCLID_SRC, 3)
    hc = abi.HipBatch(storage=abi.STORE_F32_CSC)
    hb = abi.HipBatch(storage=abi.STORE_F32_CSC)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    med = lambda v: float(np.median(v))  # noqa: E731
    cells = []
    for rho in a.rho:
        for m in a.m:
            probs = [synth.make_euclidean_problem(m, rho, seed=10000 * int(rho * 10) + 100 * m + k)
                     for k in range(a.problems)]
            plist = [(p.D1, p.D2, p.A, p.u0) for p in probs]

            def lone_loop():
                routes, kms = [], []
                for p in probs:
                    g.affinity_custom(inv, p.D1, p.D2, p.A, IPRM)
                    kms.append(g.timings().affinity_kernel_ms)
                    g.solve(p.u0)
                    routes.append(g.last_solver)
                return routes, kms

            hc.solve_custom(inv, plist, IPRM)  # warm-up of all three (first use of the sizes allocates)
            lone_loop()
            hb.solve_euclidean(plist, **INV)
            tc, tl, tb, sc, sb, lone_k = [], [], [], [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                hc.solve_custom(inv, plist, IPRM)
                tc.append((time.perf_counter() - t0) * 1e3)
                sc.append(hc.split())
                t0 = time.perf_counter()
                lone_routes, kms = lone_loop()
                tl.append((time.perf_counter() - t0) * 1e3)
                lone_k.append(sum(kms))
                t0 = time.perf_counter()
                hb.solve_euclidean(plist, **INV)
                tb.append((time.perf_counter() - t0) * 1e3)
                sb.append(hb.split())
            launches, nb, na = hc.stats()
            cell = dict(m=m, rho=rho, problems=a.problems, custom_batch_ms=med(tc), custom_loop_ms=med(tl),
                        ratio=med(tc) / med(tl), builtin_batch_ms=med(tb), custom_vs_builtin=med(tc) / med(tb),
                        custom_batch_ms_all=tc, custom_loop_ms_all=tl, builtin_batch_ms_all=tb,
                        custom_split_ms={k: med([s[k] for s in sc]) for k in sc[0]},
                        builtin_split_ms={k: med([s[k] for s in sb]) for k in sb[0]},
                        custom_fill_split=fill_split(hc, inv, plist),
                        lone_fill_kernels_ms=med(lone_k),  # the 20 lone fills' affinity_kernel_ms (kernel + build)
                        launches=launches, n_batched=nb, n_alone=na, lone_resident=int(sum(lone_routes)))
            cells.append(cell)
            print(json.dumps({k: v for k, v in cell.items() if not k.endswith("_all")}), flush=True)
    name, cus, _ = g.device_info()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=name, cus=cus, problems_per_cell=a.problems, reps=a.reps, cells=cells), f, indent=1)
    hc.close()
    hb.close()
    g.close()
    inv.close()


if __name__ == "__main__":
    main()
