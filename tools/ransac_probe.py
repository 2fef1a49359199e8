#!/usr/bin/env python3
"""tools/ransac_probe.py — what a RANSAC call over putative associations costs on the device (DESIGN.md section 9,
"RANSAC over putative associations"), written to profiles/ransac_probe.json.

The data: n points of a bumpy sphere and a moved, noisy copy, the identity as the good associations, scaled up to m
putative ones at 95 % outliers by generate_synthetic_correspondences. For m in --sizes, max_hypotheses 16 384 and
131 072 with the confidence stop disabled (confidence close to 1), the checker at 0.9 and at 0, one CHILD process per
cell runs clipper_hip_ransac_correspondences behind a warm-up. Per cell:
  ms_per_call        host clock around the call (it ends in a device wait), median of --reps
  device_ms          info.device_ms, two events around the device work, median
  hypotheses_per_s   hypotheses formed per second of device time; scored_per_s: the ones that passed both checks
  kernels            (--trace) per-kernel totals of one call from a rocprofv3 kernel trace of a child of its own, no
                     counters in it; checker off: score_fp64_fraction = 28 unfused fp64 operations per pair x survivors
                     x m over the score kernel's time, against the 78.6 TFLOP/s AMD states for the MI355X's fp64 vector
                     rate (a rate that counts a fused multiply-add as two; this kernel fuses nothing)
  host               the same call from ransac_rules.hpp on 16 host threads (tests/cpp/test_ransac_rules.cpp built with
                     g++ -O2 -ffp-contract=off), timed in the same run; only at max_hypotheses = 16 384
Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import shutil
import sqlite3
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402

MAX_DISTANCE, OUTLIERS, CONFIDENCE, ROUND = 0.02, 0.95, 1.0 - 1e-15, 4096
FP64_PEAK, OPS_PER_PAIR = 78.6e12, 28


def dataset(m: int, seed: int = 0):
    """(D1 3 x n, D2 3 x n, A m x 2): n = max(1000, m / 10) points, 5 % of the associations correct"""
    n = max(1000, m // 10)
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    P = v * (1.0 + 0.1 * np.sin(5.0 * v[:, :1]) * np.cos(4.0 * v[:, 1:2]))
    th = np.deg2rad(25.0)
    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    Q = P @ R.T + (0.3, -0.2, 0.5) + rng.uniform(-0.005, 0.005, (n, 3))
    good = np.stack([np.arange(n)] * 2, axis=1)
    A, _ = abi.generate_synthetic_correspondences(n, n, good, m, OUTLIERS, seed)
    return np.asfortranarray(P.T), np.asfortranarray(Q.T), np.ascontiguousarray(A)


def call(D1, D2, A, max_hypotheses, edge, round_size):
    return abi.ransac_correspondences(D1, D2, A, MAX_DISTANCE, edge_similarity=edge, max_hypotheses=max_hypotheses,
                                      confidence=CONFIDENCE, hypotheses_per_round=round_size)


def child(a):
    """one cell: a warm-up, then --reps timed calls (or, under rocprofv3, one); prints one JSON line"""
    D1, D2, A = dataset(a.m)
    call(D1, D2, A, a.max_hypotheses, a.edge, a.round)
    wall, dev, info = [], [], None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        _, info = call(D1, D2, A, a.max_hypotheses, a.edge, a.round)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(info.device_ms)
    d = statistics.median(dev)
    print(json.dumps(dict(m=a.m, max_hypotheses=a.max_hypotheses, edge_similarity=a.edge, round=a.round, reps=a.reps,
                          ms_per_call=statistics.median(wall), device_ms=d, status=info.status, evaluated=info.evaluated,
                          checked=info.checked, count=info.count, best_count=info.best_count,
                          rounds=info.evaluated // a.round, ms_per_round=d / (info.evaluated // a.round),
                          hypotheses_per_s=info.evaluated / (d * 1e-3), scored_per_s=info.checked / (d * 1e-3))), flush=True)


def spawn(args, m, max_hypotheses, edge, round_size, reps, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", "--m", str(m), "--max-hypotheses", str(max_hypotheses),
                          "--edge", str(edge), "--round", str(round_size), "--reps", str(reps)]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=600, **args)


def trace(m, max_hypotheses, edge, round_size):
    """per-kernel totals (ms) of the second of a child's two calls, from the rocpd database of a kernel trace"""
    if not shutil.which("rocprofv3"):
        return None
    out = tempfile.mkdtemp(prefix="ransac_probe_")
    r = spawn(dict(cwd=out), m, max_hypotheses, edge, round_size, 1,
              prefix=["rocprofv3", "--kernel-trace", "-d", out, "-o", "trace", "--"])
    dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith(".db")]
    if r.returncode != 0 or not dbs:
        shutil.rmtree(out, ignore_errors=True)
        return dict(error=(r.stderr or r.stdout)[-400:])
    rows = sqlite3.connect(dbs[0]).execute("select name, duration from kernels").fetchall()
    shutil.rmtree(out, ignore_errors=True)
    per = {}
    for name, dur in rows:
        short = name.split("(")[0].split("<")[0].split("::")[-1]
        if short.startswith("k_ransac"):
            per.setdefault(short, []).append(dur / 1e6)
    res = {k: dict(calls=len(v) // 2, total_ms=sum(v) / 2.0) for k, v in per.items()}   # (two identical calls: halves)
    res["kernels_ms"] = sum(v["total_ms"] for v in res.values())
    return res


def host_exe():
    out = os.path.join(ROOT, "tools", "_bin", "ransac_host")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_ransac_rules.cpp"), "-o", out])
    return out


def host(exe, m, max_hypotheses, edge, round_size, threads=16):
    D1, D2, A = dataset(m)
    P, B = np.ascontiguousarray(D1[:, A[:, 0]].T), np.ascontiguousarray(D2[:, A[:, 1]].T)
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(struct.pack("<3dq4iQ", MAX_DISTANCE, edge, CONFIDENCE, max_hypotheses, round_size, 3, 1, m, 0))
        f.write(P.tobytes())
        f.write(B.tobytes())
        f.flush()
        out = subprocess.check_output([exe, "time", f.name, str(threads)], timeout=900).decode().split()
    return dict(threads=threads, ms_per_call=float(out[1]), evaluated=int(out[3]), checked=int(out[5]), count=int(out[7]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--hypotheses", default="16384,131072")
    ap.add_argument("--edges", default="0.9,0.0")
    ap.add_argument("--rounds", default=str(ROUND), help="round sizes to time (the first is the one traced)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ransac_probe.json"))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--m", type=int, default=1000)
    ap.add_argument("--max-hypotheses", type=int, default=16384)
    ap.add_argument("--edge", type=float, default=0.9)
    ap.add_argument("--round", type=int, default=ROUND)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if abi.device_count() < 1:
        sys.exit("ransac_probe: no GPU visible (there is no fallback)")
    exe = None if a.no_host else host_exe()
    rounds = [int(s) for s in a.rounds.split(",")]
    res = dict(label=a.label, library=os.path.basename(abi.LIB_PATH), reps=a.reps, max_distance=MAX_DISTANCE, outliers=OUTLIERS,
               confidence=CONFIDENCE, fp64_peak=FP64_PEAK, ops_per_pair=OPS_PER_PAIR, cells=[])
    for m in [int(s) for s in a.sizes.split(",")]:
        for mh in [int(s) for s in a.hypotheses.split(",")]:
            for edge in [float(s) for s in a.edges.split(",")]:
                for rs in rounds:
                    r = spawn({}, m, mh, edge, rs, a.reps)
                    if r.returncode != 0:
                        sys.exit("ransac_probe: a cell failed; stopping here\n" + (r.stderr or r.stdout)[-800:])
                    cell = json.loads(r.stdout.strip().splitlines()[-1])
                    if a.trace and rs == rounds[0]:
                        cell["kernels"] = k = trace(m, mh, edge, rs)
                        if k and "kernels_ms" in k:
                            cell["host_wait_and_gaps_ms"] = cell["device_ms"] - k["kernels_ms"]
                            if edge == 0.0 and "k_ransac_score" in k:
                                ops = OPS_PER_PAIR * float(cell["checked"]) * m
                                k["score_fp64_ops_per_s"] = ops / (k["k_ransac_score"]["total_ms"] * 1e-3)
                                k["score_fp64_fraction"] = k["score_fp64_ops_per_s"] / FP64_PEAK
                    if exe and mh == 16384 and rs == rounds[0]:
                        cell["host"] = host(exe, m, mh, edge, rs)
                    res["cells"].append(cell)
                    print(json.dumps(cell), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
