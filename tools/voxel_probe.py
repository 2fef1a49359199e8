#!/usr/bin/env python3
"""What clipper_hip_voxel_downsample costs ("Voxel down-sampling"), on the clouds of tools/knn_grid_probe.py
(a uniform cube, and the bunny fixture resampled to the target size) at n = 100 000 and 1 000 000, with voxel_size
chosen by bisection so that an occupied voxel holds about 8 points.

  call_ms          the whole call, host arrays in, host arrays out (points, counts, trace): wall clock
  kernels_ms       between two events around the call's kernels (clipper_voxel_info_t.kernels_ms)
  sort_ms          of that, the passes of the radix sort (clipper_voxel_info_t.sort_ms); per pass, as keys per second,
                   and as bytes per second against the HBM peak: a pass reads the keys for the histogram (8 n bytes),
                   reads the pairs (12 n) and writes them (12 n), and writes and reads twice the [digit][tile] table
  host_ms          the same call restated on one host thread with std::stable_sort (tests/cpp/test_voxel_rules.cpp,
                   -O2): checks, keys, sort, segments, sums; the result is compared with the device's, bit for bit
All times are medians of `reps` runs after a warm-up. No ratio is fixed in advance: the tool reports.

  python tools/voxel_probe.py [--out profiles/voxel_probe.json] [--sizes 100000,1000000] [--reps 7]
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402
from tools.knn_grid_probe import surface, uniform  # noqa: E402

HBM_PEAK = 8.0e12     # bytes per second (HBM3E, spec: DESIGN.md 4)
TARGET = 8.0          # points per occupied voxel


def call(Pt, vs):
    return abi.voxel_down_sample(Pt, vs, return_counts=True, return_trace=True, return_info=True)


def voxel_size_for(Pt, target=TARGET):
    """bisection on voxel_size until n / n_out is within 2 % of the target"""
    n = Pt.shape[1]
    ext = float((Pt.max(axis=1) - Pt.min(axis=1)).max())
    lo, hi = ext * 1e-4, ext
    for _ in range(40):
        mid = (lo * hi) ** 0.5
        per = n / call(Pt, mid)[0].shape[1]
        if abs(per - target) <= 0.02 * target:
            return mid
        lo, hi = (mid, hi) if per < target else (lo, mid)
    return mid


def host_program(tmp):
    exe = os.path.join(tmp, "voxel_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_voxel_rules.cpp"), "-o", exe])
    return exe


def host_run(exe, tmp, P, vs, reps):
    """(median host_ms, points n_out x 3, counts, trace) of the single-thread restatement"""
    n = len(P)
    pf, of = os.path.join(tmp, "P.f64"), os.path.join(tmp, "out.bin")
    np.ascontiguousarray(P).tofile(pf)
    ms = []
    for _ in range(reps):
        out = subprocess.check_output([exe, str(n), pf, "-", repr(float(vs)), of], timeout=600).decode().split("\n")
        assert "voxel rules ok" in out
        ms.append(float([ln for ln in out if ln.startswith("host_ms")][0].split()[1]))
    raw = open(of, "rb").read()
    m = int(np.frombuffer(raw, np.int64, 1)[0])
    pts = np.frombuffer(raw, np.float64, 3 * m, 40).reshape(m, 3)
    cnt = np.frombuffer(raw, np.int32, m, 40 + 24 * m)
    trace = np.frombuffer(raw, np.int32, n, 40 + 28 * m)
    return float(np.median(ms)), pts, cnt, trace


def one(cloud, P, reps, exe, tmp):
    n = len(P)
    Pt = np.asfortranarray(P.T)
    vs = voxel_size_for(Pt)
    wall, dev, srt = [], [], []
    for k in range(reps + 1):
        t0 = time.perf_counter()
        pts, cnt, trace, info = call(Pt, vs)
        t1 = time.perf_counter()
        if k:
            wall.append((t1 - t0) * 1e3)
            dev.append(info.kernels_ms)
            srt.append(info.sort_ms)
    host_ms, hp, hc, ht = host_run(exe, tmp, P, vs, min(reps, 3))
    assert np.ascontiguousarray(pts.T).tobytes() == hp.tobytes() and np.array_equal(cnt, hc) and np.array_equal(trace, ht), \
        "the device and the host restatement differ"
    passes, ntiles = int(info.passes), -(-n // int(info.sort_tile))
    sort_ms = float(np.median(srt))
    pass_s = sort_ms * 1e-3 / max(passes, 1)
    pass_bytes = n * (8 + 12 + 12) + 4 * 256 * ntiles * 4
    row = dict(cloud=cloud, n=n, voxel_size=vs, n_out=int(pts.shape[1]), points_per_voxel=n / pts.shape[1],
               max_count=int(info.max_count), dim=[int(x) for x in info.dim], passes=passes, sort_tile=int(info.sort_tile),
               call_ms=float(np.median(wall)), kernels_ms=float(np.median(dev)), sort_ms=sort_ms,
               sort_keys_per_s_per_pass=n / pass_s, sort_pass_bytes=pass_bytes,
               sort_pass_fraction_of_hbm_peak=pass_bytes / pass_s / HBM_PEAK,
               host_stable_sort_ms=host_ms, equal_to_host=True,
               speedup_call=host_ms / float(np.median(wall)), speedup_kernels=host_ms / float(np.median(dev)))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_probe.json"))
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    res = dict(library=os.path.basename(abi.LIB_PATH), reps=a.reps, hbm_peak_bytes_per_s=HBM_PEAK, target_points_per_voxel=TARGET,
               table=[])
    with tempfile.TemporaryDirectory() as tmp:
        exe = host_program(tmp)
        for n in [int(s) for s in a.sizes.split(",") if s]:
            for cloud, make in (("uniform", uniform), ("surface", surface)):
                res["table"].append(one(cloud, make(n, n), a.reps, exe, tmp))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
