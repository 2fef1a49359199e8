#!/usr/bin/env python3
"""Where a turn of the resident solver on a row view goes (unit 0): wall-clock stamps inside the kernel
(csrc/k_rv_resident.hip.h), on the headline problem.
  CLIPPER_HIP_STAMPS=1 python tools/rvr_timeline.py [--m 10000] [--rho 0.95]
columns (us, medians over the turns): candidates + pass | tail + publish | exchange | decide
then the finer breakdown of a turn (RVR_F_* in the kernel): medians per segment, and the turn time by the turn's kind
and by its number of decision rounds
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402


FINE0, FINE_TURNS = 5120, 96  # csrc/k_rv_resident.hip.h: RVR_FINE0, RVR_FINE_TURNS, RVR_F_*
F_KIND, F_ROUNDS, F_XT, F_NORMS, F_SUMS, F_TAIL, F_ROUND, F_DECIDED, F_WAVE = 0, 1, 2, 3, 4, 5, 8, 14, 16
KINDS = ("trial", "pair", "build")


def fine_breakdown(raw, rows, n):
    """Unit 0's turns at the finer stamps: medians per segment, turn time by kind and by decision rounds."""
    nt = min(n, FINE_TURNS)
    f = raw[FINE0:FINE0 + 32 * FINE_TURNS].reshape(FINE_TURNS, 32)[:nt].astype(np.float64)
    s = rows[:n + 1, :5].astype(np.float64)
    s[n, 0] = rows[500, 2]  # (the last turn ends the launch: no turn stamps row n)
    kind = f[:, F_KIND].astype(int)
    rounds = f[:, F_ROUNDS].astype(int)
    turn = (s[1:nt + 1, 0] - s[:nt, 0]) / 100.0  # turn t: its start to the next turn's start
    pas = kind != 2
    seg = {}

    def add(name, a, b, sel=None):
        sel = pas if sel is None else sel
        v = (b - a)[sel] / 100.0
        if len(v):
            seg[name] = v

    wv = f[:, F_WAVE:F_WAVE + 8]
    wmax = wv.max(axis=1)
    add("X table", s[:nt, 0], f[:, F_XT])
    add("pass, wave 0", f[:, F_XT], wv[:, 0])
    add("pass, slowest wave", f[:, F_XT], wmax)
    add("norms + barrier", wmax, f[:, F_NORMS])
    add("cross-wave sums", f[:, F_NORMS], f[:, F_SUMS])
    add("barrier after sums", f[:, F_SUMS], s[:nt, 1])
    add("tail", s[:nt, 1], f[:, F_TAIL], np.ones(nt, bool))
    add("counts published", f[:, F_TAIL], s[:nt, 2], np.ones(nt, bool))
    add("exchange", s[:nt, 2], s[:nt, 3], np.ones(nt, bool))
    add("decision round 1", s[:nt, 3], f[:, F_ROUND], np.ones(nt, bool))
    later = rounds >= 2
    if later.any():
        last = f[np.arange(nt), F_ROUND + np.maximum(rounds, 1) - 1]
        add("later rounds (per round)", f[:, F_ROUND], f[:, F_ROUND] + (last - f[:, F_ROUND]) / np.maximum(rounds - 1, 1), later)
    else:
        last = f[:, F_ROUND]
    add("after the last round", last, f[:, F_DECIDED], np.ones(nt, bool))
    add("decided to next turn", f[:, F_DECIDED], s[1:nt + 1, 0], np.ones(nt, bool))
    print(f"   finer breakdown of unit 0's turns (us; median / mean over the turns that have the segment):")
    for k, v in seg.items():
        print(f"      {k:26s} {np.median(v):6.2f} / {v.mean():6.2f}   ({len(v)} turns)")
    for k in range(3):
        sel = kind == k
        if sel.any():
            print(f"   turn time, {KINDS[k]:5s}: {sel.sum():3d} turns, median {np.median(turn[sel]):6.2f}, mean {turn[sel].mean():6.2f} us")
    for r in sorted(set(rounds[kind == 0].tolist())):
        sel = (kind == 0) & (rounds == r)
        print(f"   turn time, trial with {r} round(s): {sel.sum():3d} turns, median {np.median(turn[sel]):6.2f}, "
              f"mean {turn[sel].mean():6.2f} us")
    print("   turns: " + " ".join(f"{KINDS[k][0]}{r}:{t:.1f}" for k, r, t in zip(kind, rounds, turn)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=10000)
    ap.add_argument("--rho", type=float, default=0.95)
    ap.add_argument("--storage", default="csc")
    ap.add_argument("--units", action="store_true", help="print every unit's pass duration of turn 6")
    a = ap.parse_args()
    p = synth.make_euclidean_problem(a.m, a.rho, seed=12345)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC if a.storage == "csc" else abi.STORE_F64_CSC)
    g.stage_inputs(p.D1, p.D2, p.A)
    g.affinity_euclidean_staged(**synth.EUCLID_BENCH_PARAMS)
    g.stage_u0(p.u0)
    for _ in range(3):
        g.solve_staged()
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        sol = g.solve_staged()
        ts.append((time.perf_counter() - t0) * 1e3)
    st = g.view_stats()
    raw = g.debug_stamps().reshape(-1)
    rows = raw[:501 * 8].reshape(501, 8)
    end = rows[500]
    n = int(end[3])
    t = rows[:n, :5].astype(np.float64)
    d = np.diff(t, axis=1) / 100.0
    turn = np.diff(np.append(t[:, 0], end[2])) / 100.0
    if n < 2:
        print(f"m={a.m}: solve {np.median(ts):.3f} ms (min {min(ts):.3f}); passes {sol.n_passes}, no resident launch")
        g.close()
        return
    med = np.median(d, axis=0)
    print(f"m={a.m} wgs={os.environ.get('CLIPPER_HIP_VIEW_RESIDENT_WGS', 'auto')}: solve {np.median(ts):.3f} ms (min {min(ts):.3f}); "
          f"passes {sol.n_passes} ({st.view_passes} on a view of {st.rows} rows), resident launches {st.resident_launches}, turns {n}")
    print(f"   per turn: candidates+pass {med[0]:.2f} | tail+publish {med[1]:.2f} | exchange {med[2]:.2f} | decide {med[3]:.2f} "
          f"| turn to turn {np.median(turn):.2f} (mean {turn.mean():.2f}, p90 {np.percentile(turn, 90):.2f}) us")
    fine_breakdown(raw, rows, n)
    per = raw[4096:4096 + 4 * 256].reshape(256, 4).astype(np.float64)
    per = per[per[:, 0] > 0]
    if len(per) and n > 6:
        t0 = per[:, 0].min()
        rel = (per - t0) / 100.0
        for name, c in (("turn start", 0), ("pass done", 1), ("published", 2), ("gathered", 3)):
            v = rel[:, c]
            print(f"   turn 6, all {len(per)} units, {name:11s}: min {v.min():6.2f}  p50 {np.median(v):6.2f}  p90 {np.percentile(v, 90):6.2f}  max {v.max():6.2f} us"
                  + (f"   (slowest units: {np.argsort(-v)[:6].tolist()})" if c == 1 else ""))
        pd = rel[:, 1] - rel[:, 0]
        if a.units:   # every unit's pass of turn 6 (beside CLIPPER_HIP_RESIDENT_DEBUG=2's plan lines on stderr)
            for i, v in enumerate(pd):
                print(f"unit {i} pass_us {v:.2f}")
        print(f"   turn 6, pass duration per unit: min {pd.min():.2f} p50 {np.median(pd):.2f} p90 {np.percentile(pd, 90):.2f} max {pd.max():.2f} us")
    print(f"   launch: slices -> LDS {(end[1] - end[0]) / 100:.2f} us, loop {(end[2] - end[1]) / 100:.2f} us, total {(end[2] - end[0]) / 100:.2f} us")
    g.close()


if __name__ == "__main__":
    main()
