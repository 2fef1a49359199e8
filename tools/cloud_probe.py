#!/usr/bin/env python3
"""tools/cloud_probe.py — what keeping the clouds on the device saves from raw scan to refined transform (DESIGN.md
section 9, "Clouds on the device"), written to profiles/cloud_probe.json.

For n in --sizes (default 10 000, 100 000, 1 000 000): two jittered resamplings of the bunny fixture
(tests/golden/bunny_points_4096.f32, scaled to the unit cube; the second moved by 3 degrees and 0.02) run the chain
  voxel -> normals + FPFH -> match -> stage + Euclidean fill + solve -> transform -> point-to-plane ICP
once through the host-buffer calls and once through handles (DeviceCloud / DevicePairs), in the same process, after a
warm-up of both, as medians of --reps (5) runs. The voxel size is fixed (0.02), so the down-sampled clouds saturate at
the number of occupied voxels of the shell around the model and the brute-force descriptor match stays affordable at
every size: no size stops early. The probe ASSERTS that both chains return the same bytes (pairs, distances, selected
set, closed-form transform, refined transform, ICP history). Per stage and for the whole chain it reports
  host_ms / handle_ms   the wall time of the calls (time.perf_counter around them; every call has waited for the device)
  device_ms             what the stage itself measures between two events, where it does (voxel kernels, the ICP loop);
                        null for the other stages and for the chain: the probe puts no events of its own around them
  host_bytes / handle_bytes   ESTIMATES of what the calls move over the bus: not measured, but counted from the sizes of
                        the arrays each call takes and returns (the formulas stand beside each stage below)
  ratio                 host_ms / handle_ms
--host-only times the host-buffer chain alone: with CLIPPER_HIP_LIB naming the parent commit's build it gives the
"before" of the host-buffer calls on the same machine; --label names the build in the output (default: "this build").
Needs a GPU; there is no fallback."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import registration as reg  # noqa: E402

VOXEL, SIGMA, EPS, MAXD = 0.02, 0.01, 0.04, 0.04
STAGES = ["voxel", "features", "match", "solve", "transform", "icp"]


def scans(n: int, seed: int = 0):
    base = np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_points_4096.f32"), dtype=np.float32).reshape(-1, 3)
    base = reg.scale_to_cube(base.astype(np.float64), 1.0)
    rng = np.random.default_rng(seed)
    th = np.deg2rad(3.0)
    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    P0 = base[rng.integers(len(base), size=n)] + rng.uniform(-0.004, 0.004, (n, 3))
    P1 = (base[rng.integers(len(base), size=n)] + rng.uniform(-0.004, 0.004, (n, 3))) @ R.T + 0.02
    return np.asfortranarray(P0.T), np.asfortranarray(P1.T)


class Clock:
    def __init__(self):
        self.ms, self.dev, self.bytes = {}, {}, {}

    def stage(self, name, fn, nbytes=0, dev=None):
        t0 = time.perf_counter()
        out = fn()
        self.ms[name] = (time.perf_counter() - t0) * 1e3
        self.bytes[name] = self.bytes.get(name, 0) + int(nbytes(out) if callable(nbytes) else nbytes)
        if dev is not None:
            self.dev[name] = float(dev(out))
        return out


def _solve(g, u0):
    g.affinity_euclidean_staged(sigma=SIGMA, epsilon=EPS)
    g.stage_u0(u0)
    s = g.solve_staged()
    return g.get_selected_associations(), s


def host_chain(P0, P1, g, c: Clock):
    n = P0.shape[1]
    v0, v1 = c.stage("voxel", lambda: (abi.voxel_down_sample(P0, VOXEL, return_info=True), abi.voxel_down_sample(P1, VOXEL, return_info=True)),
                     nbytes=lambda o: 2 * 24 * n + 24 * (o[0][0].shape[1] + o[1][0].shape[1]),
                     dev=lambda o: o[0][1].kernels_ms + o[1][1].kernels_ms)
    Q0, Q1 = v0[0], v1[0]
    m0, m1 = Q0.shape[1], Q1.shape[1]
    (F0, N0), (F1, N1) = c.stage("features", lambda: (abi.fpfh_from_points(Q0), abi.fpfh_from_points(Q1)),
                                 nbytes=(24 + 33 * 8 + 24) * (m0 + m1))
    A, sqd = c.stage("match", lambda: abi.match_descriptors(F0, F1, knn=1, mutual=True),
                     nbytes=40 * 8 * (m0 + m1) + 12 * (m0 + m1))   # padded rows up; forward and backward lists (K = 1) down
    u0 = np.random.default_rng(1).random(len(A))

    def solve():
        g.stage_inputs(Q0, Q1, A)
        return _solve(g, u0)
    sel, s = c.stage("solve", solve, nbytes=24 * (m0 + m1) + 8 * len(A) + 16 * len(A))
    T = c.stage("transform", lambda: abi.estimate_rigid_transform(Q0, Q1, sel), nbytes=0)
    Ti, info = c.stage("icp", lambda: abi.icp(Q0, Q1, T_init=T, method=abi.ICP_POINT_TO_PLANE, N_tgt=N1, max_distance=MAXD),
                       nbytes=24 * m0 + 48 * m1, dev=lambda o: o[1].device_ms)
    return dict(A=A, sqd=sqd, sel=sel, u=s.u, T=T, Ti=Ti, hist=info.history, m0=m0, m1=m1, pairs=len(A), selected=len(sel),
                fitness=info.fitness, rmse=info.inlier_rmse, iterations=info.iterations)


def handle_chain(P0, P1, g, c: Clock):
    n = P0.shape[1]

    def voxel():
        with abi.DeviceCloud(P0) as r0, abi.DeviceCloud(P1) as r1:
            (q0, i0), (q1, i1) = r0.voxel_down_sample(VOXEL, return_info=True), r1.voxel_down_sample(VOXEL, return_info=True)
        return q0, q1, i0.kernels_ms + i1.kernels_ms
    q0, q1, _ = c.stage("voxel", voxel, nbytes=2 * 24 * n, dev=lambda o: o[2])
    with q0, q1:
        m0, m1 = len(q0), len(q1)
        c.stage("features", lambda: (q0.fpfh_from_points(), q1.fpfh_from_points()), nbytes=0)
        pairs = c.stage("match", lambda: q0.match(q1, knn=1, mutual=True), nbytes=4)
        with pairs:
            m = len(pairs)
            u0 = np.random.default_rng(1).random(m)

            def solve():
                g.stage_inputs_clouds(q0, q1, pairs)
                return _solve(g, u0)
            sel, s = c.stage("solve", solve, nbytes=8 * m + 8 + 16 * m)
            k = len(sel)
            T = c.stage("transform", lambda: abi.estimate_rigid_transform(q0.gather_points(sel[:, 0]), q1.gather_points(sel[:, 1]),
                                                                          np.stack([np.arange(k)] * 2, axis=1)),
                        nbytes=2 * (4 + 24) * k)
            Ti, info = c.stage("icp", lambda: q0.icp(q1, T_init=T, method=abi.ICP_POINT_TO_PLANE, max_distance=MAXD), nbytes=128 + 64,
                               dev=lambda o: o[1].device_ms)
            A, sqd = pairs.download()
    return dict(A=A, sqd=sqd, sel=sel, u=s.u, T=T, Ti=Ti, hist=info.history, m0=m0, m1=m1, pairs=len(A), selected=len(sel),
                fitness=info.fitness, rmse=info.inlier_rmse, iterations=info.iterations)


def median_of(clocks, field):
    return {k: statistics.median(getattr(c, field)[k] for c in clocks) for k in getattr(clocks[0], field)}


def spread_of(clocks):
    tot = [sum(c.ms.values()) for c in clocks]
    return [min(tot), max(tot)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10000, 100000, 1000000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--search", choices=["brute", "grid", "auto"], default="auto")
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--label", default="this build", help="names the library under test in the output")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_probe.json"))
    a = ap.parse_args()
    abi.knn_set_search({"brute": abi.KNN_BRUTE, "grid": abi.KNN_GRID, "auto": abi.KNN_AUTO}[a.search])
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    name = g.device_info()[0]
    rows = []
    for n in a.sizes:
        P0, P1 = scans(n)
        chains = [("host", host_chain)] + ([] if a.host_only else [("handle", handle_chain)])
        res, clocks = {}, {}
        for label, fn in chains:
            fn(P0, P1, g, Clock())                                   # warm-up
            clocks[label] = []
            for _ in range(a.reps):
                c = Clock()
                res[label] = fn(P0, P1, g, c)
                clocks[label].append(c)
        h = res["host"]
        row = dict(n=n, voxel_size=VOXEL, search=a.search, points_after_voxel=[h["m0"], h["m1"]], pairs=h["pairs"],
                   selected=h["selected"], icp_iterations=h["iterations"], fitness=h["fitness"], inlier_rmse=h["rmse"], stages={})
        hm, hb, hd = median_of(clocks["host"], "ms"), clocks["host"][0].bytes, median_of(clocks["host"], "dev")
        row["host_chain_ms"], row["host_chain_ms_spread"] = sum(hm.values()), spread_of(clocks["host"])
        row["host_chain_bytes"] = sum(hb.values())
        if not a.host_only:
            d = res["handle"]
            same = all(np.asarray(h[k]).tobytes() == np.asarray(d[k]).tobytes() for k in ("A", "sqd", "sel", "u", "T", "Ti", "hist"))
            assert same, f"n = {n}: the two chains differ"
            row["same_bytes"] = True
            dm, db, dd = median_of(clocks["handle"], "ms"), clocks["handle"][0].bytes, median_of(clocks["handle"], "dev")
            row["handle_chain_ms"], row["handle_chain_ms_spread"] = sum(dm.values()), spread_of(clocks["handle"])
            row["handle_chain_bytes"] = sum(db.values())
            row["ratio"] = row["host_chain_ms"] / row["handle_chain_ms"]
        for s in STAGES:
            row["stages"][s] = dict(host_ms=hm[s], host_bytes=hb[s], host_device_ms=hd.get(s))
            if not a.host_only:
                row["stages"][s].update(handle_ms=dm[s], handle_bytes=db[s], handle_device_ms=dd.get(s), ratio=hm[s] / dm[s])
        rows.append(row)
        print(json.dumps(row), flush=True)
    g.close()
    out = dict(device=name, reps=a.reps, library=a.label, host_only=a.host_only,
               notes=dict(device_ms="only where a stage reports its own event pair (voxel, icp); null elsewhere, none for the chain",
                          bytes="estimates from array sizes, not measured"),
               rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
