"""Times the wide route of the semidefinite relaxation (clipper_hip_sdp_set_route, DESIGN.md section 11 "The wide
route") beside the workgroup route and the host model: synthetic Euclidean problems with the bench parameters, 70 %
outliers, the reference's default tolerances (1e-3). At n = 64 and 128 both routes run, alternating in one process;
at n = 129, 256, 512 and 1024 the wide route alone. One warm-up per route and size, then the medians of --rounds
rounds. One JSON line per size and route: the whole solve, ms per iteration, Jacobi sweeps per iteration, launches per
iteration (wide route: every sweep is np launches, an iteration has 7 more, 5 in the first; the sweeps of the dual
checks are counted, their 5 fixed launches and the rescalings of U are not), next to the numpy model
(tests/sdp_model.py) timed on the host in the same run for the same iterations.
A solve that is still iterating after --time-limit seconds stops there (timed_out) and reports what it has.

  python tools/sdp_wide_probe.py [--out profiles/sdp_wide_probe.json] [--both 64,128] [--wide 129,256,512,1024]
                                 [--rounds 5] [--time-limit 8]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402
from tests import sdp_model as sm  # noqa: E402

ROUTE_NAMES = {abi.SDP_ROUTE_WORKGROUP: "workgroup", abi.SDP_ROUTE_WIDE: "wide"}


def solve(M, C, prm, route):
    abi.sdp_set_route(route)
    try:
        t0 = time.perf_counter()
        r = abi.sdp_solve(M, C, prm)
        return (time.perf_counter() - t0) * 1e3, r
    finally:
        abi.sdp_set_route(abi.SDP_ROUTE_WORKGROUP)


def case(n: int, routes: list, rounds: int, time_limit: float) -> list:
    p = synth.make_euclidean_problem(n, 0.7, seed=12345)
    g = abi.HipClipper(storage=abi.STORE_F64)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    M, C = g.get_affinity_matrix(), g.get_constraint_matrix()
    prm = abi.SdpParams(eps_abs=1e-3, eps_rel=1e-3, max_iters=20000, time_limit_secs=time_limit)
    for route in routes:  # warm-up: module load, allocations
        solve(M, C, prm, route)
    walls = {route: [] for route in routes}
    per_iter = {route: [] for route in routes}
    last = {}
    for _ in range(rounds):
        for route in routes:  # alternating
            ms, r = solve(M, C, prm, route)
            walls[route].append(ms)
            per_iter[route].append(r.info.t_solve * 1e3 / max(r.iters, 1))
            last[route] = r
    iters = max(r.iters for r in last.values())
    t0 = time.perf_counter()
    ref = sm.solve(M, C, max_iters=iters, eps_abs=1e-3, eps_rel=1e-3)
    model_ms = (time.perf_counter() - t0) * 1e3
    np_ = n + (n & 1)
    rows = []
    for route in routes:
        r = last[route]
        sweeps = r.info.sweeps / max(r.iters, 1)
        rows.append({
            "n": n, "outliers": 0.7, "eps": 1e-3, "route": ROUTE_NAMES[route], "rounds": rounds,
            "solve_ms_median": statistics.median(walls[route]), "solve_ms_all": walls[route],
            "ms_per_iter_median": statistics.median(per_iter[route]),
            "iters": r.iters, "converged": r.info.converged, "timed_out": r.info.timed_out,
            "sweeps_per_iter": sweeps,
            "launches_per_iter": sweeps * np_ + 7 if route == abi.SDP_ROUTE_WIDE else 1.0 / 8,
            "pobj": r.pobj, "dobj": r.dobj, "nodes": len(r.nodes),
            "model_ms": model_ms, "model_iters": ref["iters"], "model_ms_per_iter": model_ms / max(ref["iters"], 1),
            "model_pobj": ref["pobj"], "same_nodes_as_model": r.nodes.tolist() == ref["nodes"],
        })
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdp_wide_probe.json"))
    ap.add_argument("--both", default="64,128")
    ap.add_argument("--wide", default="129,256,512,1024")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--time-limit", type=float, default=8.0)
    a = ap.parse_args()
    plan = [(int(x), [abi.SDP_ROUTE_WORKGROUP, abi.SDP_ROUTE_WIDE]) for x in a.both.split(",") if x]
    plan += [(int(x), [abi.SDP_ROUTE_WIDE]) for x in a.wide.split(",") if x]
    rows = []
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for n, routes in plan:
        for row in case(n, routes, a.rounds, a.time_limit):
            print(json.dumps(row), flush=True)
            rows.append(row)
        with open(a.out, "w") as f:  # (rewritten after every size: a long run leaves what it has)
            for row in rows:
                f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
