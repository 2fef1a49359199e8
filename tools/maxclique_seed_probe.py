"""Times the seeded maximum-clique call (clipper_hip_max_clique_seeded, DESIGN.md section 9 "Seeded calls") against
the unseeded one on the synthetic Euclidean problems with the bench parameters (95 % outliers, F32 slices): m = 1 000,
2 048, 10 000 (the bench problem) and 30 000, under a time limit. Per size, in one run: the unseeded EXACT call, then
solve(), then the calls seeded with solve()'s node list. One JSON line per size: the seed given / kept / the seed
clique, the clique found (omega when not timed out), roots searched / pruned and B&B nodes of both EXACT calls, and the
wall time of the KCORE, HEU, SEED_ONLY and EXACT calls (each includes the graph build and the core numbers, which every
call redoes, so the differences are the phases). Only the clique calls are inside the timed regions; a call is warmed
up once and the best of three is kept, unless one call takes more than 5 s (then it is run once).

  python tools/maxclique_seed_probe.py [--out profiles/maxclique_seed_probe.json] [--sizes 1000,...] [--time-limit 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402


def best_of(call, repeat_below_s: float = 5.0):
    """(best wall ms, the last result); the first call is the warm-up unless it alone takes repeat_below_s"""
    t0 = time.perf_counter()
    res = call()
    first = time.perf_counter() - t0
    if first >= repeat_below_s:
        return first * 1e3, res, 1
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        res = call()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3, res, 3


def case(m: int, time_limit: float) -> dict:
    p = synth.make_euclidean_problem(m, 0.95, seed=12345)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    out = {"m": m, "rho": 0.95, "time_limit_s": time_limit}

    def counters(prefix, nodes, info):
        out.update({prefix + "clique": len(nodes), prefix + "timed_out": info.timed_out,
                    prefix + "heuristic_size": info.heuristic_size, prefix + "roots_searched": info.roots_searched,
                    prefix + "roots_pruned": info.roots_pruned, prefix + "bb_nodes": info.bb_nodes})

    ms, (nodes, info), n = best_of(lambda: g.max_clique(abi.MC_EXACT, time_limit=time_limit))
    out.update(K=info.max_core, edges=info.edges, unseeded_exact_ms=ms, unseeded_exact_runs=n)
    counters("unseeded_", nodes, info)
    unseeded = nodes.tolist()
    out["kcore_ms"] = best_of(lambda: g.max_clique(abi.MC_KCORE))[0]
    out["unseeded_heu_ms"] = best_of(lambda: g.max_clique(abi.MC_HEU, time_limit=time_limit))[0]

    t0 = time.perf_counter()
    sol = g.solve(p.u0)
    out["solve_ms"] = (time.perf_counter() - t0) * 1e3  # (one call, not warmed up: reported, not compared)
    seed = sol.nodes.tolist()
    out["solve_nodes"] = len(seed)

    ms, (nodes, info, si), _ = best_of(lambda: g.max_clique(abi.MC_SEED_ONLY, seed=seed))
    out.update(seed_only_ms=ms, seed_given=si.seed_given, seed_kept=si.seed_kept, seed_size=si.seed_size)
    ms, (nodes, info, si), _ = best_of(lambda: g.max_clique(abi.MC_HEU, time_limit=time_limit, seed=seed))
    out.update(seeded_heu_ms=ms, seeded_heu_size=len(nodes), seeded_heu_winner=si.winner)
    ms, (nodes, info, si), n = best_of(lambda: g.max_clique(abi.MC_EXACT, time_limit=time_limit, seed=seed))
    out.update(seeded_exact_ms=ms, seeded_exact_runs=n, winner=si.winner)
    counters("seeded_", nodes, info)
    out["same_list_as_unseeded"] = nodes.tolist() == unseeded
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,2048,10000,30000")
    ap.add_argument("--time-limit", type=float, default=30.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for m in (int(x) for x in a.sizes.split(",")):
        r = case(m, a.time_limit)
        rows.append(r)
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump({"device": abi.HipClipper().device_info()[0], "cases": rows}, f, indent=1)


if __name__ == "__main__":
    main()
