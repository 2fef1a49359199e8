"""Times the maximum-clique methods (clipper_hip_max_clique) on the synthetic Euclidean problems
with the bench parameters: m = 1 000, 2 048, 10 000 (the bench problem), 30 000 and 100 000 (under a time limit).
One JSON line per case: K, HEU's size, the clique found (omega when not timed out), roots searched / pruned, the
device time of every method, and the CPU model's time on the same graph (tests/maxclique_model.py; m <= 10 000).

  python tools/maxclique_probe.py [--out profiles/maxclique_probe.json] [--sizes 1000,2048,...] [--time-limit 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from clipper_amd import _abi as abi  # noqa: E402
from clipper_amd import synth  # noqa: E402


def case(m: int, time_limit: float, model_max_m: int) -> dict:
    p = synth.make_euclidean_problem(m, 0.95, seed=12345)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    out = {"m": m, "rho": 0.95, "time_limit_s": time_limit}
    t0 = time.perf_counter()
    g.core_numbers()
    out["core_ms"] = (time.perf_counter() - t0) * 1e3
    for name, meth in (("kcore", abi.MC_KCORE), ("heu", abi.MC_HEU), ("exact", abi.MC_EXACT)):
        nodes, info = g.max_clique(meth, time_limit=time_limit)
        out[name + "_ms"] = info.seconds * 1e3
        out[name + "_size"] = len(nodes)
        if meth == abi.MC_EXACT:
            out.update(K=info.max_core, edges=info.edges, heuristic_size=info.heuristic_size, clique=len(nodes),
                       timed_out=info.timed_out, roots_searched=info.roots_searched, roots_pruned=info.roots_pruned,
                       bb_nodes=info.bb_nodes)
    out["model_s"] = None
    if m <= model_max_m:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import maxclique_model as mm
        adj = mm.adjacency_from_matrix(g.get_constraint_matrix())
        t0 = time.perf_counter()
        core = mm.core_numbers(adj)
        heu = mm.heu(adj, core)
        w = mm.omega(adj, lower=len(heu))
        out["model_s"] = time.perf_counter() - t0
        out["model_omega"] = w
        out["model_heu"] = len(heu)
    g.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,2048,10000,30000,100000")
    ap.add_argument("--time-limit", type=float, default=30.0)
    ap.add_argument("--model-max-m", type=int, default=10000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for m in (int(x) for x in a.sizes.split(",")):
        r = case(m, a.time_limit, a.model_max_m)
        rows.append(r)
        print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump({"device": abi.HipClipper().device_info()[0], "cases": rows}, f, indent=1)


if __name__ == "__main__":
    main()
