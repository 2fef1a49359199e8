"""Times the semidefinite relaxation (clipper_hip_sdp) on synthetic Euclidean problems with the
bench parameters: N = 20, 64 and 128 associations, 70 % outliers, the reference's default tolerances (1e-3) and
tight ones (1e-6). One JSON line per case: the device's wall time, iterations, Jacobi sweeps, pobj / dobj and the
selection, next to the CPU model's (tests/sdp_model.py, numpy eigh) on the same M and C.

  python tools/sdp_probe.py [--out profiles/sdp_probe.json] [--sizes 20,64,128] [--reps 3]
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
from tests import sdp_model as sm  # noqa: E402


def case(n: int, eps: float, reps: int) -> dict:
    p = synth.make_euclidean_problem(n, 0.7, seed=12345)
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    prm = abi.SdpParams(eps_abs=eps, eps_rel=eps, max_iters=20000)
    g.sdp(prm)  # (first call: module load, LDS attribute)
    walls = []
    for _ in range(reps):
        t0 = time.perf_counter()
        nodes, r = g.sdp(prm)
        walls.append((time.perf_counter() - t0) * 1e3)
    M, C = g.get_affinity_matrix(), g.get_constraint_matrix()
    t0 = time.perf_counter()
    ref = sm.solve(M, C, max_iters=20000, eps_abs=eps, eps_rel=eps)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    return {"n": n, "outliers": 0.7, "eps": eps, "gpu_ms_min": min(walls), "gpu_ms_all": walls,
            "gpu_iters": r.iters, "gpu_sweeps": r.info.sweeps, "gpu_converged": r.info.converged,
            "gpu_pobj": r.pobj, "gpu_dobj": r.dobj, "gpu_rho": r.info.rho, "gpu_nodes": len(nodes),
            "gpu_ms_per_iter": r.info.t_solve * 1e3 / max(r.iters, 1),
            "cpu_model_ms": cpu_ms, "cpu_model_iters": ref["iters"], "cpu_model_pobj": ref["pobj"],
            "cpu_model_dobj": ref["dobj"], "cpu_model_nodes": len(ref["nodes"]),
            "same_nodes": nodes.tolist() == ref["nodes"]}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sdp_probe.json"))
    ap.add_argument("--sizes", default="20,64,128")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    rows = []
    for n in [int(x) for x in a.sizes.split(",")]:
        for eps in (1e-3, 1e-6):
            row = case(n, eps, a.reps)
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
