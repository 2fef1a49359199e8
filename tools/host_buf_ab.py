#!/usr/bin/env python3
"""A/B of two builds of libclipper_hip.so on what the host side does around the kernels: the wall times of calls that
create, grow, reuse and release device buffers, pinned buffers and events (csrc/host_buf.hpp's owners against the raw
pointers before them), and bench.py's headline, host-buffers and m = 100 000 step times (--part bench).

The rounds, the alternation A, B, A2 and the reading of a row are tools/fill_policy_ab.py's: a row passes when
median(B) <= median(A) + the largest |A - A2| of a round.

  python tools/host_buf_ab.py --a PARENT.so --b RESULT.so [--rounds 5] [--part host|bench] [--out profiles/host_buf_ab.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fill_policy_ab as ab  # noqa: E402

REPS = 7


def child_host():
    sys.path.insert(0, ROOT)
    import numpy as np
    from clipper_amd import _abi as abi
    from clipper_amd import synth
    out = {}

    def wall_ms(call, reps=REPS):
        call()  # (warm-up: code objects, the allocator's pools)
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    def lone(p):
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
        g.solve(p.u0)
        g.close()

    for m in (512, 3000):
        p = synth.make_euclidean_problem(m, 0.9, seed=m)
        out[f"create + score + solve + close m={m} F32_CSC (wall)"] = wall_ms(lambda: lone(p))
    probs = [synth.make_euclidean_problem(512, [0.5, 0.7, 0.9][k % 3], seed=7000 + k) for k in range(20)]
    inputs = [(q.D1, q.D2, q.A, q.u0) for q in probs]

    def batch():
        b = abi.HipBatch(storage=abi.STORE_F32_CSC)
        b.solve_euclidean(inputs, **synth.EUCLID_BENCH_PARAMS)
        b.close()
    out["batch of 20 problems of m=512: create + solve + close (wall)"] = wall_ms(batch)
    rng = np.random.default_rng(7)
    src = np.asfortranarray(rng.random((3, 2000)))
    tgt = np.asfortranarray(src + rng.normal(0.0, 0.002, src.shape))
    out["icp point-to-point n=2000, 20 iterations (wall)"] = wall_ms(
        lambda: abi.icp(src, tgt, max_distance=0.05, max_iterations=20, rel_fitness=0.0, rel_rmse=0.0))
    P = np.asfortranarray(rng.random((3, 100000)))
    out["voxel_down_sample n=100000 (wall)"] = wall_ms(lambda: abi.voxel_down_sample(P, (8.0 / 100000) ** (1.0 / 3.0)))
    print("AB_CHILD " + json.dumps(out), flush=True)


if __name__ == "__main__":
    ab.main(parts={"host": child_host},
            what="the host side's owning types (host_buf.hpp): parent (A) against result (B), tools/host_buf_ab.py",
            out=os.path.join(ROOT, "profiles", "host_buf_ab.json"))
