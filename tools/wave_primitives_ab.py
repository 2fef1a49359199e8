#!/usr/bin/env python3
"""A/B of two builds of libclipper_hip.so on the kernels that share k_wave.hip.h's folds and scans: the device times of
the point-cloud front end (the grid search with its cell-table scan, the brute-force search, voxel down-sampling with
its sort, ICP, descriptor matching), and bench.py's headline and m = 100 000 step times (--part bench).

The rounds, the alternation A, B, A2 and the reading of a row are tools/fill_policy_ab.py's: a row passes when
median(B) <= median(A) + the largest |A - A2| of a round.

  python tools/wave_primitives_ab.py --a PARENT.so --b RESULT.so [--rounds 5] [--part frontend|bench]
                                     [--out profiles/wave_primitives_ab.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fill_policy_ab as ab  # noqa: E402

REPS = 5


def child_frontend():
    sys.path.insert(0, ROOT)
    import numpy as np
    from clipper_amd import _abi as abi
    out = {}

    def median_of(call, reps=REPS):
        call()  # (warm-up: buffers, code objects)
        return statistics.median(call() for _ in range(reps))

    def knn_ms(Q, P, K, mode):
        abi.knn_set_search(mode)
        abi.knn(Q, P, K)
        return abi.knn_last_search().kernels_ms

    rng = np.random.default_rng(7)
    P10k, Q10k = np.asfortranarray(rng.random((3, 10000))), np.asfortranarray(rng.random((3, 10000)))
    for K in (1, 8):
        out[f"knn brute force 10k x 10k K={K}, kernels"] = median_of(lambda: knn_ms(Q10k, P10k, K, abi.KNN_BRUTE))
    for n in (100000, 1000000):
        P = np.asfortranarray(rng.random((3, n)))
        for K in (1, 16):
            out[f"knn grid self-search n={n} K={K}, kernels (bin + scan + slabs + query)"] = median_of(
                lambda: knn_ms(P, P, K, abi.KNN_GRID))
        vs = (8.0 / n) ** (1.0 / 3.0)  # about 8 points per occupied voxel of the unit cube

        def voxel(which):
            return getattr(abi.voxel_down_sample(P, vs, return_info=True)[1], which)
        out[f"voxel n={n}, kernels"] = median_of(lambda: voxel("kernels_ms"))
        out[f"voxel n={n}, sort passes (hist + row scan + scatter)"] = median_of(lambda: voxel("sort_ms"))
    abi.knn_set_search(abi.KNN_GRID)
    src = np.asfortranarray(P[:, :100000])
    tgt = np.asfortranarray(src + rng.normal(0.0, 0.002, src.shape))
    out["icp point-to-point n=100000, 20 iterations, device loop"] = median_of(
        lambda: abi.icp(src, tgt, max_distance=0.05, max_iterations=20, rel_fitness=0.0, rel_rmse=0.0)[1].device_ms, 3)
    F0, F1 = np.asfortranarray(rng.random((33, 10000))), np.asfortranarray(rng.random((33, 10000)))

    def match():
        t0 = time.perf_counter()
        abi.match_descriptors(F0, F1, knn=1, mutual=True)
        return (time.perf_counter() - t0) * 1e3
    out["match 10k x 10k d=33 K=1 mutual, whole call (wall)"] = min(match() for _ in range(REPS + 1))
    print("AB_CHILD " + json.dumps(out), flush=True)


if __name__ == "__main__":
    ab.main(parts={"frontend": child_frontend},
            what="k_wave.hip.h's shared folds and scans: parent (A) against result (B), tools/wave_primitives_ab.py",
            out=os.path.join(ROOT, "profiles", "wave_primitives_ab.json"))
