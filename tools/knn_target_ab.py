#!/usr/bin/env python3
"""A/B of two builds of libclipper_hip.so on the calls that search a cloud (csrc/host_knn_grid.hpp's KnnTarget against
the raw-pointer index and the cloud's untyped bag before it): the device allocations each call makes (--part
allocations: counts, equal or not) and the wall times of the whole calls (--part wall), on host buffers and on
DeviceClouds, under both routes of the search.

The rounds, the alternation A, B, A2 and the reading of a wall row are tools/fill_policy_ab.py's: a row passes when
median(B) <= median(A) + the largest |A - A2| of a round.

  python tools/knn_target_ab.py --a PARENT.so --b RESULT.so [--rounds 5] [--part wall|allocations|bench]
                                [--out profiles/knn_target_ab.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import fill_policy_ab as ab  # noqa: E402

REPS = ab.FILLS  # (the harness records it as the calls behind one median)
OUT = os.path.join(ROOT, "profiles", "knn_target_ab.json")


def _scene(n):
    import numpy as np
    rng = np.random.default_rng(n)
    src = np.asfortranarray(rng.random((3, n)))
    return src, np.asfortranarray(src + rng.normal(0.0, 0.002, src.shape))


def _routes(abi):
    return (("brute", abi.KNN_BRUTE), ("grid", abi.KNN_GRID))


def child_allocations():
    """allocations (device buffers, pinned buffers, events) per call, once warmed: row -> count"""
    sys.path.insert(0, ROOT)
    from clipper_amd import _abi as abi
    out = {}
    src, tgt = _scene(2000)
    icp_kw = dict(max_distance=0.05, max_iterations=5, rel_fitness=0.0, rel_rmse=0.0)

    def count(call):
        a0 = abi.debug_live_resources()["allocations"]
        call()
        return abi.debug_live_resources()["allocations"] - a0

    for name, mode in _routes(abi):
        abi.knn_set_search(mode)
        host = {"estimate_normals": lambda: abi.estimate_normals(tgt), "fpfh_from_points": lambda: abi.fpfh_from_points(tgt),
                "estimate_covariances": lambda: abi.estimate_covariances(tgt), "icp": lambda: abi.icp(src, tgt, **icp_kw),
                "knn": lambda: abi.knn(src, tgt, 8)}
        for call, f in host.items():
            f()  # (warm: code objects, the search's events)
            out[f"host-buffer {call} n=2000 {name}"] = count(f)
        with abi.DeviceCloud(src) as cs, abi.DeviceCloud(tgt) as ct:
            # in this order under the grid route the first stage builds ct's index, the later ones query it
            cloud = {"estimate_normals": lambda: ct.estimate_normals(), "fpfh_from_points": lambda: ct.fpfh_from_points(),
                     "estimate_covariances": lambda: ct.estimate_covariances(),
                     "evaluate_registration (a K = 1 search)": lambda: cs.evaluate_registration(ct, None, 0.05)}
            for call, f in cloud.items():
                out[f"DeviceCloud {call} n=2000 {name}, first"] = count(f)
                out[f"DeviceCloud {call} n=2000 {name}, again"] = count(f)
        with abi.DeviceCloud(src) as cs, abi.DeviceCloud(tgt) as ct:
            out[f"DeviceCloud icp n=2000 {name}, first against the target"] = count(lambda: cs.icp(ct, **icp_kw))
            out[f"DeviceCloud icp n=2000 {name}, second against the target"] = count(lambda: cs.icp(ct, **icp_kw))
    print("AB_CHILD " + json.dumps(out), flush=True)


def child_wall():
    sys.path.insert(0, ROOT)
    from clipper_amd import _abi as abi
    out = {}
    icp_kw = dict(max_iterations=20, rel_fitness=0.0, rel_rmse=0.0)

    def wall_ms(call):
        call()  # (warm-up: code objects, the allocator's pools)
        ms = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            call()
            ms.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ms)

    def chain(src, tgt, maxd):
        with abi.DeviceCloud(src) as cs, abi.DeviceCloud(tgt) as ct:
            ct.estimate_normals().compute_fpfh().estimate_covariances()
            cs.icp(ct, max_distance=maxd, **icp_kw)
            cs.icp(ct, max_distance=maxd, **icp_kw)

    for n in (2000, 100000):
        src, tgt = _scene(n)
        maxd = 0.05 if n == 2000 else 0.02
        for name, mode in _routes(abi):
            abi.knn_set_search(mode)
            out[f"estimate_normals n={n} {name} (wall)"] = wall_ms(lambda: abi.estimate_normals(tgt))
            out[f"fpfh_from_points n={n} {name} (wall)"] = wall_ms(lambda: abi.fpfh_from_points(tgt))
            out[f"icp point-to-point n={n} {name}, 20 iterations (wall)"] = wall_ms(
                lambda: abi.icp(src, tgt, max_distance=maxd, **icp_kw))
            if mode == abi.KNN_GRID:
                out[f"knn K=8 n={n} grid (wall)"] = wall_ms(lambda: abi.knn(src, tgt, 8))
            out[f"DeviceCloud create, normals, FPFH, covariances, two ICPs, close n={n} {name} (wall)"] = wall_ms(
                lambda: chain(src, tgt, maxd))
    print("AB_CHILD " + json.dumps(out), flush=True)


def allocations(argv):
    """one fresh child per build; the counts must be equal row by row"""
    arg = {k: argv[argv.index(k) + 1] for k in ("--a", "--b", "--out") if k in argv}
    a = ab.run_child(os.path.abspath(arg["--a"]), "allocations")
    b = ab.run_child(os.path.abspath(arg["--b"]), "allocations")
    rows = {row: {"unit": "allocations", "parent": a[row], "result": b.get(row), "equal": a[row] == b.get(row)} for row in a}
    out = arg.get("--out", OUT)
    rec = json.load(open(out)) if os.path.exists(out) else {"what": WHAT, "rows": {}}
    rec["allocations"] = rows
    rec["allocations_all_equal"] = all(v["equal"] for v in rows.values()) and set(a) == set(b)
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for row, v in rows.items():
        print(f"{row}: parent {v['parent']} result {v['result']} {'ok' if v['equal'] else 'DIFFERENT'}")
    return 0 if rec["allocations_all_equal"] else 1


WHAT = "the search target's owner (host_knn_grid.hpp's KnnTarget): parent (A) against result (B), tools/knn_target_ab.py"

if __name__ == "__main__":
    if "--part" in sys.argv and sys.argv[sys.argv.index("--part") + 1] == "allocations":
        sys.exit(child_allocations() if "--child" in sys.argv else allocations(sys.argv))
    ab.main(parts={"wall": child_wall}, what=WHAT, out=OUT)
