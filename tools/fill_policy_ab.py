#!/usr/bin/env python3
"""A/B of two builds of libclipper_hip.so on the affinity fill: `affinity_kernel_ms` (clipper_hip_get_timings) of every
fill kernel family on synthetic problems at 95 % outliers, and bench.py's headline and m = 100 000 step times.

Every measurement runs in a fresh child process (CLIPPER_HIP_LIB selects the build): one warm-up fill, then the median
of FILLS timed fills. The builds alternate — A, B, and A once more as `A2` — for ROUNDS rounds; a row's figure is the
median of its round medians, and the largest |A - A2| between the two series of the SAME build within a round is the
row's noise figure (`spread`). B passes a row when median(B) <= median(A) + spread. That is the widest reading of "spread
between round medians", so each row also records the narrow one (`parent_median_gap` = |median(A) - median(A2)|) and
in how many rounds B was above both A and A2 (`rounds_result_slowest`): a sign that holds in every round is not noise,
whatever the spread says.

  python tools/fill_policy_ab.py --a PARENT.so --b RESULT.so --a-commit X --b-commit Y [--rounds 5] [--part kernels|bench]
                                 [--out profiles/fill_policy_ab.json]
A second --part run merges its rows into the same file."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = 7

# row -> (invariant, m, storage, shards, CLIPPER_HIP_AFFINITY mode, the fill kernel it runs)
ROWS = {
    "euclid m=10000 F32_CSC": ("euclid", 10000, "F32_CSC", 1, None, "k_affinity_sym<EuclidInv<3>, float>"),
    "euclid m=30000 F32_CSC": ("euclid", 30000, "F32_CSC", 1, None, "k_affinity_sym<EuclidInv<3>, float>"),
    "euclid m=10000 F64_CSC": ("euclid", 10000, "F64_CSC", 1, None, "k_affinity_sym<EuclidInv<3>, double>"),
    "euclid m=10000 F64_CSC 2 shards": ("euclid", 10000, "F64_CSC", 2, None, "k_affinity_rect<EuclidInv<3>, double, 64>"),
    "euclid m=10000 F32_CSC 2 shards": ("euclid", 10000, "F32_CSC", 2, None, "k_affinity_rect<EuclidInv<3>, float, 128>"),
    "euclid m=10000 F64 dense": ("euclid", 10000, "F64", 1, None, "k_affinity_compact<double, EuclidInv<3>>"),
    "euclid m=10000 F64 dense plain": ("euclid", 10000, "F64", 1, "plain", "k_affinity_plain<double, EuclidInv<3>>"),
    "pointnormal m=10000 F32_CSC": ("pointnormal", 10000, "F32_CSC", 1, None, "k_affinity_sym<PointNormalInv, float>"),
    "pointnormal m=10000 F32_CSC 2 shards": ("pointnormal", 10000, "F32_CSC", 2, None, "k_affinity_rect<PointNormalInv, float, 128>"),
    "pointnormal m=10000 F64_CSC 2 shards": ("pointnormal", 10000, "F64_CSC", 2, None, "k_affinity_rect<PointNormalInv, double, 64>"),
}


def child_kernels():
    sys.path.insert(0, ROOT)
    from clipper_amd import _abi as abi
    from clipper_amd import synth
    problems = {}
    out = {}
    for row, (inv, m, storage, shards, mode, _) in ROWS.items():
        if (inv, m) not in problems:
            make = synth.make_euclidean_problem if inv == "euclid" else synth.make_pointnormal_problem
            problems[(inv, m)] = make(m, 0.95, seed=12345)
        p = problems[(inv, m)]
        if mode:
            os.environ["CLIPPER_HIP_AFFINITY"] = mode
        else:
            os.environ.pop("CLIPPER_HIP_AFFINITY", None)
        g = abi.HipClipper(storage=getattr(abi, "STORE_" + storage), group=[0] * shards if shards > 1 else None)
        ms = []
        for k in range(FILLS + 1):
            if inv == "euclid":
                g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
            else:
                g.score_pairwise_consistency_pointnormal(p.D1, p.D2, p.A, **p.meta["invariant"])
            if k > 0:  # (the first fill sizes the arenas and warms the code up)
                ms.append(g.timings().affinity_kernel_ms)
        g.close()
        out[row] = statistics.median(ms)
    print("AB_CHILD " + json.dumps(out), flush=True)


def run_child(lib, part):
    env = dict(os.environ, CLIPPER_HIP_LIB=lib)
    env.pop("CLIPPER_HIP_AFFINITY", None)
    if part != "bench":  # (the tool that was started: tools/wave_primitives_ab.py brings a part of its own)
        r = subprocess.run([sys.executable, os.path.abspath(sys.argv[0]), "--child", "--part", part], env=env,
                           capture_output=True, text=True, timeout=300)
        line = next((l for l in r.stdout.splitlines() if l.startswith("AB_CHILD ")), None)
        if r.returncode != 0 or line is None:
            raise SystemExit(f"child failed ({r.returncode}) on {lib}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        return json.loads(line[len("AB_CHILD "):])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "10", "--warmup", "2",
                        "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=400, cwd=ROOT)
    line = next((l for l in reversed(r.stdout.splitlines()) if l.startswith("{")), None)
    if r.returncode != 0 or line is None:
        raise SystemExit(f"bench.py failed ({r.returncode}) on {lib}:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    j = json.loads(line)
    rows = {"bench.py headline step (m=10000)": j["value"], "bench.py m=100000 step": j["scaling_probe"]["ms_per_step"]}
    if "ms_per_step_host_buffers" in j:  # (the same step with its inputs in host memory: what the host side costs)
        rows["bench.py headline step from host buffers (m=10000)"] = j["ms_per_step_host_buffers"]
    return rows


def main(parts=None, what="affinity fill: parent (A) against result (B), tools/fill_policy_ab.py",
         out=os.path.join(ROOT, "profiles", "fill_policy_ab.json")):
    """parts: name -> the function a child process runs (it prints one AB_CHILD line of row -> ms)"""
    parts = parts or {"kernels": child_kernels}
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--a")
    ap.add_argument("--b")
    ap.add_argument("--a-commit", default="")
    ap.add_argument("--b-commit", default="")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--part", choices=[*parts, "bench"], default=next(iter(parts)))
    ap.add_argument("--out", default=out)
    a = ap.parse_args()
    if a.child:
        return parts[a.part]()
    libs = {"A": os.path.abspath(a.a), "B": os.path.abspath(a.b), "A2": os.path.abspath(a.a)}
    for lib in libs.values():  # one run of each that does not count: the code objects and the file cache warm
        run_child(lib, a.part)
    series = {k: [] for k in libs}
    for r in range(a.rounds):
        for k, lib in libs.items():
            series[k].append(run_child(lib, a.part))
            print(f"round {r} {k}: {series[k][-1]}", flush=True)
    rows = {}
    for row in series["A"][0]:
        col = {k: [x[row] for x in series[k]] for k in libs}
        spread = max(abs(x - y) for x, y in zip(col["A"], col["A2"]))
        ma, mb = statistics.median(col["A"]), statistics.median(col["B"])
        rows[row] = {"unit": "ms", "parent": round(ma, 5), "result": round(mb, 5), "spread": round(spread, 5),
                     "parent_again": round(statistics.median(col["A2"]), 5), "rounds": a.rounds,
                     "parent_median_gap": round(abs(ma - statistics.median(col["A2"])), 5),
                     "rounds_result_slowest": sum(b > max(x, y) for x, y, b in zip(col["A"], col["A2"], col["B"])),
                     "round_medians": {k: [round(x, 5) for x in v] for k, v in col.items()},
                     "within_noise": mb <= ma + spread}
        if row in ROWS:
            rows[row]["kernel"] = ROWS[row][5]
    rec = {"what": what, "rows": {}}
    if os.path.exists(a.out):
        rec = json.load(open(a.out))
    rec["parent_commit"], rec["result_commit"] = a.a_commit, a.b_commit
    rec["fills_per_median"] = FILLS
    rec["rows"].update(rows)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    for row, v in rows.items():
        print(f"{row}: parent {v['parent']} result {v['result']} spread {v['spread']} gap {v['parent_median_gap']} "
              f"slowest in {v['rounds_result_slowest']}/{a.rounds} {'ok' if v['within_noise'] else 'ABOVE'}")


if __name__ == "__main__":
    main()
