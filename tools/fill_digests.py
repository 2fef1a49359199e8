#!/usr/bin/env python3
"""Record tests/golden/fill_route_digests.json: sha256 digests of what every affinity fill route writes on the cases of
tests/fill_digest_cases.py, with the toolchain they belong to (exp, acos and sqrt come from the device libraries, so
the digests are those of one compiler release and one set of flags). Run on a GPU, on a build whose fill kernels are
known good; tests/test_gpu_fill_digests.py asserts the record from then on.
  python tools/fill_digests.py [--out PATH] [--check]     (--check: compare with the record instead of writing it)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from clipper_amd import build as b  # noqa: E402
from tests import fill_digest_cases as fdc  # noqa: E402
from tests.test_gpu_fill_boundaries import _routes  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "fill_route_digests.json")


def toolchain():
    v = subprocess.run([b.HIPCC, "--version"], capture_output=True, text=True).stdout.splitlines()
    return {"hipcc": next((l for l in v if "HIP version" in l), v[0] if v else "unknown"),
            "clang": next((l for l in v if "clang version" in l), ""),
            "flags": " ".join(b.HIP_FLAGS)}


def main():
    out = GOLDEN
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    d = fdc.digests(_routes)
    again = fdc.digests(_routes)
    assert d == again, "two runs of the same build disagree: " + str([k for k in d if d[k] != again[k]][:5])
    if "--check" in sys.argv:
        want = json.load(open(GOLDEN))["digests"]
        bad = sorted(k for k in want if d.get(k) != want[k])
        print(f"{len(want) - len(bad)} of {len(want)} digests match" + (f"; differing: {bad}" if bad else ""))
        return 1 if bad or set(d) != set(want) else 0
    with open(out, "w") as f:
        json.dump({"toolchain": toolchain(), "m": fdc.M, "outlier_ratio": fdc.RHO, "digests": d}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(d)} digests -> {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
