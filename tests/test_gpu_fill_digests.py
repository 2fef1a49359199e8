"""Every affinity fill route writes the bits it wrote when tests/golden/fill_route_digests.json was recorded
(tools/fill_digests.py): M and C of every (storage, shards, CLIPPER_HIP_AFFINITY mode) route of
test_gpu_fill_boundaries._routes, and clipper_hip_view_matvec through a row view, on the cases of
tests/fill_digest_cases.py. The other fill tests compare routes with each other and with the oracle; this one pins them
to a record, so that a restatement of a score that moves one bit on all routes at once does not pass unseen."""
import json
import os

import pytest

from tests import fill_digest_cases as fdc
from tests.test_gpu_fill_boundaries import _routes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fill_route_digests.json")


def test_every_fill_route_writes_the_recorded_bits():
    rec = json.load(open(GOLDEN))
    want = rec["digests"]
    got = fdc.digests(_routes)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    bad = sorted(k for k in want if got[k] != want[k])
    assert not bad, (
        f"{len(bad)} of {len(want)} digests differ, first cases (case/storage/shards/mode/matrix): {bad[:8]}. The digests "
        f"belong to the recorded toolchain ({rec['toolchain']['hipcc']}; {rec['toolchain']['clang']}; flags "
        f"{rec['toolchain']['flags']}): exp, acos and sqrt come from the device libraries, so a new compiler release may "
        f"move them without a change to the fill kernels — check that before recording again with tools/fill_digests.py.")
