"""Everything the host side allocates has an owner that releases it (csrc/host_buf.hpp: DevBuf, PinnedBuf, Event; the
counts are clipper_hip_debug_live_resources'). One ROUND opens, uses and closes one of everything that holds device
memory, pinned memory or events: contexts of all four storages that grow and then reuse their buffers (m = 512, the
resident launch; 3000; 512 again), the resident launch on a view, a streamed view, the live sub-problem with its child
contexts, an explicit constraint matrix, the maximum-clique and SDP calls of a context and of a batch, a user-defined
invariant's fill, the stand-alone searches, the voxel grid, the normals, both ICPs, and profiling's event pairs. After
a first round (per-thread caches such as the search's events exist from then on) a second round must leave the
counts where it found them; while its contexts are open the counts are above that; and a context that solves again at
one size allocates nothing."""
import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth

pytestmark = pytest.mark.gpu

INV = synth.EUCLID_BENCH_PARAMS
HELD = ("device_buffers", "device_bytes", "pinned_buffers", "events")
EUCLID_SRC = r"""
#include <hip/hip_runtime.h>
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) {
    const double t1 = ai[k] - aj[k];
    const double t2 = bi[k] - bj[k];
    s1 = fma(t1, t1, s1);
    s2 = fma(t2, t2, s2);
  }
  const double c = fabs(sqrt(s1) - sqrt(s2));
  return (c < params[1]) ? exp(-0.5 * c * c / (params[0] * params[0])) : 0.0;
}
"""


def make_problems():
    """the inputs of a round"""
    rng = np.random.default_rng(99)
    P = rng.uniform(-1.0, 1.0, (3, 2000))
    c, s = np.cos(0.05), np.sin(0.05)
    T = np.array([[c, -s, 0, 0.02], [s, c, 0, -0.01], [0, 0, 1, 0.01], [0, 0, 0, 1.0]])
    U = np.triu((rng.random((300, 300)) < 0.08) * rng.uniform(0.1, 1.0, (300, 300)), 1)
    M = U + U.T + np.eye(300)
    Cm = (M != 0).astype(np.float64)
    i, j = np.argwhere(np.triu(M, 1) != 0)[0]
    Cm[i, j] = Cm[j, i] = 0.0   # not the pattern of M: the explicit constraint store
    return dict(small=synth.make_euclidean_problem(512, 0.9, seed=11), mid=synth.make_euclidean_problem(3000, 0.9, seed=3),
                view=synth.make_euclidean_problem(10000, 0.95, seed=12345), sub=synth.make_euclidean_problem(16000, 0.9, seed=31),
                m300=synth.make_euclidean_problem(300, 0.9, seed=5), MC=(M, Cm),
                batch=[synth.make_euclidean_problem(200, [0.5, 0.7, 0.9][k % 3], seed=7000 + k) for k in range(8)],
                cloud=P, moved=T[:3, :3] @ P + T[:3, 3:4])


@pytest.fixture(scope="module")
def problems():
    return make_problems()   # (made once)


def _held(c):
    return {k: c[k] for k in HELD}


def _score_solve(g, p):
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **INV)
    return g.solve(p.u0)


def _round(pr):
    """one of everything, all closed again; returns the counts as they stood while the m = 300 context and the batch
    were open, and the allocations made by the second and by the third solve of open contexts at one size"""
    repeat = {}
    for storage in (abi.STORE_F32, abi.STORE_F64, abi.STORE_F32_CSC, abi.STORE_F64_CSC):
        g = abi.HipClipper(storage=storage)
        if storage == abi.STORE_F32_CSC:
            g.set_profiling(True)
        for key in ("small", "mid", "small"):   # grows, then reuses
            _score_solve(g, pr[key])
        a0 = abi.debug_live_resources()["allocations"]
        g.solve(pr["small"].u0)
        a1 = abi.debug_live_resources()["allocations"]
        g.solve(pr["small"].u0)
        repeat[f"storage {storage}, m = 512"] = (a1 - a0, abi.debug_live_resources()["allocations"] - a1)
        g.close()
    for key, row_view in (("view", 0), ("view", 2), ("sub", 0)):   # the resident launch on a view; a streamed view; the live sub-problem
        g = abi.HipClipper(storage=abi.STORE_F32_CSC)
        g.set_row_view(row_view)
        _score_solve(g, pr[key])
        a0 = abi.debug_live_resources()["allocations"]
        g.solve(pr[key].u0)
        a1 = abi.debug_live_resources()["allocations"]
        g.solve(pr[key].u0)
        repeat[f"{key}, row_view {row_view}"] = (a1 - a0, abi.debug_live_resources()["allocations"] - a1)
        g.close()
    sdp = abi.SdpParams(eps_abs=1e-3, eps_rel=1e-3, max_iters=40)
    g = abi.HipClipper(storage=abi.STORE_F32)
    g.set_matrix_data(*pr["MC"])
    g.solve(np.full(300, 1.0))
    _score_solve(g, pr["m300"])
    g.max_clique()
    b = abi.HipBatch(storage=abi.STORE_F32_CSC)
    b.solve_euclidean([(p.D1, p.D2, p.A, p.u0) for p in pr["batch"]], **INV)
    b.max_clique()
    route = abi.sdp_set_route(abi.SDP_ROUTE_AUTO)   # (n = 300 and 200: the wide route's slab; n = 100: the workgroup route's arrays)
    try:
        g.sdp(sdp)
        b.sdp(sdp)
        M100 = pr["MC"][0][:100, :100]
        abi.sdp_solve(M100, (M100 != 0).astype(np.float64), sdp)
    finally:
        abi.sdp_set_route(route)
    with abi.HipInvariant(EUCLID_SRC, 3) as inv:
        c = abi.HipClipper(storage=abi.STORE_F32_CSC)
        p = pr["m300"]
        c.affinity_custom(inv, p.D1, p.D2, p.A, [INV["sigma"], INV["epsilon"], INV["mindist"]])
        c.solve(p.u0)
        c.close()
    open_counts = abi.debug_live_resources()
    b.close()
    g.close()
    P, Q = pr["cloud"], pr["moved"]
    before = abi.knn_search()
    try:
        for route in (abi.KNN_BRUTE, abi.KNN_GRID):
            abi.knn_set_search(route)
            abi.knn(P, Q, 4)
    finally:
        abi.knn_set_search(before)
    abi.voxel_down_sample(P, 0.1)
    abi.estimate_normals(P)
    abi.icp(P, Q, max_distance=0.5, max_iterations=5)
    abi.icp_generalized(P, abi.estimate_covariances(P), Q, abi.estimate_covariances(Q), max_distance=0.5, max_iterations=5)
    return open_counts, repeat


def test_a_round_leaves_nothing_behind(problems):
    _round(problems)
    base = abi.debug_live_resources()
    open_counts, repeat = _round(problems)
    after = abi.debug_live_resources()
    print("baseline", base, "\nopen", open_counts, "\nafter", after, "\nrepeated solves", repeat)
    assert _held(after) == _held(base)
    assert all(open_counts[k] > base[k] for k in HELD), (open_counts, base)   # the counting counts
    assert after["allocations"] > base["allocations"]
    # the second and the third solve of an open context at one size: nothing is allocated ...
    sub = repeat.pop("sub, row_view 0")
    assert all(v == (0, 0) for v in repeat.values()), repeat
    # ... except on the live sub-problem's path: sub_prepare builds the child context anew for every hand-over
    # (sub_stage -> ensure_problem(child, nS)), and ensure_problem replaces all of a context's arrays whenever the size
    # differs from the one it holds: nS differs from hand-over to hand-over, so every solve allocates the child's arrays
    # again. The same count in every solve: 46 for this problem.
    assert sub == (46, 46), sub
