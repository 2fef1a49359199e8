"""Executable model (numpy) of the SELECTION of the live sub-problem (clipper_amd/csrc/k_subproblem.hip.h,
host_subproblem.hpp: sub_select): which associations a solve keeps when it drops the rest for good, and the N it hands
to the decision's bound. Integers only. Test infrastructure: tests/test_subproblem_model.py checks on the CPU that the
contract implies the two facts the exactness argument needs; the kernels are compared with it on the GPU
(tests/test_gpu_sub_selection.py, tests/test_gpu_sub_small.py).

The view's slices (tests/slices_model.py) hold the entries of M[rows, :] in chunks of 128 VIEW rows, a column's entries
of a chunk padded to whole quads of 4; a slice's header carries the quads per column. k_sub_colcount adds them up.
"""
from __future__ import annotations

import numpy as np

from tests.slices_model import SUB, W

THETA = 0.4             # SUB_THETA
N0_CAP = 2_000_000_000


def select(pattern: np.ndarray, rows, s: float) -> dict:
    """pattern: m x m bool, both triangles, zero diagonal (what the storage holds); rows: the view's rows, ascending;
    s: sum(u). Everything the selection leaves behind."""
    pattern = np.asarray(pattern, dtype=bool)
    rows = np.asarray(rows, dtype=np.int64)
    m = pattern.shape[0]
    assert pattern.shape == (m, m) and rows.ndim == 1 and np.all(np.diff(rows) > 0)
    assert rows.size == 0 or (rows[0] >= 0 and rows[-1] < m)
    mp = (m + W - 1) // W * W
    # cnt[c]: the quads of lane c, x 4, over the chunks of 128 VIEW rows — every chunk's entries padded to whole quads
    cnt = np.zeros(mp, dtype=np.int64)
    for k in range((rows.size + SUB - 1) // SUB):
        nnz = pattern[rows[SUB * k:SUB * k + SUB]].sum(axis=0, dtype=np.int64)
        cnt[:m] += 4 * ((nnz + 3) // 4)
    # n0 = min(floor((0.4 s) s), 2e9): fp64, in this order of multiplication
    n0d = np.floor((np.float64(THETA) * np.float64(s)) * np.float64(s))
    n0 = int(n0d) if n0d < 2.0e9 else N0_CAP
    in_view = np.zeros(mp, dtype=bool)
    in_view[rows] = True
    flags = in_view | (cnt > n0)            # (cnt = 0 in [m, mp): never in S)
    colmap = np.flatnonzero(flags)
    nS = int(colmap.size)
    pos = np.full(mp, -1, dtype=np.int64)   # k_rv_scatter: -1 outside S, the padding included
    pos[colmap] = np.arange(nS)
    outside = cnt[:m][~flags[:m]]
    ncol = int(outside.max()) if outside.size else 0
    return dict(cnt=cnt, n0=n0, flags=flags, nS=nS, colmap=colmap, pos=pos, ncol=ncol,
                entries=int(cnt[flags].sum()), N_used=max(1, ncol) + (nS - int(rows.size)), mp=mp)
