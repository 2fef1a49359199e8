"""The walk that writes a tile's slices (slice_emit_lds, k_csc.hip.h) on matrices known exactly without an oracle
(tests/fill_emit_shapes_gen.py, proven on the CPU oracle by tests/test_fill_emit_shapes_cpu.py): 1.0 on K x K off the
diagonal and 0 elsewhere, with K chosen so that the columns of a slice hold 0, 1, 3, 4, 5, 63, 64, 65, 127 and 128
entries — quad padding, rows in the lower / upper half of the row mask alone, in its outer words alone, the 63 / 64
boundary, full columns (maxq = 32: more than one so[] entry) beside empty ones — at m on and off the tile edge. Every
fill route must give the matrix bit for bit, and the products through a row view of rows inside and outside K
(clipper_hip_view_matvec: k_affinity_rect on a row list) the exact integer sums. (clipper_hip_view_matvec always scores
its view from the staged points; the third caller of the walk, k_slice_filter_rows, builds views only inside a solve
of at least 3000 associations and is held to the rectangular fill's bits by tests/test_gpu_rowview.py.)"""
import numpy as np
import pytest

from clipper_amd import _abi as abi
from tests import fill_emit_shapes_gen as gen
from tests.test_gpu_fill_boundaries import CSCS, _routes, _set_mode

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(gen.CASES))
def test_every_route_writes_the_stated_matrix_bit_for_bit(monkeypatch, name):
    p = gen.make(name)
    E = p.expected()
    off = ~np.eye(p.m, dtype=bool)
    for storage, n, mode in _routes(3):
        _set_mode(monkeypatch, mode)
        g = abi.HipClipper(storage=storage, group=[0] * n if n > 1 else None)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **gen.PARAMS)
        Mg, Cg = g.get_affinity_matrix(), g.get_constraint_matrix()
        g.close()
        bad = np.argwhere((Mg != E) & off)
        assert bad.size == 0, (name, storage, n, mode, bad[:5].tolist())
        assert np.array_equal(Cg[off], E[off]), (name, storage, n, mode)
    monkeypatch.delenv("CLIPPER_HIP_AFFINITY", raising=False)


@pytest.mark.parametrize("name", list(gen.CASES))
def test_products_through_a_row_view_are_the_exact_sums(monkeypatch, name):
    monkeypatch.delenv("CLIPPER_HIP_AFFINITY", raising=False)
    p = gen.make(name)
    E = p.expected()
    rows, x = p.rows_in_and_out(), p.x()
    xm = np.zeros(p.m)
    xm[rows] = x[rows]
    want = E @ xm
    for storage in CSCS:
        # the view scored again from the points: k_affinity_rect
        g = abi.HipClipper(storage=storage)
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **gen.PARAMS)
        yM, yC = g.view_matvec(rows, x)
        zM, zC = g.matvec(xm)                      # and through the matrix's own slices
        g.close()
        assert np.array_equal(yM, want) and np.array_equal(yC, want), (name, storage, "rect")
        assert np.array_equal(zM, want) and np.array_equal(zC, want), (name, storage, "matrix")
