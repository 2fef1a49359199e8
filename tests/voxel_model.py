"""The contract of clipper_hip_voxel_downsample (clipper_amd/csrc/voxel_rules.hpp, DESIGN.md section 9, "Voxel
down-sampling") restated in numpy, bit for bit, and the table of clouds the CPU and the GPU tests share.

1. lo, hi: the exact per-axis minimum and maximum. inv = 1.0 / voxel_size, once. v_a(x) = floor((x_a - lo_a) * inv),
   clamped to 0 .. dim_a - 1 with dim_a = v_a(hi) + 1. The origin is the cloud's own minimum corner.
2. key = (v_z * dim_y + v_y) * dim_x + v_x (unsigned 64 bit); every dim_a <= 2^21.
3. Row r of the output is the r-th distinct key in ascending order.
4. A voxel's members in ascending original index, in chunks of 512; a chunk is added up one member after the other
   from +0.0 over (x - lo), the chunk sums in chunk order from +0.0; centroid = lo_a + tot_a / count.
5. Normals: the same sum s of the members' normals, l2 = (s0 s0 + s1 s1) + s2 s2, s_a / sqrt(l2), or (0, 0, 1) when l2 == 0.

np.add.accumulate adds strictly in sequence, which is what makes this a model of the bits."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHUNK = 512
MAX_DIM = 1 << 21
SORT_TILE = 2048          # k_sort.hip.h's tile, as the library reports it (clipper_voxel_info_t.sort_tile)


def grid(P, voxel_size):
    """(lo, inv, dim) of the cloud P (n x 3)"""
    P = np.asarray(P, np.float64)
    lo, hi = P.min(axis=0), P.max(axis=0)
    inv = np.float64(1.0) / np.float64(voxel_size)
    d = np.floor((hi - lo) * inv) + 1.0
    if not np.all((d >= 1.0) & (d <= MAX_DIM)):
        raise ValueError("more than 2^21 voxels along an axis")
    return lo, inv, d.astype(np.int64)


def cells(P, voxel_size):
    """the voxel (v_x, v_y, v_z) of every point, n x 3 int64"""
    lo, inv, dim = grid(P, voxel_size)
    v = np.floor((np.asarray(P, np.float64) - lo) * inv)
    return np.minimum(np.maximum(v, 0.0), (dim - 1).astype(np.float64)).astype(np.int64)


def keys(P, voxel_size):
    """the cell number of every point, n uint64"""
    _, _, dim = grid(P, voxel_size)
    v = cells(P, voxel_size).astype(np.uint64)
    dx, dy = np.uint64(dim[0]), np.uint64(dim[1])
    return (v[:, 2] * dy + v[:, 1]) * dx + v[:, 0]


def passes(dim):
    """8-bit passes of the radix sort: ceil(bitlength(cells - 1) / 8)"""
    ncell = int(dim[0]) * int(dim[1]) * int(dim[2])
    return ((ncell - 1).bit_length() + 7) // 8


def _seq_sum(V):
    """the rows of V added one after the other from +0.0"""
    return np.add.accumulate(np.vstack([np.zeros((1, V.shape[1])), V]), axis=0)[-1]


def chunked_sum(V):
    """rule 4 over the rows of V (members x 3, in the order they are to be taken)"""
    parts = np.array([_seq_sum(V[b:b + CHUNK]) for b in range(0, len(V), CHUNK)])
    return _seq_sum(parts)


def voxel_down_sample(P, voxel_size, N=None, reverse=False):
    """dict(points n_out x 3, normals n_out x 3 | None, counts, trace, keys (of the rows), dim, passes, max_count).
    reverse: take every voxel's members in descending index (NOT the contract: what the sharpness tests compare with)"""
    P = np.asarray(P, np.float64)
    n = len(P)
    if n == 0:
        return dict(points=np.zeros((0, 3)), normals=None if N is None else np.zeros((0, 3)), counts=np.zeros(0, np.int32),
                    trace=np.zeros(0, np.int32), keys=np.zeros(0, np.uint64), dim=np.zeros(3, np.int64), passes=0, max_count=0)
    lo, inv, dim = grid(P, voxel_size)
    k = keys(P, voxel_size)
    order = np.argsort(k, kind="stable")
    sk = k[order]
    head = np.ones(n, bool)
    head[1:] = sk[1:] != sk[:-1]
    starts = np.flatnonzero(head)
    ends = np.append(starts[1:], n)
    row_of_sorted = np.cumsum(head) - 1
    trace = np.zeros(n, np.int32)
    trace[order] = row_of_sorted
    m = len(starts)
    pts, nrm = np.zeros((m, 3)), (None if N is None else np.zeros((m, 3)))
    rel = P - lo
    for r, (s, e) in enumerate(zip(starts, ends)):
        mem = order[s:e][::-1] if reverse else order[s:e]
        pts[r] = lo + chunked_sum(rel[mem]) / np.float64(e - s)
        if N is not None:
            t = chunked_sum(np.asarray(N, np.float64)[mem])
            l2 = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            nrm[r] = (0.0, 0.0, 1.0) if l2 == 0.0 else t / np.sqrt(l2)
    counts = (ends - starts).astype(np.int32)
    return dict(points=pts, normals=nrm, counts=counts, trace=trace, keys=sk[starts], dim=dim, passes=passes(dim),
                max_count=int(counts.max()))


# ---- the clouds of the tests ------------------------------------------------------------------------------------------

def bunny4096():
    return np.fromfile(os.path.join(ROOT, "tests", "golden", "bunny_points_4096.f32"), dtype="<f4").reshape(-1, 3).astype(np.float64)


def unit_normals(n, seed):
    N = np.random.default_rng(seed).normal(size=(n, 3))
    return N / np.linalg.norm(N, axis=1)[:, None]


def _lattice(cellsxyz, per, seed, jitter=0.4):
    """`per` points in each of the given lattice cells (integer corners, voxel_size 1), jittered inside the cell, in a
    shuffled order; the first point is the origin itself, so that lo == 0 and the cells are the voxels"""
    rng = np.random.default_rng(seed)
    c = np.repeat(np.asarray(cellsxyz, np.float64), per, axis=0)
    P = c + rng.random(c.shape) * jitter
    P = P[rng.permutation(len(P))]
    return np.vstack([np.zeros((1, 3)), P])


def _one_voxel(n, seed):
    return np.random.default_rng(seed).random((n, 3)), 2.0


def _chunk_edges():
    rng = np.random.default_rng(11)
    parts = [np.column_stack([k + 0.1 + 0.8 * rng.random(c), 0.1 + 0.8 * rng.random(c), 0.1 + 0.8 * rng.random(c)])
             for k, c in enumerate((510, 512, 513, 1024, 1025))]                  # (the origin below is voxel 0's 511th)
    P = np.vstack(parts)
    return np.vstack([np.zeros((1, 3)), P[rng.permutation(len(P))]]), 1.0


def tile_case(n, form, seed=5):
    """n points around the sort's tile size: 'equal' (one voxel: no pass at all), 'equal_far' (one voxel but for the last
    point, which makes the grid 300 wide: two passes over keys that are all equal but one), 'descending' (the keys fall
    with the input index) and 'random' (555 cells, many duplicates)"""
    rng = np.random.default_rng(seed + n)
    off = rng.random((n, 3)) * 0.4
    off[0] = 0.0
    c = np.zeros((n, 3))
    if form == "equal_far":
        c[-1] = (299.0, 0.0, 0.0)
    elif form == "descending":
        c[:, 0] = np.arange(n - 1, -1, -1)
        off[-1] = 0.0                                                            # (the origin is the last point here)
    elif form == "random":
        c = np.column_stack([rng.integers(0, 37, n), rng.integers(0, 5, n), rng.integers(0, 3, n)]).astype(np.float64)
        c[0] = 0.0
    elif form != "equal":
        raise ValueError(form)
    return c + off, 1.0


TILE_FORMS = ("equal", "equal_far", "descending", "random")

# corner -> the passes its grid needs (dim = corner + 1)
PASS_CORNERS = {1: (15, 3, 3), 2: (255, 255, 0), 3: (255, 255, 255), 4: (2047, 2047, 1023), 5: (16383, 8191, 8191),
                6: (65535, 65535, 65535), 7: (524287, 524287, 262143), 8: (1048575, 1048575, 1048575)}


def passes_case(p):
    """lattice cloud whose grid needs p passes: the origin, the corner, and 60 random cells of 5 points each"""
    corner = np.array(PASS_CORNERS[p], np.int64)
    rng = np.random.default_rng(100 + p)
    inner = np.column_stack([rng.integers(0, c + 1, 60) for c in corner])
    return _lattice(np.vstack([inner, corner[None, :]]), 5, 200 + p), 1.0


def top_digit_case():
    """keys j * 2^16, j = 0..15: three passes, and only the last one sees a digit that is not zero"""
    cellsxyz = [(0, 0, j << 16) for j in range(16)]
    return _lattice(cellsxyz, 9, 31), 1.0


def faces_case():
    """every point of the 5 x 5 x 5 lattice of spacing 0.25 (exactly on the voxel faces; the maximum corner 1.0 lands in
    voxel 4 = dim - 1), twice, and 300 points in between"""
    g = np.arange(5) * 0.25
    L = np.array([(x, y, z) for z in g for y in g for x in g])
    rng = np.random.default_rng(17)
    P = np.vstack([L, rng.random((300, 3)), L])
    return P[rng.permutation(len(P))], 0.25


def uniform5000():
    return np.random.default_rng(0).random((5000, 3)), 0.05


def planar_case():
    P = np.random.default_rng(3).random((3000, 3))
    P[:, 2] = 0.375
    return P, 0.04


def opposite_normals_case():
    """two voxels: in the first the two normals cancel exactly, in the second they do not"""
    P = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.1, 0.1, 0.1], [1.2, 0.2, 0.2]])
    N = np.array([[0.6, 0.0, 0.8], [-0.6, 0.0, -0.8], [0.0, 1.0, 0.0], [0.0, 0.6, 0.8]])
    return P, 1.0, N


def _cases():
    c = {
        "n1": lambda: (np.array([[0.3, -1.5, 2.0]]), 0.1, None),
        "two_in_one": lambda: (np.array([[0.0, 0.0, 0.0], [0.01, 0.02, 0.03]]), 0.1, None),
        "identical64": lambda: (np.tile(np.array([[1.25, -3.5, 0.7]]), (64, 1)), 0.1, None),
        "one_voxel_700": lambda: _one_voxel(700, 1) + (None,),
        "chunk_edges": lambda: _chunk_edges() + (None,),
        "top_digit": lambda: top_digit_case() + (None,),
        "faces": lambda: faces_case() + (None,),
        "uniform5000": lambda: uniform5000() + (None,),
        "shifted_1e6": lambda: (uniform5000()[0] + 1e6, 0.05, None),
        "planar": lambda: planar_case() + (None,),
        "bunny4096": lambda: (bunny4096(), 0.01, None),
        "normals5000": lambda: uniform5000() + (unit_normals(5000, 9),),
        "one_voxel_700_normals": lambda: _one_voxel(700, 1) + (unit_normals(700, 2),),
        "opposite_normals": opposite_normals_case,
    }
    for p in PASS_CORNERS:
        c[f"passes{p}"] = (lambda p=p: passes_case(p) + (None,))
    for n in (SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 1):
        for form in TILE_FORMS:
            c[f"tile_{n}_{form}"] = (lambda n=n, form=form: tile_case(n, form) + (None,))
    return c


CASES = _cases()
_models = {}


def case_model(name):
    """(P, voxel_size, N, model) of a case of the table, computed once and shared"""
    if name not in _models:
        P, vs, N = CASES[name]()
        _models[name] = (P, vs, N, voxel_down_sample(P, vs, N))
    return _models[name]
