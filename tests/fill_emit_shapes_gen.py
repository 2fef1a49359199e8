"""Problems whose affinity matrix is known exactly without an oracle, built to reach every branch of the walk that
writes a tile's slices (slice_emit_lds, k_csc.hip.h) — used by tests/test_gpu_fill_emit_shapes.py on the device and
proven on the CPU oracle by tests/test_fill_emit_shapes_cpu.py.

Associations are (i, i), EuclideanDistance. For an index set K model and data points are identical, so every pair
inside K has c = |l1 - l2| = 0 and scores exp(0) = 1.0 exactly; every i outside K gets a data point FAR apart from
every other data point, so a pair touching it has c >> epsilon and scores 0. M is ones on K x K off the diagonal and
zero elsewhere, and the entries a column c of K has inside the 128 rows of chunk k are |K in chunk k| - [c in chunk k].
"""
import numpy as np

CHUNK = 128   # rows of a tile / of a slice
GROUP = 64    # columns of a slice
EPS = 0.5
PARAMS = dict(sigma=0.25, epsilon=EPS, mindist=0.0)
FAR = 1000.0  # spacing of the outsiders' data points; the model lies in the unit cube (distances <= sqrt 3)

# the per-(column, chunk) entry counts the cases below must reach between them: quad padding (1, 3, 5), one full quad
# (4), the 63 / 64 / 65 boundary of the row mask's halves, a full column (127 with the diagonal out, 128: maxq = 32,
# more than one so[] entry), and nothing at all
WANTED_COUNTS = {0, 1, 3, 4, 5, 63, 64, 65, 127, 128}


def _rows(*spec):
    """K from (chunk, rows inside the chunk) pairs"""
    return np.unique(np.concatenate([CHUNK * k + np.asarray(list(r), dtype=np.int64) for k, r in spec]))


# name -> (m, K). The row masks are walked as four 32-bit words: the sets inside a chunk also put rows in the lower
# half alone, the upper half alone, the two outer words with the inner ones empty, and single inner words.
CASES = {
    # one edge tile: every column 126 entries (31 quads and a half)
    "m127_all": (127, np.arange(127)),
    # one full diagonal tile: 127
    "m128_all": (128, np.arange(128)),
    # chunk 0 full (127 / 128), chunk 1 is one row (1 entry for the columns of chunk 0, 0 for its own)
    "m129_all": (129, np.arange(129)),
    # lower half alone (64 rows: 63 / 64), upper half alone; the last chunk's one row outside K
    "m257_halves": (257, _rows((0, range(0, 64)), (1, range(64, 128)))),
    # the outer words alone (rows 5 and 100), one inner word alone (rows 40 .. 44: 4 / 5), a row in every word
    "m257_words": (257, _rows((0, (5, 100)), (1, range(40, 45)), (2, (0,)))),
    # both ends of the tile order, full and sparse columns in one slice: chunk 0 full, 65 rows across the halves'
    # boundary (64 / 65), 4 rows (3 / 4) of which only two columns share a 64-column group with 62 empty ones,
    # and the last chunk's one row
    "m385_mixed": (385, _rows((0, range(128)), (1, range(31, 96)), (2, (0, 63, 64, 127)), (3, (0,)))),
    # few columns of K in every group: 128-entry columns beside 0-entry ones (maxq = 32, tot = 0 on most lanes)
    "m385_sparse_cols": (385, _rows((0, range(128)), (1, (3,)), (2, (70,)))),
    # nothing at all outside one pair, and an empty K
    "m385_pair": (385, np.array([130, 300])),
    "m129_none": (129, np.array([], dtype=np.int64)),
}


class Problem:
    def __init__(self, m, K):
        self.m, self.K = int(m), np.asarray(K, dtype=np.int64)
        rng = np.random.default_rng(1000 + self.m + 7 * self.K.size)
        P = rng.random((3, self.m))
        Q = P.copy()
        out = np.setdiff1d(np.arange(self.m), self.K)
        Q[:, out] = 0.0
        Q[0, out] = FAR * (1.0 + np.arange(out.size))
        self.D1, self.D2 = np.ascontiguousarray(P), np.ascontiguousarray(Q)
        self.A = np.stack([np.arange(self.m), np.arange(self.m)], axis=1).astype(np.int32)

    def expected(self):
        """M (and C) off the diagonal: ones on K x K"""
        E = np.zeros((self.m, self.m))
        E[np.ix_(self.K, self.K)] = 1.0
        np.fill_diagonal(E, 0.0)
        return E

    def counts(self):
        """{entries of a column inside a chunk} over every (column, chunk) of the matrix"""
        E = self.expected()
        out = set()
        for k in range(0, self.m, CHUNK):
            out |= set(np.count_nonzero(E[k:k + CHUNK], axis=0).tolist())
        return out

    def rows_in_and_out(self):
        """a row list for a view: rows of K and rows outside it, ascending, not a multiple of anything"""
        rng = np.random.default_rng(self.m + self.K.size)
        out = np.setdiff1d(np.arange(self.m), self.K)
        pick = [s[rng.random(s.size) < 0.6] for s in (self.K, out)]
        rows = np.unique(np.concatenate(pick + [self.K[:1], out[:1]]))
        return rows.astype(np.int32)

    def x(self):
        """small integers: every sum of the products below is exact in fp32 and fp64"""
        return np.random.default_rng(self.m).integers(1, 8, self.m).astype(np.float64)


def make(name):
    return Problem(*CASES[name])
