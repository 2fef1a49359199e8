"""Problems whose fp64 affinity decisions sit exactly on the thresholds of the fill (tests/test_gpu_fill_boundaries.py).

Association i is (i, i): point P[i] of the first set against Q[i] of the second. The associations come in
  * COUPLES (i, i + 1): P[i + 1] - P[i] and Q[i + 1] - Q[i] are chosen so that l1, l2 and c = |l1 - l2| of the pair
    are exact dyadic numbers in fp64 — one side an axis-aligned offset, the other a Pythagorean one ((3, 4) -> 5,
    (1, 2, 2) -> 3, (1, 2, 2, 4) -> 5, ... times a dyadic k, axes and signs shuffled) — so the fma chain, the square
    root and the subtraction of euclidean_distance.cpp:18-28 are all exact, whatever sqrt or libm do:
        "eq"     c == EPS                  "below"  c == EPS - H             "above"  c == EPS + H
        "md1"    l1 == LMD, c == EPS / 2   "md2"    l2 == LMD, c == EPS / 2  (LMD: the shortest length of all couples)
  * an INLIER cluster: Q = P + T + noise on the grid, every pair of it within EPS / 4 (a dense block for the solver);
  * everything else between them scores whatever it scores (the oracle says what).
Coordinates lie on a dyadic grid of at most ~40 significant bits around a common dyadic offset; the fp32 copies of the
points (the prefilter's input) lose their low bits from offset 2^10 on.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

H = 2.0 ** -12            # step of c around EPS
EPS = 96 * H              # 0.0234375
LMD = 2.0 ** -3           # the mindist boundary length
KINDS = ("eq", "below", "above", "md1", "md2")

_PYTHAGOREAN = {  # integer offsets with an integer length, by dimension (zero-padded to d)
    2: [((3, 4), 5), ((5, 12), 13), ((8, 15), 17)],
    3: [((3, 4), 5), ((1, 2, 2), 3), ((2, 3, 6), 7), ((2, 6, 9), 11)],
    5: [((3, 4), 5), ((1, 2, 2), 3), ((1, 2, 2, 4), 5), ((1, 1, 1, 1), 2), ((1, 1, 1, 2, 3), 4), ((1, 1, 3, 5), 6)],
}


@dataclass
class BoundaryProblem:
    D1: np.ndarray          # d x m (PointNormal: 6 x m)
    D2: np.ndarray
    A: np.ndarray           # m x 2
    u0: np.ndarray
    couples: dict           # kind -> int array [k, 2] of association pairs (i, i + 1)
    inliers: np.ndarray     # association indices of the inlier cluster
    offset: float


def _vec(rng, d, pyth):
    """an integer offset in dimension d and its integer length: Pythagorean, or a signed unit axis"""
    v = np.zeros(d)
    if pyth:
        comps, hyp = _PYTHAGOREAN[d][rng.integers(len(_PYTHAGOREAN[d]))]
        axes = rng.permutation(d)[:len(comps)]
        v[axes] = np.asarray(comps, float) * rng.choice([-1.0, 1.0], len(comps))
        return v, float(hyp)
    v[rng.integers(d)] = rng.choice([-1.0, 1.0])
    return v, 1.0


def make(m: int, d: int, offset_exp: int | None, seed: int, n_inliers: int | None = None,
         pointnormal: bool = False) -> BoundaryProblem:
    """m associations in dimension d (PointNormal: d = 3 positions + unit-axis normals), coordinates around
    2^offset_exp (None: around the origin)."""
    rng = np.random.default_rng(seed)
    dim = 3 if pointnormal else d
    offset = 0.0 if offset_exp is None else 2.0 ** offset_exp
    grid = 2.0 ** -20                                          # base points: ~38 bits below 2^18
    box = 64.0
    n_in = n_inliers if n_inliers is not None else max(12, min(60, m // 8))
    n_cpl = (m - n_in) // 2
    n_in = m - 2 * n_cpl
    P = np.zeros((m, dim))
    Q = np.zeros((m, dim))
    base = lambda k: offset + np.round(rng.uniform(0, box, (k, dim)) / grid) * grid
    couples = {k: [] for k in KINDS}
    for c in range(n_cpl):
        i = 2 * c
        kind = KINDS[c % len(KINDS)]
        P[i], Q[i] = base(1)[0], base(1)[0]
        if kind in ("md1", "md2"):
            short, long_ = LMD, LMD + EPS / 2                 # the shortest lengths of all couples
            v_s, _ = _vec(rng, dim, False)
            v_l, _ = _vec(rng, dim, False)
            va, vb = v_s * short, v_l * long_
            if kind == "md2":
                va, vb = vb, va
        else:
            cc = {"eq": EPS, "below": EPS - H, "above": EPS + H}[kind]
            vp, hyp = _vec(rng, dim, True)
            k = float(rng.integers(64, 1024)) * 2.0 ** -8      # L = hyp * k in [0.75, 68): >= 4 LMD + EPS
            L = hyp * k
            L2 = L - cc if rng.random() < 0.5 else L + cc
            vq, _ = _vec(rng, dim, False)
            va, vb = vp * k, vq * L2
            if rng.random() < 0.5:
                va, vb = vb, va
        P[i + 1], Q[i + 1] = P[i] + va, Q[i] + vb
        couples[kind].append((i, i + 1))
    # the inlier cluster: Q = P + T + noise (multiples of 2^-12 up to 2^-9 per coordinate)
    ins = np.arange(2 * n_cpl, m)
    T = np.round(rng.uniform(-8, 8, dim) / H) * H
    P[ins] = base(len(ins))
    Q[ins] = P[ins] + T + rng.integers(-8, 9, (len(ins), dim)) * H
    order = rng.permutation(m)                                   # couples and inliers spread over the list
    inv = np.empty(m, int)
    inv[order] = np.arange(m)
    P, Q = P[order], Q[order]
    couples = {k: np.sort(inv[np.asarray(v, int)], axis=1).reshape(-1, 2) for k, v in couples.items()}
    inliers = np.sort(inv[ins])
    if pointnormal:                                              # the same unit axis on both sides of a pair
        axis = rng.integers(3, size=m)
        for kind in KINDS:
            axis[couples[kind][:, 1]] = axis[couples[kind][:, 0]]
        N = np.eye(3)[axis] * rng.choice([-1.0, 1.0], (m, 1))
        for kind in KINDS:
            N[couples[kind][:, 1]] = N[couples[kind][:, 0]]
        P, Q = np.hstack([P, N]), np.hstack([Q, N])
    A = np.stack([np.arange(m), np.arange(m)], axis=1).astype(np.int32)
    u0 = np.random.default_rng(seed + 1).random(m)
    return BoundaryProblem(D1=np.ascontiguousarray(P.T), D2=np.ascontiguousarray(Q.T), A=A, u0=u0, couples=couples,
                           inliers=inliers, offset=offset)


def lengths(p: BoundaryProblem, kind: str):
    """exact (l1, l2) of the couples of a kind, from the coordinates (asserts that they are exact)"""
    i, j = p.couples[kind][:, 0], p.couples[kind][:, 1]
    dim = 3 if p.D1.shape[0] == 6 else p.D1.shape[0]
    t1, t2 = p.D1[:dim, j] - p.D1[:dim, i], p.D2[:dim, j] - p.D2[:dim, i]
    s1, s2 = np.sum(t1 * t1, axis=0), np.sum(t2 * t2, axis=0)
    l1, l2 = np.sqrt(s1), np.sqrt(s2)
    assert np.array_equal(l1 * l1, s1) and np.array_equal(l2 * l2, s2), "a couple's length is not exact"
    return l1, l2


# The threshold settings a problem is filled with: (name, epsilon, mindist). Across them every kind of couple is
# both kept and dropped; `expected` says which.
SETTINGS = (
    ("eps", EPS, 0.0),
    ("eps_up_md", float(np.nextafter(EPS, np.inf)), LMD),
    ("eps_down_md_up", float(np.nextafter(EPS, -np.inf)), float(np.nextafter(LMD, np.inf))),
)


def expected(setting: str, kind: str) -> bool:
    """is a couple of this kind scored (non-zero) under this setting (clipper.cpp / euclidean_distance.cpp rules)"""
    if kind == "below":
        return True
    if kind == "above":
        return False
    if kind == "eq":
        return setting == "eps_up_md"                     # c < eps only when eps is one ulp above c
    return setting != "eps_down_md_up"                    # md1 / md2: l < mindist only for mindist = next(LMD)


def make_live(m_synth: int, rho: float, seed: int, n_in: int = 400, per_kind: int = 8,
              offset_exp: int | None = 12) -> BoundaryProblem:
    """Boundary pairs INSIDE the clique a solve selects, next to a synthetic registration problem (clipper_amd.synth:
    unit-cube points, 1 - rho of them consistent — the bulk on which a solve builds row views and hands over to the
    live sub-problem).

    The clique: n_in associations with Q = P + T + noise (P on the grid in a box of 8 around 2^offset_exp, noise of
    at most H on the 2nd / 3rd coordinate only), and `per_kind` associations b of each kind, each anchored at its own
    clique member a, displaced along +x: P[b] - P[a] = l1 e_x and Q[b] - Q[a] = l2 e_x with l1, l2 exact —
        eq / below / above   l1 = L (dyadic, 1/4 .. 1), l2 = L + c with c = EPS / EPS - H / EPS + H
        md1                  l1 = LMD, l2 = LMD + EPS / 2
        md2                  P[b] - P[a] = -(LMD + EPS / 2) e_x, Q[b] - Q[a] = -LMD e_x   (l2 = LMD)
    Every other pair of the clique differs from a translation by (c_b - c_b') e_x plus the noise: |l1 - l2| <=
    sqrt(c^2 + 8 H^2) < c + H / 20 (triangle inequality), so a kept boundary pair is all that stands between a and b
    and the rest of the clique. `couples[kind]` holds the (a, b) pairs (association indices, ascending)."""
    from clipper_amd import synth
    s = synth.make_euclidean_problem(m_synth, rho, seed=seed)
    rng = np.random.default_rng(seed + 1)
    grid = 2.0 ** -20
    offset = 0.0 if offset_exp is None else 2.0 ** offset_exp
    nb = per_kind * len(KINDS)
    n = n_in + nb
    P = offset + np.round(rng.uniform(0, 8, (n, 3)) / grid) * grid
    T = np.round(rng.uniform(-4, 4, 3) / H) * H
    noise = np.zeros((n, 3))
    noise[:, 1:] = rng.integers(-1, 2, (n, 2)) * H
    Q = P + T + noise
    anchors = rng.choice(n_in, nb, replace=False)
    couples = {}
    for q, kind in enumerate(KINDS):
        pairs = []
        for t in range(per_kind):
            a, b = int(anchors[q * per_kind + t]), n_in + q * per_kind + t
            if kind in ("eq", "below", "above"):
                L = float(rng.integers(64, 257)) * 2.0 ** -8
                l1, l2 = L, L + {"eq": EPS, "below": EPS - H, "above": EPS + H}[kind]
            elif kind == "md1":
                l1, l2 = LMD, LMD + EPS / 2
            else:
                l1, l2 = -(LMD + EPS / 2), -LMD
            P[b] = P[a] + np.array([l1, 0.0, 0.0])
            Q[b] = Q[a] + np.array([l2, 0.0, 0.0])
            pairs.append((a, b))
        couples[kind] = np.asarray(pairs)
    order = rng.permutation(n)                                    # boundary associations spread over the clique
    inv = np.empty(n, int)
    inv[order] = np.arange(n)
    P, Q = P[order], Q[order]
    n1, n2 = s.D1.shape[1], s.D2.shape[1]
    A = np.vstack([s.A, np.stack([n1 + np.arange(n), n2 + np.arange(n)], axis=1)]).astype(np.int32)
    couples = {k: np.sort(m_synth + inv[v], axis=1) for k, v in couples.items()}
    u0 = np.concatenate([s.u0, np.random.default_rng(seed + 2).random(n)])
    return BoundaryProblem(D1=np.hstack([s.D1, P.T]), D2=np.hstack([s.D2, Q.T]), A=A, u0=u0, couples=couples,
                           inliers=m_synth + np.sort(inv[:n_in]), offset=offset)


def make_embedded(m_synth: int, rho: float, seed: int, m: int, offset_exp: int | None) -> BoundaryProblem:
    """A synthetic registration problem (clipper_amd.synth: unit-cube points, a consistent inlier set — the shape on
    which a solve builds row views) with the couples of make(m, 3, offset_exp) appended as associations of their own."""
    from clipper_amd import synth
    s = synth.make_euclidean_problem(m_synth, rho, seed=seed)
    b = make(m, 3, offset_exp, seed=seed + 1)
    n1, n2 = s.D1.shape[1], s.D2.shape[1]
    A = np.vstack([s.A, b.A + np.array([n1, n2], np.int32)]).astype(np.int32)
    couples = {k: v + m_synth for k, v in b.couples.items()}
    return BoundaryProblem(D1=np.hstack([s.D1, b.D1]), D2=np.hstack([s.D2, b.D2]), A=A, u0=np.concatenate([s.u0, b.u0]),
                           couples=couples, inliers=b.inliers + m_synth, offset=b.offset)
