"""Degenerate graphs and value edges for the semidefinite relaxation (tests/test_sdp_edge_cases_cpu.py,
tests/test_gpu_sdp_edge_cases.py): the families of tests/degenerate_cases.py handed to the SDP
entry points, two equal cliques, and a planted problem scaled from 2^-126 to 2^127. Named cases with fixed seeds.

SdpCase.kind names the property the case is there for; the CPU test checks it on the model (tests/sdp_model.py) before
any GPU test may ask for it:
  "edgeless"    M = C = I: the optimum is 1
  "complete"    M = 1 everywhere, C complete: n
  "uniform"     complete with M_off = 0.5 at dyadic 1 / sqrt(n): 1 + (n - 1) / 2
  "cliques"     two disjoint cliques a > b and isolated vertices: a, the nodes are the larger clique
  "eqcliques"   two disjoint cliques of EQUAL size and isolated vertices: a, and the top eigenvalue of X is double (the
                rounding's eigenvector is any vector of a plane: the nodes are not compared)
  "star", "path"    perfect graphs of clique number 2: the optimum is 2, reached after hundreds or thousands of iterations
  "uzero"       weights in [0.5, 3), C = I: every pair forbidden, 1
  "ccomplete"   weights in [0.5, 3), C complete: lambda_max(M) (M >= 0: its Perron vector is feasible)
  "tiefill"     weights in [2, 5), C = pattern(M): no closed form; certificate and model only
  "ladder"      a planted problem s M, s from 2^-10 to 2^10: s times the optimum at s = 1, the planted clique selected
  "tiny"        s = 2^-60, 2^-126: the stopping rule's eps_abs passes at iteration 1 with X = I / n
  "huge"        s = 2^52 ... 2^127: the eigenvalues of W reach 2^53 and the simplex rule finds no valid support

Every quick kind (one or two iterations) comes at n = 1, 2, 3 (a pad index), 64, 65 (a pad index), 128 and, on the wide
route alone, 129. The kinds that iterate come at the smallest sizes that still show the behaviour; `model_iters` is the
model's count (checked by the CPU test), `max_iters` the cap the GPU test uses: twice that, so that a case within a step
of a threshold does not flip. path-65 is capped at 200 on purpose (5141 uncapped): the unconverged branch. star-65 and
path-33 run on the workgroup route alone: the wide route, whose iteration is a chain of some hundred launches, has
star-33 and path-17."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import degenerate_cases as dc

WG, WIDE = "workgroup", "wide"
QUICK_N = (1, 2, 3, 64, 65, 128)
WIDE_ONLY_N = 129
TIGHT = 1e-6
NODES_COMPARED = ("edgeless", "complete", "uniform", "cliques", "uzero", "star", "tiefill", "ladder")
NODES_LEFT_OUT = ("path", "ccomplete", "eqcliques")   # margins of 0.003 and 0.0003 to 0.007; a double top eigenvalue
# ("tiny" and "huge" are rungs of the ladder, not kinds of their own: at X = I / n every eigenvalue is equal and evec1
# is whatever the eigensolver's basis holds, and on the huge rungs the model is no bar at all)
MARGIN = 0.05                                        # the rounding margin below which nodes are not compared


@dataclass
class SdpCase:
    name: str
    kind: str
    M: np.ndarray                 # symmetric, unit diagonal times the scale
    C: np.ndarray
    eps_abs: float
    eps_rel: float
    max_iters: int                # the GPU test's cap
    model_iters: int | None       # the model's count (None: the model is not the bar; see `huge`)
    converges: bool = True        # the model converges under max_iters
    opt: float | None = None      # the known optimum of <M, X> (ladder, tiny: a feasible value, a lower bound of it)
    nodes: tuple | None = None    # the selection the property names (the larger clique, the planted clique)
    routes: tuple = (WG, WIDE)
    handed: dc.Case | None = None  # the degenerate_cases.Case behind it (set_matrix_data, set_sparse_matrix_data)

    @property
    def n(self) -> int:
        return self.M.shape[0]

    @property
    def eps(self) -> dict:
        return dict(eps_abs=self.eps_abs, eps_rel=self.eps_rel, max_iters=self.max_iters)

    @property
    def compare_nodes(self) -> bool:
        return self.kind in NODES_COMPARED


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


def _from_handed(c: dc.Case, kind, eps, model_iters, max_iters=None, converges=True, opt=None, nodes=None, routes=None):
    M, Cm = c.dense()
    _freeze(M, Cm)
    n = c.m
    if routes is None:
        routes = (WIDE,) if n > 128 else (WG, WIDE)
    return SdpCase(c.name, kind, M, Cm, eps, eps, 2 * model_iters if max_iters is None else max_iters, model_iters,
                   converges, opt, None if nodes is None else tuple(int(i) for i in nodes), routes, c)


def equal_cliques(m, a, seed=4):
    """two disjoint cliques of a vertices each among m, scattered by a permutation; the rest isolated"""
    assert 2 * a <= m
    rng = np.random.default_rng(seed + m)
    perm = rng.permutation(m)
    one, two = np.sort(perm[:a]), np.sort(perm[a:2 * a])
    W = np.zeros((m, m))
    W[np.ix_(one, one)] = 1.0
    W[np.ix_(two, two)] = 1.0
    return dc._handed(f"eqcliques-{m}", "eqcliques", m, dc._u0(seed + 7 * m, m), W, groups=(one, two))


def _quick_iters(kind, m):
    """the model's iteration counts on the quick kinds (tests/test_sdp_edge_cases_cpu.py holds them)"""
    if kind == "edgeless" or m == 1:
        return 1
    if kind == "ccomplete":
        return {2: 1, 3: 3}.get(m, 2)
    return 2


def _clique_sizes(m):
    """(a, b) with a > b >= 1 and a + b <= m, isolated vertices left over where m allows"""
    return {3: (2, 1), 64: (30, 20), 65: (30, 20), 128: (60, 40), 129: (60, 40)}[m]


def quick_cases():
    out = []
    for m in QUICK_N + (WIDE_ONLY_N,):
        out.append(_from_handed(dc.edgeless(m), "edgeless", TIGHT, 1, opt=1.0))
        out.append(_from_handed(dc.complete_ones(m), "complete", TIGHT, _quick_iters("complete", m), opt=float(m)))
        if m >= 3:
            a, b = _clique_sizes(m)
            c = dc.two_cliques(m, a, b)
            out.append(_from_handed(c, "cliques", TIGHT, 2, opt=float(a), nodes=c.groups[0]))
        if m >= 64:   # (two equal cliques of more than one vertex and an isolated rest)
            e = equal_cliques(m, m // 3)
            out.append(_from_handed(e, "eqcliques", TIGHT, 2, opt=float(m // 3)))
        c = dc.weights_c_complete(m)
        Mc, _ = c.dense()
        out.append(_from_handed(c, "ccomplete", TIGHT, _quick_iters("ccomplete", m), opt=float(np.linalg.eigvalsh(Mc)[-1])))
    for m in (4, 64):
        out.append(_from_handed(dc.complete_half_uniform(m), "uniform", TIGHT, 2, opt=1.0 + (m - 1) / 2.0))
    return out


def iterating_cases():
    """(the figures: the model's, under the schedule of DESIGN.md 11; tests/test_sdp_edge_cases_cpu.py holds them)"""
    return [
        _from_handed(dc.star(9), "star", 1e-6, 342, opt=2.0),
        _from_handed(dc.star(17), "star", 1e-6, 927, opt=2.0),
        _from_handed(dc.star(33), "star", 1e-3, 1143, opt=2.0),
        _from_handed(dc.star(65), "star", 1e-3, 1696, opt=2.0, routes=(WG,)),
        _from_handed(dc.path(17), "path", 1e-3, 990, opt=2.0),
        # (path-33 takes 4.2 s per solve on the wide route and every case is solved twice there: the wide route has the
        # next smaller path)
        _from_handed(dc.path(33), "path", 1e-3, 3025, opt=2.0, routes=(WG,)),
        _from_handed(dc.path(65), "path", 1e-3, 200, max_iters=200, converges=False, opt=2.0),
        _from_handed(dc.weights_c_identity(33), "uzero", 1e-6, 94, opt=1.0),
        _from_handed(dc.weights_c_identity(65), "uzero", 1e-6, 128, opt=1.0),
        _from_handed(dc.weights_tiefill(33, 0.3), "tiefill", 1e-6, 400),
        _from_handed(dc.weights_tiefill(65, 0.3), "tiefill", 1e-3, 973),
    ]


# ---- the scale ladder ------------------------------------------------------------------------------------------------

def planted(n, seed=12):
    """density 0.3, weights in [0.1, 1), a planted clique of n // 4 vertices at weight 0.9, unit diagonal,
    C = pattern(M). Returns (M, C, the clique ascending)."""
    rng = np.random.default_rng(seed + n)
    up = np.triu(rng.random((n, n)) < 0.3, 1)
    W = np.where(up, rng.uniform(0.1, 1.0, (n, n)), 0.0)
    K = np.sort(rng.permutation(n)[:n // 4])
    W[np.ix_(K, K)] = 0.9
    W = np.triu(W, 1)
    M = W + W.T + np.eye(n)
    Cm = (M != 0).astype(float)
    return M, Cm, K


def planted_value(n) -> float:
    """<M, X> of the planted clique's indicator over its size at s = 1: feasible, so the optimum is no smaller (the model
    finds exactly it: 3.7 at n = 17, 7.3 at n = 33). The two bars that use `opt` need a lower bound of the optimum only."""
    return 1.0 + 0.9 * (n // 4 - 1)


LADDER = {17: ((-10, 309), (0, 74), (4, 339), (10, 2802)), 33: ((-10, 224), (0, 79), (4, 299))}   # (log2 s, model iterations)
LADDER_EPS_REL = 1e-4
TINY_EXP = (-60, -126)
HUGE_EXP = (52, 60, 100, 127)
HUGE_N, HUGE_MAX_ITERS = 17, 40


def ladder_cases():
    out = []
    for n, rungs in LADDER.items():
        M, Cm, K = planted(n)
        for e, iters in rungs:
            Ms = M * 2.0 ** e      # (a power of two: every entry scales exactly)
            _freeze(Ms, Cm)
            out.append(SdpCase(f"ladder-{n}-2^{e}", "ladder", Ms, Cm, 0.0, LADDER_EPS_REL, 2 * iters, iters,
                               opt=planted_value(n) * 2.0 ** e, nodes=tuple(int(i) for i in K)))
    return out


def tiny_cases():
    out = []
    for n in (17, 33):
        M, Cm, _ = planted(n)
        for e in TINY_EXP:
            Ms = M * 2.0 ** e
            _freeze(Ms, Cm)
            out.append(SdpCase(f"tiny-{n}-2^{e}", "tiny", Ms, Cm, TIGHT, TIGHT, 2, 1, opt=planted_value(n) * 2.0 ** e))
    return out


def huge_cases():
    """the inputs on which the simplex rule finds no valid support (lambda_max(W) >= 2^53): the model is no bar here,
    the certificate's own inequalities are"""
    M, Cm, _ = planted(HUGE_N)
    out = []
    for e in HUGE_EXP:
        Ms = M * 2.0 ** e
        _freeze(Ms, Cm)
        out.append(SdpCase(f"huge-{HUGE_N}-2^{e}", "huge", Ms, Cm, TIGHT, TIGHT, HUGE_MAX_ITERS, None, converges=False))
    return out


def all_cases():
    return quick_cases() + iterating_cases() + ladder_cases() + tiny_cases() + huge_cases()


def by_name():
    return {c.name: c for c in all_cases()}


def margin(ev, thr) -> float:
    """the rounding margin (tests/test_gpu_sdp.py::_margin_ok's figure): how far, against the largest entry, the entry
    of evec1 nearest the threshold lies from it"""
    a = np.abs(np.asarray(ev))
    return float(np.min(np.abs(a - thr)) / a.max())
