"""CPU checks of the seeded maximum-clique call ("Seeded calls"): the model of
tests/maxclique_seed_model.py against networkx, the new plan functions of host_mcplan.hpp (g++ only), and the new C
declarations against the ctypes binding (gcc only). The GPU side is tests/test_gpu_maxclique_seeded.py."""
import ctypes
import os
import subprocess

import networkx as nx
import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import build
from tests import maxclique_model as mm
from tests import maxclique_seed_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PS = [0.05, 0.2, 0.5, 0.8]


def _gnp(n, p, rng):
    a = np.triu(rng.random((n, n)) < p, 1)
    return a | a.T


def _nx(adj):
    return nx.from_numpy_array(adj.astype(int))


def _is_maximal_clique(adj, Q):
    g = _nx(adj)
    Q = list(Q)
    if len(set(Q)) != len(Q) or not all(g.has_edge(a, b) for i, a in enumerate(Q) for b in Q[i + 1:]):
        return False
    common = set(range(adj.shape[0])) - set(Q)
    for v in Q:
        common &= set(g.neighbors(v))
    return not common


def _graphs(p, count=40):
    rng = np.random.default_rng(1000 + int(p * 100))
    for _ in range(count):
        n = int(rng.integers(1, 81))
        yield _gnp(n, p, rng), rng


@pytest.mark.parametrize("p", PS)
def test_seed_clique_is_a_maximal_clique(p):
    for adj, rng in _graphs(p):
        n = adj.shape[0]
        core = mm.core_numbers(adj)
        for size in {1, min(n, 3), int(rng.integers(1, n + 1)), n}:
            S = rng.choice(n, size, replace=False).tolist()
            q0, kept = sm.seed_clique(adj, core, S)
            assert _is_maximal_clique(adj, q0), (n, S, q0)
            assert 1 <= kept <= len(q0) and set(q0[:kept]) <= set(S)
        assert sm.seed_clique(adj, core, []) == ([], 0)


@pytest.mark.parametrize("p", PS)
def test_a_clique_is_kept_whole(p):
    for adj, rng in _graphs(p):
        core = mm.core_numbers(adj)
        g = _nx(adj)
        cliques = list(nx.find_cliques(g))
        for Q in (cliques[0], cliques[-1], max(cliques, key=len)):
            S = Q[:max(1, len(Q) - int(rng.integers(0, 2)))]  # a clique, maximal or one short of it
            q0, kept = sm.seed_clique(adj, core, S)
            assert set(S) <= set(q0) and kept == len(S), (S, q0)
            assert _is_maximal_clique(adj, q0)


@pytest.mark.parametrize("p", PS)
def test_the_order_of_the_list_does_not_matter(p):
    for adj, rng in _graphs(p):
        n = adj.shape[0]
        core = mm.core_numbers(adj)
        S = rng.choice(n, int(rng.integers(1, n + 1)), replace=False)
        want = sm.seed_clique(adj, core, S.tolist())
        for _ in range(3):
            assert sm.seed_clique(adj, core, rng.permutation(S).tolist()) == want
        assert sm.seed_clique(adj, core, sorted(S.tolist(), reverse=True)) == want


@pytest.mark.parametrize("p", PS)
def test_a_planted_clique_survives_junk(p):
    """S = a planted clique P of k vertices plus 30 % random other vertices J, in random order. Inside S a planted
    vertex has degS >= k - 1. When every vertex of J that is not adjacent to all of P has degS < k - 1, the reduction
    takes such a vertex only after all of P (it is dropped when the first planted vertex it is not adjacent to is taken,
    and every planted vertex stays a candidate until taken, being adjacent to all of P and to every other vertex
    taken before it, which is then adjacent to all of P): Q0 contains P. That is asserted wherever the condition
    holds; it is a condition on the input, and it cannot be dropped: in G(n, 0.8) a vertex of J has about
    0.8 (1.3 k - 1) > k - 1 neighbours in S, is taken first and removes the planted vertices it is not adjacent to (the
    first instance drawn here at p = 0.8, n = 55, k = 13, loses planted vertex 15 that way). Where the condition does
    not hold Q0 is still a maximal clique that holds the vertices of P adjacent to everything taken."""
    rng = np.random.default_rng(2000 + int(p * 100))
    held = 0
    for _ in range(25):
        n = int(rng.integers(30, 81))
        k = int(rng.integers(10, 21))
        adj = _gnp(n, p, rng)
        Pl = rng.choice(n, k, replace=False)
        adj[np.ix_(Pl, Pl)] = True
        np.fill_diagonal(adj, False)
        others = np.setdiff1d(np.arange(n), Pl)
        junk = rng.choice(others, max(1, int(round(0.3 * k))), replace=False)
        S = np.concatenate([Pl, junk])
        q0, kept = sm.seed_clique(adj, mm.core_numbers(adj), rng.permutation(S).tolist())
        assert _is_maximal_clique(adj, q0) and 1 <= kept <= len(q0)
        taken = q0[:kept]
        assert all(v in q0 for v in Pl.tolist() if all(adj[v, u] for u in taken if u != v))
        degS = adj[np.ix_(S, S)].sum(axis=1)[k:]
        whole = adj[np.ix_(junk, Pl)].all(axis=1)
        if np.all(whole | (degS < k - 1)):
            held += 1
            assert set(Pl.tolist()) <= set(q0), (n, k, sorted(Pl.tolist()), q0)
            assert kept >= k
    print(f"p = {p}: the condition held in {held} of 25 instances")
    if p <= 0.5:
        assert held > 0


@pytest.mark.parametrize("p", PS)
def test_seeded_results_are_maximum_cliques_in_all_three_cases(p):
    cases = set()
    for adj, rng in _graphs(p, count=30):
        n = adj.shape[0]
        core = mm.core_numbers(adj)
        heu = mm.heu(adj, core)
        best = sm.maximum_clique(adj)
        w = len(nx.max_weight_clique(_nx(adj), weight=None)[0]) if adj.any() else 0
        assert len(best) == w and (w == 0 or mm.is_clique(adj, best))
        seeds = [best, best[:1], rng.choice(n, int(rng.integers(1, n + 1)), replace=False).tolist(), [int(rng.integers(n))]]
        for S in seeds:
            if not S:
                continue
            lst, winner, b = sm.seeded_exact(adj, S, best, core, heu)
            assert len(lst) == w, (S, lst, winner)
            if w:
                assert mm.is_clique(adj, lst) and winner in (0, 1, 2) and len(heu) <= b <= w
                cases.add(winner)
                q0 = sorted(sm.seed_clique(adj, core, S)[0])
                if winner == 2:
                    assert lst == q0 and len(q0) == b >= len(heu)
                elif winner == 1:
                    assert lst == best and len(heu) == w and (len(q0) < len(heu) or len(q0) < 2)
                else:
                    assert lst == best and b < w
                hl, hw, hb = sm.seeded_heu(adj, S, core, heu)
                assert hb == b and mm.is_clique(adj, hl) and len(hl) == b and hw == (2 if hl == q0 and len(q0) >= len(heu) else 1)
    if p >= 0.2:
        assert cases == {0, 1, 2}, cases


def test_small_cases_by_hand():
    # a path 0 - 1 - 2 and an isolated vertex 3
    adj = np.zeros((4, 4), bool)
    for a, b in ((0, 1), (1, 2)):
        adj[a, b] = adj[b, a] = True
    core = mm.core_numbers(adj)
    assert sm.seed_clique(adj, core, [0, 2]) == ([0, 1], 1)     # degS 0, 0: vertex 0; extended by its neighbour
    assert sm.seed_clique(adj, core, [2, 1, 0]) == ([1, 0], 2)  # degS(1) = 2; then 0 before 2
    assert sm.seed_clique(adj, core, [3]) == ([3], 1)           # an isolated vertex: a clique of one
    assert sm.seed_clique(adj, core, [3, 2]) == ([2, 1], 1)     # (2 and 3 tie at degS 0: the smaller index)
    assert sm.seeded_exact(adj, [3], [0, 1], core) == ([0, 1], 1, 2)  # behaves as unseeded
    assert sm.seeded_exact(adj, [2], [0, 1], core) == ([1, 2], 2, 2)  # ties go to the seed clique
    assert sm.seeded_heu(adj, [2], core) == ([1, 2], 2, 2)
    e = np.zeros((3, 3), bool)
    assert sm.seeded_exact(e, [1], []) == ([], 0, 0) and sm.seeded_heu(e, [1]) == ([], 0, 0)


def test_seed_plan_header(tmp_path):
    exe = str(tmp_path / "test_mc_seed_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "clipper_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_mc_seed_plan.cpp"), "-o", exe])
    out = subprocess.check_output([exe], timeout=300).decode()
    assert "mc seed plan ok" in out


def test_seeded_abi_matches_header(tmp_path):
    src = tmp_path / "mcs.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "clipper_hip.h"\nint main(void){'
                   'printf("%d %zu %zu %zu %zu %zu\\n", CLIPPER_HIP_MC_SEED_ONLY, sizeof(clipper_maxclique_seed_info_t),'
                   'offsetof(clipper_maxclique_seed_info_t, seed_given), offsetof(clipper_maxclique_seed_info_t, seed_kept),'
                   'offsetof(clipper_maxclique_seed_info_t, seed_size), offsetof(clipper_maxclique_seed_info_t, winner));'
                   'int (*f)(clipper_hip_t*, int, double, const int32_t*, int32_t, clipper_maxclique_info_t*,'
                   ' clipper_maxclique_seed_info_t*) = clipper_hip_max_clique_seeded;'
                   'int (*g)(clipper_hip_batch_t*, int, double, const int32_t*, const int64_t*, clipper_maxclique_info_t*,'
                   ' clipper_maxclique_seed_info_t*) = clipper_hip_batch_max_clique_seeded;'
                   'return f == 0 || g == 0;}\n')
    exe = tmp_path / "mcs"
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", os.path.dirname(build.build_hip()), "-lclipper_hip",
                           f"-Wl,-rpath,{os.path.dirname(build.HIP_LIB)}", "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = abi.MaxCliqueSeedInfo
    assert got[0] == abi.MC_SEED_ONLY == 3
    assert got[1] == ctypes.sizeof(S) == 16
    assert got[2:] == [getattr(S, n).offset for n in ("seed_given", "seed_kept", "seed_size", "winner")]
    L = abi.load_library()
    vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)
    assert L.clipper_hip_max_clique_seeded.argtypes == [vp, ctypes.c_int, ctypes.c_double, ip, ctypes.c_int32,
                                                        ctypes.POINTER(abi.MaxCliqueInfo), ctypes.POINTER(S)]
    assert L.clipper_hip_batch_max_clique_seeded.argtypes == [vp, ctypes.c_int, ctypes.c_double, ip,
                                                              ctypes.POINTER(ctypes.c_int64),
                                                              ctypes.POINTER(abi.MaxCliqueInfo), ctypes.POINTER(S)]
    # the unseeded structure and entry points are as they were
    assert ctypes.sizeof(abi.MaxCliqueInfo) == 56 and len(L.clipper_hip_max_clique.argtypes) == 4


def test_refusals_before_the_device():
    L = abi.load_library()
    assert L.clipper_hip_max_clique_seeded(None, abi.MC_EXACT, 0.0, None, -1, None, None) == -1
    assert L.clipper_hip_batch_max_clique_seeded(None, abi.MC_EXACT, 0.0, None, None, None, None) == -1


def test_facade_surfaces():
    import clipper_amd
    cp = clipper_amd.load_clipperpy()
    prm = cp.MCParams()
    assert prm.warm_start is False
    prm.warm_start = True
    assert prm.warm_start is True
    h = open(os.path.join(ROOT, "include", "clipper", "clipper.h")).read()
    assert "bool warm_start = false;" in h
    assert "void solveAsMaximumClique(const maxclique::Params& params, const std::vector<int>& seed);" in h
