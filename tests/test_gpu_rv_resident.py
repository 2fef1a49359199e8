"""The resident solver on a row view (csrc/k_rv_resident.hip.h; include/clipper_hip.h: clipper_hip_set_row_view
mode 2 switches it off): once a view fits the LDS of the chip, the iterations on it (clipper.cpp:226-280) run as
ONE launch of workgroups that keep complete columns of the view on chip. It starts from a prepared pass and
leaves one behind; whatever it does must be the streaming launches' result — the oracle's — up to the order of
the sums over the view's rows."""
import os

import numpy as np
import pytest

from clipper_amd import _abi as abi
from clipper_amd import synth
from oracle import clipper_ref as ref

pytestmark = pytest.mark.gpu


def _oracle(p):
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    return r.solve(p.u0)


def _ctx(p, storage, mode):
    g = abi.HipClipper(storage=storage)
    g.set_row_view(mode)
    g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    return g


@pytest.mark.parametrize("storage", [abi.STORE_F32_CSC, abi.STORE_F64_CSC])
@pytest.mark.parametrize("m,rho,seed", [(10000, 0.95, 12345), (10000, 0.95, 4), (6000, 0.9, 6777), (12000, 0.97, 5)])
def test_resident_on_a_view_equals_the_streamed_view_and_the_oracle(storage, m, rho, seed):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    sr = _oracle(p)
    g1, g2 = _ctx(p, storage, 0), _ctx(p, storage, 2)
    s1, s2 = g1.solve(p.u0), g2.solve(p.u0)
    st1, st2 = g1.view_stats(), g2.view_stats()
    assert st2.resident_launches == 0 and st2.builds >= 1
    assert st1.builds >= 1
    if st2.rows <= 1024 and st2.builds == 1:   # (a view of more rows is streamed as before)
        assert st1.resident_launches >= 1, (st1.builds, st1.rows, st1.resident_launches)
    for s in (s1, s2):
        assert s.nodes.tolist() == sr.nodes.tolist()
        assert s.ifinal == sr.ifinal
        assert abs(s.score - sr.score) <= 1e-6 * abs(sr.score)
    assert abs(s1.score - s2.score) <= 1e-10 * abs(s2.score)
    assert np.allclose(s1.u, s2.u, rtol=0, atol=1e-8)
    assert abs(s1.n_trials - s2.n_trials) <= max(2, s2.n_trials // 20)
    assert abs(s1.n_trials - sr.n_trials) <= max(2, sr.n_trials // 20)
    assert st1.view_passes >= 1
    # bit-reproducible from solve to solve (the exchange has a fixed order of additions)
    s1b = g1.solve(p.u0)
    assert np.array_equal(s1b.u, s1.u) and s1b.n_trials == s1.n_trials and s1b.n_passes == s1.n_passes
    print(f"m={m} rho={rho} storage={storage}: rows {st1.rows}, passes {s1.n_passes} ({st1.view_passes} on the view, "
          f"{st1.resident_launches} resident launch), trials {s1.n_trials} / streamed {s2.n_trials} / oracle {sr.n_trials}")
    g1.close()
    g2.close()


def test_headline_trials_and_ordered_list():
    """BASELINE's headline problem: 66 trials, the oracle's ordered node list."""
    p = synth.make_euclidean_problem(10000, 0.95, seed=12345)
    sr = _oracle(p)
    g = _ctx(p, abi.STORE_F32_CSC, 0)
    s = g.solve(p.u0)
    st = g.view_stats()
    assert st.resident_launches == 1
    assert s.nodes.tolist() == sr.nodes.tolist()
    assert s.n_trials == sr.n_trials == 66
    assert s.ifinal == sr.ifinal and abs(s.score - sr.score) <= 1e-9 * abs(sr.score)
    g.close()


def test_one_context_across_views_of_different_sizes():
    """One context scores and solves problems of changing size in turn: its plan image (a large plan, then a small one,
    in the same pinned buffer) and its exchange buffer (whose epochs go on from launch to launch) are reused. Each
    solve is a fresh context's solve of the same problem, at the level the first test holds two contexts to."""
    problems = [(10000, 0.95, 12345), (6000, 0.9, 6777), (10000, 0.95, 4), (6000, 0.9, 6777)]
    fresh = {}
    for key in dict.fromkeys(problems):
        p = synth.make_euclidean_problem(key[0], key[1], seed=key[2])
        gf = _ctx(p, abi.STORE_F32_CSC, 0)
        fresh[key] = (p, gf.solve(p.u0), gf.view_stats().resident_launches)
        gf.close()
    g = abi.HipClipper(storage=abi.STORE_F32_CSC)
    g.set_row_view(0)
    for key in problems:
        p, sf, launches = fresh[key]
        g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
        s = g.solve(p.u0)
        st = g.view_stats()
        assert s.nodes.tolist() == sf.nodes.tolist(), key
        assert s.ifinal == sf.ifinal, key
        assert abs(s.score - sf.score) <= 1e-10 * abs(sf.score), key
        assert np.allclose(s.u, sf.u, rtol=0, atol=1e-8), key
        if launches >= 1:
            assert st.resident_launches >= 1, (key, st.builds, st.rows, st.resident_launches)
    g.close()


@pytest.mark.parametrize("budget", [0, 1, 2, 3, 5, 9])
def test_leaving_after_a_few_exchanges_hands_a_prepared_pass_back(budget, monkeypatch):
    """CLIPPER_HIP_VIEW_RESIDENT_MAX_EXCHANGES (test knob): the launch leaves after that many iterations — in
    front of a window pass or of a penalty update's pair-mode pass, wherever the budget ends — and the
    streaming launches queued behind it carry on from the prepared pass it committed."""
    p = synth.make_euclidean_problem(10000, 0.95, seed=12345)
    sr = _oracle(p)
    monkeypatch.setenv("CLIPPER_HIP_VIEW_RESIDENT_MAX_EXCHANGES", str(budget))
    g = _ctx(p, abi.STORE_F32_CSC, 0)
    s = g.solve(p.u0)
    st = g.view_stats()
    assert st.resident_launches >= 1
    assert s.nodes.tolist() == sr.nodes.tolist() and s.ifinal == sr.ifinal
    assert abs(s.score - sr.score) <= 1e-9 * abs(sr.score)
    assert abs(s.n_trials - sr.n_trials) <= 2
    monkeypatch.delenv("CLIPPER_HIP_VIEW_RESIDENT_MAX_EXCHANGES")
    g.close()


@pytest.mark.parametrize("wgs", [96, 200])
def test_other_numbers_of_units(wgs, monkeypatch):
    """CLIPPER_HIP_VIEW_RESIDENT_WGS: another split of the view's columns over the workgroups (other lane groups,
    other pieces) — the same decisions, the sums associated differently."""
    p = synth.make_euclidean_problem(10000, 0.95, seed=12345)
    sr = _oracle(p)
    monkeypatch.setenv("CLIPPER_HIP_VIEW_RESIDENT_WGS", str(wgs))
    g = _ctx(p, abi.STORE_F32_CSC, 0)
    s = g.solve(p.u0)
    assert g.view_stats().resident_launches == 1
    assert s.nodes.tolist() == sr.nodes.tolist() and s.ifinal == sr.ifinal and s.n_trials == sr.n_trials
    assert abs(s.score - sr.score) <= 1e-9 * abs(sr.score)
    monkeypatch.delenv("CLIPPER_HIP_VIEW_RESIDENT_WGS")
    g.close()


def test_a_launch_that_gives_up_changes_nothing(monkeypatch):
    """A time-out of the exchange (forced: CLIPPER_HIP_VIEW_RESIDENT_TIMEOUT_TICKS=-1) commits nothing: the
    entry state is intact and the streaming launches run every iteration — bit for bit the solve of mode 2."""
    p = synth.make_euclidean_problem(10000, 0.95, seed=12345)
    g2 = _ctx(p, abi.STORE_F32_CSC, 2)
    s2 = g2.solve(p.u0)
    monkeypatch.setenv("CLIPPER_HIP_VIEW_RESIDENT_TIMEOUT_TICKS", "-1")
    g = _ctx(p, abi.STORE_F32_CSC, 0)
    s = g.solve(p.u0)
    st = g.view_stats()
    assert st.resident_giveups >= 1 and st.resident_launches == 0   # (reported, not counted as a launch that ran)
    assert np.array_equal(s.u, s2.u) and s.n_trials == s2.n_trials and s.nodes.tolist() == s2.nodes.tolist()
    monkeypatch.delenv("CLIPPER_HIP_VIEW_RESIDENT_TIMEOUT_TICKS")
    # the context backs off: its next solve streams its view without trying (bit for bit mode 2 again) ...
    s3 = g.solve(p.u0)
    st3 = g.view_stats()
    assert st3.resident_launches == 0 and st3.resident_giveups == 0 and st3.builds >= 1
    assert np.array_equal(s3.u, s2.u) and s3.n_trials == s2.n_trials
    # ... and the one after tries again — nothing forces a time-out now: the launch runs
    s4 = g.solve(p.u0)
    st4 = g.view_stats()
    assert st4.resident_launches == 1 and st4.resident_giveups == 0
    assert s4.nodes.tolist() == s2.nodes.tolist() and s4.n_trials == s2.n_trials
    g.close()
    g2.close()


def _tenant(ready, device, workgroups, lds_bytes, ms):
    from clipper_amd import _abi as abi2
    abi2.debug_occupy(device, 1, 0, 0.0)      # (the runtime is up before the parent is told)
    ready.set()
    abi2.debug_occupy(device, workgroups, lds_bytes, ms)


def test_another_tenant_on_the_device_costs_milliseconds_not_seconds():
    """A SECOND PROCESS holds the whole LDS of 40 CUs for half a second (a kernel that sleeps): the 246 units of the
    resident launch cannot all be resident, its first exchange times out — after 2 ms (round 4: 0.2 s) —, nothing is
    committed, and the streaming launches, which need no co-residency, finish the solve: within 10 ms, with the
    streamed views' result bit for bit. The give-up is reported and the context backs off (VERDICT r04 item 8,
    ADVICE r04)."""
    import multiprocessing as mp
    import time
    p = synth.make_euclidean_problem(10000, 0.95, seed=12345)
    g2 = _ctx(p, abi.STORE_F32_CSC, 2)
    s2 = g2.solve(p.u0)
    g = _ctx(p, abi.STORE_F32_CSC, 0)
    s0 = g.solve(p.u0)                         # warm: buffers, the view's arenas, the kernels' code objects
    assert g.view_stats().resident_launches == 1 and g.view_stats().resident_giveups == 0
    ctx = mp.get_context("spawn")
    ready = ctx.Event()
    child = ctx.Process(target=_tenant, args=(ready, 0, 40, 159 * 1024, 500.0))
    child.start()
    try:
        assert ready.wait(120.0), "the tenant process did not come up"
        time.sleep(0.1)                        # its kernel is on the device
        t0 = time.perf_counter()
        s = g.solve(p.u0)
        dt = time.perf_counter() - t0
    finally:
        child.join(60.0)
    st = g.view_stats()
    print(f"solve beside a tenant: {dt * 1e3:.2f} ms, resident launches {st.resident_launches}, give-ups {st.resident_giveups}")
    assert child.exitcode == 0
    assert st.resident_giveups == 1 and st.resident_launches == 0, (st.resident_launches, st.resident_giveups)
    assert np.array_equal(s.u, s2.u) and s.n_trials == s2.n_trials and s.nodes.tolist() == s2.nodes.tolist()
    # (a bound that a loaded box keeps — the regression it guards against was 200 ms)
    assert dt < 100e-3, f"{dt * 1e3:.1f} ms"
    s3 = g.solve(p.u0)                         # backing off: streamed, no attempt
    assert g.view_stats().resident_launches == 0 and g.view_stats().resident_giveups == 0
    s4 = g.solve(p.u0)                         # the tenant is gone: the launch runs again
    assert g.view_stats().resident_launches == 1
    assert s4.nodes.tolist() == s0.nodes.tolist() and s4.n_trials == s0.n_trials
    g.close()
    g2.close()


def test_two_inner_iterations_still_give_a_sound_answer():
    """maxiniters = 2 cuts every inner loop off after two steps: the homotopy advances from unconverged points and the
    reference's own answer depends on the order of its sums (profiles/r05_maxiniters_adjudication.md: the two oracles
    disagree with each other there), so nothing can be pinned — but every route must still end on a sound answer: the
    planted inliers (precision >= 0.95 against the ground truth), as many nodes as round(score), and an objective
    within a few percent of the oracle's."""
    p = synth.make_euclidean_problem(9000, 0.95, seed=314)
    prm = ref.Params(maxiniters=2)
    rr = ref.RefClipper(prm)
    rr.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    so = rr.solve(p.u0)
    for storage in (abi.STORE_F32_CSC, abi.STORE_F64_CSC):
        for mode in (0, 2, 1):   # resident on a view / streamed views / no views
            g = _ctx(p, storage, mode)
            g.params.maxiniters = 2
            s = g.solve(p.u0)
            sel = g.get_selected_associations()
            prec, rec = synth.precision_recall(sel, p.Agt)
            assert len(s.nodes) == int(np.floor(s.score + 0.5)), (storage, mode)
            assert prec >= 0.95 and rec >= 0.5, (storage, mode, prec, rec)
            assert abs(s.score - so.score) <= 0.05 * abs(so.score), (storage, mode, s.score, so.score)
            g.close()


def test_matrix_without_points_and_parameter_variants():
    """A matrix that was handed over (its views are filtered out of its own slices) and solver parameters that
    move the exits around (few inner iterations: many penalty updates; a loose line search)."""
    p = synth.make_euclidean_problem(4000, 0.9, seed=99)
    r = ref.RefClipper()
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    M, Cm = r.get_affinity_matrix(), r.get_constraint_matrix()
    for kw in ({}, {"maxiniters": 3, "maxoliters": 30}, {"beta": 0.5, "maxlsiters": 12}, {"tol_u": 1e-5, "tol_F": 1e-6}, {"rescale_u0": 0}):
        # (each oracle solve: a fraction of a second here — a line search capped at a few trials never converges and
        # runs the reference's loops to their limits: hours on the CPU)
        prm = ref.Params()
        for k, v in kw.items():
            setattr(prm, k, v)
        rr = ref.RefClipper(prm)
        rr.set_matrix_data(M, Cm)
        so = rr.solve(p.u0)
        g = abi.HipClipper(storage=abi.STORE_F64_CSC)
        g.set_matrix_data(M, Cm)
        for k, v in kw.items():
            setattr(g.params, k, v)
        s = g.solve(p.u0)
        st = g.view_stats()
        assert s.nodes.tolist() == so.nodes.tolist(), kw
        assert s.ifinal == so.ifinal and abs(s.score - so.score) <= 1e-9 * abs(so.score), kw
        assert abs(s.n_trials - so.n_trials) <= max(2, so.n_trials // 20), (kw, s.n_trials, so.n_trials)
        print(f"{kw}: views {st.builds}, rows {st.rows}, resident launches {st.resident_launches}, trials {s.n_trials} (oracle {so.n_trials})")
        g.close()


def _random_cases(n, seed=20260927):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        m = int(rng.integers(3000, 22000))
        rho = float(rng.choice([0.8, 0.88, 0.92, 0.95, 0.97]))
        out.append((m, rho, int(rng.integers(1, 10**6)), k))
    return out


@pytest.mark.parametrize("m,rho,seed,k", _random_cases(14))
def test_random_sizes_resident_equals_streamed(m, rho, seed, k):
    """Seeded random sizes and outlier ratios between the smallest problem that gets a window (views need one) and the
    largest whose view can fit the chip: whatever the policy decides — no view, a streamed view, a resident launch,
    a launch that leaves early — the solve equals the solve with streamed views; every third case also the oracle."""
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    storage = abi.STORE_F64_CSC if k % 2 else abi.STORE_F32_CSC
    g1, g2 = _ctx(p, storage, 0), _ctx(p, storage, 2)
    s1, s2 = g1.solve(p.u0), g2.solve(p.u0)
    st1 = g1.view_stats()
    assert s1.nodes.tolist() == s2.nodes.tolist() and s1.ifinal == s2.ifinal
    assert abs(s1.score - s2.score) <= 1e-10 * abs(s2.score)
    assert abs(s1.n_trials - s2.n_trials) <= max(2, s2.n_trials // 20)
    if k % 3 == 0 and m <= 11000:   # (the oracle's solve: seconds up to here, a minute at the upper end of the range)
        sr = _oracle(p)
        assert s1.nodes.tolist() == sr.nodes.tolist() and s1.ifinal == sr.ifinal
        assert abs(s1.score - sr.score) <= 1e-6 * abs(sr.score)
    print(f"m={m} rho={rho} storage={storage}: views {st1.builds} (rows {st1.rows}), resident launches {st1.resident_launches}, "
          f"passes {s1.n_passes} ({st1.view_passes} on a view), trials {s1.n_trials} / streamed {s2.n_trials}")
    g1.close()
    g2.close()


def test_a_row_outside_the_view_becomes_live_inside_the_launch():
    """m = 20 000, rho = 0.97, seed 8: three iterations into the resident launch a row OUTSIDE its view gets a
    positive gradient. The launch leaves a window whose candidates at that row are not zero: its norms must
    include the row (SolverState::resume = 3: raw sums over the view, completed by the launch that runs the pass).
    Round 4 found this with a randomized A/B: the norms went out summed over the view only, the line search behind
    them rejected 99 step sizes before it recovered — same answer, 190 trials instead of the oracle's 95 (the
    oracle's solve takes 8 s at this size and is not repeated here: the streamed views are held against it
    elsewhere, and 95 is asserted)."""
    p = synth.make_euclidean_problem(20000, 0.97, seed=8)
    g1, g2 = _ctx(p, abi.STORE_F32_CSC, 0), _ctx(p, abi.STORE_F32_CSC, 2)
    s1, s2 = g1.solve(p.u0), g2.solve(p.u0)
    st1 = g1.view_stats()
    assert st1.resident_launches >= 2 and st1.builds == 2   # (left once for the row, entered again on the next view)
    assert s2.n_trials == 95 and abs(s1.n_trials - 95) <= 2
    assert s1.nodes.tolist() == s2.nodes.tolist() and s1.ifinal == s2.ifinal
    assert abs(s1.score - s2.score) <= 1e-10 * abs(s2.score)
    assert abs(s1.n_passes - s2.n_passes) <= 5   # (the streamed route repeats a window whose single-candidate pass guessed wrong: SolverState::weff)
    g1.close()
    g2.close()


# Solver parameters that cut the inner loop short (clipper.h:33 maxiniters) on problems whose view goes to the resident
# solver. profiles/r05_maxiniters_adjudication.md: with maxiniters = 2 the reference's OWN answer depends on the order
# of its sums (the C++ oracle and the numpy statement of the same loop end on different `ifinal` in more than half of
# the problems two GPU paths disagreed on in round 4) — nothing can be pinned there. From five inner iterations on
# everything agrees: the two oracles with each other (checked on these six when they were chosen), and both GPU routes
# with them — which is what this test pins.
_TRUNCATED = [
    (11152, 0.95, 994540, dict(beta=0.1, maxlsiters=99, maxiniters=20, maxoliters=6, tol_u=1e-8, tol_F=1e-12, rescale_u0=0, eps=1e-7)),
    (11883, 0.97, 685350, dict(beta=0.25, maxlsiters=12, maxiniters=5, maxoliters=1000, tol_u=1e-8, tol_F=1e-7, rescale_u0=1, eps=1e-9)),
    (9094, 0.95, 214975, dict(beta=0.25, maxlsiters=20, maxiniters=5, maxoliters=1000, tol_u=1e-8, tol_F=1e-7, rescale_u0=0, eps=1e-9)),
    (7517, 0.92, 850845, dict(beta=0.25, maxlsiters=12, maxiniters=5, maxoliters=6, tol_u=1e-6, tol_F=1e-7, rescale_u0=0, eps=1e-7)),
    (16038, 0.97, 702307, dict(beta=0.25, maxlsiters=12, maxiniters=200, maxoliters=40, tol_u=1e-10, tol_F=1e-7, rescale_u0=0, eps=1e-9)),
    (14399, 0.97, 590658, dict(beta=0.1, maxlsiters=12, maxiniters=5, maxoliters=1000, tol_u=1e-8, tol_F=1e-12, rescale_u0=0, eps=1e-9)),
]


@pytest.mark.parametrize("m,rho,seed,kw", _TRUNCATED)
def test_inner_loops_of_five_or_more_iterations_agree_with_the_oracle(m, rho, seed, kw):
    p = synth.make_euclidean_problem(m, rho, seed=seed)
    r = ref.RefClipper(ref.Params(**kw))
    r.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
    so = r.solve(p.u0)
    launches = 0
    for storage in (abi.STORE_F64_CSC, abi.STORE_F32_CSC):
        for mode in (0, 2):
            g = abi.HipClipper(storage=storage)
            g.set_row_view(mode)
            for k, v in kw.items():
                setattr(g.params, k, v)
            g.score_pairwise_consistency_euclidean(p.D1, p.D2, p.A, **synth.EUCLID_BENCH_PARAMS)
            s = g.solve(p.u0)
            st = g.view_stats()
            launches += st.resident_launches
            assert sorted(s.nodes.tolist()) == sorted(so.nodes.tolist()), (storage, mode)
            assert s.ifinal == so.ifinal, (storage, mode, s.ifinal, so.ifinal)
            assert abs(s.score - so.score) <= 1e-6 * abs(so.score), (storage, mode)
            assert abs(s.n_trials - so.n_trials) <= max(2, so.n_trials // 20), (storage, mode, s.n_trials, so.n_trials)
            g.close()
    assert launches >= 1   # (each of these problems' views fits the chip: the default route went through a resident launch)
