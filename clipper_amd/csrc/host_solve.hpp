// host_solve.hpp — the solve of one context (CLIPPER::solve -> findDenseClique, clipper.cpp:172-323)
// and the context's teardown. Part of clipper_hip.hip (one translation unit; included there, in order).
//
// The state machine lives in device memory (SolverState); one iteration is k_gemv (decide, then stream M against a
// window of V candidates) and k_tail. A solve: the per-solve resets (solve_begin); the whole solve as one launch where
// the slices fit (resident_solve, host_resident.hpp); otherwise the streaming launches (solve_streamed) — one process
// keeps a few iterations queued ahead of what the device reports retired in a pinned record and handles the holds
// (solve_in_process, solve_hold), several processes run batches between state snapshots (solve_multi_process); the
// final u, rounding and the result (solve_finish); the timings of the profiling event pairs (solve_timings).
#pragma once

namespace {

// make_ctx's counterpart (a batch's children and the live sub-problem's contexts go the same way)
void destroy_ctx(Ctx* h) {
  if (!h) return;
  for (auto& s : h->sh) {
    hipSetDevice(s.device);
    if (s.stream) hipStreamSynchronize(s.stream);
  }
  if (h->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(h->comm);
  sub_free(h);  // (the live sub-problem's context borrows this one's stream: before the stream goes)
  std::vector<std::pair<int, hipStream_t>> streams;  // (this context's own: a borrowed one stays)
  for (auto& s : h->sh)
    if (s.stream && !h->borrowed_stream) streams.emplace_back(s.device, s.stream);
  const int dev0 = h->sh.empty() ? -1 : h->sh[0].device;
  h->sh.clear();  // every shard's buffers and events, before its stream
  for (auto& ds : streams) {
    hipSetDevice(ds.first);
    hipStreamDestroy(ds.second);
  }
  if (dev0 >= 0) hipSetDevice(dev0);
  delete h;  // the context's own events and pinned arrays, the resident solvers' buffers
}

// the pinned staging of the final u (the device writes it), large enough for this context's m
int ensure_u_pinned(Ctx* h) {
  if (h->u_pinned.cap >= static_cast<size_t>(h->m)) return 0;
  h->u_pinned.reset();
  HIPCHK(hipSetDevice(h->sh[0].device));
  HIPCHK(h->u_pinned.alloc(static_cast<size_t>(h->m), hipHostMallocMapped | hipHostMallocCoherent));
  return 0;
}

// utils::selectInlierAssociations (utils.cpp:101-108): the associations of `nodes`, column-major k x 2, into `out`
void selected_associations(const Ctx* h, const std::vector<int32_t>& nodes, int32_t* out) {
  const size_t k = nodes.size();
  for (size_t r = 0; r < k; ++r) {
    const size_t a = static_cast<size_t>(nodes[r]);
    out[r] = h->A[a];
    out[k + r] = h->A[static_cast<size_t>(h->m) + a];
  }
}

// rounding — clipper.cpp:287-310 with utils.cpp:33-68, on the host (a lone solve and every problem of a batch)
int round_nodes(Ctx* h, int rounding, const std::vector<double>& u, double F, std::vector<int32_t>& nodes) {
  const int64_t m = static_cast<int64_t>(u.size());
  nodes.clear();
  if (rounding == CLIPPER_ROUNDING_NONZERO) {
    for (int64_t i = 0; i < m; ++i)
      if (u[static_cast<size_t>(i)] > 0.0) nodes.push_back(static_cast<int32_t>(i));
  } else if (rounding == CLIPPER_ROUNDING_DSD) {
    // :294-300 — exact densest subgraph of the graph induced by the non-zero entries of u; where u == 0 (every pair
    // forbidden: the iteration ends at the zero vector) the list is empty, which dsd::solve reads as EVERY node
    // (dsd.cpp:278-284) — as clipper_hip_densest_subgraph does with k <= 0
    std::vector<int32_t> S;
    for (int64_t i = 0; i < m; ++i)
      if (u[static_cast<size_t>(i)] > 0.0) S.push_back(static_cast<int32_t>(i));
    if (S.empty())
      for (int64_t i = 0; i < m; ++i) S.push_back(static_cast<int32_t>(i));
    if (int rc = densest_subgraph_of(h, S, nodes)) return rc;
  } else {
    const int omega = static_cast<int>(std::round(F));  // :305
    nodes = indices_of_k_largest(u, omega);             // :308
  }
  return 0;
}

// the solve's parameters, checked, as the kernels take them (a lone solve and every problem of a batch)
int solver_params(const clipper_params_t* P, SolverParams& prm) {
  if (!P) return fail(CLIPPER_HIP_E_INVALID, "params are required");
  if (P->rounding != CLIPPER_ROUNDING_NONZERO && P->rounding != CLIPPER_ROUNDING_DSD_HEU &&
      P->rounding != CLIPPER_ROUNDING_DSD)
    return fail(CLIPPER_HIP_E_INVALID, "unknown rounding mode %d", P->rounding);
  if (P->maxlsiters < 1) return fail(CLIPPER_HIP_E_INVALID, "maxlsiters must be >= 1");
  prm = SolverParams{P->tol_u, P->tol_F, P->beta, P->eps, P->maxiniters, P->maxoliters, P->maxlsiters};
  return 0;
}

void solve_info(clipper_solve_info_t& info, const SolveShared& fin) {  // (num_nodes and seconds: the caller's)
  info.score = fin.F;
  info.d = fin.d;
  info.ifinal = fin.ifinal;
  info.n_passes = fin.n_passes;
  info.n_trials = fin.n_trials;
}

// CLIPPER_HIP_HOST_TIMING: where the host side of a solve goes (us since entry, to stderr)
struct SolveMarks {
  const std::chrono::high_resolution_clock::time_point t0 = std::chrono::high_resolution_clock::now();
  const bool on = [] { static const bool env = std::getenv("CLIPPER_HIP_HOST_TIMING") != nullptr; return env; }();
  std::vector<std::pair<const char*, double>> marks;
  void operator()(const char* what) {
    if (on) marks.emplace_back(what, std::chrono::duration<double, std::micro>(std::chrono::high_resolution_clock::now() - t0).count());
  }
};

// the per-solve resets, and the state the prologue starts from
int solve_begin(Ctx* h, bool rescale, SolverState& init) {
  h->rv_stats = clipper_hip_view_stats_t{};
  h->ev_used = 0;
  std::fill(h->ev_xchg_used.begin(), h->ev_xchg_used.end(), 0);
  if (h->profiling) {  // marks of the previous solve
    const size_t n = static_cast<size_t>(std::min<int64_t>(h->launch_counter + 1, KIND_CAP));
    std::memset(h->kind, 0, n);
    HIPCHK(hipSetDevice(h->sh[0].device));
    HIPCHK(hipMemsetAsync(h->sh[0].marks, 0, n, h->sh[0].stream));
  }
  h->launch_counter = 0;
  std::memset(&init, 0, sizeof(init));
  init.alpha = 1.0;
  for (int l = 0; l < VS; ++l) init.nrm[l] = 1.0;
  init.nlive = init.nout = static_cast<int32_t>(std::min<int64_t>(h->m, 0x7fffffff));  // unknown until a tail counts
  init.rv_last = -100;
  init.zero_run = 2;  // (no line search has rejected anything yet: the first windows multiply candidate 0 alone)
  // with rescaling the first iteration runs the pair pass on u0; without, it only normalises
  init.phase = rescale ? PH_RESCALE : PH_NORMALIZE;
  init.stage = rescale ? ST_PASS : ST_RESULTS;
  rowview_drop(h);  // a solve starts without a view: what it builds is a function of this solve alone
  rvr_begin_solve(h);
  sub_begin_solve(h);
  h->rvp = rowview_policy(h);
  return ensure_u_pinned(h);
}

// after a hold: the hold lifted, launches counted from the device's iteration count, the idle ones' event pairs dropped
void hold_rewind(Ctx* h) {
  volatile HostMirror* hm = h->mirror;
  hm->hold = 0;
  h->launch_counter = hm->iters;
  while (h->ev_used > 0 && h->ev_launch_index[static_cast<size_t>(h->ev_used - 1)] >= hm->iters) --h->ev_used;
}

void sub_account(Ctx* h) {  // the passes since the hand-over ran on the sub-problem
  h->sub.sub_passes += std::max<int64_t>(0, h->mirror->n_passes - h->sub.passes_at_entry);
}

// HOLD_ROW_VIEW: the view is built from exactly the state that asked (k_solver.hip.h, LIVE ROWS)
int solve_hold_view(Ctx* h, const SolverParams& prm, int64_t& queued, SolveMarks& mark) {
  int rc;
  bool built = false;
  if ((rc = rowview_build(h, built))) return rc;
  mark("view built");
  const bool early = h->early_decide_done;  // the decide-only iteration went out behind the fill (host_rowview.hpp):
  h->early_decide_done = false;             // the hold is lifted, rv_fresh was used by it
  if (early) ++queued;
  else h->rv_fresh = built;
  if (built && h->vres.ready) {
    // The view fits the LDS of the chip: the iterations on it run as ONE launch (k_rv_resident.hip.h).
    // A decide-only iteration turns the held decision into a prepared pass; the resident launch starts
    // from it and leaves a prepared pass (or the end of the solve) for whatever is queued behind it.
    if (!early) {
      if ((rc = enqueue_iteration(h, prm, true))) return rc;
      ++queued;
    }
    bool launched = false;
    if ((rc = rvr_enqueue(h, prm, launched))) return rc;
    mark("resident queued");
  }
  if ((rc = rowview_finish_plan(h))) return rc;  // (a work list put off while the resident launch was prepared)
  // a view the resident solver does not take: the live sub-problem of its rows is prepared now, and entered
  // when the decision finds that nothing outside it can come back to life
  if (built && !h->vres.ready && !early) {
    // (an optimisation: if it cannot be prepared — no memory for the child's buffers — the solve goes on without)
    if (int r2 = sub_prepare(h)) {
      if (r2 != CLIPPER_HIP_E_NOMEM) return r2;
      (void)hipGetLastError();
      h->sub.ready = false;
    }
    mark("sub-problem prepared");
  }
  return 0;
}

// The decision put the solve on hold (HostMirror::hold says why): whatever was queued behind it does nothing.
// The host does what was asked and lifts the hold; `queued` counts what the device will retire.
int solve_hold(Ctx* h, const SolverParams& prm, int64_t& queued, SolveMarks& mark) {
  volatile HostMirror* hm = h->mirror;
  mark("hold seen");
  if (mark.on)
    std::fprintf(stderr, "[solve] hold: iters %lld passes %lld trials %lld view passes %lld live %d of which outside the view %d\n",
                 static_cast<long long>(hm->iters), static_cast<long long>(hm->n_passes), static_cast<long long>(hm->n_trials),
                 static_cast<long long>(hm->n_view_passes), static_cast<int>(hm->hold_nlive), static_cast<int>(hm->nout));
  // (No drain: the iterations queued behind the hold do nothing but move the state between its two copies, in
  // stream order — the build's launches queue behind them and read copy h->par, where the last of them leaves it;
  // the build itself waits for the stream once. An in-process GROUP holds on every shard: its streams are drained,
  // the shards' builds are not ordered with each other otherwise.)
  int rc;
  if (h->sh.size() > 1 && (rc = sync_all(h))) return rc;
  std::atomic_thread_fence(std::memory_order_acquire);
  const int reason = hm->hold;
  hold_rewind(h);
  queued = hm->iters;  // the iterations that did nothing never counted
  switch (reason) {
    case HOLD_SUB_ENTER:  // the hand-over to the live sub-problem (host_subproblem.hpp)
      if ((rc = sub_enter(h, prm))) return rc;
      ++queued;  // (its decide-only iteration)
      mark("sub-problem entered");
      return 0;
    case HOLD_SUB_LEAVE:  // ... and the way back
      sub_account(h);
      if ((rc = sub_leave(h))) return rc;
      mark("sub-problem left");
      return 0;
    default: return solve_hold_view(h, prm, queued, mark);
  }
}

// One process: the deciding workgroup reports progress into pinned host memory; the host keeps RUN_AHEAD iterations
// queued ahead of what the device has retired and stops queueing the moment `done` shows up — no memcpy, no event, no
// host wait in the loop.
int solve_in_process(Ctx* h, const SolverParams& prm, SolveShared& fin, SolveMarks& mark) {
  volatile HostMirror* hm = h->mirror;
  Shard& s0 = h->sh[0];
  int64_t queued = 0;
  uint64_t spins = 0;
  h->rv_fresh = false;
  int rc;
  while (!hm->done) {
    if (hm->hold) {
      if ((rc = solve_hold(h, prm, queued, mark))) return rc;
      continue;
    }
    if (hm->iters > queued) queued = hm->iters;  // (a resident launch retired many iterations at once)
    if (queued - hm->iters < RUN_AHEAD) {
      // (while the solve runs on the live sub-problem the same launches go out with the child context's arguments)
      if ((rc = enqueue_iteration(h->sub.active ? h->sub.use : h, prm, false))) return rc;
      ++queued;
      spins = 0;
    } else if ((++spins & 0xfffff) == 0) {
      // the device has not retired an iteration for a long time: make sure it is still alive
      hipError_t q = hipStreamQuery(s0.stream);
      if (q != hipSuccess && q != hipErrorNotReady)
        return fail(CLIPPER_HIP_E_HIP, "solver stream failed: %s", hipGetErrorString(q));
      if (q == hipSuccess && !hm->done && queued - hm->iters >= RUN_AHEAD)
        return fail(CLIPPER_HIP_E_HIP, "solver made no progress (iters %lld of %lld queued)",
                    static_cast<long long>(hm->iters), static_cast<long long>(queued));
    }
  }
  mark("done seen");
  std::atomic_thread_fence(std::memory_order_acquire);
  if (h->sub.active) {  // the solve ended on the live sub-problem (its deciding workgroup wrote u through the list of S)
    sub_account(h);
    h->sub.active = false;
  }
  fin = mirror_result(hm);
  h->rv_stats.view_passes = hm->n_view_passes;
  return 0;
}

// Several processes: every rank must queue the same number of iterations (each holds a collective), so the decision
// to stop rests on state snapshots only, which are bit-identical on all ranks. Batch n+1 is queued before the snapshot
// after batch n is read.
int solve_multi_process(Ctx* h, const SolverParams& prm, SolveShared& fin) {
  Shard& s0 = h->sh[0];
  int batch = SOLVE_BATCH;
  if (const char* e = std::getenv("CLIPPER_HIP_SOLVE_BATCH")) batch = std::max(1, std::atoi(e));  // tuning knob, same on every rank
  HIPCHK(hipSetDevice(s0.device));
  h->rv_fresh = false;
  int rc = run_batched_with_holds(
      batch, [&]() { return enqueue_iteration(h, prm, false); },
      [&](int slot) -> int {
        HIPCHK(hipSetDevice(s0.device));
        HIPCHK(hipMemcpyAsync(&h->host_state[slot], s0.shared, sizeof(SolveShared), hipMemcpyDeviceToHost, s0.stream));
        HIPCHK(hipEventRecord(h->ev_poll[slot], s0.stream));
        return 0;
      },
      [&](int slot, int& st) -> int {
        HIPCHK(hipEventSynchronize(h->ev_poll[slot]));
        st = h->host_state[slot].done != 0 ? 1 : (h->host_state[slot].hold != 0 ? 2 : 0);
        return 0;
      },
      [&]() -> int {
        // every rank reads the hold from the same snapshot: all of them have queued the same
        // iterations, so draining cannot wait for a peer; then each builds its columns of the view
        if (int r2 = sync_all(h)) return r2;
        hold_rewind(h);
        bool built = false;
        if (int r2 = rowview_build(h, built)) return r2;
        h->rv_fresh = built;
        // a view small enough for the resident solver: every rank runs it on a replica of the view (no exchange
        // for the iterations inside the launch; host_rv_resident.hpp)
        if (built)
          if (int r2 = rvr_replica_handover(h, prm)) return r2;
        return 0;
      },
      nullptr);
  if (rc) return rc;
  if ((rc = sync_all(h))) return rc;
  HIPCHK(hipSetDevice(s0.device));
  HIPCHK(hipMemcpy(&fin, s0.shared, sizeof(fin), hipMemcpyDeviceToHost));
  h->rv_stats.view_passes = h->mirror->n_view_passes;
  return 0;
}

// the streaming launches: the prologue, then one process's run-ahead loop or the ranks' batched one
int solve_streamed(Ctx* h, const SolverParams& prm, const SolverState& init, SolveShared& fin, SolveMarks& mark) {
  // prologue, one launch per shard: pending vector = u0 (T pair 0, nrm = 1), state, counters
  h->par = 0;
  std::memset(h->mirror, 0, sizeof(HostMirror));
  std::atomic_thread_fence(std::memory_order_seq_cst);
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    const SolveArgs a = solve_args(h, s, prm, 0, false);
    hipLaunchKernelGGL(k_init, dim3(static_cast<unsigned>(ceil_div(h->m, 256))), dim3(256), 0, s.stream, a, init, s.st, s.X[0]);
  }
  mark("init queued");
  int rc;
  if (!h->multiproc) {
    h->solve_prm = &prm;  // (the view build queues its early decide-only iteration with them: host_rowview.hpp)
    rc = solve_in_process(h, prm, fin, mark);
    h->solve_prm = nullptr;
  } else {
    rc = solve_multi_process(h, prm, fin);
  }
  if (rc) return rc;
  rvr_end_solve(h);  // (launches of the resident solver on a view that gave up: counted, the context backs off)
  return 0;
}

// the final u, rounding, the result and the view statistics
int solve_finish(Ctx* h, int rounding, const SolveShared& fin, double* u_out, clipper_solve_info_t* info, SolveMarks& mark) {
  Shard& s0 = h->sh[0];
  const int64_t m = h->m;
  const size_t vbytes = static_cast<size_t>(m) * sizeof(double);
  int rc;
  HIPCHK(hipSetDevice(s0.device));
  if (h->multiproc) {
    const double* u_dev = s0.pt + ((static_cast<int64_t>(fin.ubp & 1) * h->V + fin.ubv) * 2 + 0) * h->mp;
    HIPCHK(hipMemcpyAsync(h->u_pinned, u_dev, vbytes, hipMemcpyDeviceToHost, s0.stream));
    if (h->profiling)
      HIPCHK(hipMemcpyAsync(h->kind, s0.marks, static_cast<size_t>(std::min<int64_t>(h->launch_counter, KIND_CAP)),
                            hipMemcpyDeviceToHost, s0.stream));
    if ((rc = sync_all(h))) return rc;
  } else {
    // one process: the deciding workgroup wrote u into the pinned buffer before it raised `done`;
    // the few no-op launches still queued drain behind the caller's back (stream order keeps
    // every later call behind them)
    HIPCHK(hipGetLastError());
  }
  std::vector<double>& u = h->u_host;  // (kept from solve to solve: no allocation on the way out)
  u.assign(h->u_pinned.p, h->u_pinned.p + m);
  std::vector<int32_t> nodes;
  if ((rc = round_nodes(h, rounding, u, fin.F, nodes))) return rc;
  h->nodes = nodes;
  if (u_out) std::memcpy(u_out, u.data(), vbytes);
  mark("rounded");
  if (mark.on) {
    std::fprintf(stderr, "[solve]");
    for (const auto& mk : mark.marks) std::fprintf(stderr, " %s %.1f |", mk.first, mk.second);
    std::fprintf(stderr, "\n");
  }
  const double secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - mark.t0).count();
  h->tm.solve_total_ms = secs * 1e3;
  if (info) {
    solve_info(*info, fin);
    info->seconds = secs;
    info->num_nodes = static_cast<int32_t>(nodes.size());
  }
  h->rv_stats.passes = fin.n_passes;
  h->rv_stats.sub_leaves = h->sub.leaves;
  h->rv_stats.sub_passes = h->sub.sub_passes;
  h->rv_stats.sub_build_ms = h->sub.build_ms;
  if (h->rv_stats.sub_entries > 0 && h->sub.use) {
    h->rv_stats.sub_rows = h->sub.nS;
    // what a pass on it streams: the slices, or (a mostly non-zero sub-problem) the dense fp32 store
    h->rv_stats.sub_bytes = h->sub.use->csc_valid ? static_cast<int64_t>(h->sub.use->sh[0].s_bytes)
                                                   : static_cast<int64_t>(algorithmic_gemv_bytes(h->sub.use));
    h->rv_stats.sub_dense = h->sub.use->csc_valid ? 0 : 1;
  }
  return 0;
}

// mat-vec timings from the event pairs
int solve_timings(Ctx* h) {
  h->tm.gemv_avg_us = h->tm.gemv_min_us = 0.0;
  h->tm.gemv_launches = 0;
  h->tm.gemv_bytes = algorithmic_gemv_bytes(h);
  h->tm.gemv_useful_bytes = h->csc_valid ? static_cast<double>(h->sh[0].s_entries) * (h->esize() + 1.0) : h->tm.gemv_bytes;
  if (!h->profiling || h->ev_used <= 0) return 0;
  // only launches that streamed M count: the device marked every iteration it ran (PassMark); launches queued past
  // convergence have no mark
  const uint8_t* kind = h->kind;
  const int64_t iters_run = std::min<int64_t>(h->launch_counter, KIND_CAP);
  double sum = 0.0, mn = 1e30, vsum = 0.0, ssum = 0.0, xs = 0.0;
  int64_t nreal = 0, nview = 0, nsub = 0, nx = 0;
  for (int k = 0; k < h->ev_used; ++k) {
    const int64_t li = h->ev_launch_index[static_cast<size_t>(k)];
    if (li >= iters_run || kind[static_cast<size_t>(li)] == MARK_NONE) continue;
    float ms = 0.f;
    if (h->ev_xchg_used[static_cast<size_t>(k)]) {  // the exchange of the same iteration (column shards)
      HIPCHK(hipEventElapsedTime(&ms, h->ev_xchg[2 * k], h->ev_xchg[2 * k + 1]));
      xs += ms;
      ++nx;
    }
    HIPCHK(hipEventElapsedTime(&ms, h->ev_pairs[2 * k], h->ev_pairs[2 * k + 1]));
    const uint8_t mk = kind[static_cast<size_t>(li)];
    if (mk == MARK_VIEW) {  // the launch streamed the row view, not M
      vsum += ms;
      ++nview;
    } else if (mk == MARK_SUB_WINDOW) {  // a window pass on the live sub-problem
      ssum += ms;
      ++nsub;
    } else if (mk == MARK_WINDOW) {  // (a pair-mode pass, one vector, is not the window pass the roofline is about)
      sum += ms;
      mn = std::min<double>(mn, ms);
      ++nreal;
    }
  }
  h->tm.exchange_avg_us = 0.0;
  h->tm.exchange_samples = 0;
  h->tm.exchange_bytes = static_cast<double>(nslot(h->V)) * static_cast<double>(h->W) * sizeof(double);
  if (nx > 0) {
    h->tm.exchange_avg_us = xs / static_cast<double>(nx) * 1e3;
    h->tm.exchange_samples = nx;
  }
  if (nview > 0) {
    h->rv_stats.view_pass_avg_us = vsum / static_cast<double>(nview) * 1e3;
    h->rv_stats.view_pass_samples = nview;
  }
  if (nsub > 0) {
    h->rv_stats.sub_pass_avg_us = ssum / static_cast<double>(nsub) * 1e3;
    h->rv_stats.sub_pass_samples = nsub;
  }
  if (nreal > 0) {
    h->tm.gemv_avg_us = sum / static_cast<double>(nreal) * 1e3;
    h->tm.gemv_min_us = mn * 1e3;
    h->tm.gemv_launches = nreal;
  }
  return 0;
}

// The solve of a context whose u0 is staged (a lone solve; a problem of a batch that runs alone).
int solve_staged(Ctx* h, const clipper_params_t* P, double* u_out, clipper_solve_info_t* info) {
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (!h->u0_staged) return fail(CLIPPER_HIP_E_STATE, "clipper_hip_stage_u0 not called");
  if (P && P->rounding == CLIPPER_ROUNDING_DSD && h->multiproc)
    return fail(CLIPPER_HIP_E_SCOPE, "Rounding::DSD needs the induced sub-matrix on one host: not available on a multi-process shard");
  SolverParams prm;
  int rc;
  if ((rc = solver_params(P, prm))) return rc;
  SolveMarks mark;
  SolverState init;
  if ((rc = solve_begin(h, P->rescale_u0 != 0, init))) return rc;
  SolveShared fin{};
  bool resident = false;
  if ((rc = resident_solve(h, prm, P->rescale_u0 != 0, fin, resident))) return rc;
  h->last_solver = resident ? 1 : 0;
  if (!resident && (rc = solve_streamed(h, prm, init, fin, mark))) return rc;
  if ((rc = solve_finish(h, P->rounding, fin, u_out, info, mark))) return rc;
  return solve_timings(h);
}

int stage_u0(Ctx* h, const double* u0) {  // u0 to every shard
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  const size_t vbytes = static_cast<size_t>(h->m) * sizeof(double);
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipMemcpyAsync(s.u0, u0, vbytes, hipMemcpyHostToDevice, s.stream));
  }
  if (int rc = sync_all(h)) return rc;
  h->u0_staged = true;
  return 0;
}

// stage_u0, then the solve; `seconds` and the solve's total time count both
int solve(Ctx* h, const double* u0, const clipper_params_t* P, double* u_out, clipper_solve_info_t* info) {
  const auto t0 = std::chrono::high_resolution_clock::now();
  if (int rc = stage_u0(h, u0); rc || (rc = solve_staged(h, P, u_out, info))) return rc;
  const double secs = std::chrono::duration<double>(std::chrono::high_resolution_clock::now() - t0).count();
  h->tm.solve_total_ms = secs * 1e3;
  if (info) info->seconds = secs;
  return 0;
}

}  // namespace
