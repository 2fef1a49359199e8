// host_subproblem.hpp — the LIVE SUB-PROBLEM (k_subproblem.hip.h): when it is prepared, the hand-over of a running
// solve to it and the way back.
// Part of clipper_hip.hip (one translation unit; included there, in order).
//
// The sub-problem is a child CONTEXT on the parent's device and stream: the same fill (k_affinity_sym on the gathered
// points of the associations of S), the same planner, the same launches (k_gemv_slices, k_tail) — only their
// arguments differ (solve_args: sub_state = 2, the parent's progress record and pinned u, the list of S for the final
// u). The solver's state machine does not know: it continues from a prepared pass (SolverState::resume) on other arrays.
#pragma once

namespace {

// The size threshold: SUB_MIN_M, or CLIPPER_HIP_SUBPROBLEM_MIN_M of the environment as the process starts, until
// clipper_hip_debug_sub_min_m (test infrastructure) sets another one, process-wide; a value <= 0 brings the initial one back.
std::atomic<long long> g_sub_min_m{0};
int64_t sub_min_m() {
  static const int64_t initial = std::getenv("CLIPPER_HIP_SUBPROBLEM_MIN_M") ? std::atoll(std::getenv("CLIPPER_HIP_SUBPROBLEM_MIN_M")) : SUB_MIN_M;
  const long long set = g_sub_min_m.load(std::memory_order_relaxed);
  return set > 0 ? static_cast<int64_t>(set) : initial;
}
int debug_sub_min_m(long long min_m) {
  g_sub_min_m.store(min_m > 0 ? min_m : 0, std::memory_order_relaxed);
  return 0;
}

bool sub_enabled(const Ctx* h) {
  static const bool env_off = [] {
    const char* e = std::getenv("CLIPPER_HIP_SUBPROBLEM");
    return e && std::atoi(e) == 0;
  }();
  return !env_off && h->sub_mode != 1 && h->parent == nullptr && h->sh.size() == 1 && h->world == 1 && !h->multiproc &&
         h->csc_valid && !h->explicitC && h->m >= sub_min_m() && rect_fill_possible(h);
}

void sub_begin_solve(Ctx* h) {
  SubProblem& sp = h->sub;
  sp.ready = sp.active = false;
  sp.entries = 0;
  sp.sub_passes = sp.leaves = 0;
  sp.build_ms = 0.0;
  sp.last = SubLast{};
}

void sub_free(Ctx* h) {
  SubProblem& sp = h->sub;
  for (Ctx** pc : {&sp.ctx, &sp.ctx_dense}) {
    if (*pc) {
      (*pc)->sh[0].stream = nullptr;  // (the parent's: not the child's to destroy)
      destroy_ctx(*pc);
      *pc = nullptr;
    }
  }
  sp.use = nullptr;
  static_cast<SubBufs&>(sp) = SubBufs{};
  sp.ready = sp.active = false;
  sp.last = SubLast{};
}

// the child's point tables and association pairs, gathered on the device from the parent's (stage_inputs without
// host data); everything else of the child as after stage_inputs
int sub_stage(Ctx* h, Ctx* c, int64_t nS) {
  Shard& s = h->sh[0];
  Shard& cs = c->sh[0];
  c->V_forced = h->V;      // the state's point slots and partial scalars are laid out by the window size
  c->resident_mode = 1;    // (a solve that is handed over mid-way never starts on the resident solver)
  c->rv_mode = 1;          // no views inside it: its rows are the live rows
  c->nodes.clear();
  c->fill.kind = 0;
  rowview_drop(c);
  int rc = ensure_problem(c, nS);
  if (rc) return rc;
  const int d = h->staged_d;
  const int64_t qs = round_up(nS, 64);
  const size_t np = static_cast<size_t>(d) * qs;
  HIPCHK(cs.P1.grow(np));
  HIPCHK(cs.P2.grow(np));
  HIPCHK(cs.P1f.grow(np));
  HIPCHK(cs.P2f.grow(np));
  HIPCHK(cs.Adev.grow(static_cast<size_t>(2 * nS)));
  dim3 grid(static_cast<unsigned>(ceil_div(qs, 256))), block(256);
  hipLaunchKernelGGL(k_sub_gather_points, grid, block, 0, s.stream, s.P1, s.P1f, d, h->staged_pstride, s.Adev, h->m,
                     h->sub.colmap, nS, qs, cs.P1, cs.P1f, cs.Adev, 0);
  hipLaunchKernelGGL(k_sub_gather_points, grid, block, 0, s.stream, s.P2, s.P2f, d, h->staged_pstride, s.Adev, h->m,
                     h->sub.colmap, nS, qs, cs.P2, cs.P2f, cs.Adev, 1);
  c->staged_d = d;
  c->staged_pstride = qs;
  c->staged_maxabs = h->staged_maxabs;  // (the prefilter's guard: the same threshold, the same scores)
  c->plain_affinity = h->plain_affinity;
  c->strip_affinity = h->strip_affinity;
  return 0;
}

// THE SELECTION (k_subproblem.hip.h), stated once for a running solve (sub_prepare) and for the stand-alone call
// (sub_select_rows): on the view RV, whose rows `in_view` flags, with sum(u) read from `sum_u` on the device —
// cnt[0, mp), S as flags[0, mp), its ascending list colmap[0, nS) and the inverse pos[0, mp), the record. Synchronous:
// a few launches and one wait.
int sub_select(Ctx* h, Shard& s, const SliceView& RV, const uint8_t* in_view, const double* sum_u) {
  SubProblem& sp = h->sub;
  const int64_t m = h->m, mp = h->mp;
  const int nblk = static_cast<int>(ceil_div(m, RV_BLK));
  if (static_cast<size_t>(mp) > sp.pos.cap) {  // the five lists go together, then come together (`pos` is made last: its capacity is theirs)
    sp.cnt.reset(), sp.flags.reset(), sp.colmap.reset(), sp.view_kept.reset(), sp.pos.reset();
    HIPCHK(sp.cnt.alloc(static_cast<size_t>(mp)));
    HIPCHK(sp.flags.alloc(static_cast<size_t>(mp)));
    HIPCHK(sp.colmap.alloc(static_cast<size_t>(mp)));
    HIPCHK(sp.view_kept.alloc(static_cast<size_t>(mp)));
    HIPCHK(sp.pos.alloc(static_cast<size_t>(mp)));
  }
  HIPCHK(sp.blk.grow(static_cast<size_t>(nblk) + 2));
  if (!sp.nout_acc) HIPCHK(sp.nout_acc.alloc(8));
  static_assert(sizeof(SubRecord) <= 64, "the record fits its 64 pinned bytes");
  if (!sp.rec) HIPCHK(sp.rec.alloc_bytes(64, hipHostMallocMapped | hipHostMallocCoherent));
  sp.rec->nS = -1;
  sp.rec->ncol = -1;
  sp.rec->n0 = -1;
  sp.last = SubLast{};
  std::atomic_thread_fence(std::memory_order_seq_cst);
  static_assert(SL_H == 1, "k_sub_colcount reads the quads of sub-block 0 alone: with more sub-blocks per chunk it has to sum all of them");
  hipLaunchKernelGGL(k_sub_begin, dim3(1), dim3(64), 0, s.stream, sp.nout_acc);
  hipLaunchKernelGGL(k_sub_colcount, dim3(static_cast<unsigned>(ceil_div(RV.ncg, 4))), dim3(256), 0, s.stream, RV, sp.cnt, mp);
  hipLaunchKernelGGL(k_sub_flags, dim3(static_cast<unsigned>(nblk)), dim3(256), 0, s.stream, sum_u, sp.cnt, in_view, m, mp,
                     sp.flags, sp.blk, sp.nout_acc, sp.view_kept);
  hipLaunchKernelGGL(k_rv_scan, dim3(1), dim3(1024), 0, s.stream, sp.blk, nblk, &sp.rec.dev->nS);
  hipLaunchKernelGGL(k_rv_scatter, dim3(static_cast<unsigned>(nblk)), dim3(256), 0, s.stream, sp.flags, m, sp.blk, sp.colmap,
                     static_cast<int64_t>(sp.pos.cap), sp.pos, mp);
  hipLaunchKernelGGL(k_sub_publish, dim3(1), dim3(64), 0, s.stream, sp.nout_acc, sp.rec.dev);
  HIPCHK(hipStreamSynchronize(s.stream));
  HIPCHK(hipGetLastError());
  std::atomic_thread_fence(std::memory_order_acquire);
  return 0;
}

// Called when a row view has just been built (the stream is idle but for the lift of the hold): select S, and if it
// is small enough build its problem. Synchronous — the selection's wait, the fill's own wait.
int sub_prepare(Ctx* h) {
  SubProblem& sp = h->sub;
  sp.ready = false;
  Shard& s = h->sh[0];
  RowView& v = s.rv;
  if (!sub_enabled(h) || !v.valid || h->vres.ready || sp.entries >= SUB_MAX_ENTRIES) return 0;
  const auto t0 = std::chrono::high_resolution_clock::now();
  HIPCHK(hipSetDevice(s.device));
  const int64_t m = h->m;
  int rc;
  if ((rc = sub_select(h, s, row_view(h, s), v.in_view[v.cur], &(s.st + h->par)->s))) return rc;
  sp.last.valid = true;  // (the read-back of test infrastructure: clipper_hip_debug_sub_last)
  sp.last.nrows = v.nrows;
  const int64_t nS = sp.rec->nS;
  static const bool host_timing = std::getenv("CLIPPER_HIP_HOST_TIMING") != nullptr;
  if (host_timing)
    std::fprintf(stderr, "[sub] view of %lld rows: S = %lld associations, N0 = %d, the largest count outside %d\n",
                 static_cast<long long>(v.nrows), static_cast<long long>(nS), sp.rec->n0, sp.rec->ncol);
  // worth a problem of its own: not much more than the view's rows, and far fewer than the full problem's columns
  if (nS < 64 || sp.rec->ncol < 0 || nS > 2 * v.nrows + 1024 || 3 * nS > m) return 0;
  // the child context(s): on the parent's device and stream (their fills, plans and launches are ordered with the
  // parent's by construction), filled with the invariant the parent's matrix was scored with
  auto build_child = [&](Ctx*& c, int storage) -> int {
    if (!c) {
      c = make_ctx(&s.device, 1, storage, 1, 0, false);
      if (!c) return CLIPPER_HIP_E_HIP;
      hipStreamDestroy(c->sh[0].stream);
      c->sh[0].stream = s.stream;
      c->parent = h;
    }
    if (int r2 = sub_stage(h, c, nS)) return r2;
    return fill_builtin(c, h->fill, nullptr);
  };
  const int storage = h->compressed ? (h->storage == CLIPPER_HIP_STORE_F64 ? CLIPPER_HIP_STORE_F64_CSC : CLIPPER_HIP_STORE_F32_CSC)
                                    : h->storage;
  // Mostly non-zero (the inliers of a registration problem are consistent with each other: M[S,S] IS the dense block the
  // slices' work list cuts by step range)? Then a dense fp32 store holds it in 4 bytes per element instead of 5.3 per
  // stored entry and its pass is k_gemv (wave-uniform multipliers, no gathers; the window from candidate tables:
  // k_sub_enter writes the pending one): 37 -> 30 us per pass at m = 100k, 236 -> 182 us at 300k (0.71 of the HBM peak).
  // How dense it will be is known before it is built: the selection summed the counts of the columns it took.
  static const bool dense_off = std::getenv("CLIPPER_HIP_SUB_DENSE") && std::atoi(std::getenv("CLIPPER_HIP_SUB_DENSE")) == 0;
  const double in_entries = static_cast<double>((static_cast<unsigned long long>(sp.rec->entries_hi) << 32) | sp.rec->entries_lo);
  const double density = in_entries / (static_cast<double>(nS) * static_cast<double>(std::max<int64_t>(1, v.nrows)));
  const bool dense = !dense_off && h->sub_mode != 2 && h->storage == CLIPPER_HIP_STORE_F32 && density >= 0.5 && nS >= 1024;
  Ctx* c = nullptr;
  if (dense) {
    rc = build_child(sp.ctx_dense, CLIPPER_HIP_STORE_F32);
    if (rc == 0 && sp.ctx_dense->has_matrix && !sp.ctx_dense->csc_valid) c = sp.ctx_dense;
    else if (rc != 0 && rc != CLIPPER_HIP_E_NOMEM) return rc;
    else (void)hipGetLastError();
  }
  if (c == nullptr) {
    if ((rc = build_child(sp.ctx, storage))) return rc;
    if (!sp.ctx->csc_valid) return 0;  // (a fill route without slices: not taken)
    c = sp.ctx;
  }
  sp.use = c;
  HIPCHK(hipSetDevice(s.device));
  sp.nS = nS;
  // N of the bound: the counts are over the VIEW's rows; on the sub-problem a row of S outside the view may come back
  // to life (it is inside S: fine) and then adds at most one entry to any column — |S \ R| on top, once and for all
  sp.ncol = static_cast<double>(std::max(1, sp.rec->ncol)) + static_cast<double>(std::max<int64_t>(0, nS - v.nrows));
  sp.ready = true;
  sp.last.built = true;
  sp.last.N_used = sp.ncol;
  sp.build_ms += std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
  if (host_timing)
    std::fprintf(stderr, "[sub] ready: %lld associations, density %.2f -> %s (%.1f MB), prepared in %.2f ms\n",
                 static_cast<long long>(nS), density, c->csc_valid ? "slices" : "a dense fp32 store",
                 (c->csc_valid ? static_cast<double>(c->sh[0].s_bytes) : algorithmic_gemv_bytes(c)) * 1e-6, sp.build_ms);
  return 0;
}

// HOLD_SUB_ENTER: the decision on the full problem found that no column outside S can come back to life. The hold is lifted,
// a decide-only iteration turns the held decision into a prepared pass, the point and the state move over.
int sub_enter(Ctx* h, const SolverParams& prm) {
  SubProblem& sp = h->sub;
  if (!sp.ready || sp.active || !sp.use) return fail(CLIPPER_HIP_E_INTERNAL, "sub-problem: a hand-over nobody prepared");
  Shard& s = h->sh[0];
  Ctx* c = sp.use;
  Shard& cs = c->sh[0];
  HIPCHK(hipSetDevice(s.device));
  hipLaunchKernelGGL(k_sub_resume, dim3(1), dim3(64), 0, s.stream, s.st + h->par, s.shared);
  if (int rc = enqueue_iteration(h, prm, true)) return rc;  // (decide-only: it does not ask for the hand-over again)
  // the final u is written through the list of S: the rest is zero
  std::memset(h->u_pinned, 0, static_cast<size_t>(h->m) * sizeof(double));
  std::atomic_thread_fence(std::memory_order_seq_cst);
  hipLaunchKernelGGL(k_sub_enter, dim3(static_cast<unsigned>(ceil_div(c->mp, 256))), dim3(256), 0, s.stream, s.st + h->par, s.pt,
                     s.cab, h->mp, h->V, sp.colmap, sp.nS, cs.st, cs.shared, cs.pt, cs.cab, c->mp,
                     c->csc_valid ? static_cast<double*>(nullptr) : cs.X[0], prm.beta);
  c->par = 0;
  c->rv_fresh = false;
  sp.active = true;
  sp.last.entered = true;
  sp.entries += 1;
  sp.launches_since_entry = 0;
  sp.passes_at_entry = h->mirror->n_passes;
  h->rv_stats.sub_entries += 1;
  return 0;
}

// HOLD_SUB_LEAVE: the decision on the sub-problem left its pass prepared — a column outside S could come back to life under
// one of the pending candidates. The point and the state go back; the full problem's launches run that pass.
int sub_leave(Ctx* h) {
  SubProblem& sp = h->sub;
  if (!sp.active || !sp.use) return fail(CLIPPER_HIP_E_INTERNAL, "sub-problem: nothing to leave");
  Shard& s = h->sh[0];
  Ctx* c = sp.use;
  Shard& cs = c->sh[0];
  HIPCHK(hipSetDevice(s.device));
  hipLaunchKernelGGL(k_sub_leave, dim3(static_cast<unsigned>(ceil_div(h->mp, 256))), dim3(256), 0, s.stream, cs.st + c->par, cs.pt,
                     cs.cab, c->mp, h->V, sp.pos, s.rv.in_view[s.rv.cur], h->m, s.pt, s.cab, h->mp, sp.nout_acc);
  hipLaunchKernelGGL(k_sub_leave_state, dim3(1), dim3(256), 0, s.stream, cs.st + c->par, s.st + h->par, s.shared, sp.nout_acc);
  sp.active = false;
  sp.leaves += 1;
  if (sp.entries >= SUB_MAX_ENTRIES) sp.ready = false;
  return 0;
}

// ---- test infrastructure: the selection by itself, and the read-back of a solve's last one ------------------------

// the lists and the record of the selection the buffers hold, to the host (arrays of `capacity` >= mp elements;
// `rows`: the view's rows, from the flags k_sub_flags kept)
int sub_copy_out(Ctx* h, int64_t capacity, int32_t* cnt, uint8_t* flags, int32_t* colmap, int32_t* pos, int32_t* rows,
                 clipper_hip_sub_selection_t* out) {
  SubProblem& sp = h->sub;
  Shard& s = h->sh[0];
  const int64_t m = h->m, mp = h->mp;
  if (capacity < mp) return fail(CLIPPER_HIP_E_INVALID, "capacity %lld < %lld (the padded length)", static_cast<long long>(capacity), static_cast<long long>(mp));
  const int64_t nS = sp.rec->nS;
  if (nS < 0 || nS > m || sp.rec->n0 < 0 || sp.rec->ncol < 0) return fail(CLIPPER_HIP_E_HIP, "sub-problem: the selection's record did not arrive");
  HIPCHK(hipSetDevice(s.device));
  HIPCHK(hipStreamSynchronize(s.stream));
  int32_t acc[8];
  HIPCHK(hipMemcpy(acc, sp.nout_acc, sizeof(acc), hipMemcpyDeviceToHost));
  if (cnt) HIPCHK(hipMemcpy(cnt, sp.cnt, static_cast<size_t>(mp) * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (flags) HIPCHK(hipMemcpy(flags, sp.flags, static_cast<size_t>(mp), hipMemcpyDeviceToHost));
  if (colmap && nS > 0) HIPCHK(hipMemcpy(colmap, sp.colmap, static_cast<size_t>(nS) * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (pos) HIPCHK(hipMemcpy(pos, sp.pos, static_cast<size_t>(mp) * sizeof(int32_t), hipMemcpyDeviceToHost));
  int64_t nrows = 0;
  std::vector<uint8_t> kept(static_cast<size_t>(mp));
  HIPCHK(hipMemcpy(kept.data(), sp.view_kept, kept.size(), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < mp; ++i)
    if (kept[static_cast<size_t>(i)]) {
      if (rows) rows[nrows] = static_cast<int32_t>(i);
      ++nrows;
    }
  *out = clipper_hip_sub_selection_t{};
  out->mp = mp;
  out->nS = nS;
  out->entries = static_cast<int64_t>((static_cast<unsigned long long>(sp.rec->entries_hi) << 32) | sp.rec->entries_lo);
  out->nrows = nrows;
  out->ncol = sp.rec->ncol;
  out->n0 = sp.rec->n0;
  std::memcpy(&out->s, acc + 6, sizeof(double));
  return 0;
}

// The selection alone, on the row view of the given rows (built as view_matvec builds it) with the caller's sum(u):
// exactly the launches a solve makes between a view's build and the decision to build the sub-problem.
int sub_select_rows(Ctx* h, const int32_t* rows, int64_t nrows, double sum_u, int64_t capacity, int32_t* cnt, uint8_t* flags,
                    int32_t* colmap, int32_t* pos, clipper_hip_sub_selection_t* out) {
  if (!h->has_matrix || !h->csc_valid || !csc_single(h) || h->explicitC || h->parent != nullptr || !rect_fill_possible(h))
    return fail(CLIPPER_HIP_E_STATE, "the selection needs slices of a matrix scored from staged points on one device");
  const int64_t m = h->m, mp = h->mp;
  if (!(sum_u >= 0.0) || !std::isfinite(sum_u)) return fail(CLIPPER_HIP_E_INVALID, "sum(u) must be finite and not negative");
  if (capacity < mp) return fail(CLIPPER_HIP_E_INVALID, "capacity %lld < %lld (the padded length)", static_cast<long long>(capacity), static_cast<long long>(mp));
  for (int64_t r = 0; r < nrows; ++r)
    if (rows[r] < 0 || rows[r] >= m || (r > 0 && rows[r] <= rows[r - 1]))
      return fail(CLIPPER_HIP_E_INVALID, "rows must be ascending association indices");
  Shard& s = h->sh[0];
  RowView& v = s.rv;
  HIPCHK(hipSetDevice(s.device));
  HIPCHK(hipStreamSynchronize(s.stream));
  v.valid = false;  // (its store is overwritten: the view of a later solve is built anew)
  h->sub.ready = false;
  int rc;
  HIPCHK(v.rowmap[0].grow(static_cast<size_t>(mp)));
  HIPCHK(v.rowmap[1].grow(static_cast<size_t>(mp)));
  HIPCHK(v.in_view[0].grow(static_cast<size_t>(mp)));
  HIPCHK(v.in_view[1].grow(static_cast<size_t>(mp)));
  std::vector<uint8_t> in_view(static_cast<size_t>(mp), 0);
  for (int64_t r = 0; r < nrows; ++r) in_view[static_cast<size_t>(rows[r])] = 1;
  HIPCHK(hipMemcpyAsync(v.rowmap[0], rows, static_cast<size_t>(nrows) * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(v.in_view[0], in_view.data(), in_view.size(), hipMemcpyHostToDevice, s.stream));
  HIPCHK(hipMemcpyAsync(s.u0, &sum_u, sizeof(double), hipMemcpyHostToDevice, s.stream));  // (sum(u) rides in the u0 buffer)
  h->u0_staged = false;
  if ((rc = emit_rect(h, s, v.st, v.rowmap[0], nrows, -1, -1, true, 3, "row view"))) return rc;
  if ((rc = sub_select(h, s, store_view(v.st, v.rowmap[0], nrows), v.in_view[0], s.u0))) return rc;
  return sub_copy_out(h, capacity, cnt, flags, colmap, pos, nullptr, out);
}

// The last selection of the last solve: its lists and record, the view's rows at that moment, and what became of it.
int sub_last_selection(Ctx* h, int64_t capacity, int32_t* cnt, uint8_t* flags, int32_t* colmap, int32_t* pos, int32_t* rows,
                       clipper_hip_sub_selection_t* out) {
  const SubLast last = h->sub.last;
  if (!last.valid) return fail(CLIPPER_HIP_E_STATE, "the last solve made no selection (or a stand-alone one has overwritten it)");
  if (int rc = sub_copy_out(h, capacity, cnt, flags, colmap, pos, rows, out)) return rc;
  if (out->nrows != last.nrows) return fail(CLIPPER_HIP_E_INTERNAL, "sub-problem: the kept row flags are not the view's");
  out->built = last.built ? 1 : 0;
  out->entered = last.entered ? 1 : 0;
  out->N_used = last.N_used;
  return 0;
}

}  // namespace
