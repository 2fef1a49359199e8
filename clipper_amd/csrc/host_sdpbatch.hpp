// host_sdpbatch.hpp — many semidefinite relaxations in one call, one workgroup per problem (clipper_hip_sdp_solve_batch,
// clipper_hip_batch_sdp; kernels in k_sdp.hip.h, the plan in host_sdpplan.hpp, DESIGN.md section 11 "Batches").
// Part of clipper_hip.hip (one translation unit; included there, after host_sdp.hpp).
//
// A call
//   1. checks every problem (nothing reaches the device if one is invalid),
//   2. allocates ONE slab for all problems' M, mask, X, Z, U, Q, T, mu, the small results and the launch tables, and
//      ONE array of SdpCtl, both checked against the free memory,
//   3. builds every problem's M and mask in ONE launch of k_sdp_gather_batch,
//   4. runs k_sdp_batch: INIT for all, then rounds of ITERATE (SDP_ITERS_PER_LAUNCH iterations) over the work list of
//      the problems still active (largest n first); after each round ONE copy of the control array to the host, the
//      time limit, and the list's compaction; CERTIFY for the problems that stopped unconverged,
//   5. rounds every problem on the device (k_sdp_round_batch) and reads mu, evec1, the nodes and the rounding records
//      back in ONE copy; X and Y cross only for the problems whose caller asked.
// Per problem every result is bit for bit the lone entry point's (the kernel body and its geometry are the lone
// kernel's; the host decides only WHEN a problem's next launch happens, which the iteration does not see).
// The problems that take the wide route (host_sdpwide.hpp; by the route setting and n) keep their regions of the slab
// but stay out of steps 4 and 5: after the others' certificates they run one after another on the same stream through
// the lone call's driver and tail, sharing one work slab, and their results take their places among the others'.
#pragma once

#include <memory>

#include "host_sdpplan.hpp"

namespace {

struct SdpBatchState {
  int device = 0;
  DevBuf<uint8_t> slab;  // the plan's regions, then the launch tables
  DevBuf<uint8_t> work;  // the wide route's work regions, shared by its problems in turn
  DevBuf<SdpCtl> ctl;    // device, one per problem
  clipper_sdp_plan::Plan plan;
  std::vector<int32_t> n;
  std::vector<SdpCtl> c;              // the last copy of the control array
  std::vector<uint8_t> out;           // host copy of the plan's out region and, behind it, the rounding records
  std::vector<clipper_sdp_info_t> info;
  size_t count() const { return n.size(); }
  const SdpRound& round(size_t i) const { return reinterpret_cast<const SdpRound*>(out.data() + plan.out_bytes)[i]; }
  const double* mu(size_t i) const { return reinterpret_cast<const double*>(out.data() + (plan.at[i].mu - plan.out_begin)); }
  const double* ev(size_t i) const { return reinterpret_cast<const double*>(out.data() + (plan.at[i].ev - plan.out_begin)); }
  const int32_t* nodes(size_t i) const { return reinterpret_cast<const int32_t*>(out.data() + (plan.at[i].nodes - plan.out_begin)); }
  template <typename T>
  T* dev(size_t off) const { return reinterpret_cast<T*>(slab + off); }
};

// The optional outputs of problem i of a finished call: X, Y (n x n, from the device), lambdas (ascending), evec1.
int sdp_batch_outputs(const SdpBatchState& S, size_t i, double* X_out, double* Y_out, double* lambdas_out,
                      double* evec1_out) {
  const size_t n = static_cast<size_t>(S.n[i]), nn = n * n;
  if (evec1_out) std::memcpy(evec1_out, S.ev(i), n * sizeof(double));
  if (lambdas_out) {
    std::vector<double> l(S.mu(i), S.mu(i) + n);
    std::stable_sort(l.begin(), l.end());
    std::memcpy(lambdas_out, l.data(), n * sizeof(double));
  }
  if (X_out || Y_out) HIPCHK(hipSetDevice(S.device));
  if (X_out) HIPCHK(hipMemcpy(X_out, S.dev<double>(S.plan.at[i].X), nn * sizeof(double), hipMemcpyDeviceToHost));
  if (Y_out) {
    HIPCHK(hipMemcpy(Y_out, S.dev<double>(S.plan.at[i].U), nn * sizeof(double), hipMemcpyDeviceToHost));
    const double rho = S.c[i].rho;
    for (size_t e = 0; e < nn; ++e) Y_out[e] = rho * Y_out[e];
  }
  return 0;
}

// Steps 2 to 5 on problems of sizes S.n (checked by the caller). source(i, g): where problem i's M and C are read
// from (g.M, g.mask and g.n are set here); stage(dst): fills the host copy of the plan's src region (called only
// when src_bytes > 0). after_gather(): called once the gather has finished (its sources may go).
template <class Source, class Stage, class AfterGather>
int sdp_batch_run(SdpBatchState& S, hipStream_t st, const clipper_sdp_params_t* P, int route, bool with_src, Source&& source,
                  Stage&& stage, AfterGather&& after_gather, std::chrono::steady_clock::time_point t0) {
  using clk = std::chrono::steady_clock;
  namespace plan = clipper_sdp_plan;
  auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
  const size_t count = S.count();
  S.info.assign(count, clipper_sdp_info_t{});
  if (count == 0) return 0;
  S.plan = plan::make_plan(S.n, with_src);
  const plan::Plan& L = S.plan;
  const clipper_sdpw_plan::Split routes = clipper_sdpw_plan::split(S.n, route);
  std::vector<char> is_wide(count, 0);
  size_t work_bytes = 0;
  for (int32_t i : routes.wide) {
    is_wide[static_cast<size_t>(i)] = 1;
    const clipper_sdpw_plan::Regions r = clipper_sdpw_plan::make_regions(S.n[static_cast<size_t>(i)]);
    work_bytes = std::max(work_bytes, r.bytes - r.work_begin);
  }
  // the work list of the workgroup route, in the plan's order
  const std::vector<int32_t> order = plan::compact(L.order, [&](int32_t i) { return is_wide[static_cast<size_t>(i)] != 0; });

  // ---- 2. one slab (the launch tables behind the plan's regions), one control array ---------------------------------
  const size_t off_round = L.bytes, off_args = off_round + count * sizeof(SdpRound),
               off_gsrc = off_args + count * sizeof(SdpArgs), off_rdst = off_gsrc + count * sizeof(SdpGatherSrc),
               off_list = off_rdst + count * sizeof(SdpRoundDst),
               slab_bytes = static_cast<size_t>(round_up(static_cast<int64_t>(off_list + count * sizeof(int32_t)), 256));
  static_assert(sizeof(SdpRound) % 8 == 0 && sizeof(SdpArgs) % 8 == 0 && sizeof(SdpGatherSrc) % 8 == 0, "8-byte tables");
  const size_t ctl_bytes = count * sizeof(SdpCtl);
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (slab_bytes + ctl_bytes + work_bytes > free_b)
    return fail(CLIPPER_HIP_E_NOMEM, "sdp batch: %zu problems need %zu bytes of device memory, %zu are free", count,
                slab_bytes + ctl_bytes + work_bytes, free_b);
  auto room = [](auto& buf, size_t bytes) {
    if (bytes == 0 || buf.alloc_bytes(bytes) == hipSuccess) return 0;
    (void)hipGetLastError();
    return fail(CLIPPER_HIP_E_NOMEM, "sdp batch: device allocation of %zu bytes failed", bytes);
  };
  if (int rc = room(S.slab, slab_bytes)) return rc;
  if (int rc = room(S.ctl, ctl_bytes)) return rc;
  if (int rc = room(S.work, work_bytes)) return rc;

  // ---- 3. the tables, the uploaded matrices, the gather --------------------------------------------------------------
  std::vector<uint8_t> tab(off_list - off_args);
  SdpArgs* args = reinterpret_cast<SdpArgs*>(tab.data());
  SdpGatherSrc* gsrc = reinterpret_cast<SdpGatherSrc*>(tab.data() + (off_gsrc - off_args));
  SdpRoundDst* rdst = reinterpret_cast<SdpRoundDst*>(tab.data() + (off_rdst - off_args));
  int32_t nmax = 0;
  for (size_t i = 0; i < count; ++i) {
    const plan::Regions& r = L.at[i];
    const int32_t n = S.n[i];
    nmax = std::max(nmax, n);
    args[i] = SdpArgs{S.dev<double>(r.M), S.dev<double>(r.mask), S.dev<double>(r.X), S.dev<double>(r.Z),
                      S.dev<double>(r.U), S.dev<double>(r.Q), S.dev<double>(r.T), S.dev<double>(r.mu), S.ctl + i,
                      n, plan::padded(n), static_cast<double>(P->eps_abs), static_cast<double>(P->eps_rel)};
    rdst[i] = SdpRoundDst{is_wide[i] ? nullptr : S.dev<double>(r.ev), S.dev<int32_t>(r.nodes)};
    SdpGatherSrc g{};
    g.M = S.dev<double>(r.M);
    g.mask = S.dev<double>(r.mask);
    g.n = n;
    if (int rc = source(i, g)) return rc;
    gsrc[i] = g;
  }
  std::vector<uint8_t> hsrc;
  if (L.src_bytes) {
    hsrc.resize(L.src_bytes);
    stage(hsrc.data());
    HIPCHK(hipMemcpyAsync(S.slab + L.src_begin, hsrc.data(), L.src_bytes, hipMemcpyHostToDevice, st));
  }
  HIPCHK(hipMemcpyAsync(S.slab + off_args, tab.data(), tab.size(), hipMemcpyHostToDevice, st));
  const SdpArgs* dargs = S.dev<SdpArgs>(off_args);
  const SdpGatherSrc* dgsrc = S.dev<SdpGatherSrc>(off_gsrc);
  int32_t* dlist = S.dev<int32_t>(off_list);
  const unsigned gx = static_cast<unsigned>(ceil_div(static_cast<int64_t>(nmax) * nmax, 256));
  for (size_t i0 = 0; i0 < count; i0 += 65535) {  // (the grid's y extent)
    const unsigned gy = static_cast<unsigned>(std::min<size_t>(65535, count - i0));
    hipLaunchKernelGGL(k_sdp_gather_batch, dim3(gx, gy), dim3(256), 0, st, dgsrc + i0);
    HIPCHK(hipGetLastError());
  }

  // ---- 4. INIT, the rounds of ITERATE over the active list, CERTIFY -----------------------------------------------
  if (plan::launch_lds_bytes(order, S.n) > 64 * 1024 &&
      !raise_dynamic_lds(reinterpret_cast<const void*>(k_sdp_batch), S.device, SDP_MAX_N * SDP_MAX_N * 8))
    return fail(CLIPPER_HIP_E_HIP, "sdp: cannot raise the kernel's LDS to %d bytes", SDP_MAX_N * SDP_MAX_N * 8);
  std::vector<int32_t> on_device;  // the list the device holds
  S.c.assign(count, SdpCtl{});
  // (every launch copies the whole control array back: zeros, not stale bytes, for the wide route's problems, whose
  // records are the driver's and reach S.c with their solve)
  HIPCHK(hipMemsetAsync(S.ctl, 0, ctl_bytes, st));
  // one launch over `list` and the copy of the control array that follows it
  auto launch = [&](const std::vector<int32_t>& list, int mode, int budget) -> int {
    if (list.empty()) return 0;
    if (list != on_device) {
      HIPCHK(hipMemcpyAsync(dlist, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
      HIPCHK(hipStreamSynchronize(st));  // (the copy reads `list` now, not later)
      on_device = list;
    }
    hipLaunchKernelGGL(k_sdp_batch, dim3(static_cast<unsigned>(list.size())), dim3(SDP_THREADS),
                       plan::launch_lds_bytes(list, S.n), st, dargs, static_cast<const int32_t*>(dlist), mode, budget,
                       P->max_iters);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(S.c.data(), S.ctl, ctl_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };
  if (int rc = launch(order, SDP_MODE_INIT, 0)) return rc;
  if (order.empty()) HIPCHK(hipStreamSynchronize(st));  // (the gather has read its sources)
  after_gather();
  for (int32_t i : routes.wide) {  // (their INIT proper runs with their solve: the work slab is shared)
    bool bad = false;
    if (int rc = sdpw_infeasible(st, sdpw_view(args[static_cast<size_t>(i)], S.work), bad)) return rc;
    S.c[static_cast<size_t>(i)] = SdpCtl{};
    S.c[static_cast<size_t>(i)].infeasible = bad;
  }
  for (size_t i = 0; i < count; ++i)
    if (S.c[i].infeasible)
      return fail(CLIPPER_HIP_E_INVALID, "problem %zu: %s", i, SDP_INFEASIBLE);
  const double t_setup = since(t0);
  const auto t1 = clk::now();
  auto finished = [&](int32_t i) { return S.c[static_cast<size_t>(i)].converged || S.c[static_cast<size_t>(i)].iters >= P->max_iters; };
  std::vector<int32_t> active = plan::compact(order, finished);
  int rounds = 0;
  while (!active.empty()) {
    if (P->time_limit_secs > 0 && since(t0) >= static_cast<double>(P->time_limit_secs)) {
      for (int32_t i : active) S.info[static_cast<size_t>(i)].timed_out = 1;
      break;
    }
    if (int rc = launch(active, SDP_MODE_ITERATE, SDP_ITERS_PER_LAUNCH)) return rc;
    active = plan::compact(active, finished);
    ++rounds;
  }
  // a certified bound in every outcome: lambda_max(M - Y) of the final Y
  if (int rc = launch(plan::compact(order, [&](int32_t i) { return S.c[static_cast<size_t>(i)].converged != 0; }),
                      SDP_MODE_CERTIFY, 0))
    return rc;
  // the wide route's problems, in the caller's order; what their tails return waits for the out region's copy
  struct WideOut {
    std::vector<double> mu, ev;
    std::vector<int32_t> nodes;
    int32_t top = 0;
  };
  std::vector<WideOut> wide_out(routes.wide.size());
  for (size_t k = 0; k < routes.wide.size(); ++k) {
    const size_t i = static_cast<size_t>(routes.wide[k]);
    const int64_t n = S.n[i];
    const SdpWide w = sdpw_view(args[i], S.work);
    bool infeasible = false;
    double ts = 0.0, tv = 0.0;
    if (int rc = sdpw_solve(st, w, P, t0, S.c[i], S.info[i].timed_out, infeasible, ts, tv)) return rc;
    if (infeasible)
      return fail(CLIPPER_HIP_E_INVALID, "problem %zu: %s", i, SDP_INFEASIBLE);
    WideOut& o = wide_out[k];
    o.mu.resize(static_cast<size_t>(plan::padded(S.n[i])));
    o.ev.resize(static_cast<size_t>(n));
    clipper_sdp_params_t quiet = *P;
    quiet.verbose = 0;
    if (int rc = sdp_tail(w.a.mu, w.a.Q, w.a.X, w.a.U, n, S.c[i], &quiet, CLIPPER_HIP_SDP_ROUTE_WIDE, t0, ts, tv, clk::now(),
                          o.nodes, nullptr, nullptr, nullptr, o.ev.data(), o.mu.data(), &o.top, S.info[i]))
      return rc;
  }
  const double t_solve = since(t1);
  const auto t2 = clk::now();

  // ---- 5. the rounding on the device, one copy back -----------------------------------------------------------------
  hipLaunchKernelGGL(k_sdp_round_batch, dim3(static_cast<unsigned>(count)), dim3(64), 0, st, dargs,
                     static_cast<const SdpRoundDst*>(S.dev<SdpRoundDst>(off_rdst)), S.dev<SdpRound>(off_round));
  HIPCHK(hipGetLastError());
  S.out.resize(L.out_bytes + count * sizeof(SdpRound));  // (contiguous on the device: out region, rounding records)
  HIPCHK(hipMemcpyAsync(S.out.data(), S.slab + L.out_begin, S.out.size(), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (size_t k = 0; k < routes.wide.size(); ++k) {  // the wide route's results into the host copy
    const size_t i = static_cast<size_t>(routes.wide[k]);
    const WideOut& o = wide_out[k];
    uint8_t* out = S.out.data();
    std::memcpy(out + (L.at[i].mu - L.out_begin), o.mu.data(), o.mu.size() * sizeof(double));
    std::memcpy(out + (L.at[i].ev - L.out_begin), o.ev.data(), o.ev.size() * sizeof(double));
    if (!o.nodes.empty()) std::memcpy(out + (L.at[i].nodes - L.out_begin), o.nodes.data(), o.nodes.size() * sizeof(int32_t));
    reinterpret_cast<SdpRound*>(S.out.data() + L.out_bytes)[i] = SdpRound{S.info[i].thr, static_cast<int32_t>(o.nodes.size()), o.top};
  }
  for (size_t i = 0; i < count; ++i) {
    if (is_wide[i]) continue;  // (filled by its tail)
    clipper_sdp_info_t& I = S.info[i];
    sdp_info_from_ctl(I, S.c[i]);
    I.num_nodes = S.round(i).count;
    I.thr = S.round(i).thr;
  }
  const double t_extract = since(t2), t_total = since(t0);
  for (clipper_sdp_info_t& I : S.info) {
    I.t_setup = t_setup;
    I.t_solve = t_solve;
    I.t_extract = t_extract;  // (without the copies of X and Y the caller asks for afterwards)
    I.t_total = t_total;
  }
  if (P->verbose) {
    std::printf("sdp batch: %zu problems, %d rounds of %d iterations, %.3f s\n", count, rounds, SDP_ITERS_PER_LAUNCH, t_total);
    for (size_t i = 0; i < count; ++i) {
      sdp_print_result(("  problem " + std::to_string(i)).c_str(), S.n[i], S.info[i]);
      std::printf("\n");
    }
  }
  return 0;
}

// clipper_hip_sdp_solve_batch: host matrices (column-major), lower triangles
int sdp_solve_batch_impl(int device, const clipper_sdp_problem_t* p, int32_t count, const clipper_sdp_params_t* P,
                         clipper_sdp_info_t* infos) {
  const auto t0 = std::chrono::steady_clock::now();
  if (count < 0) return fail(CLIPPER_HIP_E_INVALID, "sdp batch: count = %d", count);
  if (count == 0) return 0;
  if (!p) return fail(CLIPPER_HIP_E_INVALID, "sdp batch: the problem list is required");
  const int route = g_sdp_route.load();
  if (int rc = sdp_check_params(P, 1, route)) return rc;
  for (int32_t i = 0; i < count; ++i) {
    if (!p[i].M || !p[i].C) return fail(CLIPPER_HIP_E_INVALID, "problem %d: sdp: M and C are required", i);
    if (p[i].n < 1) return fail(CLIPPER_HIP_E_INVALID, "problem %d: sdp: empty problem (n = %lld)", i, (long long)p[i].n);
    if (p[i].n > clipper_sdpw_plan::route_limit(route))
      return fail(CLIPPER_HIP_E_SCOPE, "problem %d: sdp: n = %lld is above the device solver's limit of %d", i,
                  (long long)p[i].n, clipper_sdpw_plan::route_limit(route));
    if (int rc = sdp_check_finite(p[i].M, p[i].n, "M", i)) return rc;
    if (int rc = sdp_check_finite(p[i].C, p[i].n, "C", i)) return rc;
  }
  if (int rc = use_device(device)) return rc;
  SdpBatchState S;
  S.device = device;
  S.n.resize(static_cast<size_t>(count));
  for (int32_t i = 0; i < count; ++i) S.n[static_cast<size_t>(i)] = static_cast<int32_t>(p[i].n);
  hipStream_t st = nullptr;  // the null stream: the call is synchronous
  auto source = [&](size_t i, SdpGatherSrc& g) -> int {
    g.srcM = S.dev<double>(S.plan.at[i].srcM);
    g.srcC = S.dev<double>(S.plan.at[i].srcC);
    g.rs = 1;
    g.cs = S.n[i];
    g.ident = 0.0;
    g.f64 = 1;
    g.c_pattern_of_m = 0;
    return 0;
  };
  auto stage = [&](uint8_t* dst) {
    for (size_t i = 0; i < S.count(); ++i) {
      const size_t nn = static_cast<size_t>(S.n[i]) * S.n[i] * sizeof(double);
      std::memcpy(dst + (S.plan.at[i].srcM - S.plan.src_begin), p[i].M, nn);
      std::memcpy(dst + (S.plan.at[i].srcC - S.plan.src_begin), p[i].C, nn);
    }
  };
  if (int rc = sdp_batch_run(S, st, P, route, true, source, stage, [] {}, t0)) return rc;
  const auto t2 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < S.count(); ++i) {
    const clipper_sdp_problem_t& q = p[i];
    if (int rc = sdp_batch_outputs(S, i, q.X_out, q.Y_out, q.lambdas_out, q.evec1_out)) return rc;
    const int32_t k = S.round(i).count;
    if (q.nodes_out && k > 0) std::memcpy(q.nodes_out, S.nodes(i), static_cast<size_t>(k) * sizeof(int32_t));
  }
  const double extra = std::chrono::duration<double>(std::chrono::steady_clock::now() - t2).count();
  if (infos)
    for (size_t i = 0; i < S.count(); ++i) {
      infos[i] = S.info[i];
      infos[i].t_extract += extra;  // (the copies of X and Y)
      infos[i].t_total += extra;
    }
  return 0;
}

}  // namespace
