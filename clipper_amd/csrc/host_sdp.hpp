// host_sdp.hpp — the semidefinite relaxation (clipper_hip_sdp, clipper_hip_sdp_solve; kernels in k_sdp.hip.h,
// DESIGN.md section 11): the dense fp64 M and the mask of C on the device (gathered from the context's stores or
// uploaded), the launch loop with the time limit between launches, the final certificate and the rounding. A problem
// takes the workgroup route (k_sdp, the loop below) or the wide route (host_sdpwide.hpp) by the process's route
// setting; the rounding and the copies out (sdp_tail) are the same for both.
// Part of clipper_hip.hip (one translation unit; included there, in order).
#pragma once

namespace {

constexpr int SDP_ITERS_PER_LAUNCH = 8;  // bounded work per launch (~ms at n = 128)

// Device buffers of one call. Workgroup route: every pointer is an allocation of its own (`own`). Wide route: `slab` is the
// only allocation; M ... mu, ctl and src (when the call uploads host matrices) point into it (host_sdpwide_plan.hpp's
// regions, src behind them) and `wide` is the driver's view of it.
struct SdpBufs {
  double *M = nullptr, *mask = nullptr, *X = nullptr, *Z = nullptr, *U = nullptr, *Q = nullptr, *T = nullptr,
         *mu = nullptr, *src = nullptr;
  SdpCtl* ctl = nullptr;
  DevBuf<uint8_t> slab;
  DevBuf<void> own[10];  // M ... mu, ctl, src
  SdpWide wide{};
};

// `route`: the setting the call read (g_sdp_route); it decides the scope limit
int sdp_check_params(const clipper_sdp_params_t* P, int64_t n, int route) {
  if (!P) return fail(CLIPPER_HIP_E_INVALID, "sdp: params are required");
  if (P->max_iters < 1) return fail(CLIPPER_HIP_E_INVALID, "sdp: max_iters must be >= 1");
  if (!(P->eps_abs >= 0.0f) || !(P->eps_rel >= 0.0f)) return fail(CLIPPER_HIP_E_INVALID, "sdp: eps_abs and eps_rel must be >= 0");
  if (n < 1) return fail(CLIPPER_HIP_E_INVALID, "sdp: empty problem");
  if (n > clipper_sdpw_plan::route_limit(route))
    return fail(CLIPPER_HIP_E_SCOPE, "sdp: n = %lld is above the device solver's limit of %d", (long long)n,
                clipper_sdpw_plan::route_limit(route));
  return 0;
}

// The values of a host matrix (column-major, n x n), refused before the device is touched: only the lower triangle is
// read, so only it is checked. `what`: "M" or "C"; problem >= 0: a batch names the problem in front.
int sdp_check_finite(const double* A, int64_t n, const char* what, long long problem) {
  for (int64_t c = 0; c < n; ++c)
    for (int64_t r = c; r < n; ++r)
      if (!std::isfinite(A[r + c * n])) {
        if (problem >= 0)
          return fail(CLIPPER_HIP_E_INVALID, "problem %lld: sdp: %s: non-finite value at row %lld, column %lld", problem,
                      what, (long long)r, (long long)c);
        return fail(CLIPPER_HIP_E_INVALID, "sdp: %s: non-finite value at row %lld, column %lld", what, (long long)r,
                    (long long)c);
      }
  return 0;
}

// `taken`: the route of this problem (clipper_sdpw_plan::route_of); with_src: room for the uploaded M and C
// (2 n^2 doubles) too
int sdp_alloc(SdpBufs& b, int64_t n, const clipper_sdp_params_t* P, int taken, bool with_src) {
  const size_t src_bytes = with_src ? 2 * static_cast<size_t>(n * n) * sizeof(double) : 0;
  if (taken == CLIPPER_HIP_SDP_ROUTE_WIDE) {
    const clipper_sdpw_plan::Regions r = clipper_sdpw_plan::make_regions(static_cast<int32_t>(n));
    if (int rc = sdpw_alloc(b.slab, r.bytes + src_bytes, (long long)n)) return rc;
    if (with_src) b.src = reinterpret_cast<double*>(b.slab + r.bytes);
    auto at = [&](size_t off) { return reinterpret_cast<double*>(b.slab + off); };
    b.wide = sdpw_view(SdpArgs{at(r.M), at(r.mask), at(r.X), at(r.Z), at(r.U), at(r.Q[0]), at(r.T), at(r.mu), nullptr,
                               static_cast<int32_t>(n), clipper_sdpw_plan::padded(static_cast<int32_t>(n)),
                               static_cast<double>(P->eps_abs), static_cast<double>(P->eps_rel)},
                       b.slab + r.work_begin);
    const SdpArgs& a = b.wide.a;
    b.M = const_cast<double*>(a.M);
    b.mask = const_cast<double*>(a.mask);
    b.X = a.X;
    b.Z = a.Z;
    b.U = a.U;
    b.Q = a.Q;
    b.T = a.T;
    b.mu = a.mu;
    b.ctl = a.ctl;
    return 0;
  }
  const int64_t np = n + (n & 1);
  const size_t nn = static_cast<size_t>(n * n), pp = static_cast<size_t>(np * np);
  int k = 0;
  for (auto pr : {std::make_pair(&b.M, nn), std::make_pair(&b.mask, nn), std::make_pair(&b.X, nn),
                  std::make_pair(&b.Z, nn), std::make_pair(&b.U, nn), std::make_pair(&b.Q, pp),
                  std::make_pair(&b.T, pp), std::make_pair(&b.mu, static_cast<size_t>(np))})
  {
    if (b.own[k].alloc(pr.second * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CLIPPER_HIP_E_NOMEM, "sdp: device allocation of %zu bytes failed", pr.second * sizeof(double));
    }
    *pr.first = b.own[k++].as<double>();
  }
  HIPCHK(b.own[8].alloc(sizeof(SdpCtl)));
  b.ctl = b.own[8].as<SdpCtl>();
  if (with_src) {
    HIPCHK(b.own[9].alloc(src_bytes));
    b.src = b.own[9].as<double>();
  }
  return 0;
}

// What every refusal of an infeasible problem says (a batch puts "problem i: " in front)
constexpr const char* SDP_INFEASIBLE = "sdp: no diagonal entry of C is nonzero (the problem is infeasible)";

// What SdpCtl says, into the info (num_nodes, route, thr and the times are the caller's)
void sdp_info_from_ctl(clipper_sdp_info_t& I, const SdpCtl& c) {
  I.iters = c.iters;
  I.converged = c.converged;
  I.sweeps = c.sweeps;
  I.pobj = -c.pval;
  I.dobj = -c.dval;
  I.r_prim = c.r_prim;
  I.r_dual = c.r_dual;
  I.rho = c.rho;
}

// The verbose line of one result: `head`, the route, the counts, the outcome and the objectives; no line end
void sdp_print_result(const char* head, long long n, const clipper_sdp_info_t& I) {
  std::printf("%s%s: n = %lld, %d iterations (%d Jacobi sweeps), %s, pobj %.6g, dobj %.6g", head,
              I.route == CLIPPER_HIP_SDP_ROUTE_WIDE ? " (wide route)" : "", n, I.iters, I.sweeps,
              I.converged ? "converged" : (I.timed_out ? "timed out" : "max_iters"), I.pobj, I.dobj);
}

// The tail of every solve, whichever route it took: the rounding (sdp.cpp:244-261; the eigenpairs of X are those of the
// last projection, mu and Q on the device), the copies out and the info. I.timed_out is the caller's; t2: when the
// iteration ended. mu_out (np doubles, may be NULL): the weights as the device holds them; top_out (may be NULL): the
// first index of the largest weight.
int sdp_tail(const double* d_mu, const double* d_Q, const double* d_X, const double* d_U, int64_t n, const SdpCtl& c,
             const clipper_sdp_params_t* P, int taken, std::chrono::steady_clock::time_point t0, double t_setup,
             double t_solve, std::chrono::steady_clock::time_point t2, std::vector<int32_t>& nodes, double* X_out,
             double* Y_out, double* lambdas_out, double* evec1_out, double* mu_out, int32_t* top_out,
             clipper_sdp_info_t& I) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
  const int32_t np = static_cast<int32_t>(n + (n & 1));
  std::vector<double> mu(static_cast<size_t>(np)), Q(static_cast<size_t>(np) * np);
  HIPCHK(hipMemcpy(mu.data(), d_mu, mu.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(Q.data(), d_Q, Q.size() * sizeof(double), hipMemcpyDeviceToHost));
  int64_t top = 0;
  for (int64_t i = 1; i < n; ++i)
    if (mu[static_cast<size_t>(i)] > mu[static_cast<size_t>(top)]) top = i;
  std::vector<double> ev(static_cast<size_t>(n));
  int64_t big = 0;
  for (int64_t i = 0; i < n; ++i) {
    ev[static_cast<size_t>(i)] = Q[static_cast<size_t>(i * np + top)];
    if (std::fabs(ev[static_cast<size_t>(i)]) > std::fabs(ev[static_cast<size_t>(big)])) big = i;
  }
  if (ev[static_cast<size_t>(big)] < 0)
    for (auto& v : ev) v = -v;
  const double thr = std::fabs(ev[static_cast<size_t>(big)]) / 2.0;
  nodes.clear();
  for (int64_t i = 0; i < n; ++i)
    if (std::fabs(ev[static_cast<size_t>(i)]) > thr) nodes.push_back(static_cast<int32_t>(i));
  if (evec1_out) std::memcpy(evec1_out, ev.data(), ev.size() * sizeof(double));
  if (mu_out) std::memcpy(mu_out, mu.data(), mu.size() * sizeof(double));
  if (top_out) *top_out = static_cast<int32_t>(top);
  if (lambdas_out) {
    std::vector<double> l(mu.begin(), mu.begin() + n);
    std::stable_sort(l.begin(), l.end());
    std::memcpy(lambdas_out, l.data(), l.size() * sizeof(double));
  }
  const size_t nn = static_cast<size_t>(n * n);
  if (X_out) HIPCHK(hipMemcpy(X_out, d_X, nn * sizeof(double), hipMemcpyDeviceToHost));
  if (Y_out) {
    HIPCHK(hipMemcpy(Y_out, d_U, nn * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nn; ++i) Y_out[i] = c.rho * Y_out[i];
  }
  sdp_info_from_ctl(I, c);
  I.num_nodes = static_cast<int32_t>(nodes.size());
  I.route = taken;
  I.thr = thr;
  I.t_setup = t_setup;
  I.t_solve = t_solve;
  I.t_extract = since(t2);
  I.t_total = since(t0);
  if (P->verbose) {
    sdp_print_result("sdp", (long long)n, I);
    std::printf(", %.3f s\n", I.t_total);
  }
  return 0;
}

// The iteration on b.M / b.mask (already on the device, stream order), the certificate and the rounding.
int sdp_run(int device, hipStream_t st, SdpBufs& b, int64_t n, const clipper_sdp_params_t* P, int taken,
            std::chrono::steady_clock::time_point t0, std::vector<int32_t>& nodes, double* X_out, double* Y_out,
            double* lambdas_out, double* evec1_out, clipper_sdp_info_t* info) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
  SdpCtl c{};
  clipper_sdp_info_t I{};
  double t_setup = 0.0, t_solve = 0.0;
  if (taken == CLIPPER_HIP_SDP_ROUTE_WIDE) {
    bool infeasible = false;
    if (int rc = sdpw_solve(st, b.wide, P, t0, c, I.timed_out, infeasible, t_setup, t_solve)) return rc;
    if (infeasible) return fail(CLIPPER_HIP_E_INVALID, "%s", SDP_INFEASIBLE);
  } else {
    const int32_t np = static_cast<int32_t>(n + (n & 1));
    const int lds = np * np * static_cast<int>(sizeof(double));
    if (lds > 64 * 1024 && !raise_dynamic_lds(reinterpret_cast<const void*>(k_sdp), device, SDP_MAX_N * SDP_MAX_N * 8))
      return fail(CLIPPER_HIP_E_HIP, "sdp: cannot raise the kernel's LDS to %d bytes", SDP_MAX_N * SDP_MAX_N * 8);
    const SdpArgs a{b.M, b.mask, b.X, b.Z, b.U, b.Q, b.T, b.mu, b.ctl, static_cast<int32_t>(n), np,
                    static_cast<double>(P->eps_abs), static_cast<double>(P->eps_rel)};
    auto launch = [&](int mode, int budget) -> int {
      hipLaunchKernelGGL(k_sdp, dim3(1), dim3(SDP_THREADS), lds, st, a, mode, budget, P->max_iters);
      HIPCHK(hipGetLastError());
      return 0;
    };
    if (int rc = launch(SDP_MODE_INIT, 0)) return rc;
    HIPCHK(hipMemcpyAsync(&c, b.ctl, sizeof(SdpCtl), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (c.infeasible) return fail(CLIPPER_HIP_E_INVALID, "%s", SDP_INFEASIBLE);
    t_setup = since(t0);
    const auto t1 = clk::now();
    while (!c.converged && c.iters < P->max_iters) {
      if (P->time_limit_secs > 0 && since(t0) >= static_cast<double>(P->time_limit_secs)) {
        I.timed_out = 1;
        break;
      }
      if (int rc = launch(SDP_MODE_ITERATE, SDP_ITERS_PER_LAUNCH)) return rc;
      HIPCHK(hipMemcpyAsync(&c, b.ctl, sizeof(SdpCtl), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    if (!c.converged) {  // a certified bound in every outcome: lambda_max(M - Y) of the final Y
      if (int rc = launch(SDP_MODE_CERTIFY, 0)) return rc;
      HIPCHK(hipMemcpyAsync(&c, b.ctl, sizeof(SdpCtl), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
    }
    t_solve = since(t1);
  }
  if (int rc = sdp_tail(b.mu, b.Q, b.X, b.U, n, c, P, taken, t0, t_setup, t_solve, clk::now(), nodes, X_out, Y_out,
                        lambdas_out, evec1_out, nullptr, nullptr, I))
    return rc;
  if (info) *info = I;
  return 0;
}

// clipper_hip_sdp: the context's M and C (+ identity), gathered on the device from the store that holds each
int sdp_ctx_impl(Ctx* h, const clipper_sdp_params_t* P, double* X_out, double* Y_out, double* lambdas_out,
                 double* evec1_out, clipper_sdp_info_t* info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (h->multiproc || h->world != 1 || h->sh.size() != 1)
    return fail(CLIPPER_HIP_E_SCOPE, "sdp: one-shard contexts only (this one holds column shards)");
  const int route = g_sdp_route.load();
  if (int rc = sdp_check_params(P, h->m, route)) return rc;
  Shard& s = h->sh[0];
  const int64_t n = h->m;
  const int taken = clipper_sdpw_plan::route_of(route, n);
  HIPCHK(hipSetDevice(s.device));
  SdpBufs b;
  if (int rc = sdp_alloc(b, n, P, taken, false)) return rc;
  if (int rc = ensure_dense(h, true)) return rc;  // (a copy of the slices for this call only)
  const void* srcC = h->explicitC ? s.Cs : s.S;
  if (!s.S || !srcC) return fail(CLIPPER_HIP_E_STATE, "sdp: the store of M or C is not on the device");
  const dim3 grid(static_cast<unsigned>(ceil_div(n * n, 256))), block(256);
  dispatch_vt(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_sdp_gather<T>, grid, block, 0, s.stream, s.S.as<const T>(),
                       static_cast<const T*>(srcC), !h->explicitC, static_cast<int64_t>(h->W), int64_t{1},
                       static_cast<int32_t>(n), 1.0, b.M, b.mask);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s.stream));
  if (h->csc_valid) drop_dense(h);
  std::vector<int32_t> nodes;
  if (int rc = sdp_run(s.device, s.stream, b, n, P, taken, t0, nodes, X_out, Y_out, lambdas_out, evec1_out, info))
    return rc;
  h->nodes = nodes;
  return 0;
}

// clipper_hip_sdp_solve: host M and C (column-major), lower triangles
int sdp_solve_impl(int device, const double* M, const double* C, int64_t n, const clipper_sdp_params_t* P,
                   double* X_out, double* Y_out, double* lambdas_out, double* evec1_out, int32_t* nodes_out,
                   clipper_sdp_info_t* info) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!M || !C) return fail(CLIPPER_HIP_E_INVALID, "sdp: M and C are required");
  const int route = g_sdp_route.load();
  if (int rc = sdp_check_params(P, n, route)) return rc;
  const int taken = clipper_sdpw_plan::route_of(route, n);
  if (int rc = sdp_check_finite(M, n, "M", -1)) return rc;
  if (int rc = sdp_check_finite(C, n, "C", -1)) return rc;
  if (int rc = use_device(device)) return rc;
  SdpBufs b;
  if (int rc = sdp_alloc(b, n, P, taken, true)) return rc;
  const size_t nn = static_cast<size_t>(n * n);
  HIPCHK(hipMemcpy(b.src, M, nn * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b.src + nn, C, nn * sizeof(double), hipMemcpyHostToDevice));
  hipStream_t st = nullptr;  // the null stream: the call is synchronous
  hipLaunchKernelGGL(k_sdp_gather<double>, dim3(static_cast<unsigned>(ceil_div(n * n, 256))), dim3(256), 0, st,
                     b.src, b.src + nn, false, int64_t{1}, n, static_cast<int32_t>(n), 0.0, b.M, b.mask);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> nodes;
  if (int rc = sdp_run(device, st, b, n, P, taken, t0, nodes, X_out, Y_out, lambdas_out, evec1_out, info)) return rc;
  if (nodes_out && !nodes.empty()) std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(int32_t));
  return static_cast<int>(nodes.size());
}

}  // namespace
