// host_sdp.hpp — the semidefinite relaxation (clipper_hip_sdp, clipper_hip_sdp_solve; kernels in k_sdp.hip.h,
// DESIGN.md section 11): the dense fp64 M and the mask of C on the device (gathered from the context's stores or
// uploaded), the launch loop with the time limit between launches, the final certificate and the rounding.
// Part of clipper_hip.hip (one translation unit; included there, in order).
#pragma once

namespace {

constexpr int SDP_ITERS_PER_LAUNCH = 8;  // bounded work per launch (~ms at n = 128)
static_assert(SDP_MAX_N == CLIPPER_HIP_SDP_MAX_N, "the ABI's limit is the kernel's");

// Device buffers of one call.
struct SdpBufs {
  double *M = nullptr, *mask = nullptr, *X = nullptr, *Z = nullptr, *U = nullptr, *Q = nullptr, *T = nullptr,
         *mu = nullptr, *src = nullptr;
  SdpCtl* ctl = nullptr;
  ~SdpBufs() {
    for (void* p : {static_cast<void*>(M), static_cast<void*>(mask), static_cast<void*>(X), static_cast<void*>(Z),
                    static_cast<void*>(U), static_cast<void*>(Q), static_cast<void*>(T), static_cast<void*>(mu),
                    static_cast<void*>(src), static_cast<void*>(ctl)})
      if (p) hipFree(p);
  }
};

int sdp_check_params(const clipper_sdp_params_t* P, int64_t n) {
  if (!P) return fail(CLIPPER_HIP_E_INVALID, "sdp: params are required");
  if (P->max_iters < 1) return fail(CLIPPER_HIP_E_INVALID, "sdp: max_iters must be >= 1");
  if (!(P->eps_abs >= 0.0f) || !(P->eps_rel >= 0.0f)) return fail(CLIPPER_HIP_E_INVALID, "sdp: eps_abs and eps_rel must be >= 0");
  if (n < 1) return fail(CLIPPER_HIP_E_INVALID, "sdp: empty problem");
  if (n > SDP_MAX_N)
    return fail(CLIPPER_HIP_E_SCOPE, "sdp: n = %lld is above the device solver's limit of %d", (long long)n, SDP_MAX_N);
  return 0;
}

int sdp_alloc(SdpBufs& b, int64_t n) {
  const int64_t np = n + (n & 1);
  const size_t nn = static_cast<size_t>(n * n), pp = static_cast<size_t>(np * np);
  for (auto pr : {std::make_pair(&b.M, nn), std::make_pair(&b.mask, nn), std::make_pair(&b.X, nn),
                  std::make_pair(&b.Z, nn), std::make_pair(&b.U, nn), std::make_pair(&b.Q, pp),
                  std::make_pair(&b.T, pp), std::make_pair(&b.mu, static_cast<size_t>(np))})
    if (hipMalloc(reinterpret_cast<void**>(pr.first), pr.second * sizeof(double)) != hipSuccess) {
      *pr.first = nullptr;
      (void)hipGetLastError();
      return fail(CLIPPER_HIP_E_NOMEM, "sdp: device allocation of %zu bytes failed", pr.second * sizeof(double));
    }
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&b.ctl), sizeof(SdpCtl)));
  return 0;
}

// The iteration on b.M / b.mask (already on the device), the certificate and the rounding.
int sdp_run(int device, hipStream_t st, SdpBufs& b, int64_t n, const clipper_sdp_params_t* P,
            std::chrono::steady_clock::time_point t0, std::vector<int32_t>& nodes, double* X_out, double* Y_out,
            double* lambdas_out, double* evec1_out, clipper_sdp_info_t* info) {
  using clk = std::chrono::steady_clock;
  auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
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
  SdpCtl c{};
  if (int rc = launch(SDP_MODE_INIT, 0)) return rc;
  HIPCHK(hipMemcpyAsync(&c, b.ctl, sizeof(SdpCtl), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (c.infeasible) return fail(CLIPPER_HIP_E_INVALID, "sdp: no diagonal entry of C is nonzero (the problem is infeasible)");
  const double t_setup = since(t0);
  const auto t1 = clk::now();
  clipper_sdp_info_t I{};
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
  const double t_solve = since(t1);
  const auto t2 = clk::now();
  // ---- rounding (sdp.cpp:244-261): the eigenpairs of X are those of the last projection
  std::vector<double> mu(static_cast<size_t>(np)), Q(static_cast<size_t>(np) * np);
  HIPCHK(hipMemcpy(mu.data(), b.mu, mu.size() * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(Q.data(), b.Q, Q.size() * sizeof(double), hipMemcpyDeviceToHost));
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
  if (lambdas_out) {
    std::vector<double> l(mu.begin(), mu.begin() + n);
    std::stable_sort(l.begin(), l.end());
    std::memcpy(lambdas_out, l.data(), l.size() * sizeof(double));
  }
  const size_t nn = static_cast<size_t>(n * n);
  if (X_out) HIPCHK(hipMemcpy(X_out, b.X, nn * sizeof(double), hipMemcpyDeviceToHost));
  if (Y_out) {
    HIPCHK(hipMemcpy(Y_out, b.U, nn * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < nn; ++i) Y_out[i] = c.rho * Y_out[i];
  }
  I.iters = c.iters;
  I.converged = c.converged;
  I.num_nodes = static_cast<int32_t>(nodes.size());
  I.sweeps = c.sweeps;
  I.pobj = -c.pval;
  I.dobj = -c.dval;
  I.r_prim = c.r_prim;
  I.r_dual = c.r_dual;
  I.rho = c.rho;
  I.thr = thr;
  I.t_setup = t_setup;
  I.t_solve = t_solve;
  I.t_extract = since(t2);
  I.t_total = since(t0);
  if (P->verbose)
    std::printf("sdp: n = %lld, %d iterations (%d Jacobi sweeps), %s, pobj %.6g, dobj %.6g, %.3f s\n", (long long)n,
                I.iters, I.sweeps, I.converged ? "converged" : (I.timed_out ? "timed out" : "max_iters"), I.pobj,
                I.dobj, I.t_total);
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
  if (int rc = sdp_check_params(P, h->m)) return rc;
  Shard& s = h->sh[0];
  const int64_t n = h->m;
  HIPCHK(hipSetDevice(s.device));
  SdpBufs b;
  if (int rc = sdp_alloc(b, n)) return rc;
  if (int rc = ensure_dense(h, true)) return rc;  // (a copy of the slices for this call only)
  const void* srcC = h->explicitC ? s.Cs : s.S;
  if (!s.S || !srcC) return fail(CLIPPER_HIP_E_STATE, "sdp: the store of M or C is not on the device");
  const dim3 grid(static_cast<unsigned>(ceil_div(n * n, 256))), block(256);
  dispatch_vt(h, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_sdp_gather<T>, grid, block, 0, s.stream, static_cast<const T*>(s.S),
                       static_cast<const T*>(srcC), !h->explicitC, static_cast<int64_t>(h->W), int64_t{1},
                       static_cast<int32_t>(n), 1.0, b.M, b.mask);
  });
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(s.stream));
  if (h->csc_valid) drop_dense(h);
  std::vector<int32_t> nodes;
  if (int rc = sdp_run(s.device, s.stream, b, n, P, t0, nodes, X_out, Y_out, lambdas_out, evec1_out, info))
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
  if (int rc = sdp_check_params(P, n)) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CLIPPER_HIP_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CLIPPER_HIP_E_INVALID, "device %d out of range", device);
  HIPCHK(hipSetDevice(device));
  SdpBufs b;
  if (int rc = sdp_alloc(b, n)) return rc;
  const size_t nn = static_cast<size_t>(n * n);
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&b.src), 2 * nn * sizeof(double)));
  HIPCHK(hipMemcpy(b.src, M, nn * sizeof(double), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b.src + nn, C, nn * sizeof(double), hipMemcpyHostToDevice));
  hipStream_t st = nullptr;  // the null stream: the call is synchronous
  hipLaunchKernelGGL(k_sdp_gather<double>, dim3(static_cast<unsigned>(ceil_div(n * n, 256))), dim3(256), 0, st,
                     b.src, b.src + nn, false, int64_t{1}, n, static_cast<int32_t>(n), 0.0, b.M, b.mask);
  HIPCHK(hipGetLastError());
  std::vector<int32_t> nodes;
  if (int rc = sdp_run(device, st, b, n, P, t0, nodes, X_out, Y_out, lambdas_out, evec1_out, info)) return rc;
  if (nodes_out && !nodes.empty()) std::memcpy(nodes_out, nodes.data(), nodes.size() * sizeof(int32_t));
  return static_cast<int>(nodes.size());
}

}  // namespace
