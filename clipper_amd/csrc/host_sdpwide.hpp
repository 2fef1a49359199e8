// host_sdpwide.hpp — the wide route of the semidefinite relaxation (kernels in k_sdp_wide.hip.h, the plan in
// host_sdpwide_plan.hpp, DESIGN.md section 11 "The wide route"): one problem of n <= 1024 at a time over the whole
// chip, as a chain of launches on one stream. The process-wide route setting lives here too.
// Part of clipper_hip.hip (one translation unit; included there, before host_sdp.hpp).
//
// One ADMM iteration is
//   form, [warm start: two products], per sweep { norms, one host wait, np - 1 steps }, norms, project, update,
//   decide, one host wait, [when both residuals pass: form, warm start, the same eigensolve without Q, decide
//   (after dual), one host wait], [scale U].
// The host waits once per sweep (the "sweep again" flag) and once per iteration; it checks the time limit between
// iterations and never abandons one half-way.
#pragma once

#include "host_sdpwide_plan.hpp"

namespace {

static_assert(SDP_MAX_N == CLIPPER_HIP_SDP_MAX_N && SDP_MAX_N == clipper_sdpw_plan::WORKGROUP_MAX_N, "the ABI's limit is the kernel's");
static_assert(SDPW_MAX_N == CLIPPER_HIP_SDP_WIDE_MAX_N, "the ABI's limit is the kernel's");
static_assert(CLIPPER_HIP_SDP_ROUTE_WORKGROUP == clipper_sdpw_plan::ROUTE_WORKGROUP &&
              CLIPPER_HIP_SDP_ROUTE_AUTO == clipper_sdpw_plan::ROUTE_AUTO &&
              CLIPPER_HIP_SDP_ROUTE_WIDE == clipper_sdpw_plan::ROUTE_WIDE, "the ABI's routes are the plan's");

std::atomic<int> g_sdp_route{CLIPPER_HIP_SDP_ROUTE_WORKGROUP};  // process-wide (clipper_hip_sdp_set_route)

// One problem on the device: the regions of its slab (a batch: the problem's own, and the shared work regions)
struct SdpWide {
  SdpArgs a;  // a.Q = Q[0], a.ctl = &st->c
  double* Q[2];
  double* A[2];
  double* part;
  int32_t* pos;
  SdpWideState* st;
};

// a: the problem's own regions (M ... mu, wherever they sit), n, np and the tolerances; work: the plan's regions from
// work_begin on (the driver's, addressed from there)
inline SdpWide sdpw_view(SdpArgs a, uint8_t* work) {
  const clipper_sdpw_plan::Regions r = clipper_sdpw_plan::make_regions(a.n);
  auto w = [&](size_t off) { return work + (off - r.work_begin); };
  SdpWide v{};
  v.Q[0] = a.Q;
  v.Q[1] = reinterpret_cast<double*>(w(r.Q[1]));
  v.A[0] = reinterpret_cast<double*>(w(r.A[0]));
  v.A[1] = reinterpret_cast<double*>(w(r.A[1]));
  v.part = reinterpret_cast<double*>(w(r.part));
  v.pos = reinterpret_cast<int32_t*>(w(r.pos));
  v.st = reinterpret_cast<SdpWideState*>(w(r.state));
  a.ctl = &v.st->c;
  v.a = a;
  return v;
}

// Whether no diagonal entry of C is nonzero (k_sdpw_init alone; M and mask on the device, stream order). A batch asks
// this of its wide problems before anything iterates, so that the first infeasible problem of the call is the one named.
int sdpw_infeasible(hipStream_t st, const SdpWide& w, bool& infeasible) {
  hipLaunchKernelGGL(k_sdpw_init, dim3(1), dim3(SDP_THREADS), 0, st, w.a, w.st);
  HIPCHK(hipGetLastError());
  SdpWideState hs{};
  HIPCHK(hipMemcpyAsync(&hs, w.st, sizeof(SdpWideState), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  infeasible = hs.c.infeasible != 0;
  return 0;
}

// INIT, the iteration and the certificate of one problem whose M and mask are on the device (stream order). Leaves X,
// Z, U, mu and the eigenbasis (in w.a.Q) on the device and the final control record in c. `infeasible`: no diagonal
// entry of C is nonzero (nothing else is done then; the caller words the error).
int sdpw_solve(hipStream_t st, const SdpWide& w, const clipper_sdp_params_t* P,
               std::chrono::steady_clock::time_point t0, SdpCtl& c, int32_t& timed_out, bool& infeasible,
               double& t_setup, double& t_solve) {
  using clk = std::chrono::steady_clock;
  namespace plan = clipper_sdpw_plan;
  auto since = [](clk::time_point a) { return std::chrono::duration<double>(clk::now() - a).count(); };
  const SdpArgs& a = w.a;
  const int32_t n = a.n, np = a.np;
  const plan::StepGeom G = plan::step_geom(np);
  const dim3 one(1), wg1(SDP_THREADS), wgw(SDPW_THREADS);
  const dim3 over_pp(static_cast<unsigned>(ceil_div(static_cast<int64_t>(np) * np, SDPW_THREADS)));
  const dim3 over_nn(static_cast<unsigned>(ceil_div(static_cast<int64_t>(n) * n, SDPW_THREADS)));
  const unsigned gt = static_cast<unsigned>(ceil_div(np, SDPW_GT));
  const int32_t tiles = plan::update_tiles(n);
  SdpWideState hs{};
  auto read_state = [&]() -> int {
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&hs, w.st, sizeof(SdpWideState), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };
  int acur = 0, qcur = 0;  // the copies of A and Q that hold the current matrices
  auto form = [&](int what) {
    acur = 0;
    hipLaunchKernelGGL(k_sdpw_form, over_pp, wgw, 0, st, a, w.A[0], what);
  };
  auto warm_start = [&] {  // A <- Q^T A Q through T
    hipLaunchKernelGGL(k_sdpw_gemm, dim3(gt, gt), wgw, 0, st, static_cast<const double*>(w.A[acur]),
                       static_cast<const double*>(w.Q[qcur]), a.T, np, 0);
    hipLaunchKernelGGL(k_sdpw_gemm, dim3(gt, gt), wgw, 0, st, static_cast<const double*>(w.Q[qcur]),
                       static_cast<const double*>(a.T), w.A[acur ^ 1], np, 1);
    acur ^= 1;
  };
  // cyclic Jacobi on A[acur] until off(A) <= SDP_JACOBI_TOL ||A||_F (sdp_jacobi's rule); adds the sweeps run to sw
  auto eigensolve = [&](bool with_q, int32_t& sw) -> int {
    for (int sweep = 0; sweep < SDP_MAX_SWEEPS; ++sweep) {
      hipLaunchKernelGGL(k_sdpw_norms, one, wg1, 0, st, static_cast<const double*>(w.A[acur]), np, w.st);
      if (int rc = read_state()) return rc;
      if (!hs.again) break;
      for (int32_t t = 0; t < np - 1; ++t) {
        hipLaunchKernelGGL(k_sdpw_step, dim3(static_cast<unsigned>(G.a_tiles + (with_q ? G.q_tiles : 0))), wgw, 0, st,
                           static_cast<const double*>(w.A[acur]), w.A[acur ^ 1],
                           static_cast<const double*>(with_q ? w.Q[qcur] : nullptr), with_q ? w.Q[qcur ^ 1] : nullptr,
                           np, t);
        acur ^= 1;
        if (with_q) qcur ^= 1;
      }
      ++sw;
    }
    return 0;
  };
  auto decide = [&](int phase, int32_t sw) {
    hipLaunchKernelGGL(k_sdpw_decide, one, wg1, 0, st, a, w.st, static_cast<const double*>(w.part), tiles,
                       static_cast<const double*>(w.A[acur]), phase, sw);
  };

  infeasible = false;
  timed_out = 0;
  hipLaunchKernelGGL(k_sdpw_init, one, wg1, 0, st, a, w.st);
  hipLaunchKernelGGL(k_sdpw_init_fill, over_pp, wgw, 0, st, a, static_cast<const SdpWideState*>(w.st));
  if (int rc = read_state()) return rc;
  c = hs.c;
  t_setup = since(t0);
  if (c.infeasible) {
    infeasible = true;
    return 0;
  }
  const auto t1 = clk::now();
  while (!c.converged && c.iters < P->max_iters) {
    if (P->time_limit_secs > 0 && since(t0) >= static_cast<double>(P->time_limit_secs)) {
      timed_out = 1;
      break;
    }
    int32_t sw = 0;
    form(SDPW_FORM_PRIMAL);
    if (c.iters > 0) warm_start();
    if (int rc = eigensolve(true, sw)) return rc;
    hipLaunchKernelGGL(k_sdpw_project, one, wg1, 0, st, a, static_cast<const double*>(w.A[acur]), w.pos, w.st);
    hipLaunchKernelGGL(k_sdpw_update, dim3(static_cast<unsigned>(tiles)), wgw, 0, st, a,
                       static_cast<const double*>(w.Q[qcur]), static_cast<const int32_t*>(w.pos),
                       static_cast<const SdpWideState*>(w.st), w.part);
    decide(SDPW_DECIDE, sw);
    if (int rc = read_state()) return rc;
    if (hs.want_dual) {  // lambda_max(M - rho U+): the same eigensolve, warm-started from Q, without accumulating it
      form(SDPW_FORM_DUAL);
      warm_start();
      if (int rc = eigensolve(false, sw)) return rc;
      decide(SDPW_AFTER_DUAL, sw);
      if (int rc = read_state()) return rc;
    }
    if (hs.rescale != SDP_RESCALE_NONE) hipLaunchKernelGGL(k_sdpw_scale_u, over_nn, wgw, 0, st, a, hs.rescale);
    c = hs.c;
  }
  if (!c.converged) {  // a certified bound in every outcome: lambda_max(M - Y) of the final Y
    int32_t sw = 0;
    form(SDPW_FORM_DUAL);
    if (c.iters > 0) warm_start();
    if (int rc = eigensolve(false, sw)) return rc;
    decide(SDPW_CERTIFY, sw);
    if (int rc = read_state()) return rc;
    c = hs.c;
  }
  if (qcur != 0) HIPCHK(hipMemcpyAsync(w.Q[0], w.Q[1], static_cast<size_t>(np) * np * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  t_solve = since(t1);
  return 0;
}

// `bytes` of device memory for the wide route, checked against what is free
int sdpw_alloc(DevBuf<uint8_t>& slab, size_t bytes, long long n) {
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b)
    return fail(CLIPPER_HIP_E_NOMEM, "sdp: the wide route needs %zu bytes of device memory at n = %lld, %zu are free",
                bytes, n, free_b);
  if (slab.alloc(bytes) != hipSuccess) {
    (void)hipGetLastError();
    return fail(CLIPPER_HIP_E_NOMEM, "sdp: device allocation of %zu bytes failed", bytes);
  }
  return 0;
}

}  // namespace
