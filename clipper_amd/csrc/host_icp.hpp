// host_icp.hpp — the driver of clipper_hip_icp, clipper_hip_icp_generalized, their robust forms and
// clipper_hip_evaluate_registration ("ICP over a kept search grid", "Generalized ICP" and "Robust
// losses and trimmed ICP"), and of clipper_hip_estimate_covariances, the stage that makes the generalized metric's
// covariances. Both clouds go to the device once; the target's search index belongs to a KnnTarget (host_knn_grid.hpp:
// the frame's local, or a cloud's own), is made by knn_target_ensure at most once and queried every iteration with
// k_knn_grid<1>; the body reads the process-wide mode once; the source is binned by the target's grid once, at
// T_init, and keeps that order for all iterations (a locality hint, never a correctness input: the lists go to the
// rows of the original indices). T, the sums, the history and the candidate count stay on the device during the loop;
// the host reads the 64-byte status record once per iteration through pinned memory to decide whether to queue the
// next round: the only host wait of an iteration. The brute-force route queries one kept scratch (host_knn.hpp).
// Each layer is stated once: icp_call is the four host-buffer entry points (who, family, robust use), icp_run the
// host-buffer frame, icp_body the loop on device pointers (also under host_cloud.hpp's calls), IcpRound what a round
// reads, icp_queue_round the one dispatch to icp_round<METHOD, ROBUST>, the two launches.
// Stand-alone: needs no context. The checks are host_icp_check.hpp's (check_call), the arithmetic icp_rules.hpp's. Part
// of clipper_hip.hip (one translation unit; included there last, after host_features.hpp).
#pragma once

#include "host_icp_check.hpp"

namespace {

// what the loop needs besides device memory: a pinned record and two events, released on every path
struct IcpHostState {
  PinnedBuf<IcpRecord> rec;
  Event a, b;
};

// what a round reads, filled once before the loop: the K = 1 lists, the moved source q, the clouds and what the method
// reads of them (IcpInputs' Nt, Cs, Ct), d2 = max_distance^2, the origin of the sums, the robust settings and the
// selection's control block (read by the robust rounds alone), the partials (nb x the layout's terms), the stop rule,
// and where the step leaves the sums, T, the record and the history. All pointers: device memory.
struct IcpRound {
  const int32_t* oi;
  const double *od, *q;
  int32_t ns;
  const double *Pt, *Nt, *Cs, *Ct;
  int32_t nt;
  double d2, o[3];
  IcpRobustArgs rb;
  double* part;
  int32_t nb;
  IcpStop stop;
  double *sums, *T;
  IcpRecord* rec;
  double* hist;
  hipStream_t st;
};

// round k: the sums and the step
template <int METHOD, bool ROBUST>
void icp_round(const IcpRound& r, int k) {
  hipLaunchKernelGGL((k_icp_accumulate<METHOD, ROBUST>), dim3(static_cast<unsigned>(r.nb)), dim3(256), 0, r.st, r.oi, r.od, r.q,
                     r.ns, r.Pt, r.Nt, r.Cs, r.Ct, r.T, r.nt, r.d2, r.o[0], r.o[1], r.o[2], r.rb, r.part);
  hipLaunchKernelGGL((k_icp_step<METHOD, ROBUST>), dim3(1), dim3(256), 0, r.st, r.part, r.nb, r.stop, k, r.o[0], r.o[1], r.o[2],
                     r.sums, r.T, r.rec, r.hist);
}

// the instantiation of the method; with rb the weighted sums against the control block and the robust layout's step
void icp_queue_round(int method, const clipper_icp::Robust* rb, const IcpRound& r, int k) {
  switch (method) {
    case ICP_GENERALIZED: return rb ? icp_round<ICP_GENERALIZED, true>(r, k) : icp_round<ICP_GENERALIZED, false>(r, k);
    case ICP_POINT_TO_PLANE: return rb ? icp_round<ICP_POINT_TO_PLANE, true>(r, k) : icp_round<ICP_POINT_TO_PLANE, false>(r, k);
    default: return rb ? icp_round<ICP_POINT_TO_POINT, true>(r, k) : icp_round<ICP_POINT_TO_POINT, false>(r, k);
  }
}

// The trimming threshold of the round under the current lists: two launches per digit, nothing read by the host.
void icp_select(const int32_t* oi, const double* od, int32_t ns, double d2, double trim, IcpSelect* dctl, uint32_t* dtot,
                hipStream_t st) {
  const dim3 tiles(static_cast<unsigned>(ceil_div(ns, SELECT_TILE)));
  for (int pass = 0; pass < ICP_SELECT_PASSES; ++pass) {
    hipLaunchKernelGGL(k_select_hist<>, tiles, dim3(SELECT_THREADS), 0, st, oi, od, ns, d2, pass, dctl, dtot);
    hipLaunchKernelGGL(k_select_pick<>, dim3(1), dim3(SELECT_THREADS), 0, st, dtot, pass, trim, dctl);
  }
}

// where the inputs of a call lie on the device: the source Ps (ns x 3), the target Pt (nt x 3), Nt: the target's normals
// (point-to-plane alone), Cs, Ct: the covariances of the source and the target, 6 x n (generalized alone). target: the
// owner of what the search against Pt keeps, its index (grid route) or its bounding box (brute-force route): a cloud's
// (host_cloud.hpp), kept between calls, or a local of the host-buffer frame.
struct IcpInputs {
  const double *Ps = nullptr, *Pt = nullptr, *Nt = nullptr, *Cs = nullptr, *Ct = nullptr;
  KnnTarget* target = nullptr;
};

// THE BODY of every ICP entry point and of evaluate_registration, on device pointers. Every argument has been checked
// and the device is current. T0: column-major 4 x 4 (host). history: (max_iterations + 1) x 3 or null; corr_out: ns or
// null. rb: the robust settings (clipper_hip_icp_robust and clipper_hip_icp_generalized_robust; null: the plain rounds,
// whose launches and buffers are untouched by it), rinfo: what they report besides info. With rb the selection runs
// between the search and the sums when trim < 1, then the weighted round; the control block stays on the device.
// The host-buffer calls (icp_run) and the calls on clouds (host_cloud.hpp) both run this.
int icp_body(int device, const IcpInputs& in, int64_t ns_, int64_t nt_, const double* T0, const clipper_icp::Params& prm,
             double* T_out, clipper_icp_info_t* info, double* history, int32_t* corr_out, const clipper_icp::Robust* rb,
             clipper_icp_robust_info_t* rinfo, DevTemps& tmp) {
  const int32_t ns = static_cast<int32_t>(ns_), nt = static_cast<int32_t>(nt_);
  const bool plane = prm.method == ICP_POINT_TO_PLANE, gen = prm.method == ICP_GENERALIZED;
  const int terms = icp_layout_terms(prm.method, rb != nullptr);
  const bool trimmed = rb && rb->trim < 1.0;
  const int32_t nb = static_cast<int32_t>(ceil_div(ns, ICP_BLOCK));
  const size_t s3 = static_cast<size_t>(ns) * 3;
  const size_t nrows = static_cast<size_t>(prm.max_iterations) + 1;
  const int route = knn_route(g_knn_search.load(), 3, ns, nt);
  const double *dPs = in.Ps, *dPt = in.Pt, *dNt = in.Nt, *dCs = in.Cs, *dCt = in.Ct;

  double *dq = nullptr, *od = nullptr, *dpart = nullptr, *dsums = nullptr, *dT = nullptr, *dhist = nullptr;
  int32_t *oi = nullptr, *perm = nullptr, *visited = nullptr;
  unsigned long long* dsum = nullptr;
  IcpRecord* drec = nullptr;
  IcpSelect* dctl = nullptr;
  uint32_t* dtot = nullptr;
  IcpHostState hs;
  const size_t s1 = static_cast<size_t>(ns);
  if (int rc = tmp.alloc(device, dq, s3 * sizeof(double), od, s1 * sizeof(double), oi, s1 * sizeof(int32_t),
                         dpart, static_cast<size_t>(nb) * terms * sizeof(double), dsums, ICP_PLANE_TERMS * sizeof(double),
                         dT, 16 * sizeof(double), dhist, nrows * 3 * sizeof(double), drec, sizeof(IcpRecord)))
    return rc;
  KnnBruteScratch bs;  // (the brute-force route's partial lists: in their place among the call's buffers)
  if (route == CLIPPER_HIP_KNN_BRUTE)
    if (int rc = knn_brute_alloc(device, 1, ns, nt, bs, tmp)) return rc;
  if (int rc = tmp.alloc(device, perm, s1 * sizeof(int32_t), visited, s1 * sizeof(int32_t), dsum, sizeof(unsigned long long)))
    return rc;
  if (rb)  // (behind every buffer of the plain call)
    if (int rc = tmp.alloc(device, dctl, sizeof(IcpSelect), dtot, ICP_SELECT_RADIX * sizeof(uint32_t))) return rc;
  HIPCHK(hs.rec.alloc(1));
  HIPCHK(hs.a.create());
  HIPCHK(hs.b.create());

  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  IcpRecord first{};
  first.status = ICP_RUNNING;
  *hs.rec = first;
  HIPCHK(hipMemcpyAsync(dT, T0, 16 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(drec, hs.rec, sizeof(IcpRecord), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(dhist, 0, nrows * 3 * sizeof(double), st));
  HIPCHK(hipMemsetAsync(dsum, 0, sizeof(unsigned long long), st));

  // the target's index (grid route) or its bounding box alone, taken as the target holds it or made now: the origin of
  // the sums is the centre of the index's own box on the grid route, of the target's box on the brute-force route
  KnnTarget& target = *in.target;
  if (int rc = knn_target_ensure(target, route, device, dPt, nt, st, tmp)) return rc;
  const KnnGridIndex& ix = target.ix;  // (read on the grid route alone)
  double o[3];
  if (route == CLIPPER_HIP_KNN_GRID) icp_origin(ix.lo, ix.hi, o);
  else icp_origin(target.lo, target.hi, o);

  const double d2 = prm.max_distance * prm.max_distance;
  IcpSelect sel{};  // without trimming, for the whole call: every point within max_distance is kept
  sel.tau = d2;
  sel.any = 1;
  if (rb) {
    HIPCHK(hipMemcpyAsync(dctl, &sel, sizeof(IcpSelect), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(dtot, 0, ICP_SELECT_RADIX * sizeof(uint32_t), st));
  }
  const IcpStop stop{prm.max_iterations, static_cast<int64_t>(ns), prm.rel_fitness, prm.rel_rmse};
  const dim3 sb(static_cast<unsigned>(ceil_div(ns, 256)));
  // CLIPPER_HIP_ICP_REBIN=1 (measurement only: tools/icp_probe.py) bins the moved source anew every iteration
  const char* rebin_env = std::getenv("CLIPPER_HIP_ICP_REBIN");
  const bool rebin = rebin_env && rebin_env[0] == '1';
  KnnGridQueries gq;
  if (route == CLIPPER_HIP_KNN_GRID)
    if (int rc = knn_grid_alloc_queries(device, ix, ns, gq, tmp)) return rc;
  KgPoint* const Q = gq.Q;  // (null on the brute-force route)
  const IcpRobustArgs ra = rb ? IcpRobustArgs{rb->loss, rb->scale, rb->scale * rb->scale, dctl} : IcpRobustArgs{};
  IcpRound rnd{};  // (filled by name: every member is a pointer or a number another one could stand in for)
  rnd.oi = oi, rnd.od = od, rnd.q = dq, rnd.ns = ns;
  rnd.Pt = dPt, rnd.Nt = dNt, rnd.Cs = dCs, rnd.Ct = dCt, rnd.nt = nt;
  rnd.d2 = d2, rnd.o[0] = o[0], rnd.o[1] = o[1], rnd.o[2] = o[2], rnd.rb = ra;
  rnd.part = dpart, rnd.nb = nb, rnd.stop = stop;
  rnd.sums = dsums, rnd.T = dT, rnd.rec = drec, rnd.hist = dhist, rnd.st = st;
  HIPCHK(hipEventRecord(hs.a, st));
  int k = 0;
  for (;; ++k) {
    // the source under the current T: to q, and on the grid route to its place in the query order
    const bool ordered = k > 0 && Q && !rebin;
    hipLaunchKernelGGL(k_icp_transform<>, sb, dim3(256), 0, st, dT, dPs, ns, ordered ? perm : nullptr, dq, ordered ? Q : nullptr);
    if (route == CLIPPER_HIP_KNN_GRID) {
      if (!ordered) {  // the query order: the source at T_init in the cells of the target's grid, kept from here on
        knn_grid_bin_queries(ix, dq, ns, gq, st);
        if (!rebin) hipLaunchKernelGGL(k_icp_order<>, sb, dim3(256), 0, st, Q, ns, perm);
      }
      if (int rc = knn_grid_query_lists(ix, 1, Q, ns, od, oi, visited, st)) return rc;
      knn_grid_sum_visited(visited, ns, dsum, st);
    } else if (int rc = knn_brute_query(1, 3, dq, ns, dPt, nt, bs, od, oi, st)) {
      return rc;
    }
    if (trimmed) icp_select(oi, od, ns, d2, rb->trim, dctl, dtot, st);
    icp_queue_round(prm.method, rb, rnd, k);
    HIPCHK(hipMemcpyAsync(hs.rec, drec, sizeof(IcpRecord), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the one wait of an iteration
    if (hs.rec->status != ICP_RUNNING || k >= prm.max_iterations) break;
  }
  HIPCHK(hipEventRecord(hs.b, st));
  HIPCHK(hipGetLastError());
  if (hs.rec->status == ICP_RUNNING || hs.rec->iterations != k)
    return fail(CLIPPER_HIP_E_INTERNAL, "icp: the status record of iteration %d was not written", k);

  unsigned long long cand = 0;
  HIPCHK(hipMemcpyAsync(&cand, dsum, sizeof(cand), hipMemcpyDeviceToHost, st));
  if (T_out) HIPCHK(hipMemcpyAsync(T_out, dT, 16 * sizeof(double), hipMemcpyDeviceToHost, st));
  double wsum = 0.0;  // (of the last row: position ICP_POINT_WEIGHT_SUM of the sums the last step folded)
  if (rb) {
    HIPCHK(hipMemcpyAsync(&sel, dctl, sizeof(IcpSelect), hipMemcpyDeviceToHost, st));
    if (!plane && !gen) HIPCHK(hipMemcpyAsync(&wsum, dsums + ICP_POINT_WEIGHT_SUM, sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (history) HIPCHK(hipMemcpyAsync(history, dhist, nrows * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  std::vector<int32_t> hi_(corr_out ? static_cast<size_t>(ns) : 0);
  std::vector<double> hd_(hi_.size());
  if (corr_out) {
    HIPCHK(hipMemcpyAsync(hi_.data(), oi, hi_.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(hd_.data(), od, hd_.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, hs.a, hs.b));
  for (size_t i = 0; i < hi_.size(); ++i) corr_out[i] = icp_inlier(hi_[i], hd_[i], d2) ? hi_[i] : -1;
  if (info) {
    info->iterations = hs.rec->iterations;
    info->status = hs.rec->status;
    info->count = hs.rec->count;
    info->fitness = hs.rec->fitness;
    info->inlier_rmse = hs.rec->rmse;
    info->route = route;
    for (int a = 0; a < 3; ++a) info->dim[a] = route == CLIPPER_HIP_KNN_GRID ? ix.g.dim[a] : 0;
    info->candidates = static_cast<int64_t>(cand);
    info->device_ms = static_cast<double>(ms);
  }
  if (rinfo) {
    rinfo->within = trimmed ? sel.within : hs.rec->count;  // (untrimmed: every point within max_distance is kept)
    rinfo->weight_sum = wsum;
    rinfo->trim_sqd = sel.tau;
  }
  return 0;
}

// The host-buffer frame around the body: both clouds, and what the method reads of them, go to the device once.
// Nt / Cs / Ct as IcpInputs'. Every argument has been checked.
int icp_run(int device, const double* Ps, int64_t ns, const double* Pt, const double* Nt, const double* Cs, const double* Ct,
            int64_t nt, const double* T0, const clipper_icp::Params& prm, double* T_out, clipper_icp_info_t* info,
            double* history, int32_t* corr_out, const clipper_icp::Robust* rb = nullptr,
            clipper_icp_robust_info_t* rinfo = nullptr) {
  if (int rc = use_device(device)) return rc;
  const bool plane = prm.method == ICP_POINT_TO_PLANE, gen = prm.method == ICP_GENERALIZED;
  const size_t s3 = static_cast<size_t>(ns) * 3, t3 = static_cast<size_t>(nt) * 3;
  const size_t s6 = gen ? static_cast<size_t>(ns) * 6 : 0, t6 = gen ? static_cast<size_t>(nt) * 6 : 0;
  double *dPs = nullptr, *dPt = nullptr, *dNt = nullptr, *dCs = nullptr, *dCt = nullptr;
  DevTemps tmp;
  if (int rc = tmp.alloc(device, dPs, s3 * sizeof(double), dPt, t3 * sizeof(double), dNt, (plane ? t3 : 0) * sizeof(double)))
    return rc;
  if (gen)
    if (int rc = tmp.alloc(device, dCs, s6 * sizeof(double), dCt, t6 * sizeof(double))) return rc;
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  if (int rc = copy_up(dPs, Ps, s3, st)) return rc;
  if (int rc = copy_up(dPt, Pt, t3, st)) return rc;
  if (plane)
    if (int rc = copy_up(dNt, Nt, t3, st)) return rc;
  if (gen) {
    if (int rc = copy_up(dCs, Cs, s6, st)) return rc;
    if (int rc = copy_up(dCt, Ct, t6, st)) return rc;
  }
  KnnTarget target;  // (of this call alone)
  IcpInputs in;
  in.Ps = dPs, in.Pt = dPt, in.Nt = dNt, in.Cs = dCs, in.Ct = dCt, in.target = &target;
  return icp_body(device, in, ns, nt, T0, prm, T_out, info, history, corr_out, rb, rinfo, tmp);
}

const double ICP_IDENTITY[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

clipper_icp::Params icp_params_of(const clipper_icp_params_t* params) {
  if (!params) return clipper_icp::Params{0, 0, 0.0, 0.0, 0.0};
  return clipper_icp::Params{params->method, params->max_iterations, params->max_distance, params->rel_fitness, params->rel_rmse};
}

clipper_icp::Robust icp_robust_of(const clipper_icp_robust_t* r) {
  return r ? clipper_icp::Robust{r->loss, r->reserved, r->scale, r->trim} : clipper_icp::Robust{0, 0, 0.0, 1.0};
}

// clipper_hip_icp, clipper_hip_icp_generalized and their robust forms (use: ROBUST_REQUIRED; else robust and robust_info
// are not read): `who` names the call in a refusal, the family picks its parameter check and what it reads of c
int icp_call(const char* who, clipper_icp::Family family, clipper_icp::RobustUse use, int device, const clipper_icp::HostClouds& c,
             const double* T_init, const clipper_icp_params_t* params, const clipper_icp_robust_t* robust, double* T_out,
             clipper_icp_info_t* info, clipper_icp_robust_info_t* robust_info, double* history) {
  namespace ci = clipper_icp;
  const ci::Params h = icp_params_of(params);
  const ci::Robust rb = icp_robust_of(robust);
  const bool with_rb = use != ci::ROBUST_ABSENT;
  const std::string why = ci::check_call(family, use, params ? &h : nullptr, robust ? &rb : nullptr, T_out != nullptr, T_init, &c);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s: %s", who, why.c_str());
  return icp_run(device, c.P_src, c.n_src, c.P_tgt, c.N_tgt, c.C_src, c.C_tgt, c.n_tgt, T_init ? T_init : ICP_IDENTITY, h, T_out,
                 info, history, nullptr, with_rb ? &rb : nullptr, with_rb ? robust_info : nullptr);
}

// what the evaluation of a registration hands back of info (each output may be null)
void icp_evaluation_out(const clipper_icp_info_t& info, double* fitness, double* inlier_rmse, int64_t* count) {
  if (fitness) *fitness = info.fitness;
  if (inlier_rmse) *inlier_rmse = info.inlier_rmse;
  if (count) *count = info.count;
}

// THE BODY of the covariance stage, on device pointers: dP the cloud (n x 3), dC (n x 6) and dcn (n) its outputs. The
// lists of the search join tmp; everything is queued on st. The host-buffer call (below) and the call on a cloud
// (host_cloud.hpp) both run this.
int covariances_body(int device, const double* dP, int64_t n, const clipper_features::Neighborhood& nb, double epsilon,
                     double* dC, int32_t* dcn, hipStream_t st, DevTemps& tmp, KnnTarget& target) {
  const int K = clipper_features::list_k(nb.knn);
  const size_t no = static_cast<size_t>(n) * K;
  double* od = nullptr;
  int32_t* oi = nullptr;
  if (int rc = tmp.alloc(device, od, no * sizeof(double), oi, no * sizeof(int32_t))) return rc;
  if (int rc = knn_lists(device, K, 3, dP, n, dP, n, od, oi, st, tmp, target)) return rc;
  const int use_r = nb.radius > 0.0;
  const double w = 1.0 - epsilon;
  hipLaunchKernelGGL(k_icp_covariances<>, dim3(static_cast<unsigned>(ceil_div(n, 256))), dim3(256), 0, st, dP, n, oi, od, K,
                     nb.knn, use_r, nb.radius * nb.radius, w, dC, dcn);
  return 0;
}

// The covariances of the generalized metric: host_features.hpp's features_run with the one kernel behind the search
// changed. Every argument has been checked.
int covariances_run(int device, const double* P, int64_t n, const clipper_features::Neighborhood& nb, double epsilon,
                    double* C_out, int32_t* count_out) {
  if (int rc = use_device(device)) return rc;

  const size_t n3 = static_cast<size_t>(n) * 3, n6 = static_cast<size_t>(n) * 6, nn = static_cast<size_t>(n);
  double *dP = nullptr, *dC = nullptr;
  int32_t* dcn = nullptr;
  DevTemps tmp;
  if (int rc = tmp.alloc(device, dP, n3 * sizeof(double), dC, n6 * sizeof(double), dcn, nn * sizeof(int32_t))) return rc;
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  if (int rc = copy_up(dP, P, n3, st)) return rc;
  KnnTarget target;  // (of this call alone)
  if (int rc = covariances_body(device, dP, n, nb, epsilon, dC, dcn, st, tmp, target)) return rc;
  if (int rc = copy_down(C_out, dC, n6, st)) return rc;
  if (int rc = copy_down(count_out, dcn, nn, st)) return rc;
  HIPCHK(hipStreamSynchronize(st));  // the one wait of the call
  HIPCHK(hipGetLastError());
  return 0;
}

int estimate_covariances(int device, const double* P, int64_t n, const clipper_neighborhood_t* nb, double epsilon,
                         double* C_out, int32_t* count_out) {
  namespace cf = clipper_features;
  const cf::Neighborhood h = feat_nb(nb);
  std::string why = !P ? "null point array" : (!C_out ? "null covariance output array" : "");
  if (why.empty()) why = cf::check_neighborhood("neighbourhood", nb ? &h : nullptr);
  if (why.empty()) why = clipper_icp::check_epsilon(epsilon);
  if (why.empty()) why = cf::check_count(n);
  if (why.empty()) why = cf::check_points(P, n);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "estimate_covariances: %s", why.c_str());
  return covariances_run(device, P, n, h, epsilon, C_out, count_out);
}

int evaluate_registration(int device, const double* P_src, int64_t n_src, const double* P_tgt, int64_t n_tgt, const double* T,
                          double max_distance, double* fitness, double* inlier_rmse, int64_t* count, int32_t* corr_out) {
  namespace ci = clipper_icp;
  std::string why = ci::check_max_distance(max_distance);
  if (why.empty()) why = ci::check_cloud("source", P_src, n_src);
  if (why.empty()) why = ci::check_cloud("target", P_tgt, n_tgt);
  if (why.empty()) why = ci::check_transform("T", T);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "evaluate_registration: %s", why.c_str());
  const ci::Params h{ICP_POINT_TO_POINT, 0, max_distance, 0.0, 0.0};
  clipper_icp_info_t info{};
  if (int rc = icp_run(device, P_src, n_src, P_tgt, nullptr, nullptr, nullptr, n_tgt, T ? T : ICP_IDENTITY, h, nullptr, &info,
                       nullptr, corr_out))
    return rc;
  icp_evaluation_out(info, fitness, inlier_rmse, count);
  return 0;
}

}  // namespace
