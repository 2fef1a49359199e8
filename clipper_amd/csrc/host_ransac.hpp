// host_ransac.hpp — the driver of clipper_hip_ransac_correspondences ("RANSAC over putative
// associations"). Both clouds and the association table go to the device once; the pairs are gathered once; a round is
// four launches (hypotheses, compact, score, best) and the host reads the 64-byte round record through pinned memory
// to apply the stop rule: the only host wait of a round. The polish, the mask and the sums under the final T follow
// without a wait; one copy down ends the call. Stand-alone: needs no context. The checks are host_ransac_check.hpp's,
// the arithmetic ransac_rules.hpp's. Part of clipper_hip.hip (one translation unit; included there after host_icp.hpp).
#pragma once

#include "host_ransac_check.hpp"

namespace {

// what the rounds need besides device memory: a pinned record and two events, released on every path
struct RansacHostState {
  PinnedBuf<RansacRecord> rec;
  Event a, b;
};

template <int N>
void ransac_hypotheses_launch(int32_t H, const double* dP, const double* dB, int32_t m, uint64_t seed, uint64_t h0, double s2,
                              double* dTh, int32_t* dsamp, int32_t* drank, int32_t* dbcount, hipStream_t st) {
  hipLaunchKernelGGL((k_ransac_hypotheses<N>), dim3(static_cast<unsigned>(H / 256)), dim3(256), 0, st, dP, dB, m, seed, h0, s2,
                     dTh, dsamp, drank, dbcount);
}

// Every argument has been checked. o: the centre of the box of the gathered targets.
int ransac_run(int device, const double* D1, int64_t n1_, const double* D2, int64_t n2_, const int32_t* A, int64_t m_,
               const RansacCall& c, const double (&o)[3], double* T_out, uint8_t* inlier_out, clipper_ransac_info_t* info) {
  if (int rc = use_device(device)) return rc;

  const int32_t n1 = static_cast<int32_t>(n1_), n2 = static_cast<int32_t>(n2_), m = static_cast<int32_t>(m_);
  const int32_t H = c.hypotheses_per_round, nblk = H / 256;
  const int32_t nb = static_cast<int32_t>(ceil_div(m, ICP_BLOCK));
  const size_t sm = static_cast<size_t>(m), sH = static_cast<size_t>(H);

  double *dD1 = nullptr, *dD2 = nullptr, *dP = nullptr, *dB = nullptr, *dTh = nullptr, *dpart = nullptr, *dsums = nullptr;
  int32_t *dA = nullptr, *dsamp = nullptr, *drank = nullptr, *dbcount = nullptr, *dlist = nullptr, *dcounts = nullptr;
  uint8_t* dmask = nullptr;
  RansacRecord* drec = nullptr;
  RansacBest* dbest = nullptr;
  RansacPolish* dpol = nullptr;
  DevTemps tmp;
  RansacHostState hs;
  if (int rc = tmp.alloc(device, dD1, static_cast<size_t>(n1) * 3 * sizeof(double), dD2, static_cast<size_t>(n2) * 3 * sizeof(double),
                         dA, sm * 2 * sizeof(int32_t), dP, sm * 3 * sizeof(double), dB, sm * 3 * sizeof(double),
                         dTh, sH * RANSAC_T_DOUBLES * sizeof(double), dsamp, sH * RANSAC_MAX_SAMPLE * sizeof(int32_t),
                         drank, sH * sizeof(int32_t), dbcount, static_cast<size_t>(nblk) * sizeof(int32_t),
                         dlist, sH * sizeof(int32_t), dcounts, sH * sizeof(int32_t),
                         dpart, static_cast<size_t>(nb) * ICP_POINT_TERMS * sizeof(double), dsums, ICP_POINT_TERMS * sizeof(double),
                         dmask, sm, drec, sizeof(RansacRecord), dbest, sizeof(RansacBest), dpol, sizeof(RansacPolish)))
    return rc;
  HIPCHK(hs.rec.alloc(1));
  HIPCHK(hs.a.create());
  HIPCHK(hs.b.create());

  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  RansacRecord first{};
  first.best_key = -1;
  first.round = -1;
  *hs.rec = first;
  HIPCHK(hipMemcpyAsync(dD1, D1, static_cast<size_t>(n1) * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dD2, D2, static_cast<size_t>(n2) * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dA, A, sm * 2 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(drec, hs.rec, sizeof(RansacRecord), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(dbest, 0, sizeof(RansacBest), st));
  HIPCHK(hipEventRecord(hs.a, st));

  const dim3 mb(static_cast<unsigned>(ceil_div(m, 256)));
  hipLaunchKernelGGL(k_ransac_gather<>, mb, dim3(256), 0, st, dD1, n1, dD2, n2, dA, m, dP, dB);

  // the score grid: ceil(m / 256) workgroups per tile walker, as many walkers as fill the chip (a few workgroups per
  // compute unit), never more than the round has tiles
  int cus = 0;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
  const int64_t want = static_cast<int64_t>(cus > 0 ? cus : 256) * 8;
  const int64_t tiles = ceil_div(H, RANSAC_TILE);
  const int64_t walkers = std::min<int64_t>(tiles, std::max<int64_t>(1, ceil_div(want, static_cast<int64_t>(mb.x))));
  const dim3 sg(mb.x, static_cast<unsigned>(walkers));

  const double s2 = c.edge_similarity * c.edge_similarity, d2 = c.max_distance * c.max_distance;
  int status = RANSAC_RUNNING;
  for (int64_t round = 0;; ++round) {
    const uint64_t h0 = static_cast<uint64_t>(round) * static_cast<uint64_t>(H);
    switch (c.n_sample) {
      case 3: ransac_hypotheses_launch<3>(H, dP, dB, m, c.seed, h0, s2, dTh, dsamp, drank, dbcount, st); break;
      case 4: ransac_hypotheses_launch<4>(H, dP, dB, m, c.seed, h0, s2, dTh, dsamp, drank, dbcount, st); break;
      case 5: ransac_hypotheses_launch<5>(H, dP, dB, m, c.seed, h0, s2, dTh, dsamp, drank, dbcount, st); break;
      case 6: ransac_hypotheses_launch<6>(H, dP, dB, m, c.seed, h0, s2, dTh, dsamp, drank, dbcount, st); break;
      case 7: ransac_hypotheses_launch<7>(H, dP, dB, m, c.seed, h0, s2, dTh, dsamp, drank, dbcount, st); break;
      default: ransac_hypotheses_launch<8>(H, dP, dB, m, c.seed, h0, s2, dTh, dsamp, drank, dbcount, st); break;
    }
    hipLaunchKernelGGL(k_ransac_compact<>, dim3(1), dim3(256), 0, st, drank, dbcount, nblk, dlist, dcounts, drec);
    hipLaunchKernelGGL(k_ransac_score<>, sg, dim3(256), 0, st, dP, dB, m, d2, dTh, dlist, drec, dcounts);
    hipLaunchKernelGGL(k_ransac_best<>, dim3(1), dim3(256), 0, st, dcounts, dlist, h0, H, dTh, dsamp, drec, dbest);
    HIPCHK(hipMemcpyAsync(hs.rec, drec, sizeof(RansacRecord), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // the one wait of a round
    if (hs.rec->round != round)
      return fail(CLIPPER_HIP_E_INTERNAL, "ransac: the record of round %lld was not written", static_cast<long long>(round));
    status = ransac_stop(ransac_key_count(hs.rec->best_key), hs.rec->evaluated, m, c);
    if (status != RANSAC_RUNNING) break;
  }

  const int model = status != RANSAC_NO_MODEL;
  const int refine = model ? c.refine_iterations : 0;
  hipLaunchKernelGGL(k_ransac_polish_init<>, dim3(1), dim3(64), 0, st, dbest, model, dpol);
  for (int i = 0; i <= refine; ++i) {
    hipLaunchKernelGGL(k_ransac_terms<>, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, dP, dB, m, d2, o[0], o[1], o[2], dpol, dpart);
    hipLaunchKernelGGL(k_ransac_polish<>, dim3(1), dim3(256), 0, st, dpart, nb, i, refine, o[0], o[1], o[2], dsums, dpol);
  }
  hipLaunchKernelGGL(k_ransac_mask<>, mb, dim3(256), 0, st, dP, dB, m, d2, dpol, dmask);
  HIPCHK(hipEventRecord(hs.b, st));
  HIPCHK(hipGetLastError());

  RansacPolish pol{};
  RansacBest best{};
  HIPCHK(hipMemcpyAsync(&pol, dpol, sizeof(pol), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&best, dbest, sizeof(best), hipMemcpyDeviceToHost, st));
  if (inlier_out) HIPCHK(hipMemcpyAsync(inlier_out, dmask, sm, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, hs.a, hs.b));
  for (int a = 0; a < 16; ++a) T_out[a] = pol.T[a];
  if (info) {
    info->status = status;
    info->refined = pol.refined;
    info->evaluated = hs.rec->evaluated;
    info->checked = hs.rec->checked;
    info->best_hypothesis = model ? ransac_key_h(hs.rec->best_key) : -1;
    info->best_count = model ? ransac_key_count(hs.rec->best_key) : 0;
    info->count = static_cast<int64_t>(pol.S[0]);
    info->fitness = pol.S[0] / static_cast<double>(m);
    info->inlier_rmse = ransac_rmse(pol.S);
    for (int a = 0; a < RANSAC_MAX_SAMPLE; ++a) info->sample[a] = model ? best.sample[a] : -1;
    info->device_ms = static_cast<double>(ms);
  }
  return 0;
}

int ransac_correspondences(int device, const double* D1, int64_t n1, const double* D2, int64_t n2, const int32_t* A, int64_t m,
                           const clipper_ransac_params_t* params, double* T_out, uint8_t* inlier_out, clipper_ransac_info_t* info) {
  namespace cr = clipper_ransac;
  const cr::Params h = params ? cr::Params{params->max_distance, params->edge_similarity, params->confidence, params->max_hypotheses,
                                           params->hypotheses_per_round, params->n_sample, params->refine_iterations, params->reserved}
                              : cr::Params{};
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0}, o[3];
  std::string why = !T_out ? "null T_out" : "";
  if (why.empty()) why = cr::check_params(params ? &h : nullptr);
  if (why.empty()) why = cr::check_cloud_size("D1", D1, n1);
  if (why.empty()) why = cr::check_cloud_size("D2", D2, n2);
  if (why.empty()) why = cr::check_associations(D1, n1, D2, n2, A, m, h.n_sample, lo, hi);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "ransac_correspondences: %s", why.c_str());
  icp_origin(lo, hi, o);
  const RansacCall c{h.max_distance, h.edge_similarity, h.confidence, h.max_hypotheses, h.hypotheses_per_round, h.n_sample,
                     h.refine_iterations, params->seed};
  return ransac_run(device, D1, n1, D2, n2, A, m, c, o, T_out, inlier_out, info);
}

}  // namespace
