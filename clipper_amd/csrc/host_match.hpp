// host_match.hpp — putative associations from feature descriptors (before the path, in front of the affinity fill): the
// driver of clipper_hip_match_descriptors. Both descriptor sets go to the device once, padded with zeros to whole groups
// of 8 coordinates; the forward search (F0 -> F1) and, for the mutual check, the backward search (F1 -> F0) are queued
// on one stream with no host wait in between; the lists (n x K entries) come back and the filters of
// host_match_select.hpp run on the host, as distance_based_correspondences does with its lists. Stand-alone: needs no
// context. Part of clipper_hip.hip (one translation unit; included there after host_matrix_io.hpp, so that the search
// kernels come last in the code object).
#pragma once

#include "host_match_select.hpp"

namespace {

// the chunks the candidate set of one search is split into: k_knn's rule (enough workgroups to fill the chip, whole tiles)
struct MatchGeom {
  int S;
  int64_t chunk;
};
MatchGeom match_geom(int64_t nq, int64_t nc) {
  const int64_t qblocks = ceil_div(nq, 256);
  const int64_t tiles = ceil_div(nc, KNN_TILE);
  const int S = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(tiles, ceil_div(512, qblocks))));
  return {S, ceil_div(tiles, S) * KNN_TILE};
}

// one search: the partial lists of every chunk, then their merge. Q: nq x 8 G, C: nc x 8 G (padded rows)
template <int K, int G>
void match_run(const double* Q, int64_t nq, const double* C, int64_t nc, const MatchGeom& g, double* pd, int32_t* pi,
               double* od, int32_t* oi, hipStream_t st) {
  const unsigned qb = static_cast<unsigned>(ceil_div(nq, 256));
  hipLaunchKernelGGL((k_match_partial<K, G>), dim3(qb, static_cast<unsigned>(g.S)), dim3(256), 0, st, Q, nq, C, nc,
                     g.chunk, pd, pi);
  hipLaunchKernelGGL((k_knn_merge<K>), dim3(qb), dim3(256), 0, st, pd, pi, nq, g.S, od, oi);
}

// the instantiations that exist (k_match.hip.h): G in {1, 2, 4, 5, 8}; a narrower row runs through the next wider one
inline int match_groups(int d) {
  const int g = (d + MATCH_GROUP - 1) / MATCH_GROUP;
  return g <= 2 ? g : (g <= 4 ? 4 : (g == 5 ? 5 : 8));
}

template <int K>
void match_launch(int G, const double* Q, int64_t nq, const double* C, int64_t nc, const MatchGeom& g, double* pd,
                  int32_t* pi, double* od, int32_t* oi, hipStream_t st) {
  switch (G) {
    case 1: match_run<K, 1>(Q, nq, C, nc, g, pd, pi, od, oi, st); break;
    case 2: match_run<K, 2>(Q, nq, C, nc, g, pd, pi, od, oi, st); break;
    case 4: match_run<K, 4>(Q, nq, C, nc, g, pd, pi, od, oi, st); break;
    case 5: match_run<K, 5>(Q, nq, C, nc, g, pd, pi, od, oi, st); break;
    default: match_run<K, 8>(Q, nq, C, nc, g, pd, pi, od, oi, st); break;
  }
}

void match_search(int K, int G, const double* Q, int64_t nq, const double* C, int64_t nc, const MatchGeom& g, double* pd,
                  int32_t* pi, double* od, int32_t* oi, hipStream_t st) {
  switch (K) {
    case 1: match_launch<1>(G, Q, nq, C, nc, g, pd, pi, od, oi, st); break;
    case 2: match_launch<2>(G, Q, nq, C, nc, g, pd, pi, od, oi, st); break;
    case 4: match_launch<4>(G, Q, nq, C, nc, g, pd, pi, od, oi, st); break;
    default: match_launch<8>(G, Q, nq, C, nc, g, pd, pi, od, oi, st); break;
  }
}

inline int match_list_k(int len) { return len <= 1 ? 1 : (len <= 2 ? 2 : (len <= 4 ? 4 : 8)); }

// F0: d x n0, F1: d x n1 column-major (each descriptor contiguous). The number of associations comes back; A_out is
// column-major n x 2, sqd_out (may be null) one squared distance per row; nn_idx_out / nn_sqd_out (may be null) the
// forward lists, n0 x knn row-major.
int64_t match_descriptors(int device, const double* F0, int64_t n0, const double* F1, int64_t n1, int d,
                          const clipper_match_params_t* params, int32_t* A_out, double* sqd_out, int64_t capacity,
                          int32_t* nn_idx_out, double* nn_sqd_out) {
  namespace cm = clipper_match;
  const cm::Params prm = params ? cm::Params{params->knn, params->mutual, params->ratio, params->max_sqdist} : cm::Params{};
  std::string why = cm::check_args(F0, n0, F1, n1, d, params ? &prm : nullptr);
  if (why.empty()) why = cm::check_finite("F0", F0, n0, d);
  if (why.empty()) why = cm::check_finite("F1", F1, n1, d);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CLIPPER_HIP_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CLIPPER_HIP_E_INVALID, "device %d out of range", device);
  HIPCHK(hipSetDevice(device));

  const int G = match_groups(d), dp = G * MATCH_GROUP;
  const bool mutual = prm.mutual != 0;
  const int Kf = match_list_k(cm::forward_len(prm)), Kb = match_list_k(prm.knn);
  const MatchGeom gf = match_geom(n0, n1), gb = match_geom(n1, n0);
  const std::vector<double> h0 = cm::pad_rows(F0, n0, d, dp), h1 = cm::pad_rows(F1, n1, d, dp);
  const size_t nof = static_cast<size_t>(n0) * Kf, nob = mutual ? static_cast<size_t>(n1) * Kb : 0;
  // the partial lists of the backward search reuse the forward search's (the stream orders them)
  const size_t np = std::max(static_cast<size_t>(gf.S) * nof, static_cast<size_t>(gb.S) * nob);
  double *d0 = nullptr, *d1 = nullptr, *pd = nullptr, *odf = nullptr, *odb = nullptr;
  int32_t *pi = nullptr, *oif = nullptr, *oib = nullptr;
  DevTemps tmp;
  if (tmp.alloc(device, d0, h0.size() * sizeof(double)) || tmp.alloc(device, d1, h1.size() * sizeof(double)) ||
      tmp.alloc(device, pd, np * sizeof(double)) || tmp.alloc(device, pi, np * sizeof(int32_t)) ||
      tmp.alloc(device, odf, nof * sizeof(double)) || tmp.alloc(device, oif, nof * sizeof(int32_t)) ||
      tmp.alloc(device, odb, nob * sizeof(double)) || tmp.alloc(device, oib, nob * sizeof(int32_t))) {
    tmp.release();
    return fail(CLIPPER_HIP_E_NOMEM, "device allocation failed");
  }
  std::vector<double> fd(nof), bd(nob);
  std::vector<int32_t> fi(nof), bi(nob);
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  bool ok = hipMemcpyAsync(d0, h0.data(), h0.size() * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(d1, h1.data(), h1.size() * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok) {
    match_search(Kf, G, d0, n0, d1, n1, gf, pd, pi, odf, oif, st);
    if (mutual) match_search(Kb, G, d1, n1, d0, n0, gb, pd, pi, odb, oib, st);
    ok = hipMemcpyAsync(fd.data(), odf, nof * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
         hipMemcpyAsync(fi.data(), oif, nof * sizeof(int32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
    if (ok && mutual)
      ok = hipMemcpyAsync(bd.data(), odb, nob * sizeof(double), hipMemcpyDeviceToHost, st) == hipSuccess &&
           hipMemcpyAsync(bi.data(), oib, nob * sizeof(int32_t), hipMemcpyDeviceToHost, st) == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok && hipGetLastError() == hipSuccess;  // the one wait of the call
  }
  tmp.release();
  if (!ok) return fail(CLIPPER_HIP_E_HIP, "descriptor search failed: %s", hipGetErrorString(hipGetLastError()));

  const cm::Lists fwd{fi.data(), fd.data(), n0, Kf}, bwd{bi.data(), bd.data(), n1, Kb};
  const cm::Rows rows = cm::select(prm, fwd, bwd);
  why = cm::emit(rows, A_out, sqd_out, capacity);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  for (int64_t i = 0; i < n0; ++i)
    for (int k = 0; k < prm.knn; ++k) {
      if (nn_idx_out) nn_idx_out[i * prm.knn + k] = fi[static_cast<size_t>(i) * Kf + k];
      if (nn_sqd_out) nn_sqd_out[i * prm.knn + k] = fd[static_cast<size_t>(i) * Kf + k];
    }
  return static_cast<int64_t>(rows.i.size());
}

}  // namespace
