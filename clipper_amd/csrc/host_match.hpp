// host_match.hpp — putative associations from feature descriptors (before the path, in front of the affinity fill): the
// driver of clipper_hip_match_descriptors. Both descriptor sets go to the device once, padded with zeros to whole groups
// of 8 coordinates; the forward search (F0 -> F1) and, for the mutual check, the backward search (F1 -> F0) are queued
// on one stream with no host wait in between; the lists (n x K entries) come back and the filters of
// host_match_select.hpp run on the host, as distance_based_correspondences does with its lists. The searches are a body
// on device pointers (match_lists), which the matcher on clouds (host_cloud.hpp) runs too. Stand-alone: needs no
// context. Part of clipper_hip.hip (one translation unit; included there after host_knn.hpp, whose chunk rule and
// merge kernel it shares).
#pragma once

#include "host_match_select.hpp"

namespace {

// one search: the partial lists of every chunk, then their merge. Q: nq x 8 G, C: nc x 8 G (padded rows)
template <int K, int G>
void match_run(const double* Q, int64_t nq, const double* C, int64_t nc, const KnnGeom& g, double* pd, int32_t* pi,
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

// one search at a run-time (K, G): 0, or CLIPPER_HIP_E_INTERNAL for a pair that is not instantiated
int match_search(int K, int G, const double* Q, int64_t nq, const double* C, int64_t nc, const KnnGeom& g, double* pd,
                 int32_t* pi, double* od, int32_t* oi, hipStream_t st) {
  bool found = false;
  dispatch_k<1, 2, 4, 8>(K, [&](auto k) {
    found = dispatch_k<1, 2, 4, 5, 8>(G, [&](auto gr) {
      match_run<decltype(k)::value, decltype(gr)::value>(Q, nq, C, nc, g, pd, pi, od, oi, st);
    });
  });
  return found ? 0 : fail(CLIPPER_HIP_E_INTERNAL, "no descriptor search kernel for K = %d, G = %d", K, G);
}

// the lists of one match on the device: forward n0 x Kf, backward (mutual only) n1 x Kb; owned by the DevTemps they
// were allocated in
struct MatchLists {
  int Kf = 0, Kb = 0;
  size_t nof = 0, nob = 0;  // entries of each
  double *odf = nullptr, *odb = nullptr;
  int32_t *oif = nullptr, *oib = nullptr;
};

// THE BODY of a match, on device pointers: d0 / d1 are the padded images (n0 x 8 G, n1 x 8 G) of the two descriptor
// sets. Allocates the lists in tmp and queues the forward search and, for the mutual check, the backward search on st,
// with no host wait. The host-buffer call (below) and the call on clouds (host_cloud.hpp) both run this.
int match_lists(int device, const clipper_match::Params& prm, int G, const double* d0, int64_t n0, const double* d1,
                int64_t n1, MatchLists& L, DevTemps& tmp, hipStream_t st) {
  namespace cm = clipper_match;
  const bool mutual = prm.mutual != 0;
  L.Kf = knn_list_k(cm::forward_len(prm), 1, 8), L.Kb = knn_list_k(prm.knn, 1, 8);
  const KnnGeom gf = knn_geom(n0, n1), gb = knn_geom(n1, n0);
  L.nof = static_cast<size_t>(n0) * L.Kf, L.nob = mutual ? static_cast<size_t>(n1) * L.Kb : 0;
  // the partial lists of the backward search reuse the forward search's (the stream orders them)
  const size_t np = std::max(static_cast<size_t>(gf.S) * L.nof, static_cast<size_t>(gb.S) * L.nob);
  double* pd = nullptr;
  int32_t* pi = nullptr;
  if (int rc = tmp.alloc(device, pd, np * sizeof(double), pi, np * sizeof(int32_t), L.odf, L.nof * sizeof(double), L.oif,
                         L.nof * sizeof(int32_t), L.odb, L.nob * sizeof(double), L.oib, L.nob * sizeof(int32_t)))
    return rc;
  if (int rc = match_search(L.Kf, G, d0, n0, d1, n1, gf, pd, pi, L.odf, L.oif, st)) return rc;
  if (mutual)
    if (int rc = match_search(L.Kb, G, d1, n1, d0, n0, gb, pd, pi, L.odb, L.oib, st)) return rc;
  return 0;
}

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
  if (int rc = use_device(device)) return rc;

  const int G = match_groups(d), dp = G * MATCH_GROUP;
  const bool mutual = prm.mutual != 0;
  const int Kf = knn_list_k(cm::forward_len(prm), 1, 8), Kb = knn_list_k(prm.knn, 1, 8);
  const std::vector<double> h0 = cm::pad_rows(F0, n0, d, dp), h1 = cm::pad_rows(F1, n1, d, dp);
  const size_t nof = static_cast<size_t>(n0) * Kf, nob = mutual ? static_cast<size_t>(n1) * Kb : 0;
  double *d0 = nullptr, *d1 = nullptr;
  std::vector<double> fd(nof), bd(nob);  // (declared before tmp: its release waits for the device, so they outlive every copy)
  std::vector<int32_t> fi(nof), bi(nob);
  DevTemps tmp;
  if (int rc = tmp.alloc(device, d0, h0.size() * sizeof(double), d1, h1.size() * sizeof(double))) return rc;
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  if (int rc = copy_up(d0, h0.data(), h0.size(), st)) return rc;
  if (int rc = copy_up(d1, h1.data(), h1.size(), st)) return rc;
  MatchLists L;
  if (int rc = match_lists(device, prm, G, d0, n0, d1, n1, L, tmp, st)) return rc;
  if (int rc = copy_down(fd.data(), L.odf, nof, st)) return rc;
  if (int rc = copy_down(fi.data(), L.oif, nof, st)) return rc;
  if (mutual) {
    if (int rc = copy_down(bd.data(), L.odb, nob, st)) return rc;
    if (int rc = copy_down(bi.data(), L.oib, nob, st)) return rc;
  }
  HIPCHK(hipStreamSynchronize(st));  // the one wait of the call
  HIPCHK(hipGetLastError());

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
