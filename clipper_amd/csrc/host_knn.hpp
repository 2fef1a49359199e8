// host_knn.hpp — the nearest-neighbour search in d = 2 | 3 that puts associations together before any context exists:
// the brute-force route (a scratch of partial lists, allocated once, and a query over it, as the grid route has an
// index and a query), the one seam through which clipper_hip_knn, clipper_hip_distance_based_correspondences and the
// three feature entry points reach either route (knn_lists), and the drivers of the first two. The seam reads the
// process-wide mode once (the only read of a searching call besides icp_body's), picks the route, allocates that
// route's temporaries and queues the kernels on the caller's stream; the lists are on the device when it returns. What
// outlasts the search is the KnnTarget's the caller hands in (host_knn_grid.hpp), never tmp's. Part of clipper_hip.hip
// (one translation unit; included there behind host_matrix_io.hpp and in front of host_match.hpp, which shares the
// chunk rule: the search kernels come last in the code object).
#pragma once

#include "host_knn_grid.hpp"

namespace {

// the chunks the candidate set of one brute-force search is split into: enough workgroups to fill the chip, whole tiles
struct KnnGeom {
  int S;
  int64_t chunk;
};
KnnGeom knn_geom(int64_t nq, int64_t nc) {
  const int64_t qblocks = ceil_div(nq, 256);
  const int64_t tiles = ceil_div(nc, KNN_TILE);
  const int S = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(tiles, ceil_div(512, qblocks))));
  return {S, ceil_div(tiles, S) * KNN_TILE};
}

// what a brute-force search of n1 points needs besides its output: the chunks and their partial lists (tmp's)
struct KnnBruteScratch {
  KnnGeom g{};
  double* pd = nullptr;
  int32_t* pi = nullptr;
};

int knn_brute_alloc(int device, int K, int64_t n0, int64_t n1, KnnBruteScratch& s, DevTemps& tmp) {
  s.g = knn_geom(n0, n1);
  const size_t np = static_cast<size_t>(s.g.S) * n0 * K;
  return tmp.alloc(device, s.pd, np * sizeof(double), s.pi, np * sizeof(int32_t));
}

// the two kernels of one (K, D): the partial lists of every chunk, then their merge
template <int K, int D>
void knn_run(const double* Q, int64_t n0, const double* P1, int64_t n1, const KnnBruteScratch& s, double* od, int32_t* oi,
             hipStream_t st) {
  const dim3 qb(static_cast<unsigned>(ceil_div(n0, 256)));
  hipLaunchKernelGGL((k_knn_partial<K, D>), dim3(qb.x, static_cast<unsigned>(s.g.S)), dim3(256), 0, st, Q, n0, P1, n1,
                     s.g.chunk, s.pd, s.pi);
  hipLaunchKernelGGL((k_knn_merge<K>), qb, dim3(256), 0, st, s.pd, s.pi, n0, s.g.S, od, oi);
}

// The query over a scratch: the K nearest of P1 (n1 x d) to every row of Q (n0 x d), to od / oi. No host wait.
int knn_brute_query(int K, int d, const double* Q, int64_t n0, const double* P1, int64_t n1, const KnnBruteScratch& s,
                    double* od, int32_t* oi, hipStream_t st) {
  const bool found =
      d == 3 ? dispatch_k<1, 2, 4, 8, 16, 32>(K, [&](auto k) { knn_run<decltype(k)::value, 3>(Q, n0, P1, n1, s, od, oi, st); })
             : dispatch_k<1, 2, 4, 8, 16>(K, [&](auto k) { knn_run<decltype(k)::value, 2>(Q, n0, P1, n1, s, od, oi, st); });
  return found ? 0 : fail(CLIPPER_HIP_E_INTERNAL, "no search kernel for K = %d, d = %d", K, d);
}

// the brute-force route: k_knn's two kernels over the chunks of the searched cloud
int knn_brute_lists(int device, int K, int d, const double* dP0, int64_t n0, const double* dP1, int64_t n1, double* od,
                    int32_t* oi, hipStream_t st, DevTemps& tmp) {
  KnnBruteScratch s;
  if (int rc = knn_brute_alloc(device, K, n0, n1, s, tmp)) return rc;
  return knn_brute_query(K, d, dP0, n0, dP1, n1, s, od, oi, st);
}

// The seam. dP0: n0 x d, dP1: n1 x d on the device; od / oi: n0 x K, the caller's; K in {1, 2, 4, 8, 16, 32}. The
// route's temporaries join tmp. Returns 0 with the kernels queued on st (the grid route has waited for them), or <0.
// target: what the owner of dP1 keeps of it (a cloud's, or a local of the call); the grid route makes sure of its index.
int knn_lists(int device, int K, int d, const double* dP0, int64_t n0, const double* dP1, int64_t n1, double* od,
              int32_t* oi, hipStream_t st, DevTemps& tmp, KnnTarget& target) {
  const int route = knn_route(g_knn_search.load(), d, n0, n1);
  g_knn_stats = clipper_hip_knn_stats_t{route, {0, 0, 0}, n0, 0, CLIPPER_HIP_KNN_AUTO_MIN_N, 0.0};
  const bool timed = knn_events_begin(device, st);
  const int rc = route == CLIPPER_HIP_KNN_GRID ? knn_grid_lists(device, K, dP0, n0, dP1, n1, od, oi, st, tmp, target)
                                               : knn_brute_lists(device, K, d, dP0, n0, dP1, n1, od, oi, st, tmp);
  knn_events_end(timed && rc == 0, st);
  return rc;
}

// the knn nearest points of pcd1 (P1) to every point of pcd0 (P0), nearest first: indices, squared distances
int knn_search(int device, const double* P0, int64_t n0, const double* P1, int64_t n1, int d, int knn, int32_t* idx_out,
        double* sqd_out) {
  if (!P0 || !P1 || !idx_out || n0 < 1 || n1 < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (d != 2 && d != 3) return fail(CLIPPER_HIP_E_INVALID, "points must have 2 or 3 coordinates");
  if (knn < 1 || knn > 16) return fail(CLIPPER_HIP_E_INVALID, "knn must be in 1..16");
  if (int rc = use_device(device)) return rc;
  const int K = knn_list_k(knn, 1, 16);
  double *dP0 = nullptr, *dP1 = nullptr, *od = nullptr;
  int32_t* oi = nullptr;
  const size_t c0 = static_cast<size_t>(n0) * d, c1 = static_cast<size_t>(n1) * d, no = static_cast<size_t>(n0) * K;
  DevTemps tmp;
  if (int rc = tmp.alloc(device, dP0, c0 * sizeof(double), dP1, c1 * sizeof(double), od, no * sizeof(double), oi, no * sizeof(int32_t)))
    return rc;
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  if (int rc = copy_up(dP0, P0, c0, st)) return rc;
  if (int rc = copy_up(dP1, P1, c1, st)) return rc;
  // the route under the process-wide mode (host_knn_grid.hpp): its temporaries join tmp, its index is target's
  KnnTarget target;
  if (int rc = knn_lists(device, K, d, dP0, n0, dP1, n1, od, oi, st, tmp, target)) return rc;
  std::vector<double> hd(no);
  std::vector<int32_t> hi(no);
  HIPCHK(hipMemcpy(hd.data(), od, no * sizeof(double), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(hi.data(), oi, no * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIPCHK(hipGetLastError());
  for (int64_t i = 0; i < n0; ++i)
    for (int k = 0; k < knn; ++k) {
      idx_out[i * knn + k] = hi[static_cast<size_t>(i) * K + k];
      if (sqd_out) sqd_out[i * knn + k] = hd[static_cast<size_t>(i) * K + k];
    }
  return 0;
}

// bm_utils::get_putative_associations (bm_utils.cpp:187-229) on the GPU's nearest neighbours: the associations, n x 2
// column-major; the count comes back
int64_t distance_based_correspondences(int device, const double* P0, int64_t n0, const double* P1, int64_t n1, int d,
                                       int knn, double radius, int enforce_1to1, int32_t* A_out, int64_t capacity) {
  std::vector<int32_t> idx(static_cast<size_t>(std::max<int64_t>(n0, 0)) * std::max(knn, 0));
  std::vector<double> sqd(idx.size());
  int rc = knn_search(device, P0, n0, P1, n1, d, knn, idx.data(), sqd.data());
  if (rc) return rc;
  // bm_utils.cpp:187-229: rows (i, nn_j(i)) for i ascending, neighbours by distance, kept if within
  // the radius; one-to-one: per point of pcd1 (ascending) the FIRST closest of its claimants
  const double r2 = radius * radius;
  std::vector<std::pair<int32_t, int32_t>> rows;
  std::map<int32_t, std::vector<std::pair<int32_t, double>>> claim;
  for (int64_t i = 0; i < n0; ++i)
    for (int k = 0; k < knn; ++k) {
      const int32_t c1 = idx[static_cast<size_t>(i) * knn + k];
      const double sd = sqd[static_cast<size_t>(i) * knn + k];
      if (c1 < 0) continue;  // fewer than knn points in pcd1
      if (sd <= r2) {
        rows.emplace_back(static_cast<int32_t>(i), c1);
        if (enforce_1to1) claim[c1].emplace_back(static_cast<int32_t>(i), sd);
      }
    }
  if (enforce_1to1) {
    rows.clear();
    for (const auto& it : claim) {
      size_t best = 0;
      for (size_t q = 1; q < it.second.size(); ++q)
        if (it.second[q].second < it.second[best].second) best = q;  // std::min_element: first minimum
      rows.emplace_back(it.second[best].first, it.first);
    }
  }
  const int64_t n = static_cast<int64_t>(rows.size());
  if (n > capacity) return fail(CLIPPER_HIP_E_INVALID, "capacity %lld < %lld associations",
                                static_cast<long long>(capacity), static_cast<long long>(n));
  for (int64_t r = 0; r < n; ++r) {  // column-major n x 2, as clipper::Association
    A_out[r] = rows[static_cast<size_t>(r)].first;
    A_out[n + r] = rows[static_cast<size_t>(r)].second;
  }
  return n;
}

}  // namespace
