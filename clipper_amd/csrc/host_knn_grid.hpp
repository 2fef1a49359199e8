// host_knn_grid.hpp — the one seam through which clipper_hip_knn, clipper_hip_distance_based_correspondences and the
// three feature entry points reach the nearest-neighbour search (knn_lists), and the driver of its grid route
// ("The grid route of the search"). The seam reads the process-wide mode once, picks the route,
// allocates that route's temporaries (the brute-force route's partial lists, or the grid's tables) and queues the
// kernels on the caller's stream; the lists are on the device when it returns. Part of clipper_hip.hip (one
// translation unit; included there after host_match.hpp, whose match_geom it shares, and before host_features.hpp).
#pragma once

#include "host_knn_grid_plan.hpp"

namespace {

std::atomic<int> g_knn_search{CLIPPER_HIP_KNN_BRUTE};  // process-wide (clipper_hip_knn_set_search)
thread_local clipper_hip_knn_stats_t g_knn_stats{-1, {0, 0, 0}, 0, 0, CLIPPER_HIP_KNN_AUTO_MIN_N, 0.0};

// two events around the kernels of the calling thread's last search, kept from call to call on one device; read by
// clipper_hip_knn_last_search, after the searching call has returned (every caller of the seam waits for its stream)
struct KnnEvents {
  hipEvent_t a = nullptr, b = nullptr;
  int device = -1;
  bool pending = false;
};
thread_local KnnEvents g_knn_events;

inline bool knn_events_begin(int device, hipStream_t st) {
  KnnEvents& ev = g_knn_events;
  ev.pending = false;
  if (ev.device != device || !ev.a || !ev.b) {
    if (ev.a) hipEventDestroy(ev.a);
    if (ev.b) hipEventDestroy(ev.b);
    ev.a = ev.b = nullptr;
    ev.device = device;
    if (hipEventCreate(&ev.a) != hipSuccess || hipEventCreate(&ev.b) != hipSuccess) return false;
  }
  return hipEventRecord(ev.a, st) == hipSuccess;
}

inline void knn_events_end(bool begun, hipStream_t st) {
  g_knn_events.pending = begun && hipEventRecord(g_knn_events.b, st) == hipSuccess;
}

inline void knn_events_read() {
  KnnEvents& ev = g_knn_events;
  if (!ev.pending) return;
  ev.pending = false;
  float ms = 0.f;
  if (hipEventSynchronize(ev.b) == hipSuccess && hipEventElapsedTime(&ms, ev.a, ev.b) == hipSuccess)
    g_knn_stats.kernels_ms = static_cast<double>(ms);
  else
    (void)hipGetLastError();
}

// the route of one search under the mode the call read
inline int knn_route(int mode, int d, int64_t n0, int64_t n1) {
  const bool fits = n0 <= std::numeric_limits<int32_t>::max() && n1 <= std::numeric_limits<int32_t>::max();
  if (d != 3 || !fits) return CLIPPER_HIP_KNN_BRUTE;  // (indices are int32: beyond them only the brute-force route's casts apply)
  if (mode == CLIPPER_HIP_KNN_GRID) return CLIPPER_HIP_KNN_GRID;
  if (mode == CLIPPER_HIP_KNN_AUTO && n1 >= CLIPPER_HIP_KNN_AUTO_MIN_N) return CLIPPER_HIP_KNN_GRID;
  return CLIPPER_HIP_KNN_BRUTE;
}

template <int K>
void knn_grid_launch(const KgPoint* Q, int32_t n0, const KgPoint* S, int32_t n1, const int32_t* start, const KnnGrid& g,
                     const double* smin, const double* pmax, double* od, int32_t* oi, int32_t* visited, hipStream_t st) {
  hipLaunchKernelGGL((k_knn_grid<K>), dim3(static_cast<unsigned>(ceil_div(n0, 256))), dim3(256), 0, st, Q, n0, S, n1, start,
                     g, smin, pmax, od, oi, visited);
}

// count, scan, scatter: the cloud P in the cell order of grid g. kmin / kmax: the slab keys (null for the queries)
void knn_grid_bin(const double* P, int32_t n, const KnnGrid& g, int32_t ncells, int32_t* cell, int32_t* counts, int32_t* start,
                  int32_t* cursor, unsigned long long* kmin, unsigned long long* kmax, KgPoint* out, hipStream_t st) {
  const dim3 pb(static_cast<unsigned>(ceil_div(n, 256)));
  hipLaunchKernelGGL(k_kg_count<>, pb, dim3(256), 0, st, P, n, g, cell, counts, kmin, kmax);
  hipLaunchKernelGGL(k_kg_scan<>, dim3(1), dim3(KG_SCAN_THREADS), 0, st, counts, ncells, start, cursor);
  hipLaunchKernelGGL(k_kg_scatter<>, pb, dim3(256), 0, st, P, n, cell, cursor, out);
}

// The grid route: dP1 binned, dP0 binned by the same grid (skipped when the cloud is searched in itself), the query
// kernel, the statistics. One host wait in the middle (the bounding box comes back for the plan) and one at the end
// (the candidate count). Temporaries are tmp's: released by the caller on every path.
int knn_grid_lists(int device, int K, const double* dP0, int64_t n0_, const double* dP1, int64_t n1_, double* od, int32_t* oi,
                   hipStream_t st, DevTemps& tmp) {
  const int32_t n0 = static_cast<int32_t>(n0_), n1 = static_cast<int32_t>(n1_);
  const bool self = dP0 == dP1 && n0 == n1;
  const int nb = static_cast<int>(std::min<int64_t>(KG_BOUNDS_BLOCKS, ceil_div(n1, 256)));
  double* dpart = nullptr;
  if (tmp.alloc(device, dpart, static_cast<size_t>(nb) * 6 * sizeof(double)))
    return fail(CLIPPER_HIP_E_NOMEM, "device allocation failed");
  hipLaunchKernelGGL(k_kg_bounds<>, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, dP1, static_cast<int64_t>(n1), dpart);
  std::vector<double> part(static_cast<size_t>(nb) * 6);
  HIPCHK(hipMemcpyAsync(part.data(), dpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = 0; b < nb; ++b)
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], part[static_cast<size_t>(b) * 6 + a]);
      hi[a] = std::max(hi[a], part[static_cast<size_t>(b) * 6 + 3 + a]);
    }
  const KnnGrid g = knn_grid_plan(lo, hi, n1);
  const int32_t ncells = static_cast<int32_t>(knn_grid_cells(g));
  const int32_t nslab = g.dim[0] + g.dim[1] + g.dim[2];

  const size_t ne = static_cast<size_t>(ncells) + 1;
  KgPoint *S = nullptr, *Q = nullptr;
  int32_t *cell = nullptr, *counts = nullptr, *start = nullptr, *cursor = nullptr, *visited = nullptr;
  unsigned long long *kmin = nullptr, *kmax = nullptr, *dsum = nullptr;
  double *smin = nullptr, *pmax = nullptr;
  if (tmp.alloc(device, S, static_cast<size_t>(n1) * sizeof(KgPoint)) ||
      (!self && tmp.alloc(device, Q, static_cast<size_t>(n0) * sizeof(KgPoint))) ||
      tmp.alloc(device, cell, static_cast<size_t>(std::max(n0, n1)) * sizeof(int32_t)) ||
      tmp.alloc(device, counts, 2 * ne * sizeof(int32_t)) || tmp.alloc(device, start, ne * sizeof(int32_t)) ||
      tmp.alloc(device, cursor, ne * sizeof(int32_t)) || tmp.alloc(device, visited, static_cast<size_t>(n0) * sizeof(int32_t)) ||
      tmp.alloc(device, kmin, static_cast<size_t>(nslab) * sizeof(unsigned long long)) ||
      tmp.alloc(device, kmax, static_cast<size_t>(nslab) * sizeof(unsigned long long)) ||
      tmp.alloc(device, smin, static_cast<size_t>(nslab) * sizeof(double)) ||
      tmp.alloc(device, pmax, static_cast<size_t>(nslab) * sizeof(double)) || tmp.alloc(device, dsum, sizeof(unsigned long long)))
    return fail(CLIPPER_HIP_E_NOMEM, "device allocation failed");
  if (self) Q = S;

  // (counts: the searched cloud's, and behind them the queries')
  hipLaunchKernelGGL(k_kg_init<>, dim3(static_cast<unsigned>(std::min<int64_t>(1024, ceil_div(2 * static_cast<int64_t>(ne), 256)))),
                     dim3(256), 0, st, counts, static_cast<int64_t>(2 * ne), kmin, kmax, static_cast<int64_t>(nslab), dsum);
  knn_grid_bin(dP1, n1, g, ncells, cell, counts, start, cursor, kmin, kmax, S, st);
  hipLaunchKernelGGL(k_kg_slabs<>, dim3(6), dim3(256), 0, st, g, kmin, kmax, smin, pmax);
  if (!self) knn_grid_bin(dP0, n0, g, ncells, cell, counts + ne, nullptr, cursor, nullptr, nullptr, Q, st);
  switch (K) {
    case 1: knn_grid_launch<1>(Q, n0, S, n1, start, g, smin, pmax, od, oi, visited, st); break;
    case 2: knn_grid_launch<2>(Q, n0, S, n1, start, g, smin, pmax, od, oi, visited, st); break;
    case 4: knn_grid_launch<4>(Q, n0, S, n1, start, g, smin, pmax, od, oi, visited, st); break;
    case 8: knn_grid_launch<8>(Q, n0, S, n1, start, g, smin, pmax, od, oi, visited, st); break;
    case 16: knn_grid_launch<16>(Q, n0, S, n1, start, g, smin, pmax, od, oi, visited, st); break;
    default: knn_grid_launch<32>(Q, n0, S, n1, start, g, smin, pmax, od, oi, visited, st); break;
  }
  hipLaunchKernelGGL(k_kg_sum<>, dim3(static_cast<unsigned>(std::min<int64_t>(256, ceil_div(n0, 256)))), dim3(256), 0, st,
                     visited, static_cast<int64_t>(n0), dsum);
  unsigned long long sum = 0;
  HIPCHK(hipMemcpyAsync(&sum, dsum, sizeof(sum), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  g_knn_stats.route = CLIPPER_HIP_KNN_GRID;
  for (int a = 0; a < 3; ++a) g_knn_stats.dim[a] = g.dim[a];
  g_knn_stats.candidates = static_cast<int64_t>(sum);
  return 0;
}

// the brute-force route: k_knn's two kernels over S chunks of the searched cloud (match_geom: k_knn's own rule)
int knn_brute_lists(int device, int K, int d, const double* dP0, int64_t n0, const double* dP1, int64_t n1, double* od,
                    int32_t* oi, hipStream_t st, DevTemps& tmp) {
  const MatchGeom g = match_geom(n0, n1);
  const size_t np = static_cast<size_t>(g.S) * n0 * K;
  double* pd = nullptr;
  int32_t* pi = nullptr;
  if (tmp.alloc(device, pd, np * sizeof(double)) || tmp.alloc(device, pi, np * sizeof(int32_t)))
    return fail(CLIPPER_HIP_E_NOMEM, "device allocation failed");
  switch (K) {
    case 1: knn_launch<1>(d, dP0, n0, dP1, n1, g.S, g.chunk, pd, pi, od, oi, st); break;
    case 2: knn_launch<2>(d, dP0, n0, dP1, n1, g.S, g.chunk, pd, pi, od, oi, st); break;
    case 4: knn_launch<4>(d, dP0, n0, dP1, n1, g.S, g.chunk, pd, pi, od, oi, st); break;
    case 8: knn_launch<8>(d, dP0, n0, dP1, n1, g.S, g.chunk, pd, pi, od, oi, st); break;
    case 16: knn_launch<16>(d, dP0, n0, dP1, n1, g.S, g.chunk, pd, pi, od, oi, st); break;
    default:
      if (d != 3) return fail(CLIPPER_HIP_E_INTERNAL, "no search kernel for K = %d, d = %d", K, d);
      knn_run<32, 3>(dP0, n0, dP1, n1, g.S, g.chunk, pd, pi, od, oi, st);
      break;
  }
  return 0;
}

// The seam. dP0: n0 x d, dP1: n1 x d on the device; od / oi: n0 x K, the caller's; K in {1, 2, 4, 8, 16, 32}. The
// route's temporaries join tmp. Returns 0 with the kernels queued on st (the grid route has waited for them), or <0.
int knn_lists(int device, int K, int d, const double* dP0, int64_t n0, const double* dP1, int64_t n1, double* od,
              int32_t* oi, hipStream_t st, DevTemps& tmp) {
  const int route = knn_route(g_knn_search.load(), d, n0, n1);
  g_knn_stats = clipper_hip_knn_stats_t{route, {0, 0, 0}, n0, 0, CLIPPER_HIP_KNN_AUTO_MIN_N, 0.0};
  const bool timed = knn_events_begin(device, st);
  const int rc = route == CLIPPER_HIP_KNN_GRID ? knn_grid_lists(device, K, dP0, n0, dP1, n1, od, oi, st, tmp)
                                               : knn_brute_lists(device, K, d, dP0, n0, dP1, n1, od, oi, st, tmp);
  knn_events_end(timed && rc == 0, st);
  return rc;
}

}  // namespace
