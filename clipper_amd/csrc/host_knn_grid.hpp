// host_knn_grid.hpp — the grid route of the nearest-neighbour search ("The grid route of the
// search"), the process-wide mode that picks the route, the statistics of the last search, and the owner of what a
// search against a cloud keeps. The route is a build (knn_grid_build) followed by a query (knn_grid_query_lists). A
// KnnGridIndex OWNS its four arrays (move-only, never copied; readers take it by const reference); a KnnTarget owns the
// index, the brute-force route's bounding box and the build count of one searched cloud, and knn_target_ensure is the
// one place that makes either. Call-scoped scratch (the build's, the queries', the lists') is the caller's DevTemps'.
// Part of clipper_hip.hip (one translation unit; included by host_knn.hpp, which holds the brute-force route and the
// seam over the two).
#pragma once

#include "host_knn_grid_plan.hpp"
#include "host_knn_k.hpp"

namespace {

std::atomic<int> g_knn_search{CLIPPER_HIP_KNN_BRUTE};  // process-wide (clipper_hip_knn_set_search)
thread_local clipper_hip_knn_stats_t g_knn_stats{-1, {0, 0, 0}, 0, 0, CLIPPER_HIP_KNN_AUTO_MIN_N, 0.0};

// two events around the kernels of the calling thread's last search, kept from call to call on one device; read by
// clipper_hip_knn_last_search, after the searching call has returned (every caller of the seam waits for its stream)
struct KnnEvents {
  Event a, b;
  int device = -1;
  bool pending = false;
};
thread_local KnnEvents g_knn_events;

inline bool knn_events_begin(int device, hipStream_t st) {
  KnnEvents& ev = g_knn_events;
  ev.pending = false;
  if (ev.device != device || !ev.a || !ev.b) {
    ev.a.reset(), ev.b.reset();
    ev.device = device;
    if (ev.a.create() != hipSuccess || ev.b.create() != hipSuccess) return false;
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
  hipLaunchKernelGGL(k_row_scan<>, dim3(1), dim3(ROW_SCAN_THREADS), 0, st, counts, ncells, cursor, start, 1);
  hipLaunchKernelGGL(k_kg_scatter<>, pb, dim3(256), 0, st, P, n, cell, cursor, out);
}

// The index of a searched cloud: the cloud in cell order (S), the cells' first places (start), the grid and the slab
// tables. Built once (bounds, plan, bin, slabs: one host wait, for the bounding box), queried any number of times. It
// owns its arrays; it is there exactly when S is. lo / hi: the exact bounding box (min and max do not depend on the
// order of reduction).
struct KnnGridIndex {
  DevBuf<KgPoint> S;
  DevBuf<int32_t> start;
  DevBuf<double> smin, pmax;
  KnnGrid g{};
  int32_t n1 = 0, ncells = 0;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
};
static_assert(!std::is_copy_constructible<KnnGridIndex>::value, "an index owns its arrays: it is moved, never copied");

// the exact bounding box of the cloud dP (n x 3): k_kg_bounds' partials folded on the host. One host wait.
int knn_grid_bounds(int device, const double* dP, int32_t n, double (&lo)[3], double (&hi)[3], hipStream_t st, DevTemps& tmp) {
  const int nb = static_cast<int>(std::min<int64_t>(KG_BOUNDS_BLOCKS, ceil_div(n, 256)));
  double* dpart = nullptr;
  if (int rc = tmp.alloc(device, dpart, static_cast<size_t>(nb) * 6 * sizeof(double))) return rc;
  hipLaunchKernelGGL(k_kg_bounds<>, dim3(static_cast<unsigned>(nb)), dim3(256), 0, st, dP, static_cast<int64_t>(n), dpart);
  std::vector<double> part(static_cast<size_t>(nb) * 6);
  HIPCHK(hipMemcpyAsync(part.data(), dpart, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (int a = 0; a < 3; ++a) {
    lo[a] = INFINITY;
    hi[a] = -INFINITY;
  }
  for (int b = 0; b < nb; ++b)
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], part[static_cast<size_t>(b) * 6 + a]);
      hi[a] = std::max(hi[a], part[static_cast<size_t>(b) * 6 + 3 + a]);
    }
  return 0;
}

// The build: bounds, plan, bin, slabs of the searched cloud dP1, into ix's own arrays; the scratch joins tmp. The
// kernels behind the one wait are queued on st. Called by knn_target_ensure alone.
int knn_grid_build(int device, const double* dP1, int32_t n1, KnnGridIndex& ix, hipStream_t st, DevTemps& tmp) {
  if (int rc = knn_grid_bounds(device, dP1, n1, ix.lo, ix.hi, st, tmp)) return rc;
  ix.g = knn_grid_plan(ix.lo, ix.hi, n1);
  ix.n1 = n1;
  ix.ncells = static_cast<int32_t>(knn_grid_cells(ix.g));
  const int32_t nslab = ix.g.dim[0] + ix.g.dim[1] + ix.g.dim[2];
  const size_t ne = static_cast<size_t>(ix.ncells) + 1;
  int32_t *cell = nullptr, *counts = nullptr, *cursor = nullptr;
  unsigned long long *kmin = nullptr, *kmax = nullptr;
  const size_t np = static_cast<size_t>(n1), ns = static_cast<size_t>(nslab);
  HIPCHK(ix.S.alloc(np));
  HIPCHK(ix.start.alloc(ne));
  HIPCHK(ix.smin.alloc(ns));
  HIPCHK(ix.pmax.alloc(ns));
  if (int rc = tmp.alloc(device, cell, np * sizeof(int32_t), counts, ne * sizeof(int32_t), cursor, ne * sizeof(int32_t), kmin,
                         ns * sizeof(unsigned long long), kmax, ns * sizeof(unsigned long long)))
    return rc;
  hipLaunchKernelGGL(k_kg_init<>, dim3(static_cast<unsigned>(std::min<int64_t>(1024, ceil_div(static_cast<int64_t>(ne), 256)))),
                     dim3(256), 0, st, counts, static_cast<int64_t>(ne), kmin, kmax, static_cast<int64_t>(nslab), nullptr);
  knn_grid_bin(dP1, n1, ix.g, ix.ncells, cell, counts, ix.start, cursor, kmin, kmax, ix.S, st);
  hipLaunchKernelGGL(k_kg_slabs<>, dim3(6), dim3(256), 0, st, ix.g, kmin, kmax, ix.smin.get(), ix.pmax.get());
  return 0;
}

// What a search against one cloud keeps: the index (grid route; there when ix.S is), the bounding box as
// knn_grid_bounds folds it (brute-force route: the origin of ICP's sums), how often the index was built, and whether
// the target outlives the call (a cloud's, host_cloud.hpp) or is a host-buffer call's local.
struct KnnTarget {
  KnnGridIndex ix;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  bool has_box = false;
  int grid_builds = 0;
  const bool outlives_call;
  explicit KnnTarget(bool outlives = false) : outlives_call(outlives) {}
};

// Makes sure what `route` needs of the cloud dP (n x 3) is in t: the one statement of "build it unless it is there".
// A call-local target gains no host wait beyond the bounding box's, and the scratch joins the call's tmp. A target
// that outlives the call takes the index only once the build's kernels have been waited for and no error is pending;
// the scratch is released here. A failed build leaves t as it was.
int knn_target_ensure(KnnTarget& t, int route, int device, const double* dP, int32_t n, hipStream_t st, DevTemps& tmp) {
  DevTemps own;
  DevTemps& scratch = t.outlives_call ? own : tmp;
  if (route != CLIPPER_HIP_KNN_GRID) {
    if (t.has_box) return 0;
    if (int rc = knn_grid_bounds(device, dP, n, t.lo, t.hi, st, scratch)) return rc;
    t.has_box = true;
    return 0;
  }
  if (t.ix.S) return 0;
  KnnGridIndex ix;
  if (int rc = knn_grid_build(device, dP, n, ix, st, scratch)) return rc;
  if (t.outlives_call) {
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipGetLastError());
  }
  t.ix = std::move(ix);
  t.grid_builds++;
  return 0;
}

// The queries dP0 (n0 x 3) in the cell order of the index's grid: Q (n0 places) and the binning's scratch, tmp's;
// knn_grid_bin_queries bins into them, any number of times. No host wait.
struct KnnGridQueries {
  KgPoint* Q = nullptr;
  int32_t *cell = nullptr, *counts = nullptr, *cursor = nullptr;
};

int knn_grid_alloc_queries(int device, const KnnGridIndex& ix, int32_t n0, KnnGridQueries& q, DevTemps& tmp) {
  const size_t ne = static_cast<size_t>(ix.ncells) + 1;
  return tmp.alloc(device, q.Q, static_cast<size_t>(n0) * sizeof(KgPoint), q.cell, static_cast<size_t>(n0) * sizeof(int32_t),
                   q.counts, ne * sizeof(int32_t), q.cursor, ne * sizeof(int32_t));
}

void knn_grid_bin_queries(const KnnGridIndex& ix, const double* dP0, int32_t n0, const KnnGridQueries& q, hipStream_t st) {
  const int64_t ne = static_cast<int64_t>(ix.ncells) + 1;
  hipLaunchKernelGGL(k_kg_init<>, dim3(static_cast<unsigned>(std::min<int64_t>(1024, ceil_div(ne, 256)))), dim3(256), 0, st, q.counts,
                     ne, nullptr, nullptr, static_cast<int64_t>(0), nullptr);
  knn_grid_bin(dP0, n0, ix.g, ix.ncells, q.cell, q.counts, nullptr, q.cursor, nullptr, nullptr, q.Q, st);
}

// The query against an index: Q in the cell order of its grid (Q == ix.S for a cloud searched in itself), the lists to
// od / oi (n0 x K, rows by original index), the candidates each query visited to visited (n0). No host wait.
int knn_grid_query_lists(const KnnGridIndex& ix, int K, const KgPoint* Q, int32_t n0, double* od, int32_t* oi, int32_t* visited,
                         hipStream_t st) {
  if (!dispatch_k<1, 2, 4, 8, 16, 32>(K, [&](auto k) {
        knn_grid_launch<decltype(k)::value>(Q, n0, ix.S, ix.n1, ix.start, ix.g, ix.smin, ix.pmax, od, oi, visited, st);
      }))
    return fail(CLIPPER_HIP_E_INTERNAL, "no grid search kernel for K = %d", K);
  return 0;
}

// visited (n0) added to *dsum on the device (integer adds: the order does not matter)
void knn_grid_sum_visited(const int32_t* visited, int32_t n0, unsigned long long* dsum, hipStream_t st) {
  hipLaunchKernelGGL(k_kg_sum<>, dim3(static_cast<unsigned>(std::min<int64_t>(256, ceil_div(n0, 256)))), dim3(256), 0, st,
                     visited, static_cast<int64_t>(n0), dsum);
}

// The grid route: the target's index made sure of, dP0 binned by the same grid (skipped when the cloud is searched
// in itself), the query, the statistics. One host wait in the build (the bounding box comes back for the plan; none
// where the target holds its index already: the index depends on the cloud alone, not on K) and one at the end (the
// candidate count). Temporaries are tmp's.
int knn_grid_lists(int device, int K, const double* dP0, int64_t n0_, const double* dP1, int64_t n1_, double* od, int32_t* oi,
                   hipStream_t st, DevTemps& tmp, KnnTarget& target) {
  const int32_t n0 = static_cast<int32_t>(n0_), n1 = static_cast<int32_t>(n1_);
  const bool self = dP0 == dP1 && n0 == n1;
  if (int rc = knn_target_ensure(target, CLIPPER_HIP_KNN_GRID, device, dP1, n1, st, tmp)) return rc;
  const KnnGridIndex& ix = target.ix;
  KgPoint* Q = ix.S;
  if (!self) {
    KnnGridQueries q;
    if (int rc = knn_grid_alloc_queries(device, ix, n0, q, tmp)) return rc;
    knn_grid_bin_queries(ix, dP0, n0, q, st);
    Q = q.Q;
  }
  int32_t* visited = nullptr;
  unsigned long long* dsum = nullptr;
  if (int rc = tmp.alloc(device, visited, static_cast<size_t>(n0) * sizeof(int32_t), dsum, sizeof(unsigned long long))) return rc;
  HIPCHK(hipMemsetAsync(dsum, 0, sizeof(unsigned long long), st));
  if (int rc = knn_grid_query_lists(ix, K, Q, n0, od, oi, visited, st)) return rc;
  knn_grid_sum_visited(visited, n0, dsum, st);
  unsigned long long sum = 0;
  HIPCHK(hipMemcpyAsync(&sum, dsum, sizeof(sum), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  g_knn_stats.route = CLIPPER_HIP_KNN_GRID;
  for (int a = 0; a < 3; ++a) g_knn_stats.dim[a] = ix.g.dim[a];
  g_knn_stats.candidates = static_cast<int64_t>(sum);
  return 0;
}

}  // namespace
