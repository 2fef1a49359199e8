// k_knn_grid.hip.h — the uniform-grid route of the d = 3 nearest-neighbour search ("The grid
// route of the search"): the lists of k_knn.hip.h, bit for bit, for O(n0 * K) distance evaluations instead of n0 * n1.
// Part of kernels.hip.h (include that one): hand-written gfx950 device code. The rules (cell of a coordinate,
// lexicographic insertion, ring walk, stop rule with its proof) are knn_grid_rules.hpp's; here is which work item
// holds what.
//
// Build, over the searched cloud pcd1 (and, with the same kernels, over the queries pcd0):
//   k_kg_bounds   per-axis min / max: grid-stride over the points, one partial (6 doubles) per workgroup, the host
//                 folds the partials (min and max are exact: the order does not matter) and plans the grid
//   k_kg_init     zeroes the counts, sets the slab keys to +inf / -inf
//   k_kg_count    thread = point: its cell number (kept), one integer atomic on the cell's count, and for pcd1 the
//                 slab minima / maxima through 64-bit integer atomics on an order-preserving key of the double
//                 (a count, a minimum and a maximum do not depend on arrival order); a point that cannot improve
//                 the value it reads skips its atomic, so a slab that every point shares is not hammered
//   k_row_scan    (k_wave.hip.h) exclusive scan of the counts, one workgroup: cursor[] (used up by the scatter) and
//                 start[] (kept), ncells + 1 entries each
//   k_kg_scatter  thread = point: (x, y, z, original index) to its cell's next free place: 32 bytes, two 16-byte
//                 stores. The order of points inside a cell differs from run to run; the lists do not.
//   k_kg_slabs    six workgroups: suffix minimum / prefix maximum of the slab keys (block_scan_excl over the threads'
//                 stretches), as doubles
// Query:
//   k_knn_grid<K> thread = one query, in the cell order of the searched grid (the 64 lanes of a wave walk
//                 neighbouring cells: their loads hit the same lines), K best in registers as in k_knn_partial,
//                 rings until knn_grid_may_stop; the list goes to the query's original row.
//   k_kg_sum      the candidates visited, summed over the queries (statistics)
// A query is one loop (knn_grid_query): a step is a candidate or an advance of the ring cursor, and the number of steps
// is bounded by an integer of the grid's dimensions and n1.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_wave.hip.h"
#include "knn_grid_rules.hpp"

namespace clipper_hip {

struct alignas(16) KgPoint {
  double x, y, z;
  int32_t idx;
  int32_t pad;
};
static_assert(sizeof(KgPoint) == 32, "a binned point is two 16-byte words");

constexpr int KG_BOUNDS_BLOCKS = 256;  // partials of k_kg_bounds

// order-preserving key of a double for unsigned 64-bit min / max (every finite value and both infinities)
__device__ inline unsigned long long kg_key(double v) {
  const unsigned long long b = static_cast<unsigned long long>(__double_as_longlong(v));
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double kg_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double(static_cast<long long>(b));
}

template <int = 0>
__global__ __launch_bounds__(256) void k_kg_bounds(const double* __restrict__ P, int64_t n, double* __restrict__ part) {
  __shared__ double red[6][256];
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double v = P[i * 3 + a];
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    red[a][threadIdx.x] = lo[a];
    red[3 + a][threadIdx.x] = hi[a];
  }
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (static_cast<int>(threadIdx.x) < s) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double l = red[a][threadIdx.x + s], h = red[3 + a][threadIdx.x + s];
        if (l < red[a][threadIdx.x]) red[a][threadIdx.x] = l;
        if (h > red[3 + a][threadIdx.x]) red[3 + a][threadIdx.x] = h;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x < 6) part[blockIdx.x * 6 + threadIdx.x] = red[threadIdx.x][0];
}

// counts[0..ncount) = 0; kmin[0..nslab) = key(+inf), kmax[0..nslab) = key(-inf); *sum = 0
template <int = 0>
__global__ __launch_bounds__(256) void k_kg_init(int32_t* __restrict__ counts, int64_t ncount, unsigned long long* __restrict__ kmin,
                                                  unsigned long long* __restrict__ kmax, int64_t nslab,
                                                  unsigned long long* __restrict__ sum) {
  const int64_t step = static_cast<int64_t>(gridDim.x) * 256;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (int64_t i = i0; i < ncount; i += step) counts[i] = 0;
  for (int64_t i = i0; i < nslab; i += step) {
    kmin[i] = kg_key(INFINITY);
    kmax[i] = kg_key(-INFINITY);
  }
  if (i0 == 0 && sum) *sum = 0ull;
}

// kmin / kmax null: the queries (binned by the searched cloud's grid, no slab tables of their own)
template <int = 0>
__global__ __launch_bounds__(256) void k_kg_count(const double* __restrict__ P, int32_t n, KnnGrid g, int32_t* __restrict__ cell,
                                                   int32_t* __restrict__ counts, unsigned long long* kmin,
                                                   unsigned long long* kmax) {
  const int32_t i = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  if (i >= n) return;
  const double p[3] = {P[static_cast<int64_t>(i) * 3], P[static_cast<int64_t>(i) * 3 + 1], P[static_cast<int64_t>(i) * 3 + 2]};
  int32_t c[3];
  knn_grid_cell3(g, p, c);
  const int32_t cn = knn_grid_cell_number(g, c);
  cell[i] = cn;
  atomicAdd(&counts[cn], 1);
  if (kmin) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const unsigned long long k = kg_key(p[a]);
      unsigned long long* mn = kmin + g.off[a] + c[a];
      unsigned long long* mx = kmax + g.off[a] + c[a];
      // (a stale read is only ever less extreme than the stored value: the atomic is skipped only where it is moot)
      if (k < __atomic_load_n(mn, __ATOMIC_RELAXED)) atomicMin(mn, k);
      if (k > __atomic_load_n(mx, __ATOMIC_RELAXED)) atomicMax(mx, k);
    }
  }
}

template <int = 0>
__global__ __launch_bounds__(256) void k_kg_scatter(const double* __restrict__ P, int32_t n, const int32_t* __restrict__ cell,
                                                     int32_t* __restrict__ cursor, KgPoint* __restrict__ out) {
  const int32_t i = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  if (i >= n) return;
  const int32_t at = atomicAdd(&cursor[cell[i]], 1);
  if (at < 0 || at >= n) return;  // (cannot happen: the cursors start at a scan of these very counts)
  KgPoint p;
  p.x = P[static_cast<int64_t>(i) * 3];
  p.y = P[static_cast<int64_t>(i) * 3 + 1];
  p.z = P[static_cast<int64_t>(i) * 3 + 2];
  p.idx = i;
  p.pad = 0;
  out[at] = p;
}

// workgroup 2 a: smin of axis a (suffix minimum of kmin), workgroup 2 a + 1: pmax of axis a (prefix maximum of kmax)
template <int = 0>
__global__ __launch_bounds__(256) void k_kg_slabs(KnnGrid g, const unsigned long long* __restrict__ kmin,
                                                   const unsigned long long* __restrict__ kmax, double* __restrict__ smin,
                                                   double* __restrict__ pmax) {
  __shared__ unsigned long long wsum[4];
  const int a = static_cast<int>(blockIdx.x) >> 1;
  const bool suffix = (blockIdx.x & 1) == 0;
  const int32_t n = g.dim[a], off = g.off[a], t = static_cast<int32_t>(threadIdx.x);
  const unsigned long long* in = (suffix ? kmin : kmax) + off;
  double* out = (suffix ? smin : pmax) + off;
  const unsigned long long unit = suffix ? ~0ull : 0ull;
  auto op = [&](unsigned long long x, unsigned long long y) { return suffix ? (x < y ? x : y) : (x > y ? x : y); };
  auto at = [&](int32_t i) { return suffix ? n - 1 - i : i; };  // the suffix scan runs over the reversed table
  const int32_t len = (n + 255) / 256;
  const int64_t b64 = static_cast<int64_t>(t) * len;
  const int32_t b = b64 < n ? static_cast<int32_t>(b64) : n, e = b64 + len < n ? static_cast<int32_t>(b64 + len) : n;
  unsigned long long s = unit;
  for (int32_t i = b; i < e; ++i) s = op(s, in[at(i)]);
  unsigned long long run = block_scan_excl<4>(s, wsum, op, unit);  // the stretches in front of this thread's
  for (int32_t i = b; i < e; ++i) {
    run = op(run, in[at(i)]);
    out[at(i)] = kg_unkey(run);
  }
}

// Q: the queries in the cell order of the searched grid (Q == S for a cloud searched in itself); S: the searched cloud
// in cell order, start[c]..start[c + 1] the points of cell c. od / oi: n0 x K row-major, row = the query's original index.
template <int K>
__global__ __launch_bounds__(256) void k_knn_grid(const KgPoint* __restrict__ Q, int32_t n0, const KgPoint* __restrict__ S,
                                                   int32_t n1, const int32_t* __restrict__ start, KnnGrid g,
                                                   const double* __restrict__ smin, const double* __restrict__ pmax,
                                                   double* __restrict__ od, int32_t* __restrict__ oi,
                                                   int32_t* __restrict__ visited) {
  const int32_t i = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  if (i >= n0) return;
  const KgPoint me = Q[i];
  if (me.idx < 0 || me.idx >= n0) return;  // (cannot happen: the scatter wrote every row)
  const double q[3] = {me.x, me.y, me.z};
  double bd[K];
  int32_t bi[K];
  knn_grid_clear(bd, bi);
  const int64_t seen = knn_grid_query<K>(
      g, q, n1, smin, pmax, bd, bi,
      [&](int32_t first, int32_t last, int32_t& t, int32_t& e) {
        t = start[first];
        e = start[last + 1];
        t = t > 0 ? t : 0;
        e = e < n1 ? e : n1;
      },
      [&](int32_t t) {
        const KgPoint c = S[t];
        const double p[3] = {c.x, c.y, c.z};
        knn_grid_insert<K>(bd, bi, knn_grid_sqdist(q, p), c.idx);
      });
  const int64_t o = static_cast<int64_t>(me.idx) * K;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    od[o + k] = bd[k];
    oi[o + k] = bi[k];
  }
  visited[me.idx] = static_cast<int32_t>(seen);
}

template <int = 0>
__global__ __launch_bounds__(256) void k_kg_sum(const int32_t* __restrict__ v, int64_t n, unsigned long long* __restrict__ sum) {
  __shared__ unsigned long long red[4];
  unsigned long long s = 0;
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n; i += static_cast<int64_t>(gridDim.x) * 256)
    s += static_cast<unsigned long long>(v[i]);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(sum, red[0] + red[1] + red[2] + red[3]);
}

}  // namespace clipper_hip
