// k_voxel.hip.h — voxel down-sampling of a point cloud ("Voxel down-sampling"): one output row
// per occupied voxel, in ascending cell number, bit for bit the numpy model's. Part of kernels.hip.h (include that
// one): hand-written gfx950 device code. The rules (voxel of a point, cell number, order of addition, centroid,
// normal) are voxel_rules.hpp's, the sort k_sort.hip.h's; here is which work item holds what.
//
//   k_vx_keys      thread = point: (cell number, original index). The indices ascend, and the sort is stable: behind
//                  it the members of a voxel stand in ascending original index.
//   k_vx_heads     workgroup = tile of the sorted pairs: how many of them differ from their predecessor (the heads)
//   (k_row_scan    over the tiles' head counts: the first output row of each tile, and n_out behind the last)
//   k_vx_rows      workgroup = tile: the output row of every sorted position (the heads before it, itself included,
//                  less one), the first position of every row (start[row], and start[n_out] = n), and the trace
//   k_vx_partials  thread = sorted position: the first member of a chunk of a voxel with more than VOXEL_CHUNK
//                  members adds up its chunk. So the chunks of a crowded voxel are summed by different threads of
//                  different waves, and a launch is never longer than one chunk. Two voxels' chunks can begin in one
//                  window of VOXEL_CHUNK positions, and no more (see vx_partial_slot): the partials need 2 slots per
//                  window, not one per row.
//   k_vx_reduce    thread = output row: a voxel of up to VOXEL_CHUNK members is added up here, a longer one from its
//                  partials in chunk order; centroid, normal, count, and the largest count (an integer maximum)
// No floating-point atomics anywhere; every loop is bounded by VOXEL_CHUNK or by n / VOXEL_CHUNK.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_sort.hip.h"
#include "voxel_rules.hpp"

namespace clipper_hip {

// Where the partial sum of the chunk that begins at sorted position i goes (first: i is its voxel's first position).
// Only voxels longer than VOXEL_CHUNK have partials. Such a voxel covers more than a whole window's worth of
// positions, so two of them cannot both begin in one window, and two chunks that both continue a voxel
// (i = start + j * VOXEL_CHUNK, j >= 1, the voxel covering [i - VOXEL_CHUNK, i]) cannot lie in one window unless
// they are of the same voxel, whose chunks lie VOXEL_CHUNK apart: at most one of either kind per window.
__host__ __device__ inline int64_t vx_partial_slot(int64_t i, bool first) { return 2 * (i / VOXEL_CHUNK) + (first ? 1 : 0); }
__host__ __device__ inline int64_t vx_partial_slots(int64_t n) { return 2 * ((n + VOXEL_CHUNK - 1) / VOXEL_CHUNK) + 2; }

template <int = 0>
__global__ __launch_bounds__(256) void k_vx_keys(const double* __restrict__ P, int32_t n, VoxelGrid g,
                                                  unsigned long long* __restrict__ keys, int32_t* __restrict__ idx) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const double p[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
  keys[i] = voxel_key(g, p);
  idx[i] = static_cast<int32_t>(i);
}

// is sorted position i the first of its voxel
__device__ inline bool vx_head(const unsigned long long* __restrict__ keys, int64_t i) {
  return i == 0 || keys[i] != keys[i - 1];
}

template <int = 0>
__global__ __launch_bounds__(SORT_THREADS) void k_vx_heads(const unsigned long long* __restrict__ keys, int32_t n,
                                                            int32_t* __restrict__ tile_heads) {
  __shared__ int32_t total;
  const int t = static_cast<int>(threadIdx.x);
  if (t == 0) total = 0;
  __syncthreads();
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * SORT_TILE + t;
  int32_t mine = 0;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t i = i0 + r * SORT_THREADS;
    const bool head = i < n && vx_head(keys, i);
    mine += __popcll(__ballot(head));  // (the same number on every lane of the wave)
  }
  if ((t & 63) == 0) atomicAdd(&total, mine);
  __syncthreads();
  if (t == 0) tile_heads[blockIdx.x] = total;
}

// tile_first: the scan of tile_heads. trace may be null.
template <int = 0>
__global__ __launch_bounds__(SORT_THREADS) void k_vx_rows(const unsigned long long* __restrict__ keys,
                                                           const int32_t* __restrict__ idx, int32_t n,
                                                           const int32_t* __restrict__ tile_first, int32_t* __restrict__ row,
                                                           int32_t* __restrict__ start, int32_t* __restrict__ trace) {
  __shared__ int32_t wc[SORT_ROUNDS][SORT_WAVES];  // heads per round and wave
  const int t = static_cast<int>(threadIdx.x), wave = t >> 6, lane = t & 63;
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * SORT_TILE + t;
  unsigned long long bal[SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t i = i0 + r * SORT_THREADS;
    bal[r] = __ballot(i < n && vx_head(keys, i));
    if (lane == 0) wc[r][wave] = __popcll(bal[r]);
  }
  __syncthreads();
  int32_t run = tile_first[blockIdx.x];  // heads before this tile
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
      const int32_t c = wc[r][w];
      before += w < wave ? c : 0;
      all += c;
    }
    const int64_t i = i0 + r * SORT_THREADS;
    // the heads up to and including this position, less one
    const int32_t at = run + before + __popcll(bal[r] & ((sort_lanes_below(lane) << 1) | 1ull)) - 1;
    run += all;
    if (i < n && at >= 0 && at < n) {
      row[i] = at;
      if ((bal[r] >> lane) & 1ull) start[at] = static_cast<int32_t>(i);
      if (i == n - 1) start[at + 1] = n;
      if (trace) {
        const int32_t o = idx[i];
        if (o >= 0 && o < n) trace[o] = at;
      }
    }
  }
}

// the three numbers of a voxel's member at sorted position k: x - lo, or the normal
struct VxPointGet {
  const double* __restrict__ P;
  const int32_t* __restrict__ idx;
  double lo0, lo1, lo2;
  __host__ __device__ void operator()(int64_t k, double (&v)[3]) const {
    const int64_t o = idx[k];
    v[0] = P[o * 3] - lo0;
    v[1] = P[o * 3 + 1] - lo1;
    v[2] = P[o * 3 + 2] - lo2;
  }
};
struct VxNormalGet {
  const double* __restrict__ N;
  const int32_t* __restrict__ idx;
  __host__ __device__ void operator()(int64_t k, double (&v)[3]) const {
    const int64_t o = idx[k];
    v[0] = N[o * 3];
    v[1] = N[o * 3 + 1];
    v[2] = N[o * 3 + 2];
  }
};

// part: vx_partial_slots(n) slots of 6 doubles (point sum, normal sum). N may be null.
template <int = 0>
__global__ __launch_bounds__(256) void k_vx_partials(const double* __restrict__ P, const double* __restrict__ N, int32_t n,
                                                      VoxelGrid g, const int32_t* __restrict__ idx,
                                                      const int32_t* __restrict__ row, const int32_t* __restrict__ start,
                                                      double* __restrict__ part) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t r = row[i];
  if (r < 0 || r >= n) return;
  const int64_t s = start[r], e = start[r + 1];
  if (s < 0 || e > n || i < s || i >= e) return;  // (cannot happen: row and start describe the same segments)
  if (e - s <= VOXEL_CHUNK || (i - s) % VOXEL_CHUNK != 0) return;
  const int64_t end = i + VOXEL_CHUNK < e ? i + VOXEL_CHUNK : e;
  double* out = part + vx_partial_slot(i, i == s) * 6;
  double sum[3];
  voxel_chunk_sum(i, end, VxPointGet{P, idx, g.lo[0], g.lo[1], g.lo[2]}, sum);
  out[0] = sum[0];
  out[1] = sum[1];
  out[2] = sum[2];
  if (N) {
    voxel_chunk_sum(i, end, VxNormalGet{N, idx}, sum);
    out[3] = sum[0];
    out[4] = sum[1];
    out[5] = sum[2];
  }
}

// n_out: on the device (behind the scan of the tiles' head counts). P_out / N_out / count_out hold n rows.
template <int = 0>
__global__ __launch_bounds__(256) void k_vx_reduce(const double* __restrict__ P, const double* __restrict__ N, int32_t n,
                                                    VoxelGrid g, const int32_t* __restrict__ idx,
                                                    const int32_t* __restrict__ n_out, const int32_t* __restrict__ start,
                                                    const double* __restrict__ part, double* __restrict__ P_out,
                                                    double* __restrict__ N_out, int32_t* __restrict__ count_out,
                                                    int32_t* max_count) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int32_t rows = *n_out;
  if (r >= rows || r >= n) return;
  const int64_t s = start[r], e = start[r + 1];
  if (s < 0 || e > n || e <= s) return;  // (cannot happen)
  const int64_t count = e - s, chunks = voxel_chunks(count);
  double tot[3] = {0.0, 0.0, 0.0}, ntot[3] = {0.0, 0.0, 0.0}, sum[3];
  if (chunks == 1) {
    voxel_chunk_sum(s, e, VxPointGet{P, idx, g.lo[0], g.lo[1], g.lo[2]}, sum);
    voxel_add_chunk(tot, sum);
    if (N) {
      voxel_chunk_sum(s, e, VxNormalGet{N, idx}, sum);
      voxel_add_chunk(ntot, sum);
    }
  } else {
    for (int64_t j = 0; j < chunks; ++j) {
      const double* in = part + vx_partial_slot(s + j * VOXEL_CHUNK, j == 0) * 6;
      sum[0] = in[0];
      sum[1] = in[1];
      sum[2] = in[2];
      voxel_add_chunk(tot, sum);
      if (N) {
        sum[0] = in[3];
        sum[1] = in[4];
        sum[2] = in[5];
        voxel_add_chunk(ntot, sum);
      }
    }
  }
  double c[3];
  voxel_centroid(g, tot, static_cast<int32_t>(count), c);
  P_out[r * 3] = c[0];
  P_out[r * 3 + 1] = c[1];
  P_out[r * 3 + 2] = c[2];
  if (N) {
    double nv[3];
    voxel_normal(ntot, nv);
    N_out[r * 3] = nv[0];
    N_out[r * 3 + 1] = nv[1];
    N_out[r * 3 + 2] = nv[2];
  }
  count_out[r] = static_cast<int32_t>(count);
  // (a stale read is only ever smaller than the stored value: the atomic is skipped only where it is moot)
  const int32_t cnt = static_cast<int32_t>(count);
  if (cnt > __atomic_load_n(max_count, __ATOMIC_RELAXED)) atomicMax(max_count, cnt);
}

}  // namespace clipper_hip
