// k_sort.hip.h — a stable LSD radix sort of (u64 key, i32 index) pairs on the device, 8-bit digits (DESIGN.md section
// 9, "Voxel down-sampling"). Part of kernels.hip.h (include that one): hand-written gfx950 device code. The digit and
// the number of passes are voxel_rules.hpp's; here is which work item holds what.
//
// A pass over digit p of n pairs, cut into tiles of SORT_TILE consecutive pairs:
//   k_sort_hist     workgroup = tile: a 256-entry histogram of the tile's digits in LDS (integer atomics: a count does
//                   not depend on arrival order), written to table[digit][tile] and added to the pass's 256 totals
//   k_row_scan      (k_wave.hip.h) workgroup = digit: exclusive scan of the digit's row of the table: entry
//                   (d, t) becomes the number of pairs with digit d in the tiles before t. The 256 rows are scanned
//                   side by side; what joins them, the scan of the 256 totals, every scatter workgroup does for
//                   itself (block_scan_excl). So the first output place of tile t's pairs with digit d is
//                   (pairs with a smaller digit) + (pairs with digit d in earlier tiles).
//   k_sort_scatter  workgroup = tile: every pair to its place. The tile is striped over the workgroup, round r holds
//                   pairs r * 256 .. r * 256 + 255 in thread order, and the rounds are ranked one after the other with a
//                   per-digit running count, so equal digits keep their input order: inside a wave by the rank among
//                   the lower lanes of the peer mask (wave64 has no match-any: the mask is built from eight 64-bit
//                   ballots, one per bit of the digit), across the four waves of a round by the waves' digit counts
//                   in LDS, across rounds by the running count, across tiles by the scanned table.
// One kernel per step: no workgroup waits for another. Every loop is bounded by a constant or an integer of n. A
// computed place outside [0, n) is not stored to (it cannot happen: the places are a scan of these very counts).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_wave.hip.h"
#include "voxel_rules.hpp"

namespace clipper_hip {

constexpr int SORT_THREADS = 256;                       // a workgroup of the tile kernels: four waves
constexpr int SORT_ROUNDS = 8;                          // pairs per thread
constexpr int SORT_TILE = SORT_THREADS * SORT_ROUNDS;   // pairs per tile (reported in clipper_voxel_info_t.sort_tile)
constexpr int SORT_WAVES = SORT_THREADS / 64;

// the lanes of this wave whose digit equals this lane's, among the lanes with `valid` set (garbage on the others)
__device__ inline unsigned long long sort_peers(uint32_t digit, bool valid) {
  unsigned long long mask = __ballot(valid);
#pragma unroll
  for (int b = 0; b < SORT_DIGIT_BITS; ++b) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long bal = __ballot(valid && bit);
    mask &= bit ? bal : ~bal;
  }
  return mask;
}

// the lanes below this one
__device__ inline unsigned long long sort_lanes_below(int lane) { return (1ull << lane) - 1ull; }

template <int = 0>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_hist(const unsigned long long* __restrict__ keys, int32_t n, int pass,
                                                             int32_t ntiles, int32_t* __restrict__ table,
                                                             int32_t* __restrict__ totals) {
  __shared__ int32_t hist[SORT_RADIX];
  const int t = static_cast<int>(threadIdx.x);
  const int32_t tile = static_cast<int32_t>(blockIdx.x);
  hist[t] = 0;
  __syncthreads();
  const int64_t i0 = static_cast<int64_t>(tile) * SORT_TILE + t;
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t i = i0 + r * SORT_THREADS;
    if (i < n) atomicAdd(&hist[sort_digit(keys[i], pass)], 1);
  }
  __syncthreads();
  if (tile < ntiles) table[static_cast<int64_t>(t) * ntiles + tile] = hist[t];
  if (hist[t]) atomicAdd(&totals[t], hist[t]);
}

template <int = 0>
__global__ __launch_bounds__(SORT_THREADS) void k_sort_scatter(const unsigned long long* __restrict__ keys,
                                                                const int32_t* __restrict__ idx, int32_t n, int pass,
                                                                int32_t ntiles, const int32_t* __restrict__ first,
                                                                const int32_t* __restrict__ totals,
                                                                unsigned long long* __restrict__ keys_out,
                                                                int32_t* __restrict__ idx_out) {
  __shared__ int32_t base[SORT_RADIX];             // the next free place of a digit's pairs of this tile
  __shared__ int32_t wcnt[SORT_WAVES][SORT_RADIX];  // pairs of the current round per wave and digit
  const int t = static_cast<int>(threadIdx.x), wave = t >> 6, lane = t & 63;
  const int32_t tile = static_cast<int32_t>(blockIdx.x);
  // the thread's pairs, all loads in flight before anything waits
  const int64_t i0 = static_cast<int64_t>(tile) * SORT_TILE + t;
  unsigned long long k[SORT_ROUNDS];
  int32_t v[SORT_ROUNDS];
#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const int64_t i = i0 + r * SORT_THREADS;
    k[r] = i < n ? keys[i] : 0ull;
    v[r] = i < n ? idx[i] : 0;
  }
#pragma unroll
  for (int w = 0; w < SORT_WAVES; ++w) wcnt[w][t] = 0;
  // thread = digit: the pairs with a smaller digit (a scan of the 256 totals; base's first words are its scratch),
  // then those in earlier tiles
  const int32_t below = block_scan_excl<SORT_WAVES>(totals[t], base);
  __syncthreads();
  base[t] = below + first[static_cast<int64_t>(t) * ntiles + tile];
  __syncthreads();

#pragma unroll
  for (int r = 0; r < SORT_ROUNDS; ++r) {
    const bool valid = i0 + r * SORT_THREADS < n;
    const uint32_t d = sort_digit(k[r], pass);
    const unsigned long long peers = sort_peers(d, valid);
    const int rank = __popcll(peers & sort_lanes_below(lane));
    if (valid && rank == 0) wcnt[wave][d] = __popcll(peers);  // the lowest peer speaks for all of them
    __syncthreads();
    int32_t at = -1;
    if (valid) {
      at = base[d] + rank;
      for (int w = 0; w < wave; ++w) at += wcnt[w][d];
    }
    __syncthreads();
    {  // thread = digit: the round's pairs are behind the running count, the wave counts are zero again
      int32_t sum = 0;
#pragma unroll
      for (int w = 0; w < SORT_WAVES; ++w) {
        sum += wcnt[w][t];
        wcnt[w][t] = 0;
      }
      base[t] += sum;
    }
    __syncthreads();
    if (valid && at >= 0 && at < n) {
      keys_out[at] = k[r];
      idx_out[at] = v[r];
    }
  }
}

}  // namespace clipper_hip
