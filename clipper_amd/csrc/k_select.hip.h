// k_select.hip.h — the exact rank select behind trimmed ICP ("Robust losses and trimmed ICP"): the
// keep-th smallest squared distance among the source points within max_distance, as a most-significant-digit-first
// radix select over the 64 bits of sqd. Part of kernels.hip.h (include that one): hand-written gfx950 device code. The
// digit of a key, which keys are still candidates and which digit holds the rank are icp_rules.hpp's; here is which
// work item holds what. Two kernels per digit, ICP_SELECT_PASSES digits:
//   k_select_hist   workgroup = a tile of SELECT_TILE source points, striped over the workgroup in SELECT_ROUNDS rounds.
//                   A candidate is a point whose list entry is an inlier and whose higher digits equal the prefix found
//                   so far (read from the control block). Candidates within max_distance share their upper digits, so
//                   whole waves hit one bin: the equal-digit lanes of a wave are found with ballots (k_sort.hip.h's
//                   sort_peers) and the lowest of them adds their number to the LDS histogram with one integer atomic;
//                   the tile's histogram then goes to the pass's totals with integer atomics. A count does not depend
//                   on arrival order.
//   k_select_pick   one workgroup, thread = digit: the exclusive scan of the totals (k_wave.hip.h's block_scan_excl),
//                   icp_select_hit of every digit at once: the one that answers writes the new prefix and rank; pass 0
//                   also takes within (the sum of the totals) and keep; the last pass writes tau. The totals are zero
//                   again for the next pass.
// One kernel per step: no workgroup waits for another. Every loop is bounded by a constant. Nothing here is read by
// the host during an iteration: the weighted sums (k_icp.hip.h) read tau from the control block.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_rules.hpp"
#include "k_sort.hip.h"
#include "k_wave.hip.h"

namespace clipper_hip {

constexpr int SELECT_THREADS = 256;
constexpr int SELECT_ROUNDS = 8;                              // source points per thread
constexpr int SELECT_TILE = SELECT_THREADS * SELECT_ROUNDS;   // source points per workgroup of k_select_hist
static_assert(ICP_SELECT_RADIX == SELECT_THREADS, "k_select_pick: one thread per digit");
static_assert(ICP_SELECT_BITS == SORT_DIGIT_BITS, "sort_peers compares SORT_DIGIT_BITS bits of a digit");

// oi / od: the K = 1 lists (n entries); totals: ICP_SELECT_RADIX counts, zero on entry of a pass
template <int = 0>
__global__ __launch_bounds__(SELECT_THREADS) void k_select_hist(const int32_t* __restrict__ oi, const double* __restrict__ od,
                                                                 int32_t n, double d2, int pass,
                                                                 const IcpSelect* __restrict__ ctl,
                                                                 uint32_t* __restrict__ totals) {
  __shared__ uint32_t hist[ICP_SELECT_RADIX];
  const int t = static_cast<int>(threadIdx.x), lane = t & 63;
  const uint64_t prefix = ctl->prefix;
  if (pass > 0 && ctl->any == 0) return;  // (nothing is kept: uniform over the grid)
  hist[t] = 0;
  __syncthreads();
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * SELECT_TILE + t;
#pragma unroll
  for (int r = 0; r < SELECT_ROUNDS; ++r) {
    const int64_t i = i0 + r * SELECT_THREADS;
    bool valid = false;
    uint32_t digit = 0;
    if (i < n) {
      const double sqd = od[i];
      const uint64_t key = static_cast<uint64_t>(__double_as_longlong(sqd));
      valid = icp_inlier(oi[i], sqd, d2) && icp_select_candidate(key, prefix, pass);
      digit = icp_select_digit(key, pass);
    }
    const unsigned long long peers = sort_peers(digit, valid);
    if (valid && (peers & sort_lanes_below(lane)) == 0) atomicAdd(&hist[digit], static_cast<uint32_t>(__popcll(peers)));
  }
  __syncthreads();
  if (hist[t]) atomicAdd(&totals[t], hist[t]);
}

template <int = 0>
__global__ __launch_bounds__(SELECT_THREADS) void k_select_pick(uint32_t* __restrict__ totals, int pass, double trim,
                                                                 IcpSelect* __restrict__ ctl) {
  __shared__ int64_t wsum[SELECT_THREADS / 64];
  __shared__ int64_t total;
  const int t = static_cast<int>(threadIdx.x);
  const int64_t h = static_cast<int64_t>(totals[t]);
  totals[t] = 0;
  // the block as the pass found it, read by every thread before the barrier of the scan; written behind it
  const uint64_t prefix = pass == 0 ? 0 : ctl->prefix;
  int64_t rank = ctl->rank;
  int32_t any = ctl->any;
  const int64_t before = block_scan_excl<SELECT_THREADS / 64>(h, wsum);
  if (pass == 0) {
    if (t == SELECT_THREADS - 1) total = before + h;
    __syncthreads();
    const int64_t within = total;
    rank = icp_trim_keep(trim, within);
    any = rank > 0 ? 1 : 0;
    if (t == 0) {
      ctl->within = within;
      ctl->keep = rank;
      ctl->any = any;
      if (!any) {
        ctl->prefix = 0;
        ctl->rank = 0;
        ctl->tau = 0.0;
      }
    }
  }
  if (any && icp_select_hit(before, h, rank)) {  // (one thread)
    const uint64_t next = (prefix << ICP_SELECT_BITS) | static_cast<uint64_t>(t);
    ctl->prefix = next;
    ctl->rank = rank - before;
    if (pass == ICP_SELECT_PASSES - 1) ctl->tau = __longlong_as_double(static_cast<long long>(next));
  }
}

}  // namespace clipper_hip
