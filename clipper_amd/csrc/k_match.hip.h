// k_match.hip.h — brute-force k-nearest-neighbour search in DESCRIPTOR space (1 <= d <= 64): the feature-matching
// step in front of the path (FPFH 33, FCGF / SpinNet / Predator 32 numbers per point).
// Part of kernels.hip.h (include that one): hand-written gfx950 device code.
//
// The contract is k_knn.hip.h's, which makes the lists testable to the last bit: fp64,
// dist = dist + (q[k] - p[k]) * (q[k] - p[k]) for k = 0 .. d-1 in coordinate order from 0.0, nothing fused; lists
// ascending by (distance, index); index -1 / distance KNN_INF where the other cloud has fewer than K points. No matrix
// cores: the |a|^2 + |b|^2 - 2ab form does not give those bits.
//   k_match_partial<K, G>  grid (ceil(n0/256), S): thread = one query, its 8 G coordinates and its K best in registers;
//                          workgroup = one chunk of the other cloud; every lane looks at the same candidate at the same
//                          time, so a candidate comes through the constant address space as SCALAR loads — not whole
//                          (64 doubles = 128 SGPRs, a wave has 102) but group by group: 8 doubles = 16 SGPRs for each of
//                          MATCH_UNR candidates, whose distances are carried across the groups in MATCH_UNR VGPR pairs.
//                          The additions of one candidate therefore stay in coordinate order.
//   k_knn_merge<K>         (k_knn.hip.h) folds the S partial lists of a query in chunk order
//   k_match_pad            the zero padding of the rows on the device (descriptors that are there already: a cloud's)
//   k_match_select<EMIT>   the filters on the device (match_rules.hpp, the host's own rules): thread = one query; EMIT = 0
//                          counts its kept entries, k_row_scan (k_wave.hip.h) turns the counts into offsets, EMIT = 1
//                          writes the rows at them: i ascending, then k ascending, as clipper_match::select
// Rows are PADDED WITH ZEROS to 8 G coordinates (by the host, before the copy): (0 - 0)^2 = 0 added to a non-negative
// partial sum is exact, so the padding changes no bit, and for the same reason a narrower descriptor may run through a
// wider instantiation. Instantiated: G in {1, 2, 4, 5, 8} x K in {1, 2, 4, 8} — d <= 8 (coordinates; one group), d <= 16,
// d <= 32 (FCGF, SpinNet, Predator), d <= 40 (FPFH 33) and d <= 64. G = 3 rounds up to 4 and G = 6, 7 to 8: no descriptor
// in use has those widths, and each instantiation is an unrolled body of 8 G x MATCH_UNR pair terms in the code object.
// An LDS-tiled variant with broadcast reads was not built: see DESIGN.md 9, "Matching descriptors".
// Measured (MI355X, hipEvents around partial + merge, K = 1; tools/match_probe.py): 10k x 10k: 151 us (d = 3), 640 us
// (d = 33), 1.05 ms (d = 64); 100k x 100k: 11.4 ms, 56.4 ms, 91.5 ms = 8.7e11, 1.8e11, 1.1e11 pairs/s. At d = 3 that is
// 2.1-2.2x k_knn_partial<1, 3> on the same clouds, for 8/3 of its coordinates.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_knn.hip.h"
#include "match_rules.hpp"

namespace clipper_hip {

constexpr int MATCH_GROUP = 8;   // coordinates per group of scalar loads (16 SGPRs)
constexpr int MATCH_UNR = 4;     // candidates per batch: 4 x 16 = 64 SGPRs in flight
constexpr int MATCH_DMAX = 64;   // coordinates per descriptor

template <int K, int G>
__global__ __launch_bounds__(256) void k_match_partial(const double* __restrict__ F0, int64_t n0,
                                                        const double* __restrict__ F1, int64_t n1,
                                                        int64_t chunk, double* __restrict__ pd,
                                                        int32_t* __restrict__ pi) {
  constexpr int D = MATCH_GROUP * G;  // padded row length of both sets
  typedef const __attribute__((address_space(4))) double* cptr;
  const cptr Q1 = (cptr)F1;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t j0 = static_cast<int64_t>(blockIdx.y) * chunk;
  const int64_t j1 = (j0 + chunk < n1) ? j0 + chunk : n1;
  // a lane past the end reads the last query (and stores nothing): a select per element would put a branch and a
  // wait around each of the 8 G loads
  const int64_t iq = (i < n0) ? i : n0 - 1;
  double q[D];
#pragma unroll
  for (int k = 0; k < D; ++k) q[k] = F0[iq * D + k];
  double bd[K];
  int32_t bi[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {  // (not knn_grid_clear: through the call the insertions below compile to branches, not selects)
    bd[k] = KNN_INF;
    bi[k] = -1;
  }
  // equal distances keep the earlier (lower) index
  auto insert = [&](int64_t t, double dist) { knn_insert_first<K>(bd, bi, dist, static_cast<int32_t>(t)); };
  int64_t t = j0;
  for (; t + MATCH_UNR <= j1; t += MATCH_UNR) {
    double dist[MATCH_UNR];
#pragma unroll
    for (int u = 0; u < MATCH_UNR; ++u) dist[u] = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double p[MATCH_UNR][MATCH_GROUP];
#pragma unroll
      for (int u = 0; u < MATCH_UNR; ++u)
#pragma unroll
        for (int k = 0; k < MATCH_GROUP; ++k) p[u][k] = Q1[(t + u) * D + g * MATCH_GROUP + k];
#pragma unroll
      for (int u = 0; u < MATCH_UNR; ++u)
#pragma unroll
        for (int k = 0; k < MATCH_GROUP; ++k) {
          const double df = q[g * MATCH_GROUP + k] - p[u][k];
          dist[u] = dist[u] + df * df;
        }
      // the loads of the next group stay behind this group's arithmetic: hoisted, the groups of a wide descriptor
      // overrun the SGPR file together and the batch spills into VGPR lanes (348 spilled SGPRs at G = 8, K = 8)
      __builtin_amdgcn_sched_barrier(0);
    }
    // all MATCH_UNR distances are complete here: left alone, the compiler sinks the arithmetic of the later candidates
    // below the (divergent) insertion of the earlier ones and keeps their coordinates alive in VGPR lanes until then
#pragma unroll
    for (int u = 0; u < MATCH_UNR; ++u) asm volatile("" : "+v"(dist[u]));
#pragma unroll
    for (int u = 0; u < MATCH_UNR; ++u) insert(t + u, dist[u]);
  }
  for (; t < j1; ++t) {
    double dist = 0.0;
#pragma unroll
    for (int g = 0; g < G; ++g) {
      double p[MATCH_GROUP];
#pragma unroll
      for (int k = 0; k < MATCH_GROUP; ++k) p[k] = Q1[t * D + g * MATCH_GROUP + k];
#pragma unroll
      for (int k = 0; k < MATCH_GROUP; ++k) {
        const double df = q[g * MATCH_GROUP + k] - p[k];
        dist = dist + df * df;
      }
      __builtin_amdgcn_sched_barrier(0);  // as above: one group of a candidate in SGPRs at a time
    }
    insert(t, dist);
  }
  if (i < n0) {
    const int64_t o = (static_cast<int64_t>(blockIdx.y) * n0 + i) * K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      pd[o + k] = bd[k];
      pi[o + k] = bi[k];
    }
  }
}

// out: n x dp, row p = the d numbers of row p of F (n x d), then zeros. Thread = one number of out.
template <int = 0>
__global__ __launch_bounds__(256) void k_match_pad(const double* __restrict__ F, int64_t n, int d, int dp,
                                                    double* __restrict__ out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= n * dp) return;
  const int64_t p = e / dp;
  const int k = static_cast<int>(e - p * dp);
  out[e] = k < d ? F[p * d + k] : 0.0;
}

// The filters. fi / fd: the forward lists, n0 x fstride; bi: the backward lists' indices, n1 x bstride (read only with
// prm.mutual). EMIT = 0: cnt[i] = kept entries of query i. EMIT = 1: off[i] = the first row of query i (the exclusive
// scan of cnt); rows (i, nn_k(i)) go to A (column-major m x 2) and sqd from there on, k ascending.
template <int EMIT>
__global__ __launch_bounds__(256) void k_match_select(clipper_match::Params prm, const int32_t* __restrict__ fi,
                                                       const double* __restrict__ fd, int64_t n0, int fstride,
                                                       const int32_t* __restrict__ bi, int bstride,
                                                       int32_t* __restrict__ cnt, const int32_t* __restrict__ off,
                                                       int64_t m, int32_t* __restrict__ A, double* __restrict__ sqd) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n0) return;
  const int32_t* nn = fi + i * fstride;
  const double* sd = fd + i * fstride;
  int32_t kept = 0;
  if (clipper_match::query_passes(prm, nn, sd)) {
    const int64_t r0 = EMIT ? off[i] : 0;
    for (int k = 0; k < prm.knn; ++k) {
      if (!clipper_match::entry_kept(prm, i, k, nn, sd, bi, bstride)) continue;
      if (EMIT) {
        const int64_t r = r0 + kept;
        if (r < m) {  // (always: m is the scan's total)
          A[r] = static_cast<int32_t>(i);
          A[m + r] = nn[k];
          sqd[r] = sd[k];
        }
      }
      ++kept;
    }
  }
  if (!EMIT) cnt[i] = kept;
}

}  // namespace clipper_hip
