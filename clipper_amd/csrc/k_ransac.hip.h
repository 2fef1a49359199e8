// k_ransac.hip.h — the device side of RANSAC over putative associations ("RANSAC over putative
// associations"). Part of kernels.hip.h (include that one): hand-written gfx950 device code. The arithmetic is
// ransac_rules.hpp's; here is which work item holds what. One round is: hypotheses, compact, score, best.
//   k_ransac_gather         thread = one correspondence: its pair to the contiguous arrays P, B (3 x m each)
//   k_ransac_hypotheses<N>  thread = one hypothesis of the round: the sample, both checks and the fit in registers; the
//                           sample, T (12 doubles) and its rank among the workgroup's passing hypotheses (-1: no
//                           score) by k_wave.hip.h's workgroup scan; the workgroup's count
//   k_ransac_compact        one workgroup: the scan of the workgroups' counts, then the list of survivors in ascending
//                           h (no atomic append: the order is part of the tie rule), their counts zeroed
//   k_ransac_score          the hot path, S survivors x m correspondences: lane = one correspondence, its six doubles
//                           in registers for the whole kernel; the workgroup walks tiles of RANSAC_TILE survivors whose
//                           T it stages in LDS and reads with identical addresses (a broadcast); a ballot and a
//                           population count give a wave's count, the waves add into an LDS integer per survivor, one
//                           integer atomicAdd per survivor and workgroup goes to global. Grid: ceil(m / 256) x as many
//                           tile walkers as fill the chip; a walker strides over the tiles, so the grid needs no
//                           survivor count from the host and is never empty.
//   k_ransac_best           one workgroup: (count, -h) as one 64-bit key folded by wave_max, compared with the running
//                           best of the 64-byte record; the winner's T and sample go beside it
//   k_ransac_polish_init / k_ransac_terms / k_ransac_polish / k_ransac_mask
//                           the polish: ICP's 17 point-to-point sums over the inliers of the candidate (thread =
//                           correspondence k where ICP has source point k, icp_block_fold), one workgroup folding the
//                           partials as k_icp_step does and thread 0 taking ransac_polish_visit; the mask under the
//                           final T. The loop's state stays on the device: a finished loop makes the later launches
//                           return at once.
// Integer atomics only: every floating-point sum has one order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_icp.hip.h"
#include "k_wave.hip.h"
#include "ransac_rules.hpp"

namespace clipper_hip {

constexpr int RANSAC_TILE = 16;      // survivors per LDS tile of k_ransac_score
constexpr int RANSAC_T_DOUBLES = 12;  // a hypothesis's T as stored: entry (r, c) at c * 3 + r

template <int = 0>
__global__ __launch_bounds__(256) void k_ransac_gather(const double* __restrict__ D1, int32_t n1, const double* __restrict__ D2,
                                                        int32_t n2, const int32_t* __restrict__ A, int32_t m,
                                                        double* __restrict__ P, double* __restrict__ B) {
  const int32_t k = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  if (k >= m) return;
  const int32_t a = A[k], b = A[static_cast<int64_t>(m) + k];
  if (a < 0 || a >= n1 || b < 0 || b >= n2) return;  // (cannot happen: the rows have been checked)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    P[static_cast<int64_t>(k) * 3 + c] = D1[static_cast<int64_t>(a) * 3 + c];
    B[static_cast<int64_t>(k) * 3 + c] = D2[static_cast<int64_t>(b) * 3 + c];
  }
}

// Th: H x 12, samp: H x RANSAC_MAX_SAMPLE, rank: H, bcount: H / 256 (H = 256 gridDim.x hypotheses from h0 on)
template <int N>
__global__ __launch_bounds__(256) void k_ransac_hypotheses(const double* __restrict__ P, const double* __restrict__ B, int32_t m,
                                                            uint64_t seed, uint64_t h0, double s2, double* __restrict__ Th,
                                                            int32_t* __restrict__ samp, int32_t* __restrict__ rank,
                                                            int32_t* __restrict__ bcount) {
  __shared__ int32_t wsum[4];
  const int32_t g = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  int32_t s[N];
  double T[16];
  const bool pass = ransac_hypothesis<N>(
      seed, h0 + static_cast<uint64_t>(g), m, s2,
      [&](int32_t k, double (&p)[3], double (&b)[3]) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          p[a] = P[static_cast<int64_t>(k) * 3 + a];
          b[a] = B[static_cast<int64_t>(k) * 3 + a];
        }
      },
      s, T);
#pragma unroll
  for (int a = 0; a < N; ++a) samp[static_cast<int64_t>(g) * RANSAC_MAX_SAMPLE + a] = s[a];
#pragma unroll
  for (int a = N; a < RANSAC_MAX_SAMPLE; ++a) samp[static_cast<int64_t>(g) * RANSAC_MAX_SAMPLE + a] = -1;
  if (pass) {
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) Th[static_cast<int64_t>(g) * RANSAC_T_DOUBLES + c * 3 + r] = T[c * 4 + r];
  }
  const int32_t one = pass ? 1 : 0;
  const int32_t excl = block_scan_excl<4>(one, wsum);
  rank[g] = pass ? excl : -1;
  if (threadIdx.x == 255) bcount[blockIdx.x] = excl + one;
}

// nblk <= 256 workgroups' counts; list: H; counts: H; rec->survivors: the round's survivors
template <int = 0>
__global__ __launch_bounds__(256) void k_ransac_compact(const int32_t* __restrict__ rank, const int32_t* __restrict__ bcount,
                                                         int32_t nblk, int32_t* __restrict__ list, int32_t* __restrict__ counts,
                                                         RansacRecord* __restrict__ rec) {
  __shared__ int32_t wsum[4];
  __shared__ int32_t boff[257];
  const int32_t t = static_cast<int32_t>(threadIdx.x);
  const int32_t c = t < nblk ? bcount[t] : 0;
  const int32_t excl = block_scan_excl<4>(c, wsum);
  boff[t] = excl;
  if (t == 255) boff[256] = excl + c;
  __syncthreads();
  const int32_t total = boff[256];
  const int32_t H = nblk * 256;
  for (int32_t g = t; g < H; g += 256) {
    const int32_t r = rank[g];
    if (r >= 0) list[boff[g >> 8] + r] = g;
  }
  for (int32_t s = t; s < total; s += 256) counts[s] = 0;
  if (t == 0) rec->survivors = total;
}

// P, B: 3 x m; Th: the round's transforms; list: its survivors (rec->survivors of them); counts: one per survivor
template <int = 0>
__global__ __launch_bounds__(256) void k_ransac_score(const double* __restrict__ P, const double* __restrict__ B, int32_t m,
                                                       double d2, const double* __restrict__ Th, const int32_t* __restrict__ list,
                                                       const RansacRecord* __restrict__ rec, int32_t* __restrict__ counts) {
  __shared__ double Ts[RANSAC_TILE][RANSAC_T_DOUBLES];
  __shared__ int32_t cnt[RANSAC_TILE];
  const int32_t S = rec->survivors;
  const int32_t t = static_cast<int32_t>(threadIdx.x);
  const int32_t k = static_cast<int32_t>(blockIdx.x) * 256 + t;
  const bool have = k < m;
  double p[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
  if (have) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      p[a] = P[static_cast<int64_t>(k) * 3 + a];
      b[a] = B[static_cast<int64_t>(k) * 3 + a];
    }
  }
  const int32_t ntiles = (S + RANSAC_TILE - 1) / RANSAC_TILE;
  for (int32_t tile = static_cast<int32_t>(blockIdx.y); tile < ntiles; tile += static_cast<int32_t>(gridDim.y)) {
    const int32_t base = tile * RANSAC_TILE;
    const int32_t nin = S - base < RANSAC_TILE ? S - base : RANSAC_TILE;
    if (t < nin * RANSAC_T_DOUBLES) {
      const int32_t i = t / RANSAC_T_DOUBLES, a = t - i * RANSAC_T_DOUBLES;
      Ts[i][a] = Th[static_cast<int64_t>(list[base + i]) * RANSAC_T_DOUBLES + a];
    }
    if (t < RANSAC_TILE) cnt[t] = 0;
    __syncthreads();
    for (int32_t i = 0; i < nin; ++i) {
      double T[16], q[3];
#pragma unroll
      for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) T[c * 4 + r] = Ts[i][c * 3 + r];
      const bool in = have && ransac_inlier(ransac_sqd(T, p, b, q), d2);
      const unsigned long long vote = __ballot(in);
      if ((t & 63) == 0 && vote) atomicAdd(&cnt[i], static_cast<int32_t>(__popcll(vote)));
    }
    __syncthreads();
    if (t < nin && cnt[t]) atomicAdd(&counts[base + t], cnt[t]);
    __syncthreads();  // (the next tile overwrites Ts and cnt)
  }
}

// counts / list: the round's survivors; Th, samp: its hypotheses; H of them from h0 on
template <int = 0>
__global__ __launch_bounds__(256) void k_ransac_best(const int32_t* __restrict__ counts, const int32_t* __restrict__ list,
                                                      uint64_t h0, int32_t H, const double* __restrict__ Th,
                                                      const int32_t* __restrict__ samp, RansacRecord* __restrict__ rec,
                                                      RansacBest* __restrict__ best) {
  __shared__ long long wk[4];
  __shared__ int32_t Ssh;
  if (threadIdx.x == 0) Ssh = rec->survivors;
  __syncthreads();
  const int32_t S = Ssh;
  long long key = -1;
  for (int32_t s = static_cast<int32_t>(threadIdx.x); s < S; s += 256) {
    const long long k = ransac_key(counts[s], h0 + static_cast<uint64_t>(list[s]));
    key = k > key ? k : key;
  }
  key = wave_max(key);
  if ((threadIdx.x & 63) == 0) wk[threadIdx.x >> 6] = key;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int w = 1; w < 4; ++w) key = wk[w] > key ? wk[w] : key;
  RansacRecord r = *rec;
  if (key > r.best_key) {
    r.best_key = key;
    const int64_t g = ransac_key_h(key) - static_cast<int64_t>(h0);
    if (g >= 0 && g < H) {  // (always: the key is one of this round's)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) best->T[c * 4 + rr] = Th[g * RANSAC_T_DOUBLES + c * 3 + rr];
        best->T[c * 4 + 3] = c == 3 ? 1.0 : 0.0;
      }
#pragma unroll
      for (int a = 0; a < RANSAC_MAX_SAMPLE; ++a) best->sample[a] = samp[g * RANSAC_MAX_SAMPLE + a];
    }
  }
  r.checked += S;
  r.evaluated += H;
  r.round += 1;
  *rec = r;
}

// model != 0: the polish starts from the best hypothesis, else from the identity
template <int = 0>
__global__ __launch_bounds__(64) void k_ransac_polish_init(const RansacBest* __restrict__ best, int model,
                                                            RansacPolish* __restrict__ pol) {
  const int t = static_cast<int>(threadIdx.x);
  if (t < 16) {
    const double id = (t & 3) == (t >> 2) ? 1.0 : 0.0;
    pol->cand[t] = model ? best->T[t] : id;
    pol->T[t] = id;
  }
  if (t < ICP_POINT_TERMS) pol->S[t] = 0.0;
  if (t == 0) {
    pol->refined = 0;
    pol->done = 0;
  }
}

// part: gridDim.x x 17, the sums under pol->cand
template <int = 0>
__global__ __launch_bounds__(256) void k_ransac_terms(const double* __restrict__ P, const double* __restrict__ B, int32_t m,
                                                       double d2, double o0, double o1, double o2,
                                                       const RansacPolish* __restrict__ pol, double* __restrict__ part) {
  if (pol->done) return;  // (the same for every thread: nothing writes it while this kernel runs)
  const int32_t k = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  double t[ICP_POINT_TERMS];
#pragma unroll
  for (int a = 0; a < ICP_POINT_TERMS; ++a) t[a] = 0.0;
  if (k < m) {
    double T[16];
#pragma unroll
    for (int a = 0; a < 16; ++a) T[a] = pol->cand[a];
    const double o[3] = {o0, o1, o2};
    const double p[3] = {P[static_cast<int64_t>(k) * 3], P[static_cast<int64_t>(k) * 3 + 1], P[static_cast<int64_t>(k) * 3 + 2]};
    const double b[3] = {B[static_cast<int64_t>(k) * 3], B[static_cast<int64_t>(k) * 3 + 1], B[static_cast<int64_t>(k) * 3 + 2]};
    ransac_terms(T, p, b, d2, o, t);
  }
  icp_block_fold<ICP_POINT_TERMS>(t, part + static_cast<int64_t>(blockIdx.x) * ICP_POINT_TERMS);
}

// visit i of the polish: part (nb x 17) folded as k_icp_step folds, to sums (17 doubles of device memory); thread 0
// takes the visit
template <int = 0>
__global__ __launch_bounds__(256) void k_ransac_polish(const double* __restrict__ part, int32_t nb, int i, int refine, double o0,
                                                        double o1, double o2, double* __restrict__ sums,
                                                        RansacPolish* __restrict__ pol) {
  __shared__ int32_t done;
  if (threadIdx.x == 0) done = pol->done;
  __syncthreads();
  if (done) return;
  double v[ICP_POINT_TERMS];
#pragma unroll
  for (int a = 0; a < ICP_POINT_TERMS; ++a) v[a] = 0.0;
  for (int32_t b = static_cast<int32_t>(threadIdx.x); b < nb; b += 256) {
#pragma unroll
    for (int a = 0; a < ICP_POINT_TERMS; ++a) v[a] = v[a] + part[static_cast<int64_t>(b) * ICP_POINT_TERMS + a];
  }
  icp_block_fold<ICP_POINT_TERMS>(v, sums);
  if (threadIdx.x != 0) return;  // (thread 0 wrote the sums itself)
  double Sc[ICP_POINT_TERMS];
#pragma unroll
  for (int a = 0; a < ICP_POINT_TERMS; ++a) Sc[a] = sums[a];
  RansacPolish r = *pol;
  const double o[3] = {o0, o1, o2};
  ransac_polish_visit(r, i, refine, Sc, o);
  *pol = r;
}

// mask[k]: correspondence k is an inlier of pol->T
template <int = 0>
__global__ __launch_bounds__(256) void k_ransac_mask(const double* __restrict__ P, const double* __restrict__ B, int32_t m,
                                                      double d2, const RansacPolish* __restrict__ pol, uint8_t* __restrict__ mask) {
  const int32_t k = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  if (k >= m) return;
  double T[16], q[3];
#pragma unroll
  for (int a = 0; a < 16; ++a) T[a] = pol->T[a];
  const double p[3] = {P[static_cast<int64_t>(k) * 3], P[static_cast<int64_t>(k) * 3 + 1], P[static_cast<int64_t>(k) * 3 + 2]};
  const double b[3] = {B[static_cast<int64_t>(k) * 3], B[static_cast<int64_t>(k) * 3 + 1], B[static_cast<int64_t>(k) * 3 + 2]};
  mask[k] = ransac_inlier(ransac_sqd(T, p, b, q), d2) ? 1 : 0;
}

}  // namespace clipper_hip
