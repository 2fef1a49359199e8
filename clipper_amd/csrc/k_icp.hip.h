// k_icp.hip.h — the device side of the ICP refinement ("ICP over a kept search grid"). Part of
// kernels.hip.h (include that one): hand-written gfx950 device code. The arithmetic is icp_rules.hpp's; here is which
// work item holds what. One iteration is: the transform, the K = 1 search (k_knn_grid<1> over a kept index, or the
// brute-force kernels), the sums, the step.
//   k_icp_transform      thread = one place of the query order: source point perm[place] (or `place` itself) through
//                        T, to row idx of q (n x 3) and, for the grid route, to place `place` of the binned queries
//   k_icp_order          the permutation of a binned cloud (place -> original index), taken once at T_init
//   k_icp_accumulate<M, ROBUST>  thread = source point i in its original order: the list entry, q, the target point
//                        (and normal; generalized: the two covariances and the rotation of the device's T), the terms,
//                        the halving tree in LDS, one partial per workgroup. The tree runs over LDS rows of one term
//                        each, 8 terms at a time, so that a workgroup holds 16 KiB of LDS whatever the method.
//   k_icp_step<M, ROBUST>  one workgroup: thread t adds partials t, t + 256, ... per term, the same tree; thread 0
//                        runs icp_iterate_over (the step, the stop test, the update of T) and writes the record and
//                        the history row. T stays on the device.
//                        ROBUST (clipper_hip_icp_robust): the same two over the robust layout, a kept pair's terms
//                        weighed by its loss; kept against tau of k_select.hip.h's control block
//   k_icp_covariances    thread = one point, as k_feat_normals: the neighbourhood's covariance, its smallest
//                        eigenvector in registers, the six entries of I - (1 - epsilon) nv nv^T
// No floating-point atomics: every sum has one order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "icp_rules.hpp"
#include "k_knn_grid.hip.h"

namespace clipper_hip {

constexpr int ICP_TREE_TERMS = 8;  // terms folded per pass over the LDS tree

template <int = 0>
__global__ __launch_bounds__(256) void k_icp_transform(const double* __restrict__ T, const double* __restrict__ P, int32_t n,
                                                        const int32_t* __restrict__ perm, double* __restrict__ q,
                                                        KgPoint* __restrict__ Q) {
  const int32_t place = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  if (place >= n) return;
  const int32_t i = perm ? perm[place] : place;
  if (i < 0 || i >= n) return;  // (cannot happen: perm is a permutation)
  const double p[3] = {P[static_cast<int64_t>(i) * 3], P[static_cast<int64_t>(i) * 3 + 1], P[static_cast<int64_t>(i) * 3 + 2]};
  double t[3];
  icp_transform_point(T, p, t);
  q[static_cast<int64_t>(i) * 3] = t[0];
  q[static_cast<int64_t>(i) * 3 + 1] = t[1];
  q[static_cast<int64_t>(i) * 3 + 2] = t[2];
  if (Q) {
    KgPoint k;
    k.x = t[0];
    k.y = t[1];
    k.z = t[2];
    k.idx = i;
    k.pad = 0;
    Q[place] = k;
  }
}

template <int = 0>
__global__ __launch_bounds__(256) void k_icp_order(const KgPoint* __restrict__ Q, int32_t n, int32_t* __restrict__ perm) {
  const int32_t place = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  if (place < n) perm[place] = Q[place].idx;
}

// v: the calling thread's TERMS values; the workgroup's sums go to out[0..TERMS) (thread 0 writes them)
template <int TERMS>
__device__ inline void icp_block_fold(const double (&v)[TERMS], double* __restrict__ out) {
  __shared__ double red[ICP_TREE_TERMS][ICP_BLOCK];
  const int t = static_cast<int>(threadIdx.x);
#pragma unroll
  for (int base = 0; base < TERMS; base += ICP_TREE_TERMS) {
#pragma unroll
    for (int a = 0; a < ICP_TREE_TERMS; ++a)
      if (base + a < TERMS) red[a][t] = v[base + a];
    __syncthreads();
    for (int s = ICP_BLOCK / 2; s > 0; s >>= 1) {
      if (t < s) {
#pragma unroll
        for (int a = 0; a < ICP_TREE_TERMS; ++a)
          if (base + a < TERMS) red[a][t] = red[a][t] + red[a][t + s];
      }
      __syncthreads();
    }
    if (t == 0) {
#pragma unroll
      for (int a = 0; a < ICP_TREE_TERMS; ++a)
        if (base + a < TERMS) out[base + a] = red[a][0];
    }
    __syncthreads();
  }
}

// oi / od: the K = 1 lists (n_src entries); q: the transformed source (n_src x 3); B / Nb: the target and its normals
// (n_tgt x 3; Nb for point-to-plane alone); Ca / Cb / T: the covariances of the source and the target (n x 6) and the
// current transform (generalized alone); part: gridDim.x x TERMS
//
// the plain terms of the pair (source point i, target point j) of METHOD: what every accumulate kernel loads and forms
template <int METHOD>
__device__ inline void icp_pair_terms(int32_t i, int32_t j, double sqd, const double* __restrict__ q,
                                      const double* __restrict__ B, const double* __restrict__ Nb,
                                      const double* __restrict__ Ca, const double* __restrict__ Cb,
                                      const double* __restrict__ T, const double (&o)[3], double (&t)[icp_terms(METHOD)]) {
  const double qq[3] = {q[static_cast<int64_t>(i) * 3], q[static_cast<int64_t>(i) * 3 + 1], q[static_cast<int64_t>(i) * 3 + 2]};
  const double b[3] = {B[static_cast<int64_t>(j) * 3], B[static_cast<int64_t>(j) * 3 + 1], B[static_cast<int64_t>(j) * 3 + 2]};
  if constexpr (METHOD == ICP_POINT_TO_PLANE) {
    const double nn[3] = {Nb[static_cast<int64_t>(j) * 3], Nb[static_cast<int64_t>(j) * 3 + 1], Nb[static_cast<int64_t>(j) * 3 + 2]};
    icp_plane_terms(qq, b, nn, sqd, o, t);
  } else if constexpr (METHOD == ICP_GENERALIZED) {
    double ca[6], cb[6], Tl[12];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      ca[a] = Ca[static_cast<int64_t>(i) * 6 + a];
      cb[a] = Cb[static_cast<int64_t>(j) * 6 + a];
    }
#pragma unroll
    for (int a = 0; a < 12; ++a) Tl[a] = T[a];  // (the rotation: entries 0..2, 4..6, 8..10)
    icp_generalized_terms(qq, b, ca, cb, Tl, sqd, o, t);
  } else {
    icp_point_terms(qq, b, sqd, o, t);
  }
}

// what the robust accumulate reads besides the plain one's arguments, by value: loss, scale and k2 = scale * scale are
// run-time settings; ctl is the selection's control block on the device. ROBUST == false never reads it.
struct IcpRobustArgs {
  int loss = 0;
  double scale = 0.0, k2 = 0.0;
  const IcpSelect* ctl = nullptr;
};

// ROBUST: the weighted sums of clipper_hip_icp_robust over the robust layout (icp_layout_terms). A point is kept by
// icp_kept against tau of the control block (without trimming: max_distance^2) and its plain terms are weighed by
// icp_weight of its squared residual. Else: kept by icp_inlier, the plain terms, nothing weighed.
template <int METHOD, bool ROBUST>
__global__ __launch_bounds__(256) void k_icp_accumulate(const int32_t* __restrict__ oi, const double* __restrict__ od,
                                                         const double* __restrict__ q, int32_t n_src,
                                                         const double* __restrict__ B, const double* __restrict__ Nb,
                                                         const double* __restrict__ Ca, const double* __restrict__ Cb,
                                                         const double* __restrict__ T, int32_t n_tgt, double d2, double o0,
                                                         double o1, double o2, IcpRobustArgs rb, double* __restrict__ part) {
  constexpr int TERMS = icp_layout_terms(METHOD, ROBUST);
  const int32_t i = static_cast<int32_t>(blockIdx.x) * 256 + static_cast<int32_t>(threadIdx.x);
  double tau = 0.0;
  int32_t any = 0;
  if constexpr (ROBUST) {
    tau = rb.ctl->tau;
    any = rb.ctl->any;
  }
  double t[TERMS];
#pragma unroll
  for (int a = 0; a < TERMS; ++a) t[a] = 0.0;
  if (i < n_src) {
    const int32_t j = oi[i];
    const double sqd = od[i];
    bool kept;
    if constexpr (ROBUST) kept = icp_kept(j, sqd, d2, tau, any);
    else kept = icp_inlier(j, sqd, d2);
    if (kept && j < n_tgt) {
      const double o[3] = {o0, o1, o2};
      if constexpr (ROBUST && METHOD == ICP_POINT_TO_POINT) {
        double p[ICP_POINT_TERMS];
        icp_pair_terms<METHOD>(i, j, sqd, q, B, Nb, Ca, Cb, T, o, p);
        icp_point_terms_weighted(p, icp_weight(rb.loss, sqd, rb.scale, rb.k2), t);
      } else {
        icp_pair_terms<METHOD>(i, j, sqd, q, B, Nb, Ca, Cb, T, o, t);
        if constexpr (ROBUST) icp_plane_terms_weighted(icp_weight(rb.loss, t[28], rb.scale, rb.k2), t);
      }
    }
  }
  icp_block_fold<TERMS>(t, part + static_cast<int64_t>(blockIdx.x) * TERMS);
}

// part: nb x TERMS; sums: TERMS doubles of device memory (the folded sums, kept for the host's evaluate); T: 16; rec and
// history (may be null) on the device. ROBUST: the robust layout and its step (k_icp_accumulate<METHOD, true>'s partials).
template <int METHOD, bool ROBUST>
__global__ __launch_bounds__(256) void k_icp_step(const double* __restrict__ part, int32_t nb, IcpStop stop, int k, double o0,
                                                   double o1, double o2, double* __restrict__ sums, double* __restrict__ T,
                                                   IcpRecord* __restrict__ rec, double* __restrict__ history) {
  constexpr int TERMS = icp_layout_terms(METHOD, ROBUST);
  double v[TERMS];
#pragma unroll
  for (int a = 0; a < TERMS; ++a) v[a] = 0.0;
  for (int32_t b = static_cast<int32_t>(threadIdx.x); b < nb; b += 256) {
#pragma unroll
    for (int a = 0; a < TERMS; ++a) v[a] = v[a] + part[static_cast<int64_t>(b) * TERMS + a];
  }
  icp_block_fold<TERMS>(v, sums);
  if (threadIdx.x != 0) return;  // (thread 0 wrote the sums itself)
  double S[TERMS], Tl[16];
#pragma unroll
  for (int a = 0; a < TERMS; ++a) S[a] = sums[a];
#pragma unroll
  for (int a = 0; a < 16; ++a) Tl[a] = T[a];
  IcpRecord r = *rec;
  const double o[3] = {o0, o1, o2};
  double row[3];
  icp_iterate_over<METHOD, ROBUST>(stop, k, S, o, Tl, r, row);
#pragma unroll
  for (int a = 0; a < 16; ++a) T[a] = Tl[a];
  *rec = r;
  if (history) {
    history[static_cast<int64_t>(k) * 3] = row[0];
    history[static_cast<int64_t>(k) * 3 + 1] = row[1];
    history[static_cast<int64_t>(k) * 3 + 2] = row[2];
  }
}

// C[i] = the regularised covariance of point i (six doubles: xx, xy, xz, yy, yz, zz) over the first knn entries of its
// list that are kept, w = 1.0 - epsilon; cnt_out (may be null): how many. The lists are k_feat_normals'.
template <int = 0>
__global__ __launch_bounds__(256) void k_icp_covariances(const double* __restrict__ P, int64_t n,
                                                          const int32_t* __restrict__ li, const double* __restrict__ ld,
                                                          int stride, int knn, int use_r, double r2, double w,
                                                          double* __restrict__ C, int32_t* __restrict__ cnt_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t* row = li + i * stride;
  int cnt = 0;
  while (cnt < knn && feat_kept(row[cnt], ld[i * stride + cnt], use_r != 0, r2)) ++cnt;
  double c[6];
  icp_point_covariance(
      cnt,
      [&](int k, double (&p)[3]) {
        const int64_t j = row[k];
        p[0] = P[j * 3];
        p[1] = P[j * 3 + 1];
        p[2] = P[j * 3 + 2];
      },
      w, c);
#pragma unroll
  for (int a = 0; a < 6; ++a) C[i * 6 + a] = c[a];
  if (cnt_out) cnt_out[i] = cnt;
}

}  // namespace clipper_hip
