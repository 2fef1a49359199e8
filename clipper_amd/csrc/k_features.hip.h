// k_features.hip.h — surface normals and FPFH descriptors of a point cloud (before the path: what
// clipper_hip_match_descriptors and PointNormalDistance take in). Part of kernels.hip.h (include that one):
// hand-written gfx950 device code. The arithmetic of every kernel here is features_rules.hpp's.
//
// The neighbourhood of point i is a prefix of its nearest-neighbour list in the cloud itself (k_knn_partial<K, 3> +
// k_knn_merge<K> on (P, P): the point is in its own list), n x stride entries row-major.
//   k_feat_normals  thread = one point: two passes over its neighbours (centroid, centred covariance), the 3 x 3
//                   Jacobi in registers (every index a constant: no scratch), the sign rule
//   k_feat_spfh     thread = one (point, neighbour) pair, SLOTS threads per point and 256 / SLOTS points per
//                   workgroup: the pair feature, then three LDS atomics on the point's 33 integer counters (a
//                   histogram indexed at run time would spill from registers); count * 100 / (cnt - 1) leaves
//   k_feat_fpfh     thread = one bin of one point, 7 points per workgroup (231 of 256 lanes): a neighbour's 264-byte
//                   SPFH row is one coalesced read of 33 lanes; the sum over the neighbours runs in list order; the
//                   three group sums are taken by every lane of a group from LDS in ascending bin order
// All three are templates (k_feat_normals and k_feat_fpfh over nothing): an instantiation is emitted where the driver
// first names it, at the end of the code object, so the kernels of the fill and the solver keep their places in it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "features_rules.hpp"

namespace clipper_hip {

constexpr int FEAT_FPFH_POINTS = 256 / FEAT_DIM;  // points per workgroup of k_feat_fpfh

// N[i] = the normal of point i over the first knn entries of its list that are kept; cnt_out (may be null): how many
template <int = 0>
__global__ __launch_bounds__(256) void k_feat_normals(const double* __restrict__ P, int64_t n,
                                                       const int32_t* __restrict__ li, const double* __restrict__ ld,
                                                       int stride, int knn, int use_r, double r2,
                                                       const double* __restrict__ view, double* __restrict__ N,
                                                       int32_t* __restrict__ cnt_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t* row = li + i * stride;
  int cnt = 0;
  while (cnt < knn && feat_kept(row[cnt], ld[i * stride + cnt], use_r != 0, r2)) ++cnt;
  const double p[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
  double nv[3];
  feat_normal(
      cnt,
      [&](int k, double (&q)[3]) {
        const int64_t j = row[k];
        q[0] = P[j * 3];
        q[1] = P[j * 3 + 1];
        q[2] = P[j * 3 + 2];
      },
      p, view, nv);
  N[i * 3] = nv[0];
  N[i * 3 + 1] = nv[1];
  N[i * 3 + 2] = nv[2];
  if (cnt_out) cnt_out[i] = cnt;
}

// spfh[i][0..33) = SPFH(i) over the first knn kept entries of its list; SLOTS (a power of two >= knn) threads per point
template <int SLOTS>
__global__ __launch_bounds__(256) void k_feat_spfh(const double* __restrict__ P, const double* __restrict__ N,
                                                    int64_t n, const int32_t* __restrict__ li,
                                                    const double* __restrict__ ld, int stride, int knn, int use_r,
                                                    double r2, double* __restrict__ spfh,
                                                    int32_t* __restrict__ cnt_out) {
  constexpr int PPB = 256 / SLOTS;  // points per workgroup
  __shared__ int32_t hist[PPB][FEAT_DIM];
  __shared__ int32_t kept[PPB];
  const int t = threadIdx.x, pt = t / SLOTS, k = t % SLOTS;
  for (int e = t; e < PPB * FEAT_DIM; e += 256) (&hist[0][0])[e] = 0;
  if (t < PPB) kept[t] = 0;
  __syncthreads();
  const int64_t i = static_cast<int64_t>(blockIdx.x) * PPB + pt;
  int32_t j = -1;
  bool mine = false;
  if (i < n && k < knn) {
    j = li[i * stride + k];
    mine = feat_kept(j, ld[i * stride + k], use_r != 0, r2);
  }
  if (mine) {
    atomicAdd(&kept[pt], 1);
    if (j != static_cast<int32_t>(i)) {
      const double p1[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
      const double n1[3] = {N[i * 3], N[i * 3 + 1], N[i * 3 + 2]};
      const int64_t jj = j;
      const double p2[3] = {P[jj * 3], P[jj * 3 + 1], P[jj * 3 + 2]};
      const double n2[3] = {N[jj * 3], N[jj * 3 + 1], N[jj * 3 + 2]};
      double f[3];
      int b[3];
      feat_pair(p1, n1, p2, n2, f);
      feat_bins(f, b);
      atomicAdd(&hist[pt][b[0]], 1);
      atomicAdd(&hist[pt][b[1]], 1);
      atomicAdd(&hist[pt][b[2]], 1);
    }
  }
  __syncthreads();
  for (int e = t; e < PPB * FEAT_DIM; e += 256) {
    const int q = e / FEAT_DIM;
    const int64_t o = static_cast<int64_t>(blockIdx.x) * PPB + q;
    if (o < n) spfh[o * FEAT_DIM + (e - q * FEAT_DIM)] = static_cast<double>((&hist[0][0])[e]) * feat_spfh_scale(kept[q]);
  }
  if (cnt_out && t < PPB && static_cast<int64_t>(blockIdx.x) * PPB + t < n)
    cnt_out[static_cast<int64_t>(blockIdx.x) * PPB + t] = kept[t];
}

// F[i][0..33) = FPFH(i): the SPFH rows of the kept neighbours weighted by 1 / sqd in list order, every group of 11
// bins scaled to 100, plus SPFH(i)
template <int = 0>
__global__ __launch_bounds__(256) void k_feat_fpfh(const double* __restrict__ spfh, int64_t n,
                                                    const int32_t* __restrict__ li, const double* __restrict__ ld,
                                                    int stride, int knn, int use_r, double r2,
                                                    double* __restrict__ F) {
  __shared__ double fs[FEAT_FPFH_POINTS][FEAT_DIM];
  const int t = threadIdx.x, pt = t / FEAT_DIM, b = t - pt * FEAT_DIM;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * FEAT_FPFH_POINTS + pt;
  const bool live = pt < FEAT_FPFH_POINTS && i < n;
  double f = 0.0;
  if (live) {
    for (int k = 0; k < knn; ++k) {
      const int32_t j = li[i * stride + k];
      const double sqd = ld[i * stride + k];
      if (!feat_kept(j, sqd, use_r != 0, r2)) break;  // the kept entries are a prefix
      if (feat_weighs(j, static_cast<int32_t>(i), sqd)) f = feat_fpfh_add(f, spfh[static_cast<int64_t>(j) * FEAT_DIM + b], sqd);
    }
    fs[pt][b] = f;
  }
  __syncthreads();
  if (live) {
    const int g = (b / FEAT_BINS) * FEAT_BINS;
    double s = 0.0;
    for (int c = 0; c < FEAT_BINS; ++c) s = s + fs[pt][g + c];
    F[i * FEAT_DIM + b] = feat_fpfh_bin(f, s, spfh[i * FEAT_DIM + b]);
  }
}

}  // namespace clipper_hip
