// k_cloud.hip.h — what a cloud that lives on the device needs besides the stages' own kernels (host_cloud.hpp): the
// gather of selected points, the point-then-normal table PointNormalDistance is staged from, and the max-abs fold that
// replaces stage_inputs' host loop. Part of kernels.hip.h (include that one). Memory-trivial: 256 threads, one element
// per thread along the contiguous index, no atomics.
//   k_cloud_gather        out[3 r + c] = P[3 idx[r] + c], r < k: the selected points, in the order of the list
//   k_cloud_point_normal  out[6 p + c] = c < 3 ? P[3 p + c] : N[3 p + c - 3]: the d = 6 rows of PointNormalDistance
//   k_cloud_maxabs        out[b] = max |in[e]| over the elements workgroup b strides over (0.0 for none). A maximum of
//                         finite magnitudes does not depend on the order of the fold: a second launch of ONE workgroup
//                         over the partial results gives the value of the host's loop, bit for bit
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace clipper_hip {

constexpr int CLOUD_MAXABS_BLOCKS = 256;  // workgroups of the first launch of the fold, at most

template <int = 0>
__global__ __launch_bounds__(256) void k_cloud_gather(const double* __restrict__ P, const int32_t* __restrict__ idx,
                                                       int64_t k, double* __restrict__ out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= 3 * k) return;
  const int64_t r = e / 3;
  out[e] = P[static_cast<int64_t>(idx[r]) * 3 + (e - r * 3)];
}

template <int = 0>
__global__ __launch_bounds__(256) void k_cloud_point_normal(const double* __restrict__ P, const double* __restrict__ N,
                                                             int64_t n, double* __restrict__ out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= 6 * n) return;
  const int64_t p = e / 6;
  const int c = static_cast<int>(e - p * 6);
  out[e] = c < 3 ? P[p * 3 + c] : N[p * 3 + c - 3];
}

template <int = 0>
__global__ __launch_bounds__(256) void k_cloud_maxabs(const double* __restrict__ in, int64_t n, double* __restrict__ out) {
  __shared__ double wmax[4];
  double v = 0.0;
  for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < n; e += static_cast<int64_t>(gridDim.x) * 256) {
    const double a = fabs(in[e]);
    v = a > v ? a : v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) v = wmax[w] > v ? wmax[w] : v;
    out[blockIdx.x] = v;
  }
}

}  // namespace clipper_hip
