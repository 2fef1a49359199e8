// k_wave.hip.h — the integer folds and scans of a wave and of a workgroup, stated once for every kernel: the xor
// butterfly, the shuffle-up ladder, the exclusive prefix over a workgroup, one workgroup scanning an array in chunks
// with a carry, and the front end's scan kernel over that. Part of kernels.hip.h; every header that uses it includes
// it itself. Device-only, stateless, wave64, one-dimensional workgroups whose size is a multiple of 64, all lanes active.
//
// Integers (and exact min / max) only: their result does not depend on the order of the fold, so a kernel may move
// between these functions and a ladder of its own without moving a bit. The floating-point folds are NOT here
// (sdp_block_sum, sdp_wave_argmax, icp_block_fold, k_kg_bounds, the lane-group butterfly of k_rv_resident): their
// order is part of what they compute.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace clipper_hip {

struct WaveAdd {
  template <typename T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

// ---- folds over the 64 lanes: every lane gets the result -----------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
  static_assert(std::is_integral<T>::value, "integers only: a floating-point sum depends on its order");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_max(T v) {
  static_assert(std::is_integral<T>::value, "integers only");
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// ---- inclusive scan over the 64 lanes: lane l gets op(v of lane 0, ..., v of lane l) -------------------------------
template <typename T, class Op = WaveAdd>
__device__ __forceinline__ T wave_scan_incl(T v, Op op = Op()) {
  static_assert(std::is_integral<T>::value, "integers only");
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o, 64);
    if (lane >= o) v = op(v, t);
  }
  return v;
}

// ---- exclusive scan over a workgroup of WAVES waves ----------------------------------------------------------------
// Returns op(v of thread 0, ..., v of the thread in front of this one), `unit` for thread 0; the last thread's result
// and its v make the workgroup's total. wsum: WAVES words of LDS, free to be overwritten once every thread is past a
// later barrier. CONTAINS A BARRIER: the whole workgroup must reach it. op is associative and commutative with
// identity `unit` (k_kg_slabs: min / max over order-preserving keys).
template <int WAVES, typename T, class Op = WaveAdd>
__device__ __forceinline__ T block_scan_excl(T v, T* wsum, Op op = Op(), T unit = T(0)) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T inc = wave_scan_incl(v, op);
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  T off = unit;
  for (int w = 0; w < wave; ++w) off = op(off, wsum[w]);
  if constexpr (std::is_same<Op, WaveAdd>::value) {
    return off + inc - v;
  } else {  // (no inverse: the inclusive value of the lane in front)
    const T prev = __shfl_up(inc, 1, 64);
    return lane == 0 ? off : op(off, prev);
  }
}

// ---- one workgroup of THREADS threads scans an array ---------------------------------------------------------------
// out[i] (and out2[i], if given) = in[0] + ... + in[i - 1] for i = 0..n-1, in chunks of THREADS elements with a carry;
// returns the sum of all of them, in every thread. in == out is allowed (in place). wsum: THREADS / 64 words of LDS,
// carry: one. CONTAINS BARRIERS: the whole workgroup must reach it, with the same n. A thread's next element is in
// flight while the workgroup scans the current chunk. n = 0 is allowed: nothing is read or written, 0 is returned.
// Held on the device by tests/hip/wave_check.hip at every instantiation a kernel uses, n = 0 .. 3 THREADS, in place
// against out of place, the total in every thread, 64-bit prefixes past 2^32 inside a chunk and across the carry.
template <int THREADS, typename TIn, typename TOut, typename I>
__device__ __forceinline__ TOut block_scan_array(const TIn* in, I n, TOut* out, TOut* wsum, TOut* carry,
                                                 TOut* out2 = nullptr) {
  static_assert(THREADS % 64 == 0, "whole waves");
  const I t = static_cast<I>(threadIdx.x);
  if (t == 0) *carry = 0;
  TIn next = t < n ? in[t] : TIn(0);
  for (I b0 = 0; b0 < n; b0 += THREADS) {
    const I i = b0 + t;
    const TOut v = static_cast<TOut>(next);
    next = i + THREADS < n ? in[i + THREADS] : TIn(0);  // (0 past the end: the last chunk's total counts it)
    const TOut excl = block_scan_excl<THREADS / 64>(v, wsum);  // (its barrier also puts the carry's store in front)
    const TOut c = *carry;
    if (i < n) {
      out[i] = c + excl;
      if (out2) out2[i] = c + excl;
    }
    __syncthreads();  // every thread has read the carry and wsum
    if (t == THREADS - 1) *carry = c + excl + v;
  }
  __syncthreads();
  return *carry;
}

// ---- the front end's scan kernel (grid search, sort, voxel) --------------------------------------------------------
// Workgroup b scans row b of n int32 entries: out[b n + i] = in[b n] + ... + in[b n + i - 1]; the same into out2 if
// given; with with_total (one row only: the place lies behind the row) the row's sum goes to [n] of both.
constexpr int ROW_SCAN_THREADS = 1024;
template <int = 0>
__global__ __launch_bounds__(ROW_SCAN_THREADS) void k_row_scan(const int32_t* __restrict__ in, int32_t n, int32_t* __restrict__ out,
                                                                int32_t* __restrict__ out2, int with_total) {
  __shared__ int32_t wsum[ROW_SCAN_THREADS / 64];
  __shared__ int32_t carry;
  const int64_t row = static_cast<int64_t>(blockIdx.x) * n;
  out += row;
  if (out2) out2 += row;
  const int32_t total = block_scan_array<ROW_SCAN_THREADS>(in + row, n, out, wsum, &carry, out2);
  if (with_total && threadIdx.x == 0) {
    out[n] = total;
    if (out2) out2[n] = total;
  }
}

}  // namespace clipper_hip
