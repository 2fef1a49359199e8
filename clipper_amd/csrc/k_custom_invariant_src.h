// k_custom_invariant_src.h — the device text of a user-defined invariant's program (host_custom_invariant.hpp compiles
// it at run time with hiprtc, for gfx950). A program is: the prelude (CLIPPER_D, the parameter block), the user's
// source, the epilogue (the signature check, the fill kernels). The epilogue's fill follows k_affinity_euclid's
// geometry (k_affinity.hip.h): one thread holds 4 adjacent columns' points in registers and walks a strip of rows,
// storing a whole float4 / double4 row segment per lane into the shard's dense store S[r * ld + (c - c0)]. Element
// (r, c) of two distinct associations calls clipper_invariant on (i, j) = (min(r, c), max(r, c)), so that both triangles
// come from one call on the same arguments; the rest of the contract is the host loop's (clipper.cpp:31-64).
#pragma once

#include <cstddef>

namespace clipper_hip {

constexpr int CUSTOM_MAX_PARAMS = 16;  // doubles a fill hands to clipper_invariant (CLIPPER_HIP_INVARIANT_MAX_PARAMS)
constexpr int CUSTOM_MAX_D = 32;       // dimension of a datum (CLIPPER_HIP_INVARIANT_MAX_D)

// the fill's parameter block, as the kernels take it (by value: it lives in the kernel arguments); the prelude declares
// the same layout on the device side
struct CustomParams {
  double p[CUSTOM_MAX_PARAMS];
  double affinityeps;
};

// One problem of a batched fill (clipper_custom_fill_batch_*): its dense store S (pitch ld, columns from 0), m, its
// gathered point tables and its association list's two columns. Twin of the epilogue's clipper_fill_problem: the two
// layouts must stay identical (the asserts pin this one).
struct CustomFillProblem {
  void* S;
  long long ld;
  long long m;
  const double* P1;
  const double* P2;
  long long pstride;
  const int* A0;
  const int* A1;
};
static_assert(sizeof(CustomFillProblem) == 64, "CustomFillProblem: layout of clipper_fill_problem");
static_assert(offsetof(CustomFillProblem, ld) == 8 && offsetof(CustomFillProblem, m) == 16 &&
                  offsetof(CustomFillProblem, P1) == 24 && offsetof(CustomFillProblem, P2) == 32 &&
                  offsetof(CustomFillProblem, pstride) == 40 && offsetof(CustomFillProblem, A0) == 48 &&
                  offsetof(CustomFillProblem, A1) == 56,
              "CustomFillProblem: layout of clipper_fill_problem");

// One workgroup of a batched fill: which problem, and which tile of it the lone fill's (blockIdx.x, blockIdx.y) would
// be. Twin of the epilogue's clipper_fill_tile.
struct CustomFillTile {
  int problem;
  int cblk;    // column block: 1024 columns
  int rstrip;  // row strip: rows_per_blk rows
};
static_assert(sizeof(CustomFillTile) == 12 && offsetof(CustomFillTile, cblk) == 4 &&
                  offsetof(CustomFillTile, rstrip) == 8,
              "CustomFillTile: layout of clipper_fill_tile");

// what precedes the user's text: %d is the datum's dimension
constexpr const char* kCustomPrelude = R"CLIPPER(#line 1 "clipper_prelude"
constexpr int CLIPPER_D = %d;
constexpr int CLIPPER_MAX_PARAMS = 16;
struct clipper_fill_params {
  double p[CLIPPER_MAX_PARAMS];
  double affinityeps;
};
#line 1 "invariant"
)CLIPPER";

// what follows it: the signature check, then the fill kernels, lone and batched (extern "C": host_custom_invariant.hpp
// looks them up by name)
constexpr const char* kCustomEpilogue = R"CLIPPER(
#line 1 "clipper_fill"
typedef double (*clipper_invariant_signature)(const double*, const double*, const double*, const double*, const double*);
// a source without `__device__ double clipper_invariant(const double*, const double*, const double*, const double*,
// const double*)` fails to compile here
__device__ inline clipper_invariant_signature clipper_invariant_required() { return &clipper_invariant; }

// clipper.cpp:53-55: a score is kept only when it exceeds affinityeps (NaN is not); an fp32 underflow stays in the
// pattern as the smallest normal. This is a copy of the stored-value rule (store_value / store_score, k_affinity.hip.h:
// stated there; restated here only because this source is compiled on its own at run time — a kept score is positive,
// so the sign of the rule never shows)
template <typename T>
__device__ __forceinline__ T clipper_store_score(double scr, double affinityeps) {
  if (!(scr > affinityeps)) return T(0);
  T v = static_cast<T>(scr);
  if (v == T(0)) v = static_cast<T>(1.17549435e-38);
  return v;
}

__device__ __forceinline__ void clipper_store4(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void clipper_store4(double* p, double a, double b, double c, double d) {
  *reinterpret_cast<double4*>(p) = make_double4(a, b, c, d);
}

// S: the shard's dense store (ld = its pitch, a multiple of 4), columns [c0, c0 + ld) of M; P1, P2: the gathered point
// tables [CLIPPER_D][pstride] (column i = D1[:, A(i, 0)], D2[:, A(i, 1)]); A0, A1: the association list's two columns;
// (cblk, rstrip): this workgroup's block of 1024 columns and strip of rows_per_blk rows
template <typename T>
__device__ __forceinline__ void clipper_custom_fill(T* __restrict__ S, long long ld, long long m, long long c0,
                                                    int rows_per_blk, const double* __restrict__ P1,
                                                    const double* __restrict__ P2, long long pstride,
                                                    const int* __restrict__ A0, const int* __restrict__ A1,
                                                    const clipper_fill_params& prm, long long cblk, long long rstrip) {
  constexpr int D = CLIPPER_D;
  const long long c = (cblk * 256 + threadIdx.x) * 4;
  if (c >= ld) return;
  const long long r0 = rstrip * rows_per_blk;
  const long long r1 = (r0 + rows_per_blk < m) ? r0 + rows_per_blk : m;

  long long gc[4];
  bool valid[4];
  int a0c[4], a1c[4];
  double p1c[4][D], p2c[4][D];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long long g = c0 + c + q;
    valid[q] = g < m;
    gc[q] = valid[q] ? g : (m - 1);
    a0c[q] = A0[gc[q]];
    a1c[q] = A1[gc[q]];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      p1c[q][k] = P1[k * pstride + gc[q]];
      p2c[q][k] = P2[k * pstride + gc[q]];
    }
  }

  for (long long r = r0; r < r1; ++r) {
    const int a0r = A0[r], a1r = A1[r];
    double p1r[D], p2r[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      p1r[k] = P1[k * pstride + r];
      p2r[k] = P2[k * pstride + r];
    }
    T out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // clipper.cpp:35-38 distinctness; the diagonal fails it by construction
      const bool ok = valid[q] && (a0r != a0c[q]) && (a1r != a1c[q]);
      double scr = 0.0;
      if (ok) {
        // (i, j) = (min(r, c), max(r, c)): values chosen element by element, so that the four data stay in registers
        const bool row_first = r < gc[q];
        double ai[D], aj[D], bi[D], bj[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
          ai[k] = row_first ? p1r[k] : p1c[q][k];
          aj[k] = row_first ? p1c[q][k] : p1r[k];
          bi[k] = row_first ? p2r[k] : p2c[q][k];
          bj[k] = row_first ? p2c[q][k] : p2r[k];
        }
        scr = clipper_invariant(ai, aj, bi, bj, prm.p);
      }
      out[q] = clipper_store_score<T>(scr, prm.affinityeps);
    }
    clipper_store4(S + r * ld + c, out[0], out[1], out[2], out[3]);
  }
}

extern "C" __global__ __launch_bounds__(256) void clipper_custom_fill_f32(
    float* __restrict__ S, long long ld, long long m, long long c0, int rows_per_blk, const double* __restrict__ P1,
    const double* __restrict__ P2, long long pstride, const int* __restrict__ A0, const int* __restrict__ A1,
    clipper_fill_params prm) {
  clipper_custom_fill<float>(S, ld, m, c0, rows_per_blk, P1, P2, pstride, A0, A1, prm, blockIdx.x, blockIdx.y);
}

extern "C" __global__ __launch_bounds__(256) void clipper_custom_fill_f64(
    double* __restrict__ S, long long ld, long long m, long long c0, int rows_per_blk, const double* __restrict__ P1,
    const double* __restrict__ P2, long long pstride, const int* __restrict__ A0, const int* __restrict__ A1,
    clipper_fill_params prm) {
  clipper_custom_fill<double>(S, ld, m, c0, rows_per_blk, P1, P2, pstride, A0, A1, prm, blockIdx.x, blockIdx.y);
}

// A batch's fill (host_batchsolve.hpp): one launch for every problem. Workgroup b reads its (problem, column block,
// row strip) from tiles[b] and fills that tile of the problem's dense store exactly as the lone kernel's workgroup
// (cblk, rstrip) does (c0 = 0): every element is the same call on the same arguments, so the stores are the same bits.
// Twins of CustomFillProblem / CustomFillTile (k_custom_invariant_src.h).
struct clipper_fill_problem {
  void* S;
  long long ld;
  long long m;
  const double* P1;
  const double* P2;
  long long pstride;
  const int* A0;
  const int* A1;
};
struct clipper_fill_tile {
  int problem;
  int cblk;
  int rstrip;
};

template <typename T>
__device__ __forceinline__ void clipper_custom_fill_tile(const clipper_fill_problem* __restrict__ probs,
                                                         const clipper_fill_tile* __restrict__ tiles, int rows_per_blk,
                                                         const clipper_fill_params& prm) {
  const clipper_fill_tile t = tiles[blockIdx.x];
  const clipper_fill_problem q = probs[t.problem];
  clipper_custom_fill<T>(static_cast<T*>(q.S), q.ld, q.m, 0, rows_per_blk, q.P1, q.P2, q.pstride, q.A0, q.A1, prm,
                         t.cblk, t.rstrip);
}

extern "C" __global__ __launch_bounds__(256) void clipper_custom_fill_batch_f32(
    const clipper_fill_problem* __restrict__ probs, const clipper_fill_tile* __restrict__ tiles, int rows_per_blk,
    clipper_fill_params prm) {
  clipper_custom_fill_tile<float>(probs, tiles, rows_per_blk, prm);
}

extern "C" __global__ __launch_bounds__(256) void clipper_custom_fill_batch_f64(
    const clipper_fill_problem* __restrict__ probs, const clipper_fill_tile* __restrict__ tiles, int rows_per_blk,
    clipper_fill_params prm) {
  clipper_custom_fill_tile<double>(probs, tiles, rows_per_blk, prm);
}
)CLIPPER";

}  // namespace clipper_hip
