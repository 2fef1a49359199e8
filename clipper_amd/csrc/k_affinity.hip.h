// k_affinity.hip.h — affinity fill: k_gather_points, the invariants' policy types, k_affinity_plain / _compact (strips) /
// _sym / _rect (tiles)
// Part of kernels.hip.h (include that one): hand-written gfx950 device code of the CLIPPER hot path.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_csc.hip.h"

namespace clipper_hip {

// ------------------------------------------------------------------------------------------
// affinity fill
// ------------------------------------------------------------------------------------------

// P[k * pstride + i] = D[k + d * idx[i]] : per-association point table, structure of arrays,
// so that column data loads in the fill kernels are contiguous across lanes. Pf is the same
// table rounded to fp32 (input of the conservative prefilter of the compacting fill kernels).
__global__ __launch_bounds__(256) void k_gather_points(const double* __restrict__ D, int d,
                                                        const int32_t* __restrict__ idx,
                                                        int64_t m, int64_t pstride,
                                                        double* __restrict__ P,
                                                        float* __restrict__ Pf) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= pstride) return;
  const int64_t src = (i < m) ? idx[i] : 0;
  for (int k = 0; k < d; ++k) {
    const double v = (i < m) ? D[k + d * src] : 0.0;
    P[k * pstride + i] = v;
    Pf[k * pstride + i] = static_cast<float>(v);
  }
}

// THE stored-value rule, for every route on which a double becomes an entry of M (the fills through store_score, the
// dense setter, the sparse setter's two routes): the cast to T — a value that rounds to an fp32 subnormal stays that
// subnormal — except that a non-zero value never becomes 0: C == pattern(M) is implicit in every store, so an fp32
// underflow keeps the smallest normal, with the sign of the value, instead of leaving the pattern.
// (k_custom_invariant_src.h restates it: a source string of its own.)
template <typename T>
__device__ __forceinline__ T store_value(double v) {
  const T s = static_cast<T>(v);
  if (s == T(0) && v != 0.0) return static_cast<T>(v > 0.0 ? 1.17549435e-38 : -1.17549435e-38);
  return s;
}

template <typename T>
__device__ __forceinline__ T store_score(double scr, double affinityeps) {
  // clipper.cpp:53-55 — keep the score only when it exceeds affinityeps.
  if (!(scr > affinityeps)) return T(0);
  return store_value<T>(scr);
}

template <typename T>
__device__ __forceinline__ void store4(T* p, T a, T b, T c, T d);
template <>
__device__ __forceinline__ void store4<float>(float* p, float a, float b, float c, float d) {
  *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
template <>
__device__ __forceinline__ void store4<double>(double* p, double a, double b, double c,
                                               double d) {
  *reinterpret_cast<double4*>(p) = make_double4(a, b, c, d);
}

struct EuclidParams {
  double sigma, epsilon, mindist, affinityeps;
};

struct PointNormalParams {
  double sigp, epsp, sign, epsn, affinityeps;
};

// A coordinate of the gathered point tables [d][pstride] at a 32-bit BYTE offset from the (wave-uniform) table
// pointer: one v_lshl_add per load and the load's own base + offset addressing, instead of a 64-bit multiply-add
// per address — the exact scores' twelve gathers per surviving pair were 5.9 M of the fill kernel's 61.9 M
// wave-instructions at m = 10k, at the 64-bit rate (profiles/pmc_r04.json). The tables are d * pstride * 8 bytes:
// 14 MB at m = 300 000 with normals; the host refuses point tables beyond 2^32 bytes (stage_inputs).
__device__ __forceinline__ double pt_at(const double* __restrict__ P, uint32_t byte_off) {
  return *reinterpret_cast<const double*>(reinterpret_cast<const char*>(P) + byte_off);
}

// ------------------------------------------------------------------------------------------
// The built-in invariants: one policy type each, everything a fill kernel knows about it.
//   Params   the parameter block the C ABI fills (affinityeps included)
//   N        fp64 coordinates of a datum: what the plain kernel keeps per column in registers and `exact` gathers
//            (0: run-time dimension — the plain kernel alone, through score_rt)
//   PD       coordinates the fp32 prefilter's two squared lengths run over (0: no prefilter, no tiles)
//   score    THE exact fp64 score of a pair, from the coordinates of its two rows and two columns in registers.
//            Every kernel's scores go through it, so that all routes give the same bits (the file compiles with
//            -ffp-contract=off: fma only where spelled out). `ok`: whether the pair passed the distinctness test
//            (clipper.cpp:35-38) — the plain kernel scores every pair and says so here, a prefilter's survivors have.
//   exact    the same for row r and column g of the gathered point tables (the survivors of a prefilter)
//   threshold / prefilter_dim   for the host: what guarded_threshold() is called with
// ------------------------------------------------------------------------------------------
template <typename Inv>
__device__ __forceinline__ double exact_score(const double* __restrict__ P1, const double* __restrict__ P2,
                                              int64_t pstride, int64_t r, int64_t g,
                                              const typename Inv::Params& prm) {
  const uint32_t pb = static_cast<uint32_t>(pstride) << 3, rb = static_cast<uint32_t>(r) << 3, gb = static_cast<uint32_t>(g) << 3;
  double p1r[Inv::N], p1g[Inv::N], p2r[Inv::N], p2g[Inv::N];
#pragma unroll
  for (int k = 0; k < Inv::N; ++k) {
    p1r[k] = pt_at(P1, k * pb + rb);
    p1g[k] = pt_at(P1, k * pb + gb);
    p2r[k] = pt_at(P2, k * pb + rb);
    p2g[k] = pt_at(P2, k * pb + gb);
  }
  return Inv::score(p1r, p1g, p2r, p2g, true, prm);
}

// EuclideanDistance (euclidean_distance.cpp:13-31). D > 0: compile-time dimension (2 or 3); D == 0: run-time.
template <int D>
struct EuclidInv {
  using Params = EuclidParams;
  static constexpr int N = D;
  static constexpr int PD = D;
  static double threshold(const Params& prm) { return prm.epsilon; }
  static int prefilter_dim(int staged_d) { return staged_d; }

  // everything after the squared lengths
  static __device__ __forceinline__ double from_squares(double s1, double s2, bool ok, const Params& prm) {
    const double l1 = sqrt(s1), l2 = sqrt(s2);
    if (prm.mindist > 0 && (l1 < prm.mindist || l2 < prm.mindist)) ok = false;  // :23-25
    const double cc = fabs(l1 - l2);                                            // :28
    return (ok && cc < prm.epsilon) ? exp(-0.5 * cc * cc / (prm.sigma * prm.sigma)) : 0.0;  // :30
  }
  static __device__ __forceinline__ double score(const double* p1r, const double* p1c, const double* p2r,
                                                 const double* p2c, bool ok, const Params& prm) {
    double s1 = 0.0, s2 = 0.0;  // :18-19, sequential fma chain
#pragma unroll
    for (int k = 0; k < D; ++k) {
      const double t1 = p1r[k] - p1c[k];
      const double t2 = p2r[k] - p2c[k];
      s1 = fma(t1, t1, s1);
      s2 = fma(t2, t2, s2);
    }
    return from_squares(s1, s2, ok, prm);
  }
  // run-time dimension d (slow path): the coordinates straight from the point tables
  static __device__ __forceinline__ double score_rt(const double* __restrict__ P1, const double* __restrict__ P2,
                                                    int64_t pstride, int d, int64_t r, int64_t g, bool ok,
                                                    const Params& prm) {
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < d; ++k) {
      const double t1 = P1[k * pstride + r] - P1[k * pstride + g];
      const double t2 = P2[k * pstride + r] - P2[k * pstride + g];
      s1 = fma(t1, t1, s1);
      s2 = fma(t2, t2, s2);
    }
    return from_squares(s1, s2, ok, prm);
  }
  static __device__ __forceinline__ double exact(const double* __restrict__ P1, const double* __restrict__ P2,
                                                 int64_t pstride, int64_t r, int64_t g, const Params& prm) {
    return exact_score<EuclidInv>(P1, P2, pstride, r, g, prm);
  }
};

// PointNormalDistance: datum = [x y z nx ny nz] (pointnormal_distance.cpp:13-35). The prefilter tests only the
// point-distance residual dp (the normal residual needs acos); survivors get the full exact evaluation.
struct PointNormalInv {
  using Params = PointNormalParams;
  static constexpr int N = 6;
  static constexpr int PD = 3;
  static double threshold(const Params& prm) { return prm.epsp; }
  static int prefilter_dim(int) { return 3; }

  static __device__ __forceinline__ double score(const double* p1r, const double* p1c, const double* p2r,
                                                 const double* p2c, bool ok, const Params& prm) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double t1 = p1r[k] - p1c[k];
      const double t2 = p2r[k] - p2c[k];
      s1 = fma(t1, t1, s1);
      s2 = fma(t2, t2, s2);
    }
    const double l1 = sqrt(s1), l2 = sqrt(s2);  // :17-18
    const double dot1 = fma(p1r[5], p1c[5], fma(p1r[4], p1c[4], p1r[3] * p1c[3]));
    const double dot2 = fma(p2r[5], p2c[5], fma(p2r[4], p2c[4], p2r[3] * p2c[3]));
    double scr = 0.0;
    if (ok) {
      const double alpha1 = acos(dot1);  // :21 (NaN when |dot| > 1, as in the reference)
      const double alpha2 = acos(dot2);  // :22
      const double dp = fabs(l1 - l2);          // :25
      const double dn = fabs(alpha1 - alpha2);  // :26
      if (dp < prm.epsp && dn < prm.epsn) {     // :28
        const double sp = exp(-0.5 * dp * dp / (prm.sigp * prm.sigp));  // :29
        const double sn = exp(-0.5 * dn * dn / (prm.sign * prm.sign));  // :30
        scr = sp * sn;                                                  // :31
      }
    }
    return scr;
  }
  static __device__ __forceinline__ double exact(const double* __restrict__ P1, const double* __restrict__ P2,
                                                 int64_t pstride, int64_t r, int64_t g, const Params& prm) {
    return exact_score<PointNormalInv>(P1, P2, pstride, r, g, prm);
  }
};

// Plain fill. One thread = 4 adjacent columns of S, looping down `rows_per_blk` rows; the 4 columns'
// points and association indices stay in registers for the whole loop, the row's point is
// wave-uniform (scalar loads). Each lane stores 4 consecutive elements, a wave 256: whole
// 1 KiB (fp32) row segments per store instruction. `d`: the run-time dimension, read where Inv::N == 0.
template <typename T, typename Inv>
__global__ __launch_bounds__(256) void k_affinity_plain(
    T* __restrict__ S, int64_t ld, int64_t m, int64_t c0, int rows_per_blk, int d,
    const double* __restrict__ P1, const double* __restrict__ P2, int64_t pstride,
    const int32_t* __restrict__ A0, const int32_t* __restrict__ A1, typename Inv::Params prm) {
  const int64_t c = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) * 4;
  if (c >= ld) return;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_blk;
  const int64_t r1 = (r0 + rows_per_blk < m) ? r0 + rows_per_blk : m;
  constexpr int N = Inv::N;
  constexpr int NN = (N > 0) ? N : 1;

  int64_t gi[4];
  bool valid[4];
  int32_t a0c[4], a1c[4];
  double p1c[4][NN], p2c[4][NN];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t g = c0 + c + q;
    valid[q] = g < m;
    gi[q] = valid[q] ? g : (m - 1);
    a0c[q] = A0[gi[q]];
    a1c[q] = A1[gi[q]];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      p1c[q][k] = P1[k * pstride + gi[q]];
      p2c[q][k] = P2[k * pstride + gi[q]];
    }
  }

  for (int64_t r = r0; r < r1; ++r) {
    const int32_t a0r = A0[r], a1r = A1[r];
    double p1r[NN], p2r[NN];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      p1r[k] = P1[k * pstride + r];
      p2r[k] = P2[k * pstride + r];
    }
    T out[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      // clipper.cpp:35-38 distinctness; the diagonal (r == column) fails it by construction
      // (&: three compares of registers, handed to the score as one value — no branch of its own ahead of the score's)
      const bool ok = valid[q] & (a0r != a0c[q]) & (a1r != a1c[q]);
      double scr;
      if constexpr (N > 0) scr = Inv::score(p1r, p1c[q], p2r, p2c[q], ok, prm);
      else scr = Inv::score_rt(P1, P2, pstride, d, r, gi[q], ok, prm);
      out[q] = store_score<T>(scr, prm.affinityeps);
    }
    store4<T>(S + r * ld + c, out[0], out[1], out[2], out[3]);
  }
}

// ------------------------------------------------------------------------------------------
// Compacting fill kernels.
//
// The exact score costs ~150 fp64-rate instructions per pair (two correctly rounded sqrt, one
// division, exp / acos), yet on registration data only ~10 % of the pairs pass `c < epsilon`
// — and with 64-lane waves a plain branch saves nothing. So every pair first goes through a
// CONSERVATIVE fp32 prefilter (|l1f - l2f| >= epsilon + guard  =>  certainly c >= epsilon; the
// guard bounds the fp32 error from the data's magnitude, incl. the 1-ulp raw v_sqrt_f32), survivors are compacted into a
// per-wave LDS queue with ballot/mbcnt (no atomics, no workgroup barrier), and only they are
// evaluated exactly in fp64 — by the policy's one `score`, as in the plain kernel, so the
// results are bit-identical to it. Scores are scattered into an LDS staging tile and leave
// as whole 1 KiB row segments, so the HBM store pattern is unchanged.
// Geometry: 4 waves per workgroup, wave w owns 256 columns (4 per lane); rows are processed in
// groups of AFF_RG = 8: queue 8 KiB + staging 8 (fp32) / 16 (fp64) KiB per wave.
// ------------------------------------------------------------------------------------------

constexpr int AFF_RG = 8;

__device__ __forceinline__ uint32_t lane_prefix(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

template <typename T, typename Inv>
__global__ __launch_bounds__(256) void k_affinity_compact(
    T* __restrict__ S, int64_t ld, int64_t m, int64_t c0, int rows_per_blk,
    const double* __restrict__ P1, const double* __restrict__ P2,
    const float* __restrict__ P1f, const float* __restrict__ P2f, int64_t pstride,
    const int32_t* __restrict__ A0, const int32_t* __restrict__ A1, typename Inv::Params prm,
    float eps_guarded) {
  constexpr int PD = Inv::PD;
  __shared__ uint32_t queue[4][AFF_RG * 256];
  __shared__ T stage[4][AFF_RG][256];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t cw = static_cast<int64_t>(blockIdx.x) * 1024 + wave * 256;  // wave's first column
  const int64_t c = cw + lane * 4;
  const int64_t r0 = static_cast<int64_t>(blockIdx.y) * rows_per_blk;
  const int64_t r1 = (r0 + rows_per_blk < m) ? r0 + rows_per_blk : m;
  if (cw >= ld) return;  // whole wave outside the slice (wave-uniform)

  // column data (fp32) in registers for the prefilter
  bool valid[4];
  int32_t a0c[4], a1c[4];
  float p1c[4][PD], p2c[4][PD];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t g = c0 + c + q;
    valid[q] = (g < m) && (c + q < ld);
    const int64_t gi = (g < m) ? g : (m - 1);
    a0c[q] = A0[gi];
    a1c[q] = A1[gi];
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      p1c[q][k] = P1f[k * pstride + gi];
      p2c[q][k] = P2f[k * pstride + gi];
    }
  }
#pragma unroll
  for (int r8 = 0; r8 < AFF_RG; ++r8)
#pragma unroll
    for (int q = 0; q < 4; ++q) stage[wave][r8][lane * 4 + q] = T(0);

  for (int64_t base = r0; base < r1; base += AFF_RG) {
    // ---- phase A: fp32 prefilter + compaction of the surviving (row, column) pairs --------
    uint32_t count = 0;  // wave-uniform
#pragma unroll
    for (int r8 = 0; r8 < AFF_RG; ++r8) {
      const int64_t r = base + r8;
      if (r < r1) {  // uniform
        const int32_t a0r = A0[r], a1r = A1[r];
        float p1r[PD], p2r[PD];
#pragma unroll
        for (int k = 0; k < PD; ++k) {
          p1r[k] = P1f[k * pstride + r];
          p2r[k] = P2f[k * pstride + r];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          float s1 = 0.f, s2 = 0.f;
#pragma unroll
          for (int k = 0; k < PD; ++k) {
            const float t1 = p1r[k] - p1c[q][k];
            const float t2 = p2r[k] - p2c[q][k];
            s1 = fmaf(t1, t1, s1);
            s2 = fmaf(t2, t2, s2);
          }
          // the strip form of the prefilter (tests/prefilter_model.py)
          const float cf = fabsf(__builtin_amdgcn_sqrtf(s1) - __builtin_amdgcn_sqrtf(s2));
          // clipper.cpp:35-38 distinctness (also removes the diagonal) + conservative c < eps
          const bool cand = valid[q] && (a0r != a0c[q]) && (a1r != a1c[q]) && (cf < eps_guarded);
          const uint64_t mask = __ballot(cand);
          if (mask != 0) {  // uniform
            if (cand) queue[wave][count + lane_prefix(mask)] =
                (static_cast<uint32_t>(r8) << 16) | static_cast<uint32_t>(lane * 4 + q);
            count += static_cast<uint32_t>(__popcll(mask));
          }
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- phase B: exact fp64 score of the survivors, scattered into the staging tile -------
    for (uint32_t e = lane; e < count; e += 64) {
      const uint32_t code = queue[wave][e];
      const int r8 = static_cast<int>(code >> 16);
      const int cl = static_cast<int>(code & 0xffffu);
      const double scr = Inv::exact(P1, P2, pstride, base + r8, c0 + cw + cl, prm);
      stage[wave][r8][cl] = store_score<T>(scr, prm.affinityeps);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- phase C: whole row segments leave for HBM; the staging tile is re-zeroed ----------
    if (c < ld) {
#pragma unroll
      for (int r8 = 0; r8 < AFF_RG; ++r8) {
        const int64_t r = base + r8;
        if (r < r1) {
          T* sp = &stage[wave][r8][lane * 4];
          store4<T>(S + r * ld + c, sp[0], sp[1], sp[2], sp[3]);
          sp[0] = sp[1] = sp[2] = sp[3] = T(0);
        }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
}

// ------------------------------------------------------------------------------------------
// Symmetric fill (one shard, fp32 storage): M is symmetric and the score of (i, j) is bit-equal
// to the score of (j, i) (squares and absolute differences only), so only the 128 x 128 tiles
// of the upper block triangle are evaluated — prefilter and exact scores cost half — and every
// off-diagonal tile leaves twice: as it stands, and transposed out of an LDS image with an odd
// row pitch (bank-conflict-free column reads), both as 512-byte row segments.
// The prefilter needs no square root (prefilter_close, with E = the guarded threshold). Survivors get the
// same exact fp64 evaluation as in the other fill kernels: identical bits.
// Geometry: 8 waves; wave w owns tile rows [16w, 16w + 16), lane l tile columns 2l, 2l + 1.
// ------------------------------------------------------------------------------------------

constexpr int AT = 128;           // tile edge
constexpr int AT_PITCH = AT + 1;  // LDS image row pitch in floats
#ifndef CLIPPER_AT_WAVES
#define CLIPPER_AT_WAVES 8
#endif
constexpr int AT_WAVES = CLIPPER_AT_WAVES;       // waves per workgroup
constexpr int AT_ROWS_PER_WAVE = AT / AT_WAVES;  // tile rows a wave owns
constexpr int AT_QUEUE = 256;     // ring entries per wave: < 64 waiting + one row's 128 candidates
// (VT = float: 76.5 KiB, two workgroups per CU; VT = double — the slices with fp64 values, round 4 —: 141 KiB, one
// workgroup per CU, but every pair of the matrix is scored ONCE: the rectangular kernel, which has no mirror image,
// scores it twice)
template <typename VT = float>
constexpr int at_sym_img_bytes() { return (AT * AT_PITCH * static_cast<int>(sizeof(VT)) + 15) / 16 * 16; }
constexpr int AT_SYM_MASK_BYTES = 2 * AT * 16;  // nonzero masks of the tile's columns and of its rows
template <typename VT = float>
constexpr int at_sym_lds_bytes() { return at_sym_img_bytes<VT>() + AT_WAVES * AT_QUEUE * 4 + AT_SYM_MASK_BYTES; }
constexpr int AT_SYM_IMG_BYTES = at_sym_img_bytes<float>();
constexpr int AT_SYM_LDS_BYTES = at_sym_lds_bytes<float>();

// linear index t of the upper block triangle (row-major: (0,0) (0,1) ... (1,1) ...) -> (I, J)
__device__ __forceinline__ void tile_of(int t, int nT, int& I, int& J) {
  const float b = 2.0f * nT + 1.0f;
  int i = static_cast<int>((b - sqrtf(b * b - 8.0f * static_cast<float>(t))) * 0.5f);
  if (i < 0) i = 0;
  if (i > nT - 1) i = nT - 1;
  // first(i) = i*nT - i*(i-1)/2 is the index of tile (i, i); fix the float estimate
  while (i > 0 && i * nT - i * (i - 1) / 2 > t) --i;
  while (i + 1 < nT && (i + 1) * nT - (i + 1) * i / 2 <= t) ++i;
  I = i;
  J = i + (t - (i * nT - i * (i - 1) / 2));
}

// ---- what the two tile kernels (k_affinity_sym, k_affinity_rect) share --------------------------------------------

// A lane's NC tile columns: fp32 copies for the prefilter
template <int PD, int NC>
struct TileColumns {
  bool valid[NC];
  int32_t a0[NC], a1[NC];
  float p1[NC][PD], p2[NC][PD];
  // column q is association g where `ok`, a stand-in otherwise (never a candidate)
  __device__ __forceinline__ void load(int q, bool ok, int64_t g, int64_t m, const float* __restrict__ P1f,
                                       const float* __restrict__ P2f, int64_t pstride,
                                       const int32_t* __restrict__ A0, const int32_t* __restrict__ A1) {
    valid[q] = ok;
    const int64_t gi = ok ? g : (m - 1);
    a0[q] = A0[gi];
    a1[q] = A1[gi];
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      p1[q][k] = P1f[k * pstride + gi];
      p2[q][k] = P2f[k * pstride + gi];
    }
  }
};

// A wave's tile rows: lane i fetches row i's association and points ONCE (one vector load per quantity); the row
// loop broadcasts them with v_readlane — a scalar load per row and quantity was a chain of AT_ROWS_PER_WAVE
// dependent L2 round trips
template <int PD>
struct TileRows {
  int32_t a0, a1;
  float p1[PD], p2[PD];
  __device__ __forceinline__ void load(int64_t ri /* this lane's row: an association */, const float* __restrict__ P1f,
                                       const float* __restrict__ P2f, int64_t pstride,
                                       const int32_t* __restrict__ A0, const int32_t* __restrict__ A1) {
    a0 = A0[ri];
    a1 = A1[ri];
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      p1[k] = P1f[k * pstride + ri];
      p2[k] = P2f[k * pstride + ri];
    }
  }
  __device__ __forceinline__ void broadcast(int rr, int32_t& a0r, int32_t& a1r, float* p1r, float* p2r) const {
    a0r = __builtin_amdgcn_readlane(a0, rr);
    a1r = __builtin_amdgcn_readlane(a1, rr);
#pragma unroll
    for (int k = 0; k < PD; ++k) {
      p1r[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p1[k]), rr));
      p2r[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(p2[k]), rr));
    }
  }
};

// The fp32 squared lengths of a pair for the tile kernels' prefilter. (k_affinity_compact forms them with the same loop
// written out: called from there, this helper cost its PointNormal instantiations 8 more s_waitcnt.)
template <int PD>
__device__ __forceinline__ void prefilter_squares(const float* p1r, const float* p1c, const float* p2r,
                                                  const float* p2c, float& s1, float& s2) {
  s1 = 0.f;
  s2 = 0.f;
#pragma unroll
  for (int k = 0; k < PD; ++k) {
    const float t1 = p1r[k] - p1c[k];
    const float t2 = p2r[k] - p2c[k];
    s1 = fmaf(t1, t1, s1);
    s2 = fmaf(t2, t2, s2);
  }
}

// The sqrt-free form of the prefilter (tests/prefilter_model.py): |l1 - l2| < E  <=>  t <= 0  or  t^2 < 4 s1 s2 with
// t = s1 + s2 - E^2; the right-hand side carries a 2^-18 relative margin for the fp32 roundings of t, t^2 and s1 s2.
// `wave`: the same over the wave's lanes, every compare balloted on its own and the masks joined with scalar logic (a
// ballot of the joined predicate makes the compiler write it into a register as 0 / 1 and compare that again).
__device__ __forceinline__ bool prefilter_close(float s1, float s2, float E2, uint64_t& wave) {
  const float t = (s1 + s2) - E2;
  const bool inside = t <= 0.f, near = t * t < (4.0f * 1.0000038147f) * (s1 * s2);
  wave = __builtin_amdgcn_ballot_w64(inside) | __builtin_amdgcn_ballot_w64(near);
  return inside | near;
}

// This wave's AT_ROWS_PER_WAVE rows of a tile against the lane's NC columns: the survivors of the fp32 prefilter go
// into the wave's ring; whenever 64 are waiting they are evaluated by a full wave (the exact score is ~150 fp64-rate
// instructions: no idle lanes), the rest at the end. scatter(rl, cl): the kernel's exact score of tile element
// (rl, cl) into its image. Tile rows r0 + rl >= nrows do not exist.
template <int PD, int NC, typename Scatter>
__device__ __forceinline__ void tile_score_rows(const TileColumns<PD, NC>& col, const TileRows<PD>& row, int64_t r0,
                                                int64_t nrows, float E2, uint32_t* queue, int lane, int wave,
                                                Scatter&& scatter) {
  // exact fp64 score of queue entries [head, head + n)
  auto drain = [&](uint32_t head, uint32_t n) {
    if (lane < n) {
      const uint32_t code = queue[(head + lane) & (AT_QUEUE - 1)];
      scatter(static_cast<int>(code >> 8), static_cast<int>(code & 0xffu));
    }
  };
  uint32_t head = 0, tail = 0;  // wave-uniform
  uint64_t valid[NC];           // col.valid over the wave
#pragma unroll
  for (int q = 0; q < NC; ++q) valid[q] = __builtin_amdgcn_ballot_w64(col.valid[q]);
  // the wave's rows that exist: a scalar loop bound (tested per row against the 64-bit nrows it was a vector compare)
  const int64_t left = nrows - (r0 + wave * AT_ROWS_PER_WAVE);
  const int live = __builtin_amdgcn_readfirstlane(left < AT_ROWS_PER_WAVE ? (left > 0 ? static_cast<int>(left) : 0)
                                                                          : AT_ROWS_PER_WAVE);
  for (int rr = 0; rr < live; ++rr) {
    const int rl = wave * AT_ROWS_PER_WAVE + rr;  // tile row
    int32_t a0r, a1r;
    float p1r[PD], p2r[PD];
    row.broadcast(rr, a0r, a1r, p1r, p2r);
#pragma unroll
    for (int q = 0; q < NC; ++q) {
      float s1, s2;
      prefilter_squares<PD>(p1r, col.p1[q], p2r, col.p2[q], s1, s2);
      // clipper.cpp:35-38 distinctness (also removes the diagonal) + conservative c < eps
      // (no `&&`: the packed arithmetic runs for every pair — an exec region around it costs more. `cand` is the lane's
      // own bit of `mask`, kept beside it: the queue write's exec mask)
      const bool d0 = a0r != col.a0[q], d1 = a1r != col.a1[q];
      uint64_t close;
      const bool cand = col.valid[q] & d0 & d1 & prefilter_close(s1, s2, E2, close);
      const uint64_t mask = valid[q] & __builtin_amdgcn_ballot_w64(d0) & __builtin_amdgcn_ballot_w64(d1) & close;
      if (mask != 0) {  // uniform
        if (cand) queue[(tail + lane_prefix(mask)) & (AT_QUEUE - 1)] =
            (static_cast<uint32_t>(rl) << 8) | static_cast<uint32_t>(NC * lane + q);
        tail += static_cast<uint32_t>(__popcll(mask));
      }
    }
    if (tail - head >= 64) {  // uniform
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      while (tail - head >= 64) {
        drain(head, 64);
        head += 64;
      }
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  while (head < tail) {
    const uint32_t n = (tail - head < 64) ? tail - head : 64;
    drain(head, n);
    head += n;
  }
}

template <typename Inv, typename VT = float>
__global__ __launch_bounds__(AT_WAVES * 64, AT_WAVES / 2) void k_affinity_sym(
    VT* __restrict__ S, int64_t ld, int64_t m, int nT, const double* __restrict__ P1,
    const double* __restrict__ P2, const float* __restrict__ P1f, const float* __restrict__ P2f,
    int64_t pstride, const int32_t* __restrict__ A0, const int32_t* __restrict__ A1,
    typename Inv::Params prm, float E2 /* guarded threshold squared, rounded up */,
    CscOut O /* O.Pre != null: also write the tile's slices (k_csc.hip.h) */) {
  // 76.5 KiB of dynamic LDS (two workgroups per CU fit the 160 KiB): the image, the queues, the masks
  extern __shared__ __attribute__((aligned(16))) char sym_smem[];
  const bool stamp = O.stamps != nullptr && blockIdx.x < 800 && threadIdx.x == 0;
  long long ts[5] = {0, 0, 0, 0, 0};
  if (stamp) ts[0] = wall_clock64();
  VT* img = reinterpret_cast<VT*>(sym_smem);
  constexpr int IMG_BYTES = at_sym_img_bytes<VT>();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* queue = reinterpret_cast<uint32_t*>(sym_smem + IMG_BYTES) + wave * AT_QUEUE;
  int I, J;
  // Tiles from both ends of the row-major order towards the middle: the tiles of a dense block —
  // twice the work of the others — sit where the consistent associations sit in the list, at its
  // end in the reference's benchmark layout (bm_utils.cpp:311-314: inliers behind the outliers) or at
  // its start (matches sorted best first); launched last they are the launch's tail (195 -> 168 us
  // at m = 10k)
  const int tb = static_cast<int>(blockIdx.x);
  tile_of((tb & 1) ? static_cast<int>(gridDim.x) - 1 - (tb >> 1) : (tb >> 1), nT, I, J);
  const int64_t r0 = static_cast<int64_t>(I) * AT, c0 = static_cast<int64_t>(J) * AT;

  // this lane's two columns
  TileColumns<Inv::PD, 2> cols;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int64_t g = c0 + 2 * lane + q;
    cols.load(q, g < m, g, m, P1f, P2f, pstride, A0, A1);
  }
  // colmask[cl][4] / rowmask[rl][4]: which rows of tile column cl / columns of tile row rl hold a
  // nonzero — set by the scatter below, read by the emission of the slices
  uint32_t* colmask = reinterpret_cast<uint32_t*>(sym_smem + IMG_BYTES + AT_WAVES * AT_QUEUE * 4);
  uint32_t* rowmask = colmask + AT * 4;
  colmask[threadIdx.x] = 0;
  rowmask[threadIdx.x] = 0;
  if (S != nullptr) {  // the dense store gets the whole image: zero this wave's rows of it
#pragma unroll 4
    for (int rr = 0; rr < AT_ROWS_PER_WAVE; ++rr) {
      VT* row = img + (wave * AT_ROWS_PER_WAVE + rr) * AT_PITCH;
      row[2 * lane] = VT(0);
      row[2 * lane + 1] = VT(0);
    }
  }
  __syncthreads();  // the column masks are shared by all waves

  // this wave's rows
  TileRows<Inv::PD> rows;
  {
    const int64_t rw = r0 + wave * AT_ROWS_PER_WAVE + (lane < AT_ROWS_PER_WAVE ? lane : 0);
    rows.load(rw < m ? rw : (m - 1), P1f, P2f, pstride, A0, A1);
  }
  tile_score_rows(cols, rows, r0, m, E2, queue, lane, wave, [&](int rl, int cl) {
    const VT v = store_score<VT>(Inv::exact(P1, P2, pstride, r0 + rl, c0 + cl, prm), prm.affinityeps);
    img[rl * AT_PITCH + cl] = v;
    if (v != VT(0)) {
      atomicOr(&colmask[cl * 4 + (rl >> 5)], 1u << (rl & 31));
      atomicOr(&rowmask[rl * 4 + (cl >> 5)], 1u << (cl & 31));
    }
  });
  if (stamp) ts[1] = wall_clock64();
  __syncthreads();

  // ---- the slices (k_slices.hip.h) of the tile and of its mirror image, straight from the image:
  // (column group 2J + e, chunk I) and (column group 2I + e, chunk J), two waves per slice ----------
  if (O.Pre != nullptr) {
    static_assert(AT_WAVES == 8 && AT == SL_SUB && AT == 2 * SL_W, "four slices per tile");
    unsigned long long* base_s = reinterpret_cast<unsigned long long*>(sym_smem + IMG_BYTES);  // the queues are drained
    const int sl = wave & 3, half = wave >> 2;
    const int e = sl & 1;
    const bool mirror = sl >= 2;
    // element q of the lane's column: tile (q, 64 e + lane), or (64 e + lane, q) of the mirror
    const VT* col = mirror ? img + (64 * e + lane) * AT_PITCH : img + 64 * e + lane;
    const uint4 mk = *reinterpret_cast<const uint4*>((mirror ? rowmask : colmask) + (64 * e + lane) * 4);
    const int cg = 2 * (mirror ? I : J) + e;
    const int k = mirror ? J : I;
    const int64_t s = (cg < O.ncg && k < O.nchunks && !(mirror && I == J))
                          ? static_cast<int64_t>(cg) * O.nchunks + k : -1;
    slice_emit_lds(col, mirror ? 1 : AT_PITCH, mk, s, sl, half, O, base_s, stamp ? ts + 2 : nullptr);
    if (stamp) {
      ts[4] = wall_clock64();
      for (int i = 0; i < 5; ++i) O.stamps[blockIdx.x * 5 + i] = ts[i];
    }
  }

  // ---- the tile as it stands: this wave's rows, 512-byte segments -----------------------------
  if (S != nullptr && c0 + 2 * lane < ld) {
    for (int rr = 0; rr < AT_ROWS_PER_WAVE; ++rr) {
      const int rl = wave * AT_ROWS_PER_WAVE + rr;
      const int64_t r = r0 + rl;
      if (r < m) {
        const VT* row = img + rl * AT_PITCH + 2 * lane;
        if constexpr (sizeof(VT) == 4) *reinterpret_cast<float2*>(S + r * ld + c0 + 2 * lane) = make_float2(row[0], row[1]);
        else *reinterpret_cast<double2*>(S + r * ld + c0 + 2 * lane) = make_double2(row[0], row[1]);
      }
    }
  }
  // ---- and transposed: rows c0 + ... receive the tile's columns ------------------------------
  if (S != nullptr && I != J && r0 + 2 * lane < ld) {
    for (int cc = 0; cc < AT_ROWS_PER_WAVE; ++cc) {
      const int cl = wave * AT_ROWS_PER_WAVE + cc;
      const int64_t c = c0 + cl;
      if (c < m) {
        const VT v0 = img[(2 * lane) * AT_PITCH + cl];
        const VT v1 = img[(2 * lane + 1) * AT_PITCH + cl];
        if constexpr (sizeof(VT) == 4) *reinterpret_cast<float2*>(S + c * ld + r0 + 2 * lane) = make_float2(v0, v1);
        else *reinterpret_cast<double2*>(S + c * ld + r0 + 2 * lane) = make_double2(v0, v1);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------
// Rectangular fill: the slices of M[R, C] for a row LIST R (any subset of the associations, in
// list order — or all of them) and a column RANGE C, written straight from the LDS image of a
// 128 x TW tile exactly like k_affinity_sym writes its own (same prefilter, same exact fp64
// scores, same bits), but without the mirror image: every tile is evaluated where it is needed.
// This is the fill of everything the symmetric kernel cannot serve:
//   * fp64 values (CLIPPER_HIP_STORE_F64_CSC): the image holds doubles, the tile is 64 columns
//     wide (one slice) so that two workgroups still share a CU — no dense fp64 store at any size;
//   * column shards: C = the shard's columns, R = all rows — no dense slice, no packers;
//   * the ROW VIEW of the solver (host_rowview.hpp): R = the rows whose candidate entries can be
//     non-zero at all, C = all columns; row r' of the view is association rowmap[r'].
// Geometry as k_affinity_sym: 8 waves, wave w owns tile rows [16 w, 16 w + 16), lane l tile
// columns CPL l .. CPL l + CPL - 1 (CPL = TW / 64).
// ------------------------------------------------------------------------------------------
struct RectGeom {
  int64_t m;             // associations
  int64_t nrows;         // rows of the view
  const int32_t* rowmap; // [nrows] association of view row r' (null: r' itself)
  int64_t col0, ncols;   // the view's columns are associations [col0, col0 + ncols)
  int nTc;               // column tiles (tile t = row tile t / nTc, column tile t % nTc)
  int64_t tile0;         // first tile of this launch (a dispatch holds at most 2^32 work-items: the 11 M
                         // tiles of m = 300 000 with fp64 values take three launches)
};

template <typename VT>
constexpr int rect_tw() { return sizeof(VT) == 4 ? 128 : 64; }
// (TW = 64 for fp32 values too: a THIN view — a few row tiles — is a launch of fewer workgroups than the chip
// holds, whose duration is that of its heaviest tile, the inlier block's; half as wide, that tile takes half as long)
template <typename VT, int TW = rect_tw<VT>()>
constexpr int rect_img_bytes() { return (AT * (TW + 1) * static_cast<int>(sizeof(VT)) + 15) / 16 * 16; }
template <typename VT, int TW = rect_tw<VT>()>
constexpr int rect_lds_bytes() {
  return rect_img_bytes<VT, TW>() + AT_WAVES * AT_QUEUE * 4 + TW * 16 + AT * 4;
}

template <typename Inv, typename VT, int TW = rect_tw<VT>()>
__global__ __launch_bounds__(AT_WAVES * 64, AT_WAVES / 2) void k_affinity_rect(
    RectGeom G, const double* __restrict__ P1, const double* __restrict__ P2,
    const float* __restrict__ P1f, const float* __restrict__ P2f, int64_t pstride,
    const int32_t* __restrict__ A0, const int32_t* __restrict__ A1, typename Inv::Params prm, float E2,
    SliceOut O) {
  constexpr int CPL = TW / 64;
  constexpr int PITCH = TW + 1;
  static_assert(AT_WAVES == 8 && AT == SL_SUB && (TW == 64 || TW == 128), "a tile is as tall as a slice");
  extern __shared__ __attribute__((aligned(16))) char rect_smem[];
  VT* img = reinterpret_cast<VT*>(rect_smem);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  uint32_t* queue = reinterpret_cast<uint32_t*>(rect_smem + rect_img_bytes<VT, TW>()) + wave * AT_QUEUE;
  uint32_t* colmask = reinterpret_cast<uint32_t*>(rect_smem + rect_img_bytes<VT, TW>() + AT_WAVES * AT_QUEUE * 4);
  int32_t* rowidx = reinterpret_cast<int32_t*>(colmask + TW * 4);
  // heaviest tiles first where that is known: the consistent associations sit at the end of the
  // list in the reference's benchmark layout (bm_utils.cpp:311-314), so the column tiles run backwards
  const int64_t tile = G.tile0 + blockIdx.x;
  const int I = static_cast<int>(tile / G.nTc);
  const int J = G.nTc - 1 - static_cast<int>(tile % G.nTc);
  const int64_t r0 = static_cast<int64_t>(I) * AT;          // first view row of the tile
  const int64_t cl0 = static_cast<int64_t>(J) * TW;          // first view column of the tile

  // this lane's columns
  TileColumns<Inv::PD, CPL> cols;
#pragma unroll
  for (int q = 0; q < CPL; ++q) {
    const int64_t lc = cl0 + CPL * lane + q;
    const int64_t g = G.col0 + lc;
    cols.load(q, lc < G.ncols && g < G.m, g, G.m, P1f, P2f, pstride, A0, A1);
  }
  for (int t = threadIdx.x; t < TW * 4; t += AT_WAVES * 64) colmask[t] = 0;
  if (threadIdx.x < AT) {
    const int64_t r = r0 + threadIdx.x;
    const int64_t rc = r < G.nrows ? r : (G.nrows - 1);
    rowidx[threadIdx.x] = G.rowmap ? G.rowmap[rc] : static_cast<int32_t>(rc);
  }
  __syncthreads();

  TileRows<Inv::PD> rows;
  rows.load(rowidx[wave * AT_ROWS_PER_WAVE + (lane < AT_ROWS_PER_WAVE ? lane : 0)], P1f, P2f, pstride, A0, A1);
  tile_score_rows(cols, rows, r0, G.nrows, E2, queue, lane, wave, [&](int rl, int cl) {
    const int64_t ra = rowidx[rl], ca = G.col0 + cl0 + cl;
    const VT v = store_score<VT>(Inv::exact(P1, P2, pstride, ra, ca, prm), prm.affinityeps);
    if (v != VT(0)) {
      img[rl * PITCH + cl] = v;
      atomicOr(&colmask[cl * 4 + (rl >> 5)], 1u << (rl & 31));
    }
  });
  __syncthreads();

  // ---- the tile's CPL slices (column group cl0 / 64 + e, chunk I), two waves per slice ------------
  unsigned long long* base_s = reinterpret_cast<unsigned long long*>(rect_smem + rect_img_bytes<VT, TW>());  // the queues are drained
  const int sl = wave & 3, half = wave >> 2;
  const int e = sl < CPL ? sl : 0;
  const VT* col = img + 64 * e + lane;
  const uint4 mk = *reinterpret_cast<const uint4*>(colmask + (64 * e + lane) * 4);
  const int cg = static_cast<int>(cl0 / 64) + e;
  const int64_t s = (sl < CPL && cg < O.ncg && I < O.nchunks) ? static_cast<int64_t>(cg) * O.nchunks + I : -1;
  slice_emit_lds<VT>(col, PITCH, mk, s, sl, half, O, base_s, nullptr);
}

}  // namespace clipper_hip
