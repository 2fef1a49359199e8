// k_sdp.hip.h — the semidefinite relaxation behind CLIPPER::solveAsMSRCSDR and sdp::solve:
// ADMM on X = Z with X in the spectraplex and Z in the polyhedral set of C, one workgroup per problem, fp64
// throughout; k_sdp runs one problem, k_sdp_batch many side by side (a work list, one workgroup per entry) with the
// same body, and k_sdp_gather_batch / k_sdp_round_batch build the inputs and round the results of a batch. Host side:
// host_sdp.hpp, host_sdpbatch.hpp.
// Part of kernels.hip.h (include that one): hand-written gfx950 device code of the CLIPPER hot path.
//
// Layout of one problem (n <= SDP_MAX_N, np = n rounded up to even): M, the mask of C (1.0 / 0.0), X, Z and U are
// n x n row-major in global memory (all symmetric); Q (the eigenbasis of the last projection) and T (the warm
// start's product) are np x np; mu holds the np simplex weights of the last projection (the pad index: 0). The
// working matrix of the eigensolver is np x np in LDS (128 KiB at np = 128); Q cannot join it there and stays in
// global memory, where the L2 holds it (128 KiB).
//
// Eigensolver: cyclic Jacobi in round-robin (circle) order: in each of the np - 1 steps of a sweep the np / 2
// disjoint pairs rotate together, every 2 x 2 block of the working matrix is rotated on both sides by one work
// item (which writes its transpose too: the matrix stays exactly symmetric), and the pad index (odd n) keeps a zero
// row, so its rotations are the identity. Each projection starts from Q_prev^T W Q_prev, nearly diagonal once the
// iteration settles, and sweeps until the off-diagonal mass is below SDP_JACOBI_TOL of the whole.
//
// Every launch runs at most `budget` iterations and leaves X, Z, U, Q, mu and SdpCtl in device memory; the host
// checks the convergence flag and the time limit between launches. No grid barrier, no atomics across workgroups.
//
// The arithmetic of the iteration (constants, SdpCtl, INIT values, the formed matrices, the rotations, the simplex
// rule, one entry's update, the stopping rule, the balancing) is stated in sdp_rules.hpp, and the circle order in
// sdp_circle.hpp, for this route and the wide one (k_sdp_wide.hip.h); this file adds what a workgroup does with them:
// which work item holds which entry, and the order of every sum. The device helpers that both routes call live here
// too: sdp_block_sum, sdp_gather_entry.
// k_sdp and k_sdp_batch are one inlined function each that spills, and their register allocation moves as a whole
// when some rules are inlined from the header instead of written in place (0.7 % of the solve at n = 128). Those
// rules stay spelled out here, each marked with the name of its statement in sdp_rules.hpp, so that both kernels keep
// the instruction stream they had: sdp_norms_add, sdp_rotate_diag, sdp_init_entry, sdp_support / sdp_support_tau,
// the terms of sdp_update_entry (Z+ itself comes from sdp_z_plus), sdp_residuals, sdp_balance_factor and
// sdp_close_iteration (its schedule step, sdp_balance_advance, and the no-valid-support rule, sdp_fallback_index /
// sdp_fallback_weight, are called: one work item, off the hot path). A change to one of them in the header is made
// here too; tests/test_gpu_sdp_wide.py holds the two routes to each other.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sdp_circle.hpp"
#include "sdp_rules.hpp"

namespace clipper_hip {

constexpr int SDP_MAX_N = 128;          // the working matrix: SDP_MAX_N^2 doubles of LDS
constexpr int SDP_THREADS = 1024;

enum { SDP_MODE_INIT = 0, SDP_MODE_ITERATE = 1, SDP_MODE_CERTIFY = 2 };

struct SdpArgs {
  const double* M;
  const double* mask;
  double *X, *Z, *U, *Q, *T, *mu;
  SdpCtl* ctl;
  int32_t n, np;
  double eps_abs, eps_rel;
};

// Entry (a, b) of the dense fp64 M and of the mask of C, from stores of doubles (f64) or floats where element (r, c)
// sits at src[r * rs + c * cs]; only the lower triangle (r >= c) is read. `ident` is added to the diagonal of both (the
// context's identity, clipper.cpp:133-143); with c_pattern_of_m, C = pattern(M + ident I) and srcC is not read.
__device__ inline void sdp_gather_entry(const void* srcM, const void* srcC, int f64, int c_pattern_of_m, int64_t rs,
                                        int64_t cs, int32_t a, int32_t b, double ident, double& mv, double& mask) {
  const int32_t r = a > b ? a : b, c = a > b ? b : a;
  const int64_t e = r * rs + c * cs;
  const double d = (a == b) ? ident : 0.0;
  mv = (f64 ? static_cast<const double*>(srcM)[e] : static_cast<double>(static_cast<const float*>(srcM)[e])) + d;
  double cv = mv;
  if (!c_pattern_of_m)
    cv = (f64 ? static_cast<const double*>(srcC)[e] : static_cast<double>(static_cast<const float*>(srcC)[e])) + d;
  mask = (cv != 0.0) ? 1.0 : 0.0;
}

// Dense fp64 M and the mask of C of one problem from stores of T (float or double)
template <typename T>
__global__ void k_sdp_gather(const T* __restrict__ srcM, const T* __restrict__ srcC, bool c_pattern_of_m, int64_t rs,
                             int64_t cs, int32_t n, double ident, double* __restrict__ M, double* __restrict__ mask) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<int64_t>(n) * n) return;
  double mv, mk;
  sdp_gather_entry(srcM, srcC, sizeof(T) == sizeof(double), c_pattern_of_m, rs, cs, static_cast<int32_t>(idx / n),
                   static_cast<int32_t>(idx % n), ident, mv, mk);
  M[idx] = mv;
  mask[idx] = mk;
}

// sum of one double over a workgroup of THREADS, the same order on every call; every thread gets the result
template <int THREADS>
__device__ inline double sdp_block_sum(double v, double* red) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < THREADS / 64; ++i) s += red[i];
  return s;
}

// the pair k of step t of the circle order over np indices (np even): index np - 1 stays put, the others turn
// (stated in sdp_circle.hpp, where the host can walk it too)
__device__ inline void sdp_pair(int k, int t, int np, int& p, int& q) { clipper_sdp_circle::circle_pair(k, t, np, p, q); }

// A (LDS) <- Q^T A Q, through T (global); Q is np x np
__device__ void sdp_warm_start(double* A, const double* __restrict__ Q, double* __restrict__ T, int np) {
  const int j = threadIdx.x & 127, g = threadIdx.x >> 7;  // column j, rows g, g + 8, ...
  double acc[16];
  if (j < np) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0;
    for (int k = 0; k < np; ++k) {
      const double qv = Q[k * np + j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = g + 8 * r;
        if (i < np) acc[r] = fma(A[i * np + k], qv, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = g + 8 * r;
      if (i < np) T[i * np + j] = acc[r];
    }
  }
  __syncthreads();
  if (j < np) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0;
    for (int k = 0; k < np; ++k) {
      const double tv = T[k * np + j];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int i = g + 8 * r;
        if (i < np) acc[r] = fma(Q[k * np + i], tv, acc[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int i = g + 8 * r;
      if (i < np) A[i * np + j] = acc[r];
    }
  }
  __syncthreads();
}

// Cyclic Jacobi on the symmetric A (LDS, np x np) until off(A) <= SDP_JACOBI_TOL ||A||_F; with Q != nullptr the
// rotations are accumulated into Q (Q <- Q J). Returns the sweeps run.
__device__ int sdp_jacobi(double* A, double* __restrict__ Q, int np, double* rc, double* rs, double* rt,
                          double* red) {
  const int tid = threadIdx.x, h = np / 2;
  int sweep = 0;
  for (; sweep < SDP_MAX_SWEEPS; ++sweep) {
    double off = 0.0, all = 0.0;
    for (int idx = tid; idx < np * np; idx += SDP_THREADS) {
      const double v = A[idx];  // sdp_norms_add, spelled out (see the file comment)
      all += v * v;
      if (idx / np != idx % np) off += v * v;
    }
    off = sdp_block_sum<SDP_THREADS>(off, red);
    all = sdp_block_sum<SDP_THREADS>(all, red + SDP_THREADS / 64);
    if (!sdp_sweep_again(off, all)) break;
    for (int t = 0; t < np - 1; ++t) {
      if (tid < h) {
        int p, q;
        sdp_pair(tid, t, np, p, q);
        double c, s, tn;
        sdp_rotation(A[p * np + q], A[p * np + p], A[q * np + q], c, s, tn);
        rc[tid] = c;
        rs[tid] = s;
        rt[tid] = tn;
      }
      __syncthreads();
      // both sides of every 2 x 2 block (k, l), k <= l
      for (int idx = tid; idx < h * h; idx += SDP_THREADS) {
        const int k = idx / h, l = idx % h;
        if (k > l) continue;
        int p, q;
        sdp_pair(k, t, np, p, q);
        if (k == l) {
          const double apq = A[p * np + q];  // sdp_rotate_diag, spelled out (see the file comment)
          A[p * np + p] = A[p * np + p] - rt[k] * apq;
          A[q * np + q] = A[q * np + q] + rt[k] * apq;
          A[p * np + q] = 0.0;
          A[q * np + p] = 0.0;
          continue;
        }
        int r, s2;
        sdp_pair(l, t, np, r, s2);
        const double c1 = rc[k], s1 = rs[k], c2 = rc[l], sn2 = rs[l];
        const double apr = A[p * np + r], aps = A[p * np + s2], aqr = A[q * np + r], aqs = A[q * np + s2];
        double npr, nps, nqr, nqs;
        sdp_rotate_block(apr, aps, aqr, aqs, c1, s1, c2, sn2, npr, nps, nqr, nqs);
        sdp_store_block(A, np, p, q, r, s2, npr, nps, nqr, nqs);
      }
      if (Q) {
        for (int idx = tid; idx < np * h; idx += SDP_THREADS) {
          const int i = idx / h, k = idx % h;
          int p, q;
          sdp_pair(k, t, np, p, q);
          const double c = rc[k], s = rs[k];
          const double qp = Q[i * np + p], qq = Q[i * np + q];
          double nqp, nqq;
          sdp_rotate_q(qp, qq, c, s, nqp, nqq);
          Q[i * np + p] = nqp;
          Q[i * np + q] = nqq;
        }
      }
      __syncthreads();
    }
  }
  return sweep;
}

// d = lambda_max(M - rho U) (the pad index excluded); A and T are overwritten, Q is read
__device__ double sdp_dual_bound(const SdpArgs& g, double rho, double* A, bool warm, double* rc, double* rs,
                                 double* rt, double* red, int& sweeps) {
  const int n = g.n, np = g.np;
  for (int idx = threadIdx.x; idx < np * np; idx += SDP_THREADS) {
    const int a = idx / np, b = idx % np;
    A[idx] = (a < n && b < n) ? sdp_form_dual(g.M[a * n + b], g.U[a * n + b], rho) : 0.0;
  }
  __syncthreads();
  if (warm) sdp_warm_start(A, g.Q, g.T, np);
  sweeps += sdp_jacobi(A, nullptr, np, rc, rs, rt, red);
  double d = A[0];  // lambda_max off the diagonal: every work item scans it (k_sdpw_decide reduces it; max is exact)
  for (int i = 1; i < n; ++i) d = fmax(d, A[i * np + i]);
  __syncthreads();
  return d;
}

// LDS of one workgroup besides the working matrix (every kernel that runs sdp_body declares one)
struct SdpShared {
  double rc[SDP_MAX_N / 2], rs[SDP_MAX_N / 2], rt[SDP_MAX_N / 2];
  double lam[SDP_MAX_N], red[2 * SDP_THREADS / 64];
  int32_t pos_list[SDP_MAX_N];
  int32_t kmax, npos;
  int32_t top;  // the index that takes weight 1 when no support is valid (sdp_fallback_index)
  double tau;
  SdpCtl c;
};

// One launch's work on one problem, by one workgroup of SDP_THREADS: INIT, at most `budget` iterations, or the
// certificate. A: the working matrix (np x np doubles of LDS). Stated once for k_sdp and k_sdp_batch: the order of
// every sum depends on the geometry alone, so both give the same bits.
__device__ __forceinline__ void sdp_body(const SdpArgs& g, int32_t mode, int32_t budget, int32_t max_iters, double* A,
                                         SdpShared& sh) {
  double *rc = sh.rc, *rs = sh.rs, *rt = sh.rt, *lam = sh.lam, *red = sh.red;
  int32_t* pos_list = sh.pos_list;
  int32_t &kmax = sh.kmax, &npos = sh.npos, &top = sh.top;
  double& tau = sh.tau;
  SdpCtl& c = sh.c;
  const int tid = threadIdx.x, n = g.n, np = g.np, nn = n * n;
  if (tid == 0) c = *g.ctl;
  __syncthreads();

  if (mode == SDP_MODE_INIT) {
    // X = Z = diag(mask) / #diag(mask), U = 0, Q = I, mu = diag(X)
    if (tid == 0) {
      int cnt = 0;
      for (int i = 0; i < n; ++i) cnt += g.mask[i * n + i] != 0.0;
      kmax = cnt;
      sdp_init_ctl(c, cnt);
    }
    __syncthreads();
    const double w = sdp_init_weight(kmax);
    for (int idx = tid; idx < nn; idx += SDP_THREADS) {
      const int a = idx / n, b = idx % n;
      const double x = (a == b && g.mask[idx] != 0.0) ? w : 0.0;  // sdp_init_entry, spelled out (here and for mu)
      g.X[idx] = x;
      g.Z[idx] = x;
      g.U[idx] = 0.0;
    }
    for (int idx = tid; idx < np * np; idx += SDP_THREADS) g.Q[idx] = sdp_init_q(idx / np, idx % np);
    for (int i = tid; i < np; i += SDP_THREADS) g.mu[i] = (i < n && g.mask[i * n + i] != 0.0) ? w : 0.0;
  } else if (mode == SDP_MODE_CERTIFY) {
    int sw = 0;
    const double d = sdp_dual_bound(g, c.rho, A, c.iters > 0, rc, rs, rt, red, sw);
    if (tid == 0) {
      c.dval = d;
      c.sweeps += sw;
    }
  } else {
    for (int it = 0; it < budget; ++it) {
      if (c.converged || c.iters >= max_iters) break;
      const double rho = c.rho;
      int sw = 0;
      // ---- X+ = proj_S(Z - U + M / rho)
      for (int idx = tid; idx < np * np; idx += SDP_THREADS) {
        const int a = idx / np, b = idx % np;
        double w = 0.0;
        if (a < n && b < n) {
          const int e = a * n + b;
          w = sdp_form_primal(g.Z[e], g.U[e], g.M[e], rho);
        }
        A[idx] = w;
      }
      __syncthreads();
      if (c.iters > 0) sdp_warm_start(A, g.Q, g.T, np);
      sw += sdp_jacobi(A, g.Q, np, rc, rs, rt, red);
      // simplex projection of the eigenvalues: tau of the largest valid support; sdp_support and
      // sdp_support_tau, spelled out (see the file comment; k_sdpw_project runs the same steps through them)
      if (tid < n) lam[tid] = A[tid * np + tid];
      if (tid == 0) kmax = 0;
      __syncthreads();
      int cnt = 0;
      double sum = 0.0;
      bool ok = false;
      if (tid < n) {
        const double li = lam[tid];
        for (int j = 0; j < n; ++j)
          if (lam[j] >= li) {
            ++cnt;
            sum += lam[j];
          }
        ok = li > (sum - 1.0) / cnt;
        if (ok) atomicMax(&kmax, cnt);
      }
      __syncthreads();
      if (ok && cnt == kmax) tau = (sum - 1.0) / cnt;  // (equal sets: equal sums, the same bits)
      if (tid == 0 && kmax == 0) top = sdp_fallback_index(lam, n);  // no valid support: no tau is written, none read
      __syncthreads();
      if (tid < np) {
        const double m =
            tid < n ? (kmax == 0 ? sdp_fallback_weight(tid, top) : sdp_simplex_weight(lam[tid], tau)) : 0.0;
        g.mu[tid] = m;
        lam[tid] = m;
      }
      __syncthreads();
      if (tid == 0) {
        int k = 0;
        for (int i = 0; i < n; ++i)
          if (lam[i] > 0.0) pos_list[k++] = i;
        npos = k;
      }
      __syncthreads();
      // the positive eigenvectors into LDS (A is free): P[r][a] = Q[a][pos_list[r]]
      const int K = npos;
      for (int idx = tid; idx < K * n; idx += SDP_THREADS) {
        const int r = idx / n, a = idx % n;
        A[idx] = g.Q[a * np + pos_list[r]];
      }
      __syncthreads();
      // ---- X = sum mu_r q_r q_r^T; Z+ = proj_P(X + U); U+ = U + X - Z+; the sums of the stopping rule
      // (sdp_update_entry's terms, sdp_residuals, sdp_balance_factor and sdp_close_iteration, spelled out below)
      double rp2 = 0.0, rd2 = 0.0, xx = 0.0, zz = 0.0, uu = 0.0, mx = 0.0;
      for (int idx = tid; idx < nn; idx += SDP_THREADS) {
        const int a = idx / n, b = idx % n;
        double x = 0.0;
        for (int r = 0; r < K; ++r) x += lam[pos_list[r]] * (A[r * n + a] * A[r * n + b]);
        const double u = g.U[idx], zo = g.Z[idx];
        const double v = x + u;
        const double zn = sdp_z_plus(v, g.mask[idx] != 0.0);
        const double un = v - zn;
        g.X[idx] = x;
        g.Z[idx] = zn;
        g.U[idx] = un;
        rp2 += (x - zn) * (x - zn);
        rd2 += (zn - zo) * (zn - zo);
        xx += x * x;
        zz += zn * zn;
        uu += un * un;
        mx += g.M[idx] * x;
      }
      rp2 = sdp_block_sum<SDP_THREADS>(rp2, red);
      rd2 = sdp_block_sum<SDP_THREADS>(rd2, red + SDP_THREADS / 64);
      xx = sdp_block_sum<SDP_THREADS>(xx, red);
      zz = sdp_block_sum<SDP_THREADS>(zz, red + SDP_THREADS / 64);
      uu = sdp_block_sum<SDP_THREADS>(uu, red);
      mx = sdp_block_sum<SDP_THREADS>(mx, red + SDP_THREADS / 64);
      const double r_p = sqrt(rp2), r_d = rho * sqrt(rd2);
      const double e_pri = n * g.eps_abs + g.eps_rel * fmax(sqrt(xx), sqrt(zz));
      const double e_dual = n * g.eps_abs + g.eps_rel * rho * sqrt(uu);
      bool conv = false;
      if (r_p <= e_pri && r_d <= e_dual) {
        __syncthreads();  // U+ of every thread is written
        const double d = sdp_dual_bound(g, rho, A, true, rc, rs, rt, red, sw);
        conv = sdp_gap_closed(d, mx, g.eps_abs, g.eps_rel);
        if (tid == 0) c.dval = d;
      }
      // residual balancing; every thread rescales the entries of U it wrote
      double f = 1.0;
      const int32_t done = c.iters + 1;
      if (!conv && done == c.adapt_next) {
        if (r_p > SDP_ADAPT_MU * r_d) f = SDP_ADAPT_TAU;
        else if (r_d > SDP_ADAPT_MU * r_p) f = 1.0 / SDP_ADAPT_TAU;
      }
      const int rescale = sdp_rescale_of(f);
      if (rescale != SDP_RESCALE_NONE)
        for (int idx = tid; idx < nn; idx += SDP_THREADS) g.U[idx] = sdp_rescale_u(g.U[idx], rescale);
      __syncthreads();
      if (tid == 0) {
        sdp_balance_advance(c, done, conv, f);
        c.iters = done;
        c.r_prim = r_p;
        c.r_dual = r_d;
        c.pval = mx;
        c.converged = conv;
        c.rho = rho * f;
        c.sweeps += sw;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid == 0) *g.ctl = c;
}

__global__ void __launch_bounds__(SDP_THREADS) k_sdp(SdpArgs g, int32_t mode, int32_t budget, int32_t max_iters) {
  extern __shared__ double sdp_A[];  // np x np
  __shared__ SdpShared sh;
  sdp_body(g, mode, budget, max_iters, sdp_A, sh);
}

// ---- a batch: one workgroup per problem ("Batches") ---------------------------------------------------
//
// Workgroup b works on problem list[b] of the table, with the lone kernel's body and geometry: per problem the bits
// are k_sdp's, whatever else the launch holds and however the host cuts the launches. The dynamic LDS is that of the
// largest problem of the launch. No workgroup reads or writes another problem's buffers; there is no barrier, no
// atomic and no flag between workgroups.
__global__ void __launch_bounds__(SDP_THREADS) k_sdp_batch(const SdpArgs* __restrict__ table,
                                                           const int32_t* __restrict__ list, int32_t mode,
                                                           int32_t budget, int32_t max_iters) {
  extern __shared__ double sdp_A[];  // np x np of the launch's largest problem
  __shared__ SdpShared sh;
  const SdpArgs g = table[list[blockIdx.x]];
  if (mode == SDP_MODE_ITERATE) {  // (uniform over the workgroup: nothing to do, nothing written)
    const SdpCtl* c = g.ctl;
    if (c->converged || c->iters >= max_iters) return;
  }
  sdp_body(g, mode, budget, max_iters, sdp_A, sh);
}

// Where one problem's M and C come from (k_sdp_gather_batch): element (r, c) of the lower triangle sits at
// src[r * rs + c * cs], floats or doubles; `ident` is added to the diagonal of both (a context's identity).
struct SdpGatherSrc {
  const void* srcM;
  const void* srcC;  // unused with c_pattern_of_m
  int64_t rs, cs;
  double ident;
  double* M;
  double* mask;
  int32_t n;
  int32_t f64;             // 1: doubles, 0: floats
  int32_t c_pattern_of_m;  // C = pattern(M + ident I)
  int32_t pad;
};

// k_sdp_gather for every problem of a batch in one launch: grid (ceil(max n^2 / 256), problems)
__global__ void k_sdp_gather_batch(const SdpGatherSrc* __restrict__ table) {
  const SdpGatherSrc g = table[blockIdx.y];
  const int32_t n = g.n;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (idx >= static_cast<int64_t>(n) * n) return;
  const int32_t a = static_cast<int32_t>(idx / n), b = static_cast<int32_t>(idx % n);
  double mv, mk;
  sdp_gather_entry(g.srcM, g.srcC, g.f64, g.c_pattern_of_m, g.rs, g.cs, a, b, g.ident, mv, mk);
  g.M[idx] = mv;
  g.mask[idx] = mk;
}

// What the rounding leaves per problem besides evec1 and the node list
struct SdpRound {
  double thr;
  int32_t count;  // nodes selected
  int32_t top;    // the index of the largest mu
};

struct SdpRoundDst {
  double* ev;      // n doubles: evec1 (nullptr: the problem is not rounded here)
  int32_t* nodes;  // n int32: the selection, ascending
};

// The rounding (sdp.cpp:244-261), one wave per problem: `top` = the first index of the largest mu, evec1 = that column
// of Q with its first largest-magnitude entry made positive, thr = half that magnitude, the nodes |evec1_i| > thr
// ascending. "First index of the largest" = what a sequential scan with a strict > finds: each lane scans its indices
// in ascending order with >, the lanes are merged by (larger value, then lower index).
__device__ inline void sdp_wave_argmax(double& v, int& i) {
  for (int o = 32; o > 0; o >>= 1) {
    const double ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
}

__global__ void __launch_bounds__(64) k_sdp_round_batch(const SdpArgs* __restrict__ table,
                                                        const SdpRoundDst* __restrict__ dst,
                                                        SdpRound* __restrict__ round_out) {
  const SdpArgs g = table[blockIdx.x];
  const int lane = threadIdx.x, n = g.n, np = g.np;
  double* ev = dst[blockIdx.x].ev;
  if (!ev) return;  // a problem of the wide route: rounded by the lone call's tail (host_sdp.hpp)
  int32_t* nodes = dst[blockIdx.x].nodes;
  double bv = 0.0;
  int bi = 0x7fffffff;
  for (int i = lane; i < n; i += 64) {
    const double m = g.mu[i];
    if (bi == 0x7fffffff || m > bv) {
      bv = m;
      bi = i;
    }
  }
  if (bi == 0x7fffffff) bv = -__builtin_huge_val();  // (a lane without an index never wins)
  sdp_wave_argmax(bv, bi);
  const int top = bi;
  double e[(SDP_MAX_N + 63) / 64];
  double av = -1.0;  // (magnitudes are >= 0)
  int ai = 0x7fffffff;
#pragma unroll
  for (int k = 0; k < (SDP_MAX_N + 63) / 64; ++k) {
    const int i = lane + 64 * k;
    e[k] = i < n ? g.Q[i * np + top] : 0.0;
    if (i < n && fabs(e[k]) > av) {
      av = fabs(e[k]);
      ai = i;
    }
  }
  sdp_wave_argmax(av, ai);
  const int big = ai;
  double ebig = 0.0;
#pragma unroll
  for (int k = 0; k < (SDP_MAX_N + 63) / 64; ++k) {
    const double t = __shfl(e[k], big & 63, 64);
    if (k == (big >> 6)) ebig = t;
  }
  const bool flip = ebig < 0;
  const double thr = fabs(ebig) / 2.0;
  int base = 0;
#pragma unroll
  for (int k = 0; k < (SDP_MAX_N + 63) / 64; ++k) {
    const int i = lane + 64 * k;
    const double v = flip ? -e[k] : e[k];
    const bool sel = i < n && fabs(v) > thr;
    if (i < n) ev[i] = v;
    const unsigned long long bal = __ballot(sel);
    if (sel) nodes[base + __popcll(bal & ((1ull << lane) - 1ull))] = i;
    base += __popcll(bal);
  }
  if (lane == 0) round_out[blockIdx.x] = SdpRound{thr, base, top};
}

}  // namespace clipper_hip
