// k_sdp_wide.hip.h — the wide route of the semidefinite relaxation ("The wide route"): the ADMM
// iteration, the stopping rule and the certificate of k_sdp.hip.h for one problem of n <= SDPW_MAX_N over the whole
// chip, as a chain of launches on one stream. The working matrix of the eigensolver lives in global memory, so its
// size is not bound by one workgroup's LDS. Host side: host_sdpwide.hpp; geometry and buffers: host_sdpwide_plan.hpp.
// Part of kernels.hip.h (include that one): hand-written gfx950 device code.
//
// Launch boundaries are the only synchronisation: no grid barrier, no cooperative launch, no atomics in floating
// point, no workgroup that waits for another. Every grid and every reduction tree is a function of n alone, so two
// calls give the same bits on any device.
//
// Every rule of the iteration is the workgroup route's, read from the same place: the arithmetic from sdp_rules.hpp,
// the circle order from sdp_circle.hpp, and sdp_block_sum and SdpArgs from k_sdp.hip.h. What
// this file states is how the work is cut into launches and tiles.
//
// The eigensolver is sdp_jacobi's: cyclic Jacobi in the circle order with the same rotations. One step is ONE launch,
// k_sdpw_step: the np / 2 pairs of a step partition the indices, so every entry of A lies in exactly one 2 x 2 block
// (pair k, pair l) and every entry of Q in exactly one (row, pair); the launch reads A_src, Q_src and rewrites A_dst,
// Q_dst completely (ping-pong), and never reads what it writes. Each workgroup computes the rotations of the pairs its
// tile needs from A_src into LDS: redundant across workgroups, and cheaper than a launch of its own.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_sdpwide_plan.hpp"
#include "k_sdp.hip.h"

namespace clipper_hip {

constexpr int SDPW_MAX_N = clipper_sdpw_plan::WIDE_MAX_N;
constexpr int SDPW_THREADS = clipper_sdpw_plan::STEP_THREADS;  // the chip-wide launches
static_assert(SDPW_MAX_N <= SDP_THREADS, "the one-workgroup launches hold an index per work item");

enum { SDPW_FORM_PRIMAL = 0, SDPW_FORM_DUAL = 1 };
enum { SDPW_DECIDE = 0, SDPW_AFTER_DUAL = 1, SDPW_CERTIFY = 2 };

// device state of one problem: SdpCtl and what the driver reads between launches (one copy)
struct SdpWideState {
  SdpCtl c;
  int32_t again;      // k_sdpw_norms: the eigensolver sweeps again
  int32_t want_dual;  // k_sdpw_decide: both residuals pass, the dual bound is wanted
  int32_t rescale;    // k_sdpw_decide: SDP_RESCALE_* of U
  int32_t npos;       // k_sdpw_project: positive simplex weights
  double w;           // k_sdpw_init: 1 / #diag(mask)
  double r_p, r_d, mx;  // carried from SDPW_DECIDE to SDPW_AFTER_DUAL
};
static_assert(sizeof(SdpWideState) <= clipper_sdpw_plan::STATE_BYTES && sizeof(SdpWideState) % 8 == 0, "the plan's state region");

// ---- INIT: X = Z = diag(mask) / #diag(mask), U = 0, Q = I, mu = diag(X) -------------------------------------------
__global__ void __launch_bounds__(SDP_THREADS) k_sdpw_init(SdpArgs g, SdpWideState* __restrict__ st) {
  __shared__ int cnt;
  const int tid = threadIdx.x, n = g.n;
  if (tid == 0) cnt = 0;
  __syncthreads();
  if (tid < n && g.mask[tid * n + tid] != 0.0) atomicAdd(&cnt, 1);
  __syncthreads();
  if (tid == 0) {
    SdpWideState s{};
    sdp_init_ctl(s.c, cnt);
    s.w = sdp_init_weight(cnt);
    *st = s;
  }
}

__global__ void __launch_bounds__(SDPW_THREADS) k_sdpw_init_fill(SdpArgs g, const SdpWideState* __restrict__ st) {
  const int n = g.n, np = g.np;
  const int idx = blockIdx.x * SDPW_THREADS + threadIdx.x;
  if (idx >= np * np) return;
  const double w = st->w;
  const int a = idx / np, b = idx % np;
  g.Q[idx] = sdp_init_q(a, b);
  if (a < n && b < n) {
    const int e = a * n + b;
    const double x = sdp_init_entry(a == b && g.mask[e] != 0.0, w);
    g.X[e] = x;
    g.Z[e] = x;
    g.U[e] = 0.0;
  }
  if (idx < np) g.mu[idx] = sdp_init_entry(idx < n && g.mask[idx * n + idx] != 0.0, w);
}

// ---- form: A <- pad(Z - U + M / rho), or pad(M - rho U) for the dual bound; rho from the device's SdpCtl ----------
__global__ void __launch_bounds__(SDPW_THREADS) k_sdpw_form(SdpArgs g, double* __restrict__ A, int32_t what) {
  const int n = g.n, np = g.np;
  const int idx = blockIdx.x * SDPW_THREADS + threadIdx.x;
  if (idx >= np * np) return;
  const double rho = g.ctl->rho;
  const int a = idx / np, b = idx % np;
  double w = 0.0;
  if (a < n && b < n) {
    const int e = a * n + b;
    w = what == SDPW_FORM_DUAL ? sdp_form_dual(g.M[e], g.U[e], rho) : sdp_form_primal(g.Z[e], g.U[e], g.M[e], rho);
  }
  A[idx] = w;
}

// ---- warm start: C = op(A) B, np x np row-major, op(A) = A or A^T; every element a sum over k ascending, fma ------
// (A <- Q^T A Q is two of these through T.) 64 x 64 tile per workgroup, 4 x 4 per work item, k in slices of 16.
constexpr int SDPW_GT = 64, SDPW_GK = 16;

__global__ void __launch_bounds__(SDPW_THREADS) k_sdpw_gemm(const double* __restrict__ A, const double* __restrict__ B,
                                                            double* __restrict__ C, int32_t np, int32_t trans_a) {
  __shared__ double As[SDPW_GK][SDPW_GT + 1], Bs[SDPW_GK][SDPW_GT];
  const int tid = threadIdx.x, ty = tid / 16, tx = tid % 16;
  const int i0 = blockIdx.y * SDPW_GT, j0 = blockIdx.x * SDPW_GT;
  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
  for (int k0 = 0; k0 < np; k0 += SDPW_GK) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int idx = tid + SDPW_THREADS * e;
      int ii, kk;
      if (trans_a) {
        kk = idx / SDPW_GT;
        ii = idx % SDPW_GT;
      } else {
        ii = idx / SDPW_GK;
        kk = idx % SDPW_GK;
      }
      const int i = i0 + ii, k = k0 + kk;
      As[kk][ii] = (i < np && k < np) ? (trans_a ? A[k * np + i] : A[i * np + k]) : 0.0;
      const int bk = idx / SDPW_GT, bj = idx % SDPW_GT;
      Bs[bk][bj] = (k0 + bk < np && j0 + bj < np) ? B[(k0 + bk) * np + j0 + bj] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < SDPW_GK; ++kk) {  // (a slice past np holds zeros: fma(0, 0, acc) = acc)
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = As[kk][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = Bs[kk][tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = fma(a[r], b[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
      if (i < np && j < np) C[i * np + j] = acc[r][c];
    }
}

// ---- before each sweep: off(A)^2 and ||A||^2 in a fixed two-stage order (work item, then workgroup) ---------------
__global__ void __launch_bounds__(SDP_THREADS) k_sdpw_norms(const double* __restrict__ A, int32_t np,
                                                            SdpWideState* __restrict__ st) {
  __shared__ double red[2 * SDP_THREADS / 64];
  double off = 0.0, all = 0.0;
  for (int idx = threadIdx.x; idx < np * np; idx += SDP_THREADS) sdp_norms_add(A[idx], idx / np == idx % np, off, all);
  off = sdp_block_sum<SDP_THREADS>(off, red);
  all = sdp_block_sum<SDP_THREADS>(all, red + SDP_THREADS / 64);
  if (threadIdx.x == 0) st->again = sdp_sweep_again(off, all);
}

// ---- one Jacobi step (geometry: clipper_sdpw_plan::step_geom; Q_src == nullptr: no accumulation) -------------------
__global__ void __launch_bounds__(SDPW_THREADS) k_sdpw_step(const double* __restrict__ As, double* __restrict__ Ad,
                                                            const double* __restrict__ Qs, double* __restrict__ Qd,
                                                            int32_t np, int32_t t) {
  namespace plan = clipper_sdpw_plan;
  constexpr int TILE = plan::TILE;
  __shared__ double rc[2 * TILE], rs[2 * TILE], rt[2 * TILE];  // the pairs of the tile's rows, then of its columns
  const plan::StepGeom g = plan::step_geom(np);
  const int tid = threadIdx.x;
  const int wg = blockIdx.x;
  const bool on_a = wg < g.a_tiles;
  int kt, lt;
  if (on_a) plan::a_tile(g, wg, kt, lt);
  else kt = lt = (wg - g.a_tiles) % g.ht;
  if (tid < 2 * TILE) {
    const int k = (tid < TILE ? kt : lt) * TILE + tid % TILE;
    double c = 1.0, s = 0.0, tn = 0.0;
    if (k < g.h) {
      int p, q;
      sdp_pair(k, t, np, p, q);
      sdp_rotation(As[p * np + q], As[p * np + p], As[q * np + q], c, s, tn);
    }
    rc[tid] = c;
    rs[tid] = s;
    rt[tid] = tn;
  }
  __syncthreads();
  if (on_a) {
    int k, l;
    if (!plan::a_item(g, wg, tid, k, l)) return;
    const int i = tid / TILE, j = TILE + tid % TILE;
    int p, q;
    sdp_pair(k, t, np, p, q);
    if (k == l) {
      sdp_rotate_diag(As, Ad, np, p, q, rt[i]);
      return;
    }
    int r, s2;
    sdp_pair(l, t, np, r, s2);
    double npr, nps, nqr, nqs;
    sdp_rotate_block(As[p * np + r], As[p * np + s2], As[q * np + r], As[q * np + s2], rc[i], rs[i], rc[j], rs[j], npr,
                     nps, nqr, nqs);
    sdp_store_block(Ad, np, p, q, r, s2, npr, nps, nqr, nqs);
  } else {
    int row, k;
    if (!plan::q_item(g, wg - g.a_tiles, tid, row, k)) return;
    const int j = tid % TILE;
    int p, q;
    sdp_pair(k, t, np, p, q);
    const double c = rc[j], s = rs[j];
    const double qp = Qs[row * np + p], qq = Qs[row * np + q];
    double nqp, nqq;
    sdp_rotate_q(qp, qq, c, s, nqp, nqq);
    Qd[row * np + p] = nqp;
    Qd[row * np + q] = nqq;
  }
}

// ---- project: the eigenvalues from the diagonal, the simplex rule (the largest valid support): mu, the indices of
// the positive weights ascending in pos_list and their number in st->npos (n <= SDP_THREADS: an index per work item)
__global__ void __launch_bounds__(SDP_THREADS) k_sdpw_project(SdpArgs g, const double* __restrict__ A,
                                                              int32_t* __restrict__ pos_list,
                                                              SdpWideState* __restrict__ st) {
  __shared__ double lam[SDPW_MAX_N];
  __shared__ int32_t kmax, top;
  __shared__ double tau;
  const int tid = threadIdx.x, n = g.n, np = g.np;
  if (tid < n) lam[tid] = A[tid * np + tid];
  if (tid == 0) kmax = 0;
  __syncthreads();
  int cnt = 0;
  double sum = 0.0;
  bool ok = false;
  if (tid < n) {
    ok = sdp_support(lam, n, lam[tid], cnt, sum);
    if (ok) atomicMax(&kmax, cnt);
  }
  __syncthreads();
  if (ok && cnt == kmax) tau = sdp_support_tau(sum, cnt);  // (equal sets: equal sums, the same bits)
  if (tid == 0 && kmax == 0) top = sdp_fallback_index(lam, n);  // no valid support: no tau is written, none read
  __syncthreads();
  if (tid < np) {
    const double m = tid < n ? (kmax == 0 ? sdp_fallback_weight(tid, top) : sdp_simplex_weight(lam[tid], tau)) : 0.0;
    g.mu[tid] = m;
    lam[tid] = m;
  }
  __syncthreads();
  if (tid == 0) {
    int k = 0;
    for (int i = 0; i < n; ++i)
      if (lam[i] > 0.0) pos_list[k++] = i;
    st->npos = k;
  }
}

// ---- update (fused): X = sum mu_r q_r q_r^T over the positive weights in ascending index, Z+ = proj_P(X + U),
// U+ = U + X - Z+, and this workgroup's partials of the six sums of the stopping rule: part[s * tiles + workgroup]
constexpr int SDPW_UR = 64;  // eigenvectors per slice

__global__ void __launch_bounds__(SDPW_THREADS) k_sdpw_update(SdpArgs g, const double* __restrict__ Q,
                                                              const int32_t* __restrict__ pos_list,
                                                              const SdpWideState* __restrict__ st,
                                                              double* __restrict__ part) {
  constexpr int UT = clipper_sdpw_plan::UPDATE_TILE;
  __shared__ double Pa[UT][SDPW_UR + 1], Pb[UT][SDPW_UR + 1], mus[SDPW_UR], red[SDPW_THREADS / 64];
  const int tid = threadIdx.x, n = g.n, np = g.np, K = st->npos;
  const int side = (n + UT - 1) / UT;
  const int a0 = (blockIdx.x / side) * UT, b0 = (blockIdx.x % side) * UT;
  const int a = a0 + tid / UT, b = b0 + tid % UT;
  double x = 0.0;
  for (int r0 = 0; r0 < K; r0 += SDPW_UR) {
    const int cnt = min(SDPW_UR, K - r0);
    __syncthreads();
    for (int idx = tid; idx < UT * SDPW_UR; idx += SDPW_THREADS) {
      const int rr = idx % SDPW_UR, ii = idx / SDPW_UR;
      double va = 0.0, vb = 0.0;
      if (rr < cnt) {
        const int col = pos_list[r0 + rr];
        if (a0 + ii < n) va = Q[(a0 + ii) * np + col];
        if (b0 + ii < n) vb = Q[(b0 + ii) * np + col];
      }
      Pa[ii][rr] = va;
      Pb[ii][rr] = vb;
    }
    if (tid < cnt) mus[tid] = g.mu[pos_list[r0 + tid]];
    __syncthreads();
    for (int rr = 0; rr < cnt; ++rr) x += mus[rr] * (Pa[tid / UT][rr] * Pb[tid % UT][rr]);
  }
  SdpSums t{0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (a < n && b < n) {
    const int e = a * n + b;
    double zn, un;
    sdp_update_entry(x, g.U[e], g.Z[e], g.mask[e] != 0.0, g.M[e], zn, un, t);
    g.X[e] = x;
    g.Z[e] = zn;
    g.U[e] = un;
  }
  const int tiles = gridDim.x;
  const double sums[6] = {t.rp2, t.rd2, t.xx, t.zz, t.uu, t.mx};
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const double v = sdp_block_sum<SDPW_THREADS>(sums[s], red);
    if (tid == 0) part[s * tiles + blockIdx.x] = v;
  }
}

// ---- decide, one workgroup ------------------------------------------------------------------------------------------
// SDPW_DECIDE: reduce the partials in fixed order and apply the tolerances (sdp_residuals); when both residuals pass,
// ask for the dual bound (want_dual) and leave the rest to SDPW_AFTER_DUAL, which reads lambda_max off the diagonal of
// A; otherwise close the iteration here: convergence, residual balancing (what it does to U in `rescale`), SdpCtl.
// SDPW_CERTIFY: dval = lambda_max. `sw`: the Jacobi sweeps since SdpCtl was last written.
__global__ void __launch_bounds__(SDP_THREADS) k_sdpw_decide(SdpArgs g, SdpWideState* __restrict__ st,
                                                             const double* __restrict__ part, int32_t tiles,
                                                             const double* __restrict__ A, int32_t phase, int32_t sw) {
  __shared__ double red[2 * SDP_THREADS / 64];
  const int tid = threadIdx.x, n = g.n, np = g.np;
  double r_p, r_d, mx;
  bool conv = false;
  if (phase == SDPW_DECIDE) {
    double s[6];
    for (int k = 0; k < 6; ++k) {
      double v = 0.0;
      for (int i = tid; i < tiles; i += SDP_THREADS) v += part[k * tiles + i];
      s[k] = sdp_block_sum<SDP_THREADS>(v, red + (k & 1) * (SDP_THREADS / 64));
    }
    if (tid != 0) return;
    mx = s[5];
    if (sdp_residuals(SdpSums{s[0], s[1], s[2], s[3], s[4], s[5]}, st->c.rho, n, g.eps_abs, g.eps_rel, r_p, r_d)) {
      st->want_dual = 1;
      st->rescale = SDP_RESCALE_NONE;
      st->r_p = r_p;
      st->r_d = r_d;
      st->mx = mx;
      return;
    }
  } else {
    // lambda_max(M - rho U) off the diagonal of the eigensolver's A (the pad index excluded); sdp_dual_bound scans
    // the same diagonal in sequence (max is exact: the order does not show)
    double d = -__builtin_huge_val();
    if (tid < n) d = A[tid * np + tid];
    for (int o = 32; o > 0; o >>= 1) d = fmax(d, __shfl_xor(d, o, 64));
    if ((tid & 63) == 0) red[tid >> 6] = d;
    __syncthreads();
    if (tid != 0) return;
    for (int i = 1; i < SDP_THREADS / 64; ++i) d = fmax(d, red[i]);
    st->c.dval = d;
    if (phase == SDPW_CERTIFY) {
      st->c.sweeps += sw;
      return;
    }
    r_p = st->r_p;
    r_d = st->r_d;
    mx = st->mx;
    conv = sdp_gap_closed(d, mx, g.eps_abs, g.eps_rel);
  }
  // the iteration ends here (work item 0)
  SdpCtl c = st->c;
  const double f = sdp_balance_factor(c, c.iters + 1, conv, r_p, r_d);
  sdp_close_iteration(c, r_p, r_d, mx, conv, f, sw);
  st->c = c;
  st->want_dual = 0;
  st->rescale = sdp_rescale_of(f);
}

// ---- residual balancing: U <- U / tau or U * tau (launched only when k_sdpw_decide asked for it) --------------------
__global__ void __launch_bounds__(SDPW_THREADS) k_sdpw_scale_u(SdpArgs g, int32_t rescale) {
  const int idx = blockIdx.x * SDPW_THREADS + threadIdx.x;
  if (idx >= g.n * g.n) return;
  g.U[idx] = sdp_rescale_u(g.U[idx], rescale);
}

}  // namespace clipper_hip
