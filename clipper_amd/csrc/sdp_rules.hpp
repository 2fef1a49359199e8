// sdp_rules.hpp — the arithmetic of one ADMM iteration of the semidefinite relaxation, stated
// once for the workgroup route (k_sdp.hip.h), the wide route (k_sdp_wide.hip.h) and the host: the constants, the
// control record, the INIT values, the matrices that are eigendecomposed, the Jacobi rotation and what it does to a
// block, the simplex rule of the eigenvalues, one entry's update with the six sums of the stopping rule, the
// tolerances, the gap test, the residual balancing with its schedule and the record an iteration leaves. Plain sequential functions of
// one entry, one block or one support (sdp_store_block writes a block's eight entries, sdp_support walks the
// eigenvalues): which work item holds what and in what order a sum is reduced across work items belong to the kernels.
// Every expression rounds as written (the build runs with -ffp-contract=off): changing an expression's shape here
// changes the bits of both routes together. No HIP: builds with g++ as well (tests/cpp/test_sdp_rules.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

#include "sdp_circle.hpp"

namespace clipper_hip {

constexpr int SDP_MAX_SWEEPS = 40;
constexpr double SDP_JACOBI_TOL = 1e-13;  // stop sweeping when off(A) <= tol * ||A||_F
constexpr double SDP_RHO0 = 1.0;
constexpr int SDP_ADAPT_EVERY = 10;       // residual balancing: checked every 10 iterations at first;
constexpr double SDP_ADAPT_MU = 10.0;     // when one residual exceeds 10 times the other,
constexpr double SDP_ADAPT_TAU = 2.0;     // rho is multiplied or divided by 2 and U divided or multiplied;
constexpr int32_t SDP_ADAPT_MAX_EVERY = 1 << 30;  // the interval doubles with every reversal of the moves, up to this

// device state of one problem (the host reads it after every launch)
struct SdpCtl {
  double rho;
  double r_prim, r_dual;  // ||X - Z||_F, rho ||Z - Z_prev||_F of the last iteration
  double pval;            // <M, X>
  double dval;            // lambda_max(M - rho U): the dual bound of the last check (or certification)
  int32_t iters;
  int32_t converged;
  int32_t infeasible;     // no diagonal entry of C is nonzero
  int32_t sweeps;         // Jacobi sweeps so far (all projections and checks)
  int32_t adapt_next;     // the schedule of the residual balancing: the iteration of the next check,
  int32_t adapt_every;    // the interval between checks,
  int32_t adapt_dir;      // the direction of the last move of rho (+1 up, -1 down, 0 none yet)
  int32_t pad;
};
static_assert(sizeof(SdpCtl) == 72, "five doubles and eight int32: the hosts copy the record as it is");

// ---- INIT: X = Z = diag(mask) / #diag(mask), U = 0, Q = I, mu = diag(X) ---------------------------------------------
// cnt: the nonzero diagonal entries of the mask
SDP_HD void sdp_init_ctl(SdpCtl& c, int cnt) {
  c = SdpCtl{SDP_RHO0, 0.0, 0.0, 0.0, 0.0, 0, 0, cnt == 0, 0, SDP_ADAPT_EVERY, SDP_ADAPT_EVERY, 0, 0};
}
SDP_HD double sdp_init_weight(int cnt) { return cnt ? 1.0 / cnt : 0.0; }
// an entry of X, Z or mu; on_masked_diag: a diagonal entry that the mask keeps
SDP_HD double sdp_init_entry(bool on_masked_diag, double w) { return on_masked_diag ? w : 0.0; }
SDP_HD double sdp_init_q(int a, int b) { return (a == b) ? 1.0 : 0.0; }

// ---- the matrices that are eigendecomposed (the pad index holds zeros) ----------------------------------------------
SDP_HD double sdp_form_primal(double z, double u, double m, double rho) { return z - u + m / rho; }
SDP_HD double sdp_form_dual(double m, double u, double rho) { return m - rho * u; }

// ---- the eigensolver ------------------------------------------------------------------------------------------------
// one entry's share of off(A)^2 and ||A||_F^2
SDP_HD void sdp_norms_add(double v, bool on_diag, double& off, double& all) {
  all += v * v;
  if (!on_diag) off += v * v;
}

SDP_HD bool sdp_sweep_again(double off, double all) { return off > SDP_JACOBI_TOL * SDP_JACOBI_TOL * all; }

// The rotation that annihilates a_pq of the pair (p, q): c, s and the tangent tn (identity when a_pq = 0)
SDP_HD void sdp_rotation(double apq, double app, double aqq, double& c, double& s, double& tn) {
  c = 1.0;
  s = 0.0;
  tn = 0.0;
  if (apq != 0.0) {
    const double theta = (aqq - app) / (2.0 * apq);
    const double at = fabs(theta);
    tn = at > 1e150 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));
    if (theta < 0.0) tn = -tn;
    c = 1.0 / sqrt(tn * tn + 1.0);
    s = tn * c;
  }
}

// The diagonal block of a step (the pair's own 2 x 2), read from As and written to Ad (np x np; the same matrix or
// its other copy): the diagonal moves by tn a_pq, a_pq becomes zero exactly
SDP_HD void sdp_rotate_diag(const double* As, double* Ad, int np, int p, int q, double tn) {
  const double apq = As[p * np + q];
  Ad[p * np + p] = As[p * np + p] - tn * apq;
  Ad[q * np + q] = As[q * np + q] + tn * apq;
  Ad[p * np + q] = 0.0;
  Ad[q * np + p] = 0.0;
}

// Both sides of the 2 x 2 block (rows p, q of a pair with c1, s1; columns r, s of another with c2, sn2)
SDP_HD void sdp_rotate_block(double apr, double aps, double aqr, double aqs, double c1, double s1, double c2,
                             double sn2, double& npr, double& nps, double& nqr, double& nqs) {
  const double bpr = apr * c2 - aps * sn2, bps = apr * sn2 + aps * c2;  // columns (l)
  const double bqr = aqr * c2 - aqs * sn2, bqs = aqr * sn2 + aqs * c2;
  npr = c1 * bpr - s1 * bqr;  // rows (k)
  nps = c1 * bps - s1 * bqs;
  nqr = s1 * bpr + c1 * bqr;
  nqs = s1 * bps + c1 * bqs;
}

// The rotated block and its transpose into A (np x np): the matrix stays exactly symmetric
SDP_HD void sdp_store_block(double* A, int np, int p, int q, int r, int s, double npr, double nps, double nqr,
                            double nqs) {
  A[p * np + r] = npr;
  A[p * np + s] = nps;
  A[q * np + r] = nqr;
  A[q * np + s] = nqs;
  A[r * np + p] = npr;
  A[s * np + p] = nps;
  A[r * np + q] = nqr;
  A[s * np + q] = nqs;
}

// Q <- Q J for one row: the entries of the pair's two columns
SDP_HD void sdp_rotate_q(double qp, double qq, double c, double s, double& nqp, double& nqq) {
  nqp = c * qp - s * qq;
  nqq = s * qp + c * qq;
}

// ---- simplex projection of the eigenvalues: tau of the largest valid support -------------------------
// The support of li: the eigenvalues >= li, their number and their sum in ascending index (equal sets: equal sums,
// the same bits). Returns whether the support is valid; tau is that of the largest valid one.
SDP_HD double sdp_support_tau(double sum, int cnt) { return (sum - 1.0) / cnt; }

SDP_HD bool sdp_support(const double* lam, int n, double li, int& cnt, double& sum) {
  cnt = 0;
  sum = 0.0;
  for (int j = 0; j < n; ++j)
    if (lam[j] >= li) {
      ++cnt;
      sum += lam[j];
    }
  return li > sdp_support_tau(sum, cnt);
}

SDP_HD double sdp_simplex_weight(double lam, double tau) { return fmax(lam - tau, 0.0); }

// No valid support. In exact arithmetic the support of the largest eigenvalue alone is always valid (l > l - 1), but
// in fp64 l - 1 rounds back to l once l passes 2^53 (W = Z - U + M / rho grows with M and as rho halves), and a comparison
// with a NaN fails: then sdp_support is false for every index and no tau exists. The projection is then the limit of
// the rule: weight 1 on the first index of the largest eigenvalue (what a scan from index 0 with a strict > finds; a
// NaN gives way to the first number after it and is never chosen over one) and 0 elsewhere. Both routes take this
// when the largest valid support counts 0, and read no tau.
SDP_HD int sdp_fallback_index(const double* lam, int n) {
  int top = 0;
  for (int j = 1; j < n; ++j)
    if (lam[j] > lam[top] || (lam[top] != lam[top] && lam[j] == lam[j])) top = j;
  return top;
}

SDP_HD double sdp_fallback_weight(int i, int top) { return i == top ? 1.0 : 0.0; }

// ---- one entry's update: Z+ = proj_P(X + U), U+ = U + X - Z+, and its terms of the six sums of the stopping rule ----
struct SdpSums {
  double rp2, rd2, xx, zz, uu, mx;  // ||X - Z+||^2, ||Z+ - Z||^2, ||X||^2, ||Z+||^2, ||U+||^2, <M, X>
};

// Z+ of one entry from v = X + U: the projection onto P
SDP_HD double sdp_z_plus(double v, bool masked) { return masked ? fmax(v, 0.0) : 0.0; }

SDP_HD void sdp_update_entry(double x, double u, double z_old, bool masked, double m, double& zn, double& un,
                             SdpSums& terms) {
  const double v = x + u;
  zn = sdp_z_plus(v, masked);
  un = v - zn;
  terms.rp2 = (x - zn) * (x - zn);
  terms.rd2 = (zn - z_old) * (zn - z_old);
  terms.xx = x * x;
  terms.zz = zn * zn;
  terms.uu = un * un;
  terms.mx = m * x;
}

// ---- the stopping rule ----------------------------------------------------------------------------------------------
// The residuals and Boyd's tolerances for a variable of n * n entries; returns whether both residuals pass
SDP_HD bool sdp_residuals(const SdpSums& s, double rho, int n, double eps_abs, double eps_rel, double& r_p,
                          double& r_d) {
  r_p = sqrt(s.rp2);
  r_d = rho * sqrt(s.rd2);
  const double e_pri = n * eps_abs + eps_rel * fmax(sqrt(s.xx), sqrt(s.zz));
  const double e_dual = n * eps_abs + eps_rel * rho * sqrt(s.uu);
  return r_p <= e_pri && r_d <= e_dual;
}

// d: the dual bound lambda_max(M - rho U+), mx: <M, X>
SDP_HD bool sdp_gap_closed(double d, double mx, double eps_abs, double eps_rel) {
  return fabs(d - mx) <= eps_abs + eps_rel * fmax(fabs(d), fabs(mx));
}

// ---- residual balancing: the factor of rho after iteration `done`; U is rescaled by its inverse ---------------------
// A check is due at iteration c.adapt_next (10, 20, 30, ... while the moves keep one direction).
SDP_HD double sdp_balance_factor(const SdpCtl& c, int32_t done, bool conv, double r_p, double r_d) {
  double f = 1.0;
  if (!conv && done == c.adapt_next) {
    if (r_p > SDP_ADAPT_MU * r_d) f = SDP_ADAPT_TAU;
    else if (r_d > SDP_ADAPT_MU * r_p) f = 1.0 / SDP_ADAPT_TAU;
  }
  return f;
}

// The schedule after iteration `done` with factor f: a move that reverses the last one (up after down,
// down after up) doubles the interval between checks, so the penalty cannot go up and down for ever (the star graph's
// limit cycle); a check that moves nothing changes neither the interval nor the remembered direction, and a run whose
// moves keep one direction is checked every SDP_ADAPT_EVERY iterations, as before the schedule had a memory.
SDP_HD void sdp_balance_advance(SdpCtl& c, int32_t done, bool conv, double f) {
  if (conv || done != c.adapt_next) return;
  const int32_t dir = f > 1.0 ? 1 : (f < 1.0 ? -1 : 0);
  if (dir != 0) {
    if (c.adapt_dir == -dir && c.adapt_every <= SDP_ADAPT_MAX_EVERY / 2) c.adapt_every *= 2;
    c.adapt_dir = dir;
  }
  c.adapt_next = done > INT32_MAX - c.adapt_every ? INT32_MAX : done + c.adapt_every;
}

enum { SDP_RESCALE_NONE = 0, SDP_RESCALE_DIVIDE = 1, SDP_RESCALE_MULTIPLY = 2 };  // what a factor does to U

SDP_HD int sdp_rescale_of(double f) {
  return f == 1.0 ? SDP_RESCALE_NONE : (f == SDP_ADAPT_TAU ? SDP_RESCALE_DIVIDE : SDP_RESCALE_MULTIPLY);
}

// (call only with DIVIDE or MULTIPLY: both routes skip the pass over U when the factor is 1)
SDP_HD double sdp_rescale_u(double u, int rescale) {
  return rescale == SDP_RESCALE_DIVIDE ? u / SDP_ADAPT_TAU : u * SDP_ADAPT_TAU;
}

// The record an iteration leaves (dval is written where the dual bound is computed); f: sdp_balance_factor's
SDP_HD void sdp_close_iteration(SdpCtl& c, double r_p, double r_d, double mx, bool conv, double f, int32_t sw) {
  sdp_balance_advance(c, c.iters + 1, conv, f);
  c.iters = c.iters + 1;
  c.r_prim = r_p;
  c.r_dual = r_d;
  c.pval = mx;
  c.converged = conv;
  c.rho = c.rho * f;
  c.sweeps += sw;
}

}  // namespace clipper_hip
