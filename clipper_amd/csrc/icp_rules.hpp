// icp_rules.hpp — the rules of the ICP refinement ("ICP over a kept search grid"), stated once for
// the kernels (k_icp.hip.h), the driver (host_icp.hpp) and the host: the transform of a point, which list entry is an
// inlier, the origin the sums are taken about, the terms one source point adds (point-to-point: 17, point-to-plane and
// generalized: 30), the order in which they are added, the step of each method (the rotation of a 3 x 3 cross-covariance;
// LDL^T of the 6 x 6 normal equations and the Cayley map), the update of T and the stop rule; for the generalized
// (plane-to-plane) metric also the regularised covariance of a point. Plain sequential functions of one
// point, one set of sums or one iteration: which work item holds what belongs to the kernels. Every expression rounds as
// written (the build runs with -ffp-contract=off), no floating-point atomics anywhere, so that T_out and the history
// are functions of the inputs alone. No HIP: builds with g++ as well (tests/cpp/test_icp_rules.cpp runs whole ICPs over
// this header, tests/cpp/test_gicp_rules.cpp generalized ones); tests/icp_model.py and tests/gicp_model.py restate the
// same contract in numpy. The robust losses and the trimming of clipper_hip_icp_robust are additions at the end of each
// part (the weight of a pair, the weighted terms, the rank select of the trimming threshold): the plain rules keep their
// names and bits; tests/cpp/test_icp_robust_rules.cpp runs them, tests/icp_robust_model.py restates them.
#pragma once

#include <math.h>
#include <stdint.h>

#include "features_rules.hpp"

#define ICP_HD FEAT_HD

namespace clipper_hip {

constexpr int ICP_POINT_TO_POINT = 0, ICP_POINT_TO_PLANE = 1, ICP_GENERALIZED = 2;        // clipper_icp_params_t.method
constexpr int ICP_RUNNING = -1;                                                            // the record's status between rounds
constexpr int ICP_CONVERGED = 0, ICP_MAX_ITERATIONS = 1, ICP_TOO_FEW = 2, ICP_DEGENERATE = 3;  // clipper_icp_info_t.status
constexpr int ICP_MAX_ITERATIONS_LIMIT = 1000;
constexpr int ICP_BLOCK = 256;  // source points per workgroup of the sums: one partial each

// count, sum(q - o) 3, sum(b - o) 3, sum (b - o)(q - o)^T 9 row-major, sum sqd
constexpr int ICP_POINT_TERMS = 17;
// count, the 21 upper entries of J^T J row by row, the 6 of J^T r, sum r^2, sum sqd. (1 + 21 + 6 + 1 + 1 = 30.)
constexpr int ICP_PLANE_TERMS = 30;
// the generalized metric fills point-to-plane's positions: count, the 21 upper entries of J^T M J row by row, the 6 of
// J^T M d, d^T M d, sum sqd
constexpr int ICP_GENERALIZED_TERMS = ICP_PLANE_TERMS;
constexpr int icp_terms(int method) { return method == ICP_POINT_TO_POINT ? ICP_POINT_TERMS : ICP_PLANE_TERMS; }
// (generalized: 3, every pair gives three equations; the pivot test decides the rest)
constexpr int icp_min_count(int method) { return method == ICP_POINT_TO_PLANE ? 6 : 3; }

// The rank threshold of the point-to-plane system: DEGENERATE when a pivot of LDL^T is <= ICP_RANK_TOL times the largest
// diagonal entry of J^T J. The sums carry a relative rounding noise of about n * 2^-53 (1e-16 .. 1e-12 for the clouds
// this serves): 1e-10 sits above that noise and far below the smallest pivot ratio of any scan that constrains all six
// degrees of freedom (1e-4 and more).
constexpr double ICP_RANK_TOL = 1e-10;
// The point-to-point step is refused (DEGENERATE) when the fitted matrix is not a rotation: |det - 1| beyond this
// (a cross-covariance of rank < 2 leaves the fit undetermined).
constexpr double ICP_DET_TOL = 1e-9;

// ---- the transform of a point ---------------------------------------------------------------------------------------
// T: column-major 4 x 4 (entry (r, c) at T[c * 4 + r]); q_a = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3
ICP_HD void icp_transform_point(const double* T, const double (&p)[3], double (&q)[3]) {
  for (int a = 0; a < 3; ++a) q[a] = ((T[0 * 4 + a] * p[0] + T[1 * 4 + a] * p[1]) + T[2 * 4 + a] * p[2]) + T[3 * 4 + a];
}

// ---- correspondence -------------------------------------------------------------------------------------------------
// (j, sqd): the K = 1 entry of the search contract for q in the target. d2 = max_distance * max_distance, evaluated
// once by the caller.
ICP_HD bool icp_inlier(int32_t j, double sqd, double d2) { return feat_kept(j, sqd, true, d2); }

// ---- the origin: the centre of the target's bounding box ------------------------------------------------------------
ICP_HD void icp_origin(const double (&lo)[3], const double (&hi)[3], double (&o)[3]) {
  for (int a = 0; a < 3; ++a) o[a] = (lo[a] + hi[a]) * 0.5;
}

// ---- the terms of one inlier (a non-inlier adds +0.0 to every sum) --------------------------------------------------
ICP_HD void icp_point_terms(const double (&q)[3], const double (&b)[3], double sqd, const double (&o)[3],
                            double (&t)[ICP_POINT_TERMS]) {
  const double qo[3] = {q[0] - o[0], q[1] - o[1], q[2] - o[2]};
  const double bo[3] = {b[0] - o[0], b[1] - o[1], b[2] - o[2]};
  t[0] = 1.0;
  for (int a = 0; a < 3; ++a) {
    t[1 + a] = qo[a];
    t[4 + a] = bo[a];
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) t[7 + r * 3 + c] = bo[r] * qo[c];
  t[16] = sqd;
}

// J = [(q - o) x n, n], r = (q - b) . n
ICP_HD void icp_plane_terms(const double (&q)[3], const double (&b)[3], const double (&n)[3], double sqd,
                            const double (&o)[3], double (&t)[ICP_PLANE_TERMS]) {
  const double qo[3] = {q[0] - o[0], q[1] - o[1], q[2] - o[2]};
  const double d[3] = {q[0] - b[0], q[1] - b[1], q[2] - b[2]};
  double c[3];
  feat_cross(qo, n, c);
  const double J[6] = {c[0], c[1], c[2], n[0], n[1], n[2]};
  const double r = feat_dot(d, n);
  t[0] = 1.0;
  int at = 1;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) t[at++] = J[i] * J[j];
  for (int i = 0; i < 6; ++i) t[22 + i] = J[i] * r;
  t[28] = r * r;
  t[29] = sqd;
}

// ---- the generalized metric: the covariance of a point ---------------------------------------------------------------
// C = I - (1 - epsilon) nv nv^T of the unit vector nv: the eigenvalues (epsilon, 1, 1), epsilon along nv (Segal et
// al.'s plane-to-plane regularisation). w = 1.0 - epsilon, evaluated once by the caller. c = (xx, xy, xz, yy, yz, zz),
// feat_covariance's order. The sign of nv cancels in every product.
ICP_HD void icp_covariance_of_normal(const double (&nv)[3], double w, double (&c)[6]) {
  c[0] = 1.0 - w * (nv[0] * nv[0]);
  c[1] = 0.0 - w * (nv[0] * nv[1]);
  c[2] = 0.0 - w * (nv[0] * nv[2]);
  c[3] = 1.0 - w * (nv[1] * nv[1]);
  c[4] = 0.0 - w * (nv[1] * nv[2]);
  c[5] = 1.0 - w * (nv[2] * nv[2]);
}

// The covariance of a point from its cnt kept neighbours (features_rules.hpp's neighbourhood, covariance and smallest
// eigenvector; no sign rule): the identity below three, under which the point weighs as in point-to-point.
template <class Get>
ICP_HD void icp_point_covariance(int cnt, Get get, double w, double (&c)[6]) {
  if (cnt < 3) {
    c[0] = 1.0;
    c[1] = 0.0;
    c[2] = 0.0;
    c[3] = 1.0;
    c[4] = 0.0;
    c[5] = 1.0;
    return;
  }
  double s[6], nv[3];
  feat_covariance(cnt, get, s);
  feat_smallest_eigenvector(s, nv, nullptr);
  icp_covariance_of_normal(nv, w, c);
}

// ---- the generalized metric: the terms of one inlier ---------------------------------------------------------------------
// ca: the covariance of the source point, cb: of its target point (xx, xy, xz, yy, yz, zz); T: the current transform
// (column-major 4 x 4), R its upper-left 3 x 3. In this order, every sum of three products (u0 v0 + u1 v1) + u2 v2:
//   X = R C_a (9 entries), Y = X R^T (the upper triangle), S = C_b + Y (six entries: symmetric by construction);
//   M = S^-1 by the adjugate: the six cofactors k, det = (s00 k00 + s01 k01) + s02 k02, m = k / det (six divisions);
//   d = q - b, qo = q - o, J = [-[qo]x, I3] (3 x 6): the same xi = (w, v) about o as point-to-plane, whose row is n^T J;
//   G = M J (3 x 6): row r is (qo x m_r, m_r), m_r the row r of M;
//   H = J^T G (6 x 6, the upper entries): column j of H is (qo x g_j, g_j), g_j the column j of G;
//   e = M d, J^T e = (qo x e, e), d^T M d = d . e.
// A singular S needs no rule of its own: det rounds to 0 (or is not a number), the divisions leave non-numbers in the
// sums, and the pivot test of icp_step_plane (d > tol * big is false for a non-number) ends the call DEGENERATE with
// the previous T.
ICP_HD void icp_generalized_terms(const double (&q)[3], const double (&b)[3], const double (&ca)[6], const double (&cb)[6],
                                  const double* T, double sqd, const double (&o)[3], double (&t)[ICP_GENERALIZED_TERMS]) {
  const double R[3][3] = {{T[0], T[4], T[8]}, {T[1], T[5], T[9]}, {T[2], T[6], T[10]}};
  const double A[3][3] = {{ca[0], ca[1], ca[2]}, {ca[1], ca[3], ca[4]}, {ca[2], ca[4], ca[5]}};
  double X[3][3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 3; ++r)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 3; ++c) X[r][c] = (R[r][0] * A[0][c] + R[r][1] * A[1][c]) + R[r][2] * A[2][c];
  const double s00 = cb[0] + ((X[0][0] * R[0][0] + X[0][1] * R[0][1]) + X[0][2] * R[0][2]);
  const double s01 = cb[1] + ((X[0][0] * R[1][0] + X[0][1] * R[1][1]) + X[0][2] * R[1][2]);
  const double s02 = cb[2] + ((X[0][0] * R[2][0] + X[0][1] * R[2][1]) + X[0][2] * R[2][2]);
  const double s11 = cb[3] + ((X[1][0] * R[1][0] + X[1][1] * R[1][1]) + X[1][2] * R[1][2]);
  const double s12 = cb[4] + ((X[1][0] * R[2][0] + X[1][1] * R[2][1]) + X[1][2] * R[2][2]);
  const double s22 = cb[5] + ((X[2][0] * R[2][0] + X[2][1] * R[2][1]) + X[2][2] * R[2][2]);
  const double k00 = s11 * s22 - s12 * s12, k01 = s02 * s12 - s01 * s22, k02 = s01 * s12 - s02 * s11;
  const double k11 = s00 * s22 - s02 * s02, k12 = s01 * s02 - s00 * s12, k22 = s00 * s11 - s01 * s01;
  const double det = (s00 * k00 + s01 * k01) + s02 * k02;
  const double m00 = k00 / det, m01 = k01 / det, m02 = k02 / det, m11 = k11 / det, m12 = k12 / det, m22 = k22 / det;
  const double M[3][3] = {{m00, m01, m02}, {m01, m11, m12}, {m02, m12, m22}};
  const double qo[3] = {q[0] - o[0], q[1] - o[1], q[2] - o[2]};
  const double d[3] = {q[0] - b[0], q[1] - b[1], q[2] - b[2]};
  double G[3][6];  // M J
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int r = 0; r < 3; ++r) {
    double x[3];
    feat_cross(qo, M[r], x);
    for (int a = 0; a < 3; ++a) {
      G[r][a] = x[a];
      G[r][3 + a] = M[r][a];
    }
  }
  double H[6][6];  // J^T (M J): the entries with i <= j are used
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 6; ++j) {
    const double g[3] = {G[0][j], G[1][j], G[2][j]};
    double x[3];
    feat_cross(qo, g, x);
    for (int a = 0; a < 3; ++a) {
      H[a][j] = x[a];
      H[3 + a][j] = g[a];
    }
  }
  const double e[3] = {feat_dot(M[0], d), feat_dot(M[1], d), feat_dot(M[2], d)};
  double x[3];
  feat_cross(qo, e, x);
  t[0] = 1.0;
  int at = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = i; j < 6; ++j) t[at++] = H[i][j];
  for (int a = 0; a < 3; ++a) {
    t[22 + a] = x[a];
    t[25 + a] = e[a];
  }
  t[28] = feat_dot(d, e);
  t[29] = sqd;
}

// ---- robust losses: the weight of a kept pair, the weighted terms --------------------------------------------------------
// e: the squared residual of the pair, a value the term functions above already form: sqd (point-to-point), r * r
// (point-to-plane, position 28), d . e (generalized, position 28). k2 = scale * scale, evaluated once by the caller.
// Each weight is written in exactly this order. A non-number e leaves non-numbers in the sums (w * t of terms that are
// non-numbers themselves), and the pivot and determinant tests end the call DEGENERATE: no rule of its own. Tukey and
// Geman-McClure redescend: a pair far beyond the scale weighs nothing, so from a far start they may not converge.
constexpr int ICP_LOSS_NONE = 0, ICP_LOSS_HUBER = 1, ICP_LOSS_CAUCHY = 2, ICP_LOSS_TUKEY = 3, ICP_LOSS_GEMAN_MCCLURE = 4;

ICP_HD double icp_weight(int loss, double e, double scale, double k2) {
  if (loss == ICP_LOSS_HUBER) return e <= k2 ? 1.0 : scale / sqrt(e);
  if (loss == ICP_LOSS_CAUCHY) return 1.0 / (1.0 + e / k2);
  if (loss == ICP_LOSS_TUKEY) {
    if (!(e < k2)) return 0.0;
    const double u = 1.0 - e / k2;
    return u * u;
  }
  if (loss == ICP_LOSS_GEMAN_MCCLURE) {
    const double g = k2 / (k2 + e);
    return g * g;
  }
  return 1.0;
}

// The robust layouts. Every term becomes w * t[a] but the count (position 0) and the last term (sum sqd): count, fitness
// and rmse stay head counts and plain distances. Point-to-plane and generalized keep their 30 positions; point-to-point
// gains the sum of the weights: positions 0..15 as in icp_point_terms, 16 = sum w, 17 = sum sqd (still the last). With
// w = 1.0 every product is exact and sum w equals the count: the plain sums, bit for bit.
constexpr int ICP_POINT_ROBUST_TERMS = 18, ICP_POINT_WEIGHT_SUM = 16;
constexpr int icp_robust_terms(int method) { return method == ICP_POINT_TO_POINT ? ICP_POINT_ROBUST_TERMS : ICP_PLANE_TERMS; }
// the sums of a call: the plain layout, or the robust one
constexpr int icp_layout_terms(int method, bool robust) { return robust ? icp_robust_terms(method) : icp_terms(method); }

ICP_HD void icp_point_terms_weighted(const double (&t)[ICP_POINT_TERMS], double w, double (&out)[ICP_POINT_ROBUST_TERMS]) {
  out[0] = t[0];
  for (int a = 1; a < 16; ++a) out[a] = w * t[a];
  out[ICP_POINT_WEIGHT_SUM] = w;
  out[17] = t[16];
}

// point-to-plane and generalized, in place
ICP_HD void icp_plane_terms_weighted(double w, double (&t)[ICP_PLANE_TERMS]) {
  for (int a = 1; a < ICP_PLANE_TERMS - 1; ++a) t[a] = w * t[a];
}

// ---- the order of addition ------------------------------------------------------------------------------------------
// Work item i of a workgroup of ICP_BLOCK holds source point (block * ICP_BLOCK + i) in its original order (+0.0 past
// the end); the workgroup folds by the halving tree, stride 128 down to 1: v[i] = v[i] + v[i + s] for i < s; v[0] is
// its partial. One workgroup folds the partials: item t starts from +0.0 and adds partials t, t + 256, ... in that
// order; then the same tree. icp_tree is that tree written sequentially over ICP_BLOCK values with stride `pitch`
// (the host's copy: tests/cpp/test_icp_rules.cpp).
ICP_HD void icp_tree(double* v, int pitch) {
  for (int s = ICP_BLOCK / 2; s > 0; s >>= 1)
    for (int i = 0; i < s; ++i) v[i * pitch] = v[i * pitch] + v[(i + s) * pitch];
}

// ---- the rotation of a cross-covariance (Horn / Arun) ---------------------------------------------------------------
// 3 x 3 SVD by one-sided Jacobi on H = U S V^T (row-major); R = U diag(1, 1, det(U V^T)) V^T maximises trace(R^T H),
// the reflection fix acting on the smallest singular direction. Also behind clipper_hip_estimate_rigid_transform.
ICP_HD double icp_det3(const double* M) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

ICP_HD void rotation_from_cross_covariance(const double* H, double* R) {
  // one-sided Jacobi: rotate the columns of A = H until they are orthogonal; V accumulates
  double A[9], V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 9; ++i) A[i] = H[i];
  for (int sweep = 0; sweep < 60; ++sweep) {
    double offn = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int p = 0; p < 2; ++p)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int q = p + 1; q < 3; ++q) {
        double a = 0, b = 0, c = 0;
        for (int i = 0; i < 3; ++i) {
          a += A[i * 3 + p] * A[i * 3 + p];
          b += A[i * 3 + q] * A[i * 3 + q];
          c += A[i * 3 + p] * A[i * 3 + q];
        }
        const double rel = fabs(c) / (sqrt(a * b) + 1e-300);
        offn = offn < rel ? rel : offn;
        if (fabs(c) <= 1e-300) continue;
        const double zeta = (b - a) / (2.0 * c);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
        for (int i = 0; i < 3; ++i) {
          const double ap = A[i * 3 + p], aq = A[i * 3 + q];
          A[i * 3 + p] = cs * ap - sn * aq;
          A[i * 3 + q] = sn * ap + cs * aq;
          const double vp = V[i * 3 + p], vq = V[i * 3 + q];
          V[i * 3 + p] = cs * vp - sn * vq;
          V[i * 3 + q] = sn * vp + cs * vq;
        }
      }
    if (offn < 1e-15) break;
  }
  // singular values = column norms of A, U = A / s; the reflection fix must act on the SMALLEST singular direction
  // (the first among equal ones)
  double s[3], U[9];
  for (int j = 0; j < 3; ++j) s[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
  int smallest = 0;
  double least = s[0];
  if (s[1] < least) {
    smallest = 1;
    least = s[1];
  }
  if (s[2] < least) {
    smallest = 2;
    least = s[2];
  }
  for (int j = 0; j < 3; ++j)
    for (int i = 0; i < 3; ++i) U[i * 3 + j] = s[j] > 1e-300 ? A[i * 3 + j] / s[j] : 0.0;
  // a vanishing singular value leaves its column of U undetermined: complete it by a cross product
  if (least <= 1e-300 * (s[0] + s[1] + s[2]) || least == 0.0) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int m = 0; m < 3; ++m)
      if (m == smallest) {
        const int a = (m + 1) % 3, b = (m + 2) % 3;
        U[0 * 3 + m] = U[1 * 3 + a] * U[2 * 3 + b] - U[2 * 3 + a] * U[1 * 3 + b];
        U[1 * 3 + m] = U[2 * 3 + a] * U[0 * 3 + b] - U[0 * 3 + a] * U[2 * 3 + b];
        U[2 * 3 + m] = U[0 * 3 + a] * U[1 * 3 + b] - U[1 * 3 + a] * U[0 * 3 + b];
      }
  }
  const double sgn = icp_det3(U) * icp_det3(V) < 0 ? -1.0 : 1.0;  // det(U V^T)
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double r = 0.0;
      for (int k = 0; k < 3; ++k) r += U[i * 3 + k] * (k == smallest ? sgn : 1.0) * V[j * 3 + k];
      R[i * 3 + j] = r;
    }
}

// dT (column-major 4 x 4) of the rotation R (row-major 3 x 3) about the origin o followed by the shift v:
// x -> R (x - o) + o + v, so the translation is v_a + (o_a - (R o)_a)
ICP_HD void icp_about_origin(const double* R, const double (&v)[3], const double (&o)[3], double* dT) {
  for (int a = 0; a < 3; ++a) {
    const double Ro = (R[a * 3 + 0] * o[0] + R[a * 3 + 1] * o[1]) + R[a * 3 + 2] * o[2];
    for (int c = 0; c < 3; ++c) dT[c * 4 + a] = R[a * 3 + c];
    dT[3 * 4 + a] = v[a] + (o[a] - Ro);
    dT[a * 4 + 3] = 0.0;
  }
  dT[15] = 1.0;
}

// ---- the step, point-to-point ---------------------------------------------------------------------------------------
// S: the 17 sums. Centroids mq = sum(q - o) / n, mb = sum(b - o) / n; H_rc = S_rc - sum(b - o)_r * mq_c (the centred
// cross-covariance sum (b - mb)(q - mq)^T); dR = its rotation; the shift is mb - dR mq, about o. false: DEGENERATE.
// icp_step_point_by: the same step with the centroids divided by `n` (the robust layout: the sum of the weights).
ICP_HD bool icp_step_point_by(const double* S, double n, const double (&o)[3], double* dT) {
  const double mq[3] = {S[1] / n, S[2] / n, S[3] / n};
  const double mb[3] = {S[4] / n, S[5] / n, S[6] / n};
  double H[9], R[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) H[r * 3 + c] = S[7 + r * 3 + c] - S[4 + r] * mq[c];
  rotation_from_cross_covariance(H, R);
  double v[3];
  for (int a = 0; a < 3; ++a) v[a] = mb[a] - ((R[a * 3 + 0] * mq[0] + R[a * 3 + 1] * mq[1]) + R[a * 3 + 2] * mq[2]);
  icp_about_origin(R, v, o, dT);
  return fabs(icp_det3(R) - 1.0) <= ICP_DET_TOL;
}

ICP_HD bool icp_step_point(const double* S, const double (&o)[3], double* dT) { return icp_step_point_by(S, S[0], o, dT); }

// ---- the step, point-to-plane and generalized: the 6 x 6 step ----------------------------------------------------------
// the Cayley map of the rotation vector w: a = w / 2, K = skew(a), R = I + 2 / (1 + |a|^2) (K + K^2), K^2 = a a^T - |a|^2 I.
// An exact rotation for every w, and no sin or cos.
ICP_HD void icp_cayley(const double (&w)[3], double* R) {
  const double a[3] = {w[0] * 0.5, w[1] * 0.5, w[2] * 0.5};
  const double aa = feat_dot(a, a);
  const double s = 2.0 / (1.0 + aa);
  const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c)
      R[r * 3 + c] = (r == c ? 1.0 : 0.0) + s * (K[r * 3 + c] + (a[r] * a[c] - (r == c ? aa : 0.0)));
}

// S: the 30 sums. J^T J xi = -J^T r (generalized: J^T M J xi = -J^T M d, in the same positions) by LDL^T without
// pivoting; every loop runs in ascending order of its index. false: DEGENERATE (a pivot <= ICP_RANK_TOL * the largest
// diagonal entry, or not a number).
ICP_HD bool icp_step_plane(const double* S, const double (&o)[3], double* dT) {
  double A[6][6], L[6][6], D[6], y[6], x[6];
  int at = 1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = i; j < 6; ++j) {
      A[i][j] = S[at];
      A[j][i] = S[at];
      ++at;
    }
  double big = A[0][0];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 1; i < 6; ++i) big = A[i][i] > big ? A[i][i] : big;
  bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < j; ++k) d = d - L[j][k] * (L[j][k] * D[k]);
    ok = ok && d > ICP_RANK_TOL * big;
    D[j] = d;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int k = 0; k < j; ++k) s = s - L[i][k] * (L[j][k] * D[k]);
      L[i][j] = s / d;
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i) {
    double s = -S[22 + i];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s;
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 5; i >= 0; --i) {
    double s = y[i] / D[i];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
    x[i] = s;
  }
  const double w[3] = {x[0], x[1], x[2]}, v[3] = {x[3], x[4], x[5]};
  double R[9];
  icp_cayley(w, R);
  icp_about_origin(R, v, o, dT);
  return ok;
}

// ---- the update: T <- dT T, nothing re-orthonormalised --------------------------------------------------------------
ICP_HD void icp_compose(const double* dT, double* T) {
  double N[16];
  for (int c = 0; c < 4; ++c) {
    for (int r = 0; r < 3; ++r) {
      const double v = (dT[0 * 4 + r] * T[c * 4 + 0] + dT[1 * 4 + r] * T[c * 4 + 1]) + dT[2 * 4 + r] * T[c * 4 + 2];
      N[c * 4 + r] = c == 3 ? v + dT[3 * 4 + r] : v;
    }
    N[c * 4 + 3] = c == 3 ? 1.0 : 0.0;
  }
  for (int i = 0; i < 16; ++i) T[i] = N[i];
}

// ---- one iteration behind the sums ----------------------------------------------------------------------------------
// the record the step kernel leaves (64 bytes); the host reads it once per iteration
struct alignas(64) IcpRecord {
  int32_t iterations;  // k: T has been updated k times when the last history row was taken
  int32_t status;      // ICP_RUNNING, or why the loop ended
  int64_t count;
  double fitness, rmse;  // of the last history row
  double pad[4];
};
static_assert(sizeof(IcpRecord) == 64, "the status record is 64 bytes");

struct IcpStop {
  int max_iterations;
  int64_t n_src;
  double rel_fitness, rel_rmse;
};

// Iteration k from its sums S (the last of them sum sqd): fitness = count / n_src, rmse = sqrt(sum sqd / count) (0
// without inliers), the history row (count, fitness, rmse), then the first that holds of: CONVERGED (k >= 1, both
// changes below their bounds), TOO_FEW, MAX_ITERATIONS (k == max_iterations), DEGENERATE (the step refuses, or the
// updated T would hold a value that is not finite); else T <- dT T and the loop goes on. rec carries iteration k - 1's
// fitness and rmse in, and this iteration's out. T is touched only where the loop goes on.
// ROBUST: S is in the robust layout (icp_robust_terms), whose point-to-point centroids divide by the sum of the weights.
template <int METHOD, bool ROBUST>
ICP_HD void icp_iterate_over(const IcpStop& p, int k, const double* S, const double (&o)[3], double* T, IcpRecord& rec,
                             double* row) {
  constexpr int TERMS = icp_layout_terms(METHOD, ROBUST);
  const double cnt = S[0];
  const double fitness = cnt / static_cast<double>(p.n_src);
  const double rmse = cnt > 0.0 ? sqrt(S[TERMS - 1] / cnt) : 0.0;
  if (row) {
    row[0] = cnt;
    row[1] = fitness;
    row[2] = rmse;
  }
  int status = ICP_RUNNING;
  if (k >= 1 && fabs(fitness - rec.fitness) < p.rel_fitness && fabs(rmse - rec.rmse) < p.rel_rmse) status = ICP_CONVERGED;
  else if (cnt < static_cast<double>(icp_min_count(METHOD))) status = ICP_TOO_FEW;
  else if (k >= p.max_iterations) status = ICP_MAX_ITERATIONS;
  else {
    double dT[16], N[16];
    bool ok;
    if constexpr (METHOD != ICP_POINT_TO_POINT) ok = icp_step_plane(S, o, dT);
    else if constexpr (ROBUST) ok = icp_step_point_by(S, S[ICP_POINT_WEIGHT_SUM], o, dT);
    else ok = icp_step_point(S, o, dT);
    for (int i = 0; i < 16; ++i) N[i] = T[i];
    icp_compose(dT, N);
    bool finite = true;
    for (int i = 0; i < 16; ++i) finite = finite && fabs(N[i]) <= 1.7976931348623157e308;
    if (ok && finite)
      for (int i = 0; i < 16; ++i) T[i] = N[i];
    else
      status = ICP_DEGENERATE;
  }
  rec.iterations = k;
  rec.status = status;
  rec.count = static_cast<int64_t>(cnt);
  rec.fitness = fitness;
  rec.rmse = rmse;
}

template <int METHOD>
ICP_HD void icp_iterate(const IcpStop& p, int k, const double* S, const double (&o)[3], double* T, IcpRecord& rec, double* row) {
  icp_iterate_over<METHOD, false>(p, k, S, o, T, rec, row);
}

// ---- trimming: the threshold by an exact rank select ------------------------------------------------------------------
// Each iteration, under the current T: within = the source points whose K = 1 entry passes icp_inlier;
// keep = (int64_t)(trim * (double)within); tau = the keep-th smallest sqd among them, by value; a point is kept iff it
// passes icp_inlier and sqd <= tau (every point equal to tau is kept, so the count may exceed keep). keep == 0 keeps
// nothing (the round ends TOO_FEW); trim == 1.0 skips the selection: kept = within. sqd of a candidate is non-negative
// and finite, so its bit pattern as uint64_t orders as its value: the select is a most-significant-digit-first radix
// select on those 64 bits, ICP_SELECT_PASSES digits of ICP_SELECT_BITS. Pass p: the histogram of digit p over the
// candidates whose higher digits equal the prefix found so far, then the digit at which the running count first
// reaches the remaining rank (1-based). Every digit width gives the same tau.
constexpr int ICP_SELECT_BITS = 8, ICP_SELECT_RADIX = 1 << ICP_SELECT_BITS, ICP_SELECT_PASSES = 64 / ICP_SELECT_BITS;

ICP_HD int64_t icp_trim_keep(double trim, int64_t within) { return static_cast<int64_t>(trim * static_cast<double>(within)); }

// digit `pass` of a key, the most significant first
ICP_HD uint32_t icp_select_digit(uint64_t key, int pass) {
  return static_cast<uint32_t>(key >> (64 - ICP_SELECT_BITS * (pass + 1))) & (ICP_SELECT_RADIX - 1);
}
// do the digits of `key` above digit `pass` equal `prefix` (those digits, right-aligned)?
ICP_HD bool icp_select_candidate(uint64_t key, uint64_t prefix, int pass) {
  return pass == 0 || (key >> (64 - ICP_SELECT_BITS * pass)) == prefix;
}
// Is this the digit of the rank-th smallest candidate? before: the candidates with a smaller digit, count: with this one.
// Exactly one digit answers true when 1 <= rank <= the sum of the counts; the rank among its candidates is rank - before.
ICP_HD bool icp_select_hit(int64_t before, int64_t count, int64_t rank) { return before < rank && rank <= before + count; }

// The per-digit step: hist (ICP_SELECT_RADIX counts) and rank in; the digit and the rank among its candidates out.
// (The pick kernel asks icp_select_hit of every digit at once, `before` coming from an exclusive scan.)
ICP_HD void icp_select_step(const uint32_t* hist, int64_t rank, int& digit, int64_t& next) {
  int64_t before = 0;
  digit = ICP_SELECT_RADIX - 1;
  next = 0;
  for (int d = 0; d < ICP_SELECT_RADIX; ++d) {
    if (icp_select_hit(before, static_cast<int64_t>(hist[d]), rank)) {
      digit = d;
      next = rank - before;
      return;
    }
    before += static_cast<int64_t>(hist[d]);
  }
}

// The control block of the selection on the device (64 bytes): the weighted sums read tau and any from it, never from
// the host. Without trimming it holds tau = max_distance^2, any = 1 for the whole call.
struct alignas(64) IcpSelect {
  uint64_t prefix;  // the digits found so far, right-aligned
  int64_t rank;     // the remaining rank, 1-based
  int64_t within, keep;
  double tau;       // the threshold once the last pass has run; 0 when nothing is kept
  int32_t any;      // keep > 0
  int32_t pad[5];
};
static_assert(sizeof(IcpSelect) == 64, "the control block of the selection is 64 bytes");

ICP_HD bool icp_kept(int32_t j, double sqd, double d2, double tau, int32_t any) {
  return icp_inlier(j, sqd, d2) && any != 0 && sqd <= tau;
}

}  // namespace clipper_hip
