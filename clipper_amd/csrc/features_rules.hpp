// features_rules.hpp — the arithmetic of the point-cloud features ("Normals and FPFH"), stated
// once for the kernels (k_features.hip.h) and the host: which entries of a nearest-neighbour list form a point's
// neighbourhood, the two-pass centred covariance, the eigenvector of the smallest eigenvalue of a symmetric 3 x 3
// (cyclic Jacobi with the rotation of sdp_rules.hpp), the sign rule of a normal, the pair feature of two oriented points
// and its three bins, the SPFH scale and the FPFH weighting. Plain sequential functions of one neighbourhood, one pair
// or one bin: which work item holds what belongs to the kernels. Every expression rounds as written (the build runs
// with -ffp-contract=off); a dot product is (a0*b0 + a1*b1) + a2*b2 everywhere. No HIP: builds with g++ as well
// (tests/cpp/test_features_rules.cpp). tests/features_model.py restates the same contract in numpy.
#pragma once

#include <math.h>
#include <stdint.h>

#include "sdp_rules.hpp"

#define FEAT_HD SDP_HD

namespace clipper_hip {

constexpr int FEAT_MIN_KNN = 3, FEAT_MAX_KNN = 32;  // neighbours per point (the point itself included)
constexpr int FEAT_BINS = 11;                       // per angle
constexpr int FEAT_DIM = 3 * FEAT_BINS;             // numbers per descriptor: theta, alpha, phi
constexpr int FEAT_MAX_SWEEPS = 16;                 // of the 3 x 3 Jacobi (it converges quadratically: 4 to 6 are used)
constexpr double FEAT_JACOBI_TOL = 1e-16;           // stop sweeping when off(A) <= tol * ||A||_F
constexpr double FEAT_PI = 3.14159265358979323846;

// ---- the neighbourhood ----------------------------------------------------------------------------------------------
// entry (j, sqd) of a list (ascending, -1 / 1e300 past the end) is kept iff it exists and lies within the radius;
// r2 = radius * radius, evaluated once by the caller; use_r = radius > 0. The kept entries are a prefix of the list.
FEAT_HD bool feat_kept(int32_t j, double sqd, bool use_r, double r2) { return j >= 0 && (!use_r || sqd <= r2); }

FEAT_HD double feat_dot(const double (&a)[3], const double (&b)[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

FEAT_HD void feat_cross(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// ---- normals --------------------------------------------------------------------------------------------------------
// Two passes over the cnt kept neighbours, in list order: the centroid, then the sums of products of the centred
// coordinates, c = (xx, xy, xz, yy, yz, zz) (not divided by cnt: the eigenvectors are the same). get(k, p) fetches
// neighbour k.
template <class Get>
FEAT_HD void feat_covariance(int cnt, Get get, double (&c)[6]) {
  double m[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < cnt; ++k) {
    double p[3];
    get(k, p);
    m[0] = m[0] + p[0];
    m[1] = m[1] + p[1];
    m[2] = m[2] + p[2];
  }
  const double w = static_cast<double>(cnt);
  m[0] = m[0] / w;
  m[1] = m[1] / w;
  m[2] = m[2] / w;
  for (int a = 0; a < 6; ++a) c[a] = 0.0;
  for (int k = 0; k < cnt; ++k) {
    double p[3];
    get(k, p);
    const double x = p[0] - m[0], y = p[1] - m[1], z = p[2] - m[2];
    c[0] = c[0] + x * x;
    c[1] = c[1] + x * y;
    c[2] = c[2] + x * z;
    c[3] = c[3] + y * y;
    c[4] = c[4] + y * z;
    c[5] = c[5] + z * z;
  }
}

// One Jacobi rotation of the symmetric 3 x 3 on the pair (p, q), r the third index: a_pq becomes zero, the columns p
// and q of V turn with it. Every argument is a named scalar or a column, so that nothing is indexed at run time.
FEAT_HD void feat_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double (&vp)[3], double (&vq)[3]) {
  double c, s, tn;
  sdp_rotation(apq, app, aqq, c, s, tn);
  app = app - tn * apq;
  aqq = aqq + tn * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq;
  arq = s * rp + c * rq;
  for (int k = 0; k < 3; ++k) {
    const double x = vp[k], y = vq[k];
    vp[k] = c * x - s * y;
    vq[k] = s * x + c * y;
  }
}

// The unit eigenvector nv of the smallest eigenvalue of the symmetric matrix c = (xx, xy, xz, yy, yz, zz), by cyclic
// Jacobi (backward stable); among equal eigenvalues the first. ev (may be null): the three eigenvalues, unsorted.
FEAT_HD void feat_smallest_eigenvector(const double (&c)[6], double (&nv)[3], double* ev) {
  double a00 = c[0], a01 = c[1], a02 = c[2], a11 = c[3], a12 = c[4], a22 = c[5];
  double v0[3] = {1.0, 0.0, 0.0}, v1[3] = {0.0, 1.0, 0.0}, v2[3] = {0.0, 0.0, 1.0};
  for (int sweep = 0; sweep < FEAT_MAX_SWEEPS; ++sweep) {
    const double off = 2.0 * ((a01 * a01 + a02 * a02) + a12 * a12);
    const double all = ((a00 * a00 + a11 * a11) + a22 * a22) + off;
    if (!(off > FEAT_JACOBI_TOL * FEAT_JACOBI_TOL * all)) break;
    feat_rotate(a00, a11, a01, a02, a12, v0, v1);
    feat_rotate(a00, a22, a02, a01, a12, v0, v2);
    feat_rotate(a11, a22, a12, a01, a02, v1, v2);
  }
  const bool pick1 = a11 < a00;
  double best = pick1 ? a11 : a00;
  for (int k = 0; k < 3; ++k) nv[k] = pick1 ? v1[k] : v0[k];
  if (a22 < best) {
    best = a22;
    for (int k = 0; k < 3; ++k) nv[k] = v2[k];
  }
  const double len = sqrt(feat_dot(nv, nv));
  for (int k = 0; k < 3; ++k) nv[k] = nv[k] / len;
  if (ev) {
    ev[0] = a00;
    ev[1] = a11;
    ev[2] = a22;
  }
}

// The sign rule: towards the viewpoint (n . (view - p) >= 0), or without one the component of largest magnitude
// positive (the first such component on ties).
FEAT_HD void feat_orient(double (&nv)[3], const double (&p)[3], const double* view) {
  bool flip;
  if (view) {
    const double d[3] = {view[0] - p[0], view[1] - p[1], view[2] - p[2]};
    flip = feat_dot(nv, d) < 0.0;
  } else {
    double big = nv[0];
    if (fabs(nv[1]) > fabs(big)) big = nv[1];
    if (fabs(nv[2]) > fabs(big)) big = nv[2];
    flip = big < 0.0;
  }
  if (flip)
    for (int k = 0; k < 3; ++k) nv[k] = -nv[k];
}

// The normal of point p from its cnt kept neighbours: (0, 0, 1) below three
template <class Get>
FEAT_HD void feat_normal(int cnt, Get get, const double (&p)[3], const double* view, double (&nv)[3]) {
  if (cnt < 3) {
    nv[0] = 0.0;
    nv[1] = 0.0;
    nv[2] = 1.0;
    return;
  }
  double c[6];
  feat_covariance(cnt, get, c);
  feat_smallest_eigenvector(c, nv, nullptr);
  feat_orient(nv, p, view);
}

// ---- the pair feature (theta, alpha, phi) of (p1, n1), (p2, n2) --------------------------------------------------------
// The Darboux frame sits at the point whose normal makes the smaller angle with the line between the two; a pair
// without a line (L == 0) or without a frame (the line along that normal) has the feature (0, 0, 0).
FEAT_HD void feat_pair(const double (&p1)[3], const double (&n1)[3], const double (&p2)[3], const double (&n2)[3],
                       double (&f)[3]) {
  f[0] = 0.0;
  f[1] = 0.0;
  f[2] = 0.0;
  const double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
  const double L = sqrt(feat_dot(dp, dp));
  if (L == 0.0) return;
  const double a1 = feat_dot(n1, dp) / L, a2 = feat_dot(n2, dp) / L;
  const bool swap = fabs(a1) < fabs(a2);
  double m1[3], m2[3], d[3];
  for (int k = 0; k < 3; ++k) {
    m1[k] = swap ? n2[k] : n1[k];
    m2[k] = swap ? n1[k] : n2[k];
    d[k] = swap ? -dp[k] : dp[k];
  }
  const double phi = swap ? -a2 : a1;
  double v[3], w[3];
  feat_cross(d, m1, v);
  const double vl = sqrt(feat_dot(v, v));
  if (vl == 0.0) return;
  for (int k = 0; k < 3; ++k) v[k] = v[k] / vl;
  feat_cross(m1, v, w);
  f[0] = atan2(feat_dot(w, m2), feat_dot(m1, m2));
  f[1] = feat_dot(v, m2);
  f[2] = phi;
}

// ---- bins -----------------------------------------------------------------------------------------------------------
// where a feature falls on the 11-bin axis of its angle, before the floor
FEAT_HD double feat_coord_theta(double theta) { return 11.0 * (theta + FEAT_PI) / (2.0 * FEAT_PI); }
FEAT_HD double feat_coord_unit(double x) { return 11.0 * (x + 1.0) * 0.5; }  // alpha and phi, in [-1, 1]

FEAT_HD int feat_bin(double coord) {
  double b = floor(coord);
  if (b < 0.0) b = 0.0;
  if (b > 10.0) b = 10.0;
  return static_cast<int>(b);
}

// the three counters of the 33 a pair adds one to
FEAT_HD void feat_bins(const double (&f)[3], int (&b)[3]) {
  b[0] = feat_bin(feat_coord_theta(f[0]));
  b[1] = FEAT_BINS + feat_bin(feat_coord_unit(f[1]));
  b[2] = 2 * FEAT_BINS + feat_bin(feat_coord_unit(f[2]));
}

// ---- SPFH and FPFH --------------------------------------------------------------------------------------------------
// SPFH(i)[b] = count[b] * feat_spfh_scale(cnt(i)): one multiplication per bin, so the counts gather in any order
FEAT_HD double feat_spfh_scale(int cnt) { return cnt < 2 ? 0.0 : 100.0 / static_cast<double>(cnt - 1); }

// one neighbour's share of bin b of FPFH(i); neighbours with j == i or sqd == 0 have none
FEAT_HD bool feat_weighs(int32_t j, int32_t i, double sqd) { return j != i && sqd != 0.0; }
FEAT_HD double feat_fpfh_add(double f, double spfh_j, double sqd) { return f + spfh_j / sqd; }

// a bin of the result: f scaled by its group's sum s (the 11 bins added in ascending order from 0.0), plus SPFH(i)
FEAT_HD double feat_fpfh_bin(double f, double s, double spfh_i) {
  if (s != 0.0) f = f * (100.0 / s);
  return f + spfh_i;
}

}  // namespace clipper_hip
