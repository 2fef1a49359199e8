// host_icp_check.hpp — ICP and the evaluation of a registration, the part that needs no device: the argument checks of
// clipper_hip_icp, clipper_hip_icp_generalized, their robust forms (clipper_hip_icp_robust,
// clipper_hip_icp_generalized_robust), clipper_hip_cloud_icp, clipper_hip_estimate_covariances and
// clipper_hip_evaluate_registration. check_call at the end is a whole ICP call: every refusal of the five ICP entry
// points in the order they are tried, told the call's family, its use of robust settings and whether its clouds are
// host arrays. Pure host code (no HIP): tests/cpp/test_icp_rules.cpp, tests/cpp/test_gicp_rules.cpp and
// tests/cpp/test_icp_call_checks.cpp compile it with g++ alone. A refusal comes back as its message (empty: accepted)
// and names the offending value; the caller hands it to fail(). Every check runs before any device work.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "host_features_check.hpp"
#include "icp_rules.hpp"

namespace clipper_icp {

using clipper_match::format;

// clipper_icp_params_t, as the checks read it
struct Params {
  int method, max_iterations;
  double max_distance, rel_fitness, rel_rmse;
};

// `what` names the cloud in the message ("source", "target")
inline std::string check_cloud(const char* what, const double* P, int64_t n) {
  if (!P) return format("null %s point array", what);
  if (n < 1) return format("%s: a cloud needs at least one point (n = %lld)", what, static_cast<long long>(n));
  if (n > INT32_MAX) return format("%s: more than 2^31 - 1 points in a cloud (n = %lld)", what, static_cast<long long>(n));
  for (int64_t p = 0; p < n; ++p)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(P[p * 3 + k]))
        return format("%s: non-finite value at coordinate %d of point %lld", what, k, static_cast<long long>(p));
  return {};
}

// T: column-major 4 x 4, or null for the identity. `what`: "T_init", "T"
inline std::string check_transform(const char* what, const double* T) {
  if (!T) return {};
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 4; ++r)
      if (!std::isfinite(T[c * 4 + r])) return format("%s: non-finite value at entry (%d, %d)", what, r, c);
  for (int c = 0; c < 4; ++c)
    if (T[c * 4 + 3] != (c == 3 ? 1.0 : 0.0))
      return format("%s: the bottom row must be 0 0 0 1 (entry (3, %d) = %.17g)", what, c, T[c * 4 + 3]);
  return {};
}

inline std::string check_max_distance(double d) {
  if (!(std::isfinite(d) && d > 0.0)) return format("max_distance must be positive and finite (max_distance = %g)", d);
  return {};
}

// what every method asks of the parameters besides the method itself
inline std::string check_loop_params(const Params* p) {
  std::string why = check_max_distance(p->max_distance);
  if (!why.empty()) return why;
  if (p->max_iterations < 0 || p->max_iterations > clipper_hip::ICP_MAX_ITERATIONS_LIMIT)
    return format("max_iterations must be in 0..%d (max_iterations = %d)", clipper_hip::ICP_MAX_ITERATIONS_LIMIT, p->max_iterations);
  if (!(p->rel_fitness >= 0.0)) return format("rel_fitness must be at least 0 (rel_fitness = %g)", p->rel_fitness);
  if (!(p->rel_rmse >= 0.0)) return format("rel_rmse must be at least 0 (rel_rmse = %g)", p->rel_rmse);
  return {};
}

// the parameters of clipper_hip_icp and clipper_hip_evaluate_registration: point-to-point or point-to-plane
inline std::string check_params(const Params* p) {
  if (!p) return "null params";
  if (p->method != clipper_hip::ICP_POINT_TO_POINT && p->method != clipper_hip::ICP_POINT_TO_PLANE)
    return format("unknown method %d", p->method);
  return check_loop_params(p);
}

// clipper_hip_icp has no covariances to give the generalized metric: it names the call that takes them
inline std::string check_not_generalized(const Params* p) {
  if (p && p->method == clipper_hip::ICP_GENERALIZED)
    return "method 2 (generalized) takes per-point covariances: call clipper_hip_icp_generalized";
  return {};
}

// the parameters of clipper_hip_icp_generalized: that method alone
inline std::string check_generalized_params(const Params* p) {
  if (!p) return "null params";
  if (p->method != clipper_hip::ICP_GENERALIZED)
    return format("method must be CLIPPER_ICP_GENERALIZED (2) (method = %d)", p->method);
  return check_loop_params(p);
}

// epsilon of clipper_hip_estimate_covariances: the eigenvalue along the normal, in (0, 1]
inline std::string check_epsilon(double epsilon) {
  if (!(epsilon > 0.0 && epsilon <= 1.0)) return format("epsilon must be in (0, 1] (epsilon = %g)", epsilon);
  return {};
}

// C: 6 x n (xx, xy, xz, yy, yz, zz per point), every entry finite and every matrix positive definite: its three leading
// minors > 0, evaluated in fp64 as written (the third is the determinant of icp_generalized_terms). `what`: "source",
// "target"
inline std::string check_covariances(const char* what, const double* C, int64_t n) {
  if (!C) return format("null %s covariance array", what);
  for (int64_t p = 0; p < n; ++p) {
    const double* c = C + p * 6;
    for (int k = 0; k < 6; ++k)
      if (!std::isfinite(c[k]))
        return format("%s covariances: non-finite value at entry %d of point %lld", what, k, static_cast<long long>(p));
    const double s00 = c[0], s01 = c[1], s02 = c[2], s11 = c[3], s12 = c[4], s22 = c[5];
    const double k00 = s11 * s22 - s12 * s12, k01 = s02 * s12 - s01 * s22, k02 = s01 * s12 - s02 * s11;
    const double minor[3] = {s00, s00 * s11 - s01 * s01, (s00 * k00 + s01 * k01) + s02 * k02};
    for (int k = 0; k < 3; ++k)
      if (!(minor[k] > 0.0))
        return format("%s covariances: the matrix of point %lld is not positive definite (leading minor %d = %.17g)", what,
                      static_cast<long long>(p), k + 1, minor[k]);
  }
  return {};
}

// clipper_icp_robust_t, as the checks read it
struct Robust {
  int loss, reserved;
  double scale, trim;
};

// the robust settings of clipper_hip_icp_robust and clipper_hip_icp_generalized_robust. scale is read only with a loss.
inline std::string check_robust(const Robust* r) {
  if (!r) return "null robust";
  if (r->loss < clipper_hip::ICP_LOSS_NONE || r->loss > clipper_hip::ICP_LOSS_GEMAN_MCCLURE)
    return format("unknown loss %d (the losses are 0..%d)", r->loss, clipper_hip::ICP_LOSS_GEMAN_MCCLURE);
  if (r->reserved != 0) return format("robust: reserved must be 0 (reserved = %d)", r->reserved);
  if (r->loss != clipper_hip::ICP_LOSS_NONE && !(std::isfinite(r->scale) && r->scale > 0.0))
    return format("scale must be positive and finite with a loss (scale = %g)", r->scale);
  if (!(r->trim > 0.0 && r->trim <= 1.0)) return format("trim must be in (0, 1] (trim = %g)", r->trim);
  return {};
}

// the target's normals: needed by point-to-plane alone, and then unit (host_features_check.hpp's rule)
inline std::string check_target_normals(int method, const double* N, int64_t n) {
  if (method != clipper_hip::ICP_POINT_TO_PLANE) return {};
  if (!N) return "point-to-plane needs the target's normals (N_tgt is null)";
  return clipper_features::check_normals(N, n);
}

// ---- a whole ICP call ---------------------------------------------------------------------------------------------------
// which parameter check a call runs: clipper_hip_icp and its robust form take point-to-point and point-to-plane and name
// the other call for the generalized method; clipper_hip_icp_generalized and its robust form take that method alone; a
// call on cloud handles takes all three and checks the parameters by the method given
enum Family { FAMILY_POINT_PLANE, FAMILY_GENERALIZED, FAMILY_BY_METHOD };
// REQUIRED: a null robust is refused; OPTIONAL: checked when given; ABSENT: the call has none
enum RobustUse { ROBUST_ABSENT, ROBUST_OPTIONAL, ROBUST_REQUIRED };

// the clouds of a host-buffer call and what the methods read of them: N_tgt for point-to-plane, C_src / C_tgt (6 x n) for
// generalized
struct HostClouds {
  const double* P_src;
  int64_t n_src;
  const double* P_tgt;
  int64_t n_tgt;
  const double *N_tgt, *C_src, *C_tgt;
};

// Every refusal of an ICP call that needs no device, in the order the entry points try them: T_out, the parameters, the
// robust settings, the source, the target, T_init, then what the method reads of the clouds. host null: the clouds are
// handles, valid by construction (their state is the caller's to check). Returns the first refusal, or empty.
inline std::string check_call(Family family, RobustUse use, const Params* p, const Robust* r, bool has_T_out,
                              const double* T_init, const HostClouds* host) {
  if (!has_T_out) return "null T_out";
  const bool gen = family == FAMILY_GENERALIZED || (family == FAMILY_BY_METHOD && p && p->method == clipper_hip::ICP_GENERALIZED);
  std::string why = family == FAMILY_POINT_PLANE ? check_not_generalized(p) : std::string();
  if (why.empty()) why = gen ? check_generalized_params(p) : check_params(p);
  if (why.empty() && (use == ROBUST_REQUIRED || (use == ROBUST_OPTIONAL && r))) why = check_robust(r);
  if (why.empty() && host) why = check_cloud("source", host->P_src, host->n_src);
  if (why.empty() && host) why = check_cloud("target", host->P_tgt, host->n_tgt);
  if (why.empty()) why = check_transform("T_init", T_init);
  if (!why.empty() || !host) return why;
  if (!gen) return check_target_normals(p->method, host->N_tgt, host->n_tgt);
  why = check_covariances("source", host->C_src, host->n_src);
  return why.empty() ? check_covariances("target", host->C_tgt, host->n_tgt) : why;
}

}  // namespace clipper_icp
