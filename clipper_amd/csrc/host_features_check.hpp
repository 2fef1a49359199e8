// host_features_check.hpp — normals and FPFH, the part that needs no device: the argument checks of
// clipper_hip_estimate_normals, clipper_hip_compute_fpfh and clipper_hip_fpfh_from_points, and which list length serves
// a neighbourhood (host_knn_k.hpp's rule between 4 and 32). Pure host code (no HIP):
// tests/cpp/test_features_rules.cpp compiles it with g++ alone. A refusal comes back as its message (empty: accepted);
// the caller hands it to fail(). Every check runs before any device work.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "features_rules.hpp"
#include "host_knn_k.hpp"
#include "host_match_select.hpp"

namespace clipper_features {

using clipper_match::format;

// clipper_neighborhood_t, as the checks read it
struct Neighborhood {
  int knn;
  double radius;
};

// `what` names the neighbourhood in the message ("neighbourhood", "normal neighbourhood", "feature neighbourhood")
inline std::string check_neighborhood(const char* what, const Neighborhood* nb) {
  if (!nb) return format("null %s", what);
  if (nb->knn < clipper_hip::FEAT_MIN_KNN || nb->knn > clipper_hip::FEAT_MAX_KNN)
    return format("%s: knn must be in %d..%d (knn = %d)", what, clipper_hip::FEAT_MIN_KNN, clipper_hip::FEAT_MAX_KNN, nb->knn);
  if (!std::isfinite(nb->radius)) return format("%s: radius must be finite (radius = %g)", what, nb->radius);
  return {};
}

inline std::string check_count(int64_t n) {
  if (n < 1) return format("a cloud needs at least one point (n = %lld)", static_cast<long long>(n));
  if (n > INT32_MAX) return "more than 2^31 - 1 points in a cloud";
  return {};
}

// one scan: a NaN or an infinity among the coordinates would order arbitrarily in the search
inline std::string check_points(const double* P, int64_t n) {
  for (int64_t p = 0; p < n; ++p)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(P[p * 3 + k]))
        return format("P: non-finite value at coordinate %d of point %lld", k, static_cast<long long>(p));
  return {};
}

inline std::string check_viewpoint(const double* v) {
  for (int k = 0; v && k < 3; ++k)
    if (!std::isfinite(v[k])) return format("viewpoint: non-finite value at coordinate %d", k);
  return {};
}

// the pair feature divides by nothing that a unit normal could make zero: finite, squared length in [0.99, 1.01]
inline std::string check_normals(const double* N, int64_t n) {
  for (int64_t p = 0; p < n; ++p) {
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(N[p * 3 + k]))
        return format("N: non-finite value at coordinate %d of normal %lld", k, static_cast<long long>(p));
    const double a[3] = {N[p * 3], N[p * 3 + 1], N[p * 3 + 2]};
    const double l2 = clipper_hip::feat_dot(a, a);
    if (!(l2 >= 0.99 && l2 <= 1.01))
      return format("N: normal %lld is not of unit length (squared length = %.17g)", static_cast<long long>(p), l2);
  }
  return {};
}

// the instantiation of the search that serves knn neighbours: the shared rule between the features' 4 and 32
inline int list_k(int knn) { return clipper_hip::knn_list_k(knn, 4, 32); }

}  // namespace clipper_features
