// host_ransac_check.hpp — RANSAC over putative associations, the part that needs no device: the argument checks of
// clipper_hip_ransac_correspondences. Pure host code (no HIP): tests/cpp/test_ransac_rules.cpp compiles it with g++
// alone. A refusal comes back as its message (empty: accepted) and names the offending value; the caller hands it to
// fail(). Every check runs before any device work.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "host_icp_check.hpp"
#include "ransac_rules.hpp"

namespace clipper_ransac {

using clipper_match::format;

// clipper_ransac_params_t, as the checks read it
struct Params {
  double max_distance, edge_similarity, confidence;
  int64_t max_hypotheses;
  int32_t hypotheses_per_round, n_sample, refine_iterations, reserved;
};

inline std::string check_params(const Params* p) {
  namespace ch = clipper_hip;
  if (!p) return "null params";
  std::string why = clipper_icp::check_max_distance(p->max_distance);
  if (!why.empty()) return why;
  if (!(p->edge_similarity >= 0.0 && p->edge_similarity < 1.0))
    return format("edge_similarity must be in [0, 1) (edge_similarity = %g)", p->edge_similarity);
  if (!(p->confidence > 0.0 && p->confidence < 1.0)) return format("confidence must be in (0, 1) (confidence = %g)", p->confidence);
  if (p->max_hypotheses < 1 || p->max_hypotheses > INT32_MAX)
    return format("max_hypotheses must be in 1..2^31 - 1 (max_hypotheses = %lld)", static_cast<long long>(p->max_hypotheses));
  if (p->hypotheses_per_round < ch::RANSAC_ROUND_UNIT || p->hypotheses_per_round > ch::RANSAC_MAX_ROUND ||
      p->hypotheses_per_round % ch::RANSAC_ROUND_UNIT != 0)
    return format("hypotheses_per_round must be a multiple of %d in %d..%d (hypotheses_per_round = %d)", ch::RANSAC_ROUND_UNIT,
                  ch::RANSAC_ROUND_UNIT, ch::RANSAC_MAX_ROUND, p->hypotheses_per_round);
  if (p->n_sample < ch::RANSAC_MIN_SAMPLE || p->n_sample > ch::RANSAC_MAX_SAMPLE)
    return format("n_sample must be in %d..%d (n_sample = %d)", ch::RANSAC_MIN_SAMPLE, ch::RANSAC_MAX_SAMPLE, p->n_sample);
  if (p->refine_iterations < 0 || p->refine_iterations > ch::RANSAC_MAX_REFINE)
    return format("refine_iterations must be in 0..%d (refine_iterations = %d)", ch::RANSAC_MAX_REFINE, p->refine_iterations);
  if (p->reserved != 0) return format("reserved must be 0 (reserved = %d)", p->reserved);
  return {};
}

// `what`: "D1", "D2". The coordinates are checked where an association refers to them (check_associations).
inline std::string check_cloud_size(const char* what, const double* D, int64_t n) {
  if (!D) return format("null %s point array", what);
  if (n < 1) return format("%s: a cloud needs at least one point (n = %lld)", what, static_cast<long long>(n));
  if (n > INT32_MAX) return format("%s: more than 2^31 - 1 points in a cloud (n = %lld)", what, static_cast<long long>(n));
  return {};
}

// A: m x 2 column-major. Every row within the clouds, every referenced point finite. lo, hi (3 each, may be null):
// the exact bounding box of the m gathered points of D2, the box whose centre the polish takes its sums about.
inline std::string check_associations(const double* D1, int64_t n1, const double* D2, int64_t n2, const int32_t* A, int64_t m,
                                      int n_sample, double* lo, double* hi) {
  if (!A) return "null association array";
  if (m < n_sample)
    return format("fewer associations than a sample holds (m = %lld, n_sample = %d)", static_cast<long long>(m), n_sample);
  if (m > INT32_MAX) return format("more than 2^31 - 1 associations (m = %lld)", static_cast<long long>(m));
  for (int64_t k = 0; k < m; ++k) {
    const int32_t a = A[k], b = A[m + k];
    if (a < 0 || a >= n1 || b < 0 || b >= n2)
      return format("association row %lld out of range (%d, %d)", static_cast<long long>(k), a, b);
    for (int c = 0; c < 3; ++c) {
      if (!std::isfinite(D1[static_cast<int64_t>(a) * 3 + c]))
        return format("D1: non-finite value at coordinate %d of point %d (association row %lld)", c, a, static_cast<long long>(k));
      const double x = D2[static_cast<int64_t>(b) * 3 + c];
      if (!std::isfinite(x))
        return format("D2: non-finite value at coordinate %d of point %d (association row %lld)", c, b, static_cast<long long>(k));
      if (lo) lo[c] = (k == 0 || x < lo[c]) ? x : lo[c];
      if (hi) hi[c] = (k == 0 || x > hi[c]) ? x : hi[c];
    }
  }
  return {};
}

}  // namespace clipper_ransac
