// host_voxel_check.hpp — voxel down-sampling, the part that needs no device: the argument checks of
// clipper_hip_voxel_downsample and the plan of its grid. The scan that proves every coordinate finite reads every
// coordinate, so it yields the cloud's corners lo and hi as well: the call needs no bounds kernel and no host wait in
// its middle. Pure host code (no HIP): tests/cpp/test_voxel_rules.cpp compiles it with g++ alone. A refusal comes back
// as its message (empty: accepted), in the words of host_features_check.hpp; the caller hands it to fail().
#pragma once

#include <cmath>
#include <cstdint>
#include <string>

#include "host_features_check.hpp"
#include "voxel_rules.hpp"

namespace clipper_voxel {

using clipper_match::format;

struct Plan {
  clipper_hip::VoxelGrid g;
  int passes;
};

inline std::string check_count(int64_t n) {
  if (n < 0) return format("a cloud cannot hold a negative number of points (n = %lld)", static_cast<long long>(n));
  if (n > INT32_MAX) return "more than 2^31 - 1 points in a cloud";
  return {};
}

inline std::string check_voxel_size(double voxel_size) {
  if (!(std::isfinite(voxel_size) && voxel_size > 0.0))
    return format("voxel_size must be finite and greater than 0 (voxel_size = %g)", voxel_size);
  return {};
}

// one scan: every coordinate finite, and the corners of the cloud (min and max are exact: the order does not matter)
inline std::string check_points_bounds(const double* P, int64_t n, double (&lo)[3], double (&hi)[3]) {
  for (int k = 0; k < 3; ++k) {
    lo[k] = INFINITY;
    hi[k] = -INFINITY;
  }
  for (int64_t p = 0; p < n; ++p)
    for (int k = 0; k < 3; ++k) {
      const double v = P[p * 3 + k];
      if (!std::isfinite(v)) return format("P: non-finite value at coordinate %d of point %lld", k, static_cast<long long>(p));
      lo[k] = v < lo[k] ? v : lo[k];
      hi[k] = v > hi[k] ? v : hi[k];
    }
  return {};
}

// the normals are summed and the sum is normalised: finite is all they have to be
inline std::string check_normals_finite(const double* N, int64_t n) {
  for (int64_t p = 0; p < n; ++p)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(N[p * 3 + k]))
        return format("N: non-finite value at coordinate %d of normal %lld", k, static_cast<long long>(p));
  return {};
}

// rule 2's limit, and with it the grid and the number of sort passes
inline std::string plan(const double (&lo)[3], const double (&hi)[3], double voxel_size, Plan& out) {
  int axis = 0;
  if (!clipper_hip::voxel_plan(lo, hi, voxel_size, out.g, axis))
    return format("voxel_size = %g gives more than 2^21 voxels along axis %d (extent %g)", voxel_size, axis, hi[axis] - lo[axis]);
  out.passes = clipper_hip::sort_passes(clipper_hip::voxel_cells(out.g));
  return {};
}

// every check of the call in its order; n == 0 is accepted (the plan is then left at one cell)
inline std::string check_all(const double* P, const double* N, int64_t n, double voxel_size, const void* n_out,
                             const void* N_out, Plan& out) {
  if (!n_out) return "null n_out";
  std::string why = check_count(n);
  if (why.empty() && n > 0 && !P) why = "null point array";
  if (why.empty() && N_out && !N) why = "a normal output array needs the normals N";
  if (why.empty()) why = check_voxel_size(voxel_size);
  if (!why.empty()) return why;
  double lo[3], hi[3];
  why = check_points_bounds(P, n, lo, hi);
  if (why.empty() && N) why = check_normals_finite(N, n);
  if (!why.empty()) return why;
  if (n == 0) {
    out.g = clipper_hip::VoxelGrid{{0.0, 0.0, 0.0}, 1.0 / voxel_size, {1, 1, 1}};
    out.passes = 0;
    return {};
  }
  return plan(lo, hi, voxel_size, out);
}

}  // namespace clipper_voxel
