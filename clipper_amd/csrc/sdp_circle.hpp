// sdp_circle.hpp — the circle (round-robin) order of the Jacobi pairs of the semidefinite relaxation's eigensolver
// (DESIGN.md section 11), stated once for both routes' kernels (k_sdp.hip.h, k_sdp_wide.hip.h) and for the host, which
// walks it in tests/cpp/test_sdp_wide_plan.cpp. No HIP: builds with g++ as well. SDP_HD (host + device inline) is
// defined here; sdp_rules.hpp, the arithmetic of the iteration, uses it too.
#pragma once

#if defined(__HIPCC__)
#define SDP_HD __host__ __device__ inline
#else
#define SDP_HD inline
#endif

namespace clipper_sdp_circle {

// The pair k of step t of the circle order over np indices (np even): index np - 1 stays put, the others turn. The
// np / 2 pairs of a step partition the indices; over the np - 1 steps every unordered pair occurs once.
SDP_HD void circle_pair(int k, int t, int np, int& p, int& q) {
  const int m = np - 1;
  if (k == 0) {
    p = t;
    q = m;
  } else {
    p = (t + k) % m;
    q = (t - k + m) % m;
  }
}

}  // namespace clipper_sdp_circle
