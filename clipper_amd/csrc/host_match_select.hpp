// host_match_select.hpp — descriptor matching, the part that needs no device: the argument checks of
// clipper_hip_match_descriptors, the zero padding of the descriptor rows and the filters that turn the nearest-neighbour
// lists of the search kernels (k_match.hip.h) into associations. Pure host code (no HIP): tests/cpp/test_match_select.cpp
// compiles it with g++ alone. A refusal comes back as its message (empty: accepted); the caller hands it to fail().
//
// With nn_k(i) / sqd_k(i) the forward list of query i and bn(j) the backward list of point j, row (i, nn_k(i)), k < knn,
// is kept iff ALL of
//   nn_k(i) >= 0                                                      (the other set has that many points)
//   max_sqdist <= 0  or  sqd_k(i) <= max_sqdist
//   ratio <= 0  or  nn_1(i) < 0  or  sqd_0(i) < (ratio * ratio) * sqd_1(i)   (Lowe's test on squared distances, strict,
//                                                                      in fp64 as written; knn == 1, forward lists of 2)
//   mutual == 0  or  i is among bn(nn_k(i))[0 .. knn)
// Rows come out with i ascending, then k ascending.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "match_rules.hpp"

namespace clipper_match {

constexpr int MAX_D = 64;    // coordinates per descriptor
constexpr int MAX_KNN = 8;   // neighbours per point

// nearest-neighbour lists of n queries, row-major n x stride
struct Lists {
  const int32_t* idx;
  const double* sqd;
  int64_t n;
  int stride;
};

// the associations kept, in order: (i[r], j[r]) at squared distance sqd[r]
struct Rows {
  std::vector<int32_t> i, j;
  std::vector<double> sqd;
};

template <typename... Args>
std::string format(const char* fmt, Args... args) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), fmt, args...);
  return buf;
}

// everything about the arguments that can be said without looking at the descriptors
inline std::string check_args(const double* F0, int64_t n0, const double* F1, int64_t n1, int d, const Params* prm) {
  if (!F0 || !F1) return "null descriptor array";
  if (!prm) return "null match parameters";
  if (n0 < 1 || n1 < 1)
    return format("both descriptor sets need at least one point (n0 = %lld, n1 = %lld)", static_cast<long long>(n0),
                  static_cast<long long>(n1));
  if (n0 > INT32_MAX || n1 > INT32_MAX) return "more than 2^31 - 1 points in a descriptor set";
  if (d < 1 || d > MAX_D) return format("descriptors must have 1..%d coordinates (d = %d)", MAX_D, d);
  if (prm->knn < 1 || prm->knn > MAX_KNN) return format("knn must be in 1..%d (knn = %d)", MAX_KNN, prm->knn);
  if (!(prm->ratio >= 0.0) || !(prm->ratio < 1.0)) return format("ratio must be 0 (off) or in (0, 1) (ratio = %g)", prm->ratio);
  if (prm->ratio > 0.0 && prm->knn != 1) return format("the ratio test needs knn == 1 (knn = %d)", prm->knn);
  if (std::isnan(prm->max_sqdist)) return "max_sqdist is not a number";
  return {};
}

// one scan: a NaN or an infinity in a descriptor would order arbitrarily in the search
inline std::string check_finite(const char* what, const double* F, int64_t n, int d) {
  for (int64_t p = 0; p < n; ++p)
    for (int k = 0; k < d; ++k)
      if (!std::isfinite(F[p * d + k]))
        return format("%s: non-finite value at coordinate %d of descriptor %lld", what, k, static_cast<long long>(p));
  return {};
}

// the rows padded with zeros to the row length dp the kernels see ((0 - 0)^2 adds nothing to a distance)
inline std::vector<double> pad_rows(const double* F, int64_t n, int d, int dp) {
  std::vector<double> out(static_cast<size_t>(n) * dp, 0.0);
  for (int64_t p = 0; p < n; ++p)
    for (int k = 0; k < d; ++k) out[static_cast<size_t>(p) * dp + k] = F[p * d + k];
  return out;
}

// how long the forward lists must be: the ratio test reads the second neighbour
inline int forward_len(const Params& prm) { return prm.ratio > 0.0 ? 2 : prm.knn; }

// the filters (see the head of this file; the per-query and per-entry rules are match_rules.hpp's, which the device's
// k_match_select shares). fwd: forward_len(prm) entries per query; bwd: knn entries per point of the other set, read
// only when prm.mutual is set.
inline Rows select(const Params& prm, const Lists& fwd, const Lists& bwd) {
  Rows out;
  for (int64_t i = 0; i < fwd.n; ++i) {
    const int32_t* nn = fwd.idx + i * fwd.stride;
    const double* sd = fwd.sqd + i * fwd.stride;
    if (!query_passes(prm, nn, sd)) continue;
    for (int k = 0; k < prm.knn; ++k) {
      if (!entry_kept(prm, i, k, nn, sd, bwd.idx, bwd.stride)) continue;
      out.i.push_back(static_cast<int32_t>(i));
      out.j.push_back(nn[k]);
      out.sqd.push_back(sd[k]);
    }
  }
  return out;
}

// the rows to the caller: A_out column-major n x 2 as clipper::Association, sqd_out (may be null) one per row
inline std::string emit(const Rows& rows, int32_t* A_out, double* sqd_out, int64_t capacity) {
  const int64_t n = static_cast<int64_t>(rows.i.size());
  if (n > capacity || capacity < 0)
    return format("capacity %lld < %lld associations", static_cast<long long>(capacity), static_cast<long long>(n));
  if (n > 0 && !A_out) return "null association buffer";
  for (int64_t r = 0; r < n; ++r) {
    A_out[r] = rows.i[static_cast<size_t>(r)];
    A_out[n + r] = rows.j[static_cast<size_t>(r)];
    if (sqd_out) sqd_out[r] = rows.sqd[static_cast<size_t>(r)];
  }
  return {};
}

}  // namespace clipper_match
