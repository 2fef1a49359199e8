// match_rules.hpp — the filters of descriptor matching, stated once for the host (clipper_match::select,
// host_match_select.hpp) and the device (k_match_select, k_match.hip.h): whether a query passes Lowe's ratio test and
// whether one entry of its forward list is kept (the rules in words: the head of host_match_select.hpp). Plain
// sequential functions of one query / one entry: which work item holds what belongs to the callers. Every comparison is
// in fp64 as written (nothing here can fuse: a product is compared, never added to), so both sides keep the same rows.
// No HIP: builds with g++ as well (tests/cpp/test_match_rules.cpp drives it with a plain loop).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MATCH_HD __host__ __device__ inline
#else
#define MATCH_HD inline
#endif

namespace clipper_match {

// clipper_match_params_t, as the filters read it
struct Params {
  int knn;
  int mutual;
  double ratio;
  double max_sqdist;
};

// Lowe's test on squared distances, strict, for the whole query: nn / sd are its forward list, of at least 2 entries
// when prm.ratio > 0 (not read otherwise). A query without a second neighbour (the other set has one point) passes.
MATCH_HD bool query_passes(const Params& prm, const int32_t* nn, const double* sd) {
  if (!(prm.ratio > 0.0)) return true;
  const double r2 = prm.ratio * prm.ratio;
  return nn[1] < 0 || sd[0] < r2 * sd[1];
}

// entry k (< prm.knn) of the forward list nn / sd of query i, once the query has passed: the neighbour exists, lies
// within the bound, and (prm.mutual) has i among the first prm.knn entries of its backward list. bwd_idx: the backward
// lists, row-major with bwd_stride entries per point of the other set; read only when prm.mutual is set.
MATCH_HD bool entry_kept(const Params& prm, int64_t i, int k, const int32_t* nn, const double* sd, const int32_t* bwd_idx,
                         int bwd_stride) {
  const int32_t j = nn[k];
  if (j < 0) return false;
  if (prm.max_sqdist > 0.0 && !(sd[k] <= prm.max_sqdist)) return false;
  if (prm.mutual) {
    const int32_t* bn = bwd_idx + static_cast<int64_t>(j) * bwd_stride;
    bool found = false;
    for (int c = 0; c < prm.knn && !found; ++c) found = (bn[c] == static_cast<int32_t>(i));
    if (!found) return false;
  }
  return true;
}

}  // namespace clipper_match
