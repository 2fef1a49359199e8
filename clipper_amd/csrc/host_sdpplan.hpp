// host_sdpplan.hpp — the plan of a batched semidefinite relaxation (host_sdpbatch.hpp): where every
// problem's buffers sit in the call's one device slab, the order of the work list, its compaction between rounds and
// the dynamic LDS of a launch.
// Host-only (no HIP): tests/cpp/test_sdp_batch_plan.cpp builds it with g++.
//
// Slab layout, all offsets in bytes and multiples of 8: first the regions only the device works on, problem after
// problem (M, mask, X, Z, U: n x n doubles; Q, T: np x np doubles, np = n rounded up to even), then, when the call
// uploads host matrices, their staging (srcM, srcC: n x n doubles, the device copy of one host buffer laid out the
// same way from `src_begin` on), then the small results the host reads back in ONE copy (`out_begin`, `out_bytes`):
// every problem's mu (np doubles), evec1 (np doubles) and node list (np int32, np is even: a multiple of 8 bytes).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace clipper_sdp_plan {

struct Regions {  // byte offsets into the slab
  size_t M, mask, X, Z, U, Q, T, srcM, srcC, mu, ev, nodes;
};

struct Plan {
  std::vector<Regions> at;     // per problem, in the caller's order
  std::vector<int32_t> order;  // the work list: n descending (the long problems start first), ties by index
  size_t bytes = 0;            // the whole slab
  size_t src_begin = 0, src_bytes = 0;  // the uploaded matrices (src_bytes = 0 without them)
  size_t out_begin = 0, out_bytes = 0;  // what one D2H copy brings back
};

inline int32_t padded(int32_t n) { return n + (n & 1); }

inline Plan make_plan(const std::vector<int32_t>& n, bool with_src) {
  Plan P;
  const size_t count = n.size();
  P.at.resize(count);
  size_t o = 0;
  auto take = [&o](size_t doubles) {
    const size_t at = o;
    o += doubles * sizeof(double);
    return at;
  };
  for (size_t i = 0; i < count; ++i) {
    const size_t nn = static_cast<size_t>(n[i]) * n[i], np = padded(n[i]), pp = np * np;
    Regions& r = P.at[i];
    r.M = take(nn);
    r.mask = take(nn);
    r.X = take(nn);
    r.Z = take(nn);
    r.U = take(nn);
    r.Q = take(pp);
    r.T = take(pp);
  }
  P.src_begin = o;
  for (size_t i = 0; i < count; ++i) {
    const size_t nn = with_src ? static_cast<size_t>(n[i]) * n[i] : 0;
    P.at[i].srcM = take(nn);
    P.at[i].srcC = take(nn);
  }
  P.src_bytes = o - P.src_begin;
  P.out_begin = o;
  for (size_t i = 0; i < count; ++i) {
    const size_t np = padded(n[i]);
    P.at[i].mu = take(np);
    P.at[i].ev = take(np);
    P.at[i].nodes = take(np / 2);  // np int32
  }
  P.out_bytes = o - P.out_begin;
  P.bytes = o;
  P.order.resize(count);
  std::iota(P.order.begin(), P.order.end(), 0);
  std::stable_sort(P.order.begin(), P.order.end(), [&](int32_t a, int32_t b) { return n[a] > n[b]; });
  return P;
}

// The problems of `list` that are not finished, in the order they had. finished(i): problem i needs no more launches.
template <class Finished>
inline std::vector<int32_t> compact(const std::vector<int32_t>& list, Finished&& finished) {
  std::vector<int32_t> out;
  out.reserve(list.size());
  for (int32_t i : list)
    if (!finished(i)) out.push_back(i);
  return out;
}

// Dynamic LDS of a launch over `list`: the working matrix of its largest problem (0 for an empty list).
inline size_t launch_lds_bytes(const std::vector<int32_t>& list, const std::vector<int32_t>& n) {
  size_t np = 0;
  for (int32_t i : list) np = std::max<size_t>(np, padded(n[i]));
  return np * np * sizeof(double);
}

}  // namespace clipper_sdp_plan
