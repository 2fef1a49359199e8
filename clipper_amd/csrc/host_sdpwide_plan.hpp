// host_sdpwide_plan.hpp — the plan of the wide route of the semidefinite relaxation (host_sdpwide.hpp, kernels in
// k_sdp_wide.hip.h, DESIGN.md 11 "The wide route"): the geometry of the launch
// that runs one Jacobi step over the whole chip (the pairs' circle order is sdp_circle.hpp's), where one problem's buffers sit in its slab, and the split of a batch
// into the problems of the workgroup route and those of the wide route.
// No HIP: tests/cpp/test_sdp_wide_plan.cpp builds it with g++. The kernels include it too and take their indices from
// the functions marked SDPW_HD, so the geometry the test walks is the one the device runs. Everything here is a
// function of n alone, never of the device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "sdp_circle.hpp"

#define SDPW_HD SDP_HD

namespace clipper_sdpw_plan {

constexpr int32_t WORKGROUP_MAX_N = 128;  // the workgroup route's limit (CLIPPER_HIP_SDP_MAX_N)
constexpr int32_t WIDE_MAX_N = 1024;      // the wide route's (CLIPPER_HIP_SDP_WIDE_MAX_N)
enum { ROUTE_WORKGROUP = 0, ROUTE_AUTO = 1, ROUTE_WIDE = 2 };

constexpr int32_t TILE = 16;                    // a workgroup of the step launch: TILE x TILE work items
constexpr int32_t STEP_THREADS = TILE * TILE;
constexpr int32_t UPDATE_TILE = 16;             // the update launch: one workgroup per 16 x 16 entries of X
constexpr size_t STATE_BYTES = 256;             // the control record and the driver's flags (host_sdpwide.hpp)

SDPW_HD int32_t padded(int32_t n) { return n + (n & 1); }

using clipper_sdp_circle::circle_pair;  // the order of the Jacobi pairs (sdp_circle.hpp)

// ---- one Jacobi step as one launch ----------------------------------------------------------------------------------
// h = np / 2 pairs, ht = ceil(h / TILE) tiles of pairs. Workgroups [0, a_tiles) rotate the working matrix: workgroup
// (kt, lt), kt <= lt, work item (i, j) owns the 2 x 2 block (pair kt * TILE + i, pair lt * TILE + j) and its transpose.
// Workgroups [a_tiles, a_tiles + q_tiles) rotate the eigenbasis: workgroup (rt, kt), work item (i, j) owns
// (row rt * TILE + i, pair kt * TILE + j). A launch that does not accumulate Q has a_tiles workgroups.
struct StepGeom {
  int32_t np, h, ht, a_tiles, q_row_tiles, q_tiles;
};

SDPW_HD StepGeom step_geom(int32_t np) {
  StepGeom g;
  g.np = np;
  g.h = np / 2;
  g.ht = (g.h + TILE - 1) / TILE;
  g.a_tiles = g.ht * (g.ht + 1) / 2;
  g.q_row_tiles = (np + TILE - 1) / TILE;
  g.q_tiles = g.q_row_tiles * g.ht;
  return g;
}

// tile `idx` of the upper triangle of ht x ht tiles, row after row
SDPW_HD void a_tile(const StepGeom& g, int32_t idx, int32_t& kt, int32_t& lt) {
  kt = 0;
  while (idx >= g.ht - kt) {
    idx -= g.ht - kt;
    ++kt;
  }
  lt = kt + idx;
}

// the block of work item `tid` of A-workgroup `wg`; false: the item has none
SDPW_HD bool a_item(const StepGeom& g, int32_t wg, int32_t tid, int32_t& k, int32_t& l) {
  int32_t kt, lt;
  a_tile(g, wg, kt, lt);
  k = kt * TILE + tid / TILE;
  l = lt * TILE + tid % TILE;
  return k < g.h && l < g.h && k <= l;
}

// (row, pair) of work item `tid` of Q-workgroup `wg` (counted from 0); false: the item has none
SDPW_HD bool q_item(const StepGeom& g, int32_t wg, int32_t tid, int32_t& row, int32_t& k) {
  row = (wg / g.ht) * TILE + tid / TILE;
  k = (wg % g.ht) * TILE + tid % TILE;
  return row < g.np && k < g.h;
}

// workgroups of the update launch, = the partial sums of each of the stopping rule's six sums
SDPW_HD int32_t update_tiles(int32_t n) {
  const int32_t s = (n + UPDATE_TILE - 1) / UPDATE_TILE;
  return s * s;
}

// ---- the slab of one problem ----------------------------------------------------------------------------------------
// Byte offsets, all multiples of 8. First what a problem keeps (the regions a batch holds per problem in its own
// slab: M, mask, X, Z, U n x n doubles; Q[0], T np x np; mu np), then from `work_begin` on what only the driver needs
// while it runs (Q[1], A[0], A[1] np x np: the second copy of the eigenbasis and the working matrix twice; the
// partial sums; the positive eigenvalues' list; the state), which the wide problems of a batch share in turn.
struct Regions {
  size_t M, mask, X, Z, U, Q[2], T, mu, A[2], part, pos, state;
  size_t work_begin, bytes;
};

inline Regions make_regions(int32_t n) {
  Regions r{};
  const size_t nn = static_cast<size_t>(n) * n, np = static_cast<size_t>(padded(n)), pp = np * np;
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += bytes;
    return at;
  };
  r.M = take(8 * nn);
  r.mask = take(8 * nn);
  r.X = take(8 * nn);
  r.Z = take(8 * nn);
  r.U = take(8 * nn);
  r.Q[0] = take(8 * pp);
  r.T = take(8 * pp);
  r.mu = take(8 * np);
  r.work_begin = o;
  r.Q[1] = take(8 * pp);
  r.A[0] = take(8 * pp);
  r.A[1] = take(8 * pp);
  r.part = take(8 * 6 * static_cast<size_t>(update_tiles(n)));
  r.pos = take(4 * np);  // np int32, np even
  r.state = take(STATE_BYTES);
  r.bytes = o;
  return r;
}

// (offset, bytes) of every region, in slab order
inline std::vector<std::pair<size_t, size_t>> spans(int32_t n) {
  const Regions r = make_regions(n);
  const size_t at[] = {r.M, r.mask, r.X, r.Z, r.U, r.Q[0], r.T, r.mu, r.Q[1], r.A[0], r.A[1], r.part, r.pos, r.state};
  std::vector<std::pair<size_t, size_t>> s;
  for (size_t i = 0; i < sizeof(at) / sizeof(at[0]); ++i)
    s.emplace_back(at[i], (i + 1 < sizeof(at) / sizeof(at[0]) ? at[i + 1] : r.bytes) - at[i]);
  return s;
}

// ---- routes -----------------------------------------------------------------------------------------------------------
inline int32_t route_limit(int route) { return route == ROUTE_WORKGROUP ? WORKGROUP_MAX_N : WIDE_MAX_N; }

// the route a problem of n takes under a setting (n within route_limit): ROUTE_WORKGROUP or ROUTE_WIDE
inline int route_of(int route, int64_t n) {
  if (route == ROUTE_WIDE) return ROUTE_WIDE;
  return (route == ROUTE_AUTO && n > WORKGROUP_MAX_N) ? ROUTE_WIDE : ROUTE_WORKGROUP;
}

struct Split {
  std::vector<int32_t> workgroup, wide;  // problem indices, each in the caller's order
};

inline Split split(const std::vector<int32_t>& n, int route) {
  Split s;
  for (size_t i = 0; i < n.size(); ++i)
    (route_of(route, n[i]) == ROUTE_WIDE ? s.wide : s.workgroup).push_back(static_cast<int32_t>(i));
  return s;
}

}  // namespace clipper_sdpw_plan
