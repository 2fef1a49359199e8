// test_sdp_batch_plan.cpp — the plan of a batched semidefinite relaxation (csrc/host_sdpplan.hpp; host only, g++):
// slab regions disjoint, 8-byte aligned and of the right size, the work list's order, its compaction, the dynamic LDS
// of a launch. Built and run by tests/test_sdp_batch_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "host_sdpplan.hpp"

namespace sp = clipper_sdp_plan;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

static void check_plan(const std::vector<int32_t>& n, bool with_src) {
  const sp::Plan P = sp::make_plan(n, with_src);
  const size_t count = n.size();
  CHECK(P.at.size() == count && P.order.size() == count);
  std::vector<std::pair<size_t, size_t>> regions;  // (begin, bytes)
  for (size_t i = 0; i < count; ++i) {
    const size_t nn = static_cast<size_t>(n[i]) * n[i] * 8, np = static_cast<size_t>(n[i] + (n[i] & 1)), pp = np * np * 8;
    CHECK(sp::padded(n[i]) == static_cast<int32_t>(np) && np % 2 == 0 && np >= static_cast<size_t>(n[i]) && np <= static_cast<size_t>(n[i]) + 1);
    const sp::Regions& r = P.at[i];
    for (auto pr : {std::make_pair(r.M, nn), std::make_pair(r.mask, nn), std::make_pair(r.X, nn), std::make_pair(r.Z, nn),
                    std::make_pair(r.U, nn), std::make_pair(r.Q, pp), std::make_pair(r.T, pp),
                    std::make_pair(r.mu, np * 8), std::make_pair(r.ev, np * 8), std::make_pair(r.nodes, np * 4)})
      regions.push_back(pr);
    if (with_src) {
      regions.push_back({r.srcM, nn});
      regions.push_back({r.srcC, nn});
      CHECK(r.srcM >= P.src_begin && r.srcC + nn <= P.src_begin + P.src_bytes);
    }
    // the small results sit inside the region one copy brings back, the device-only buffers before it
    CHECK(r.mu >= P.out_begin && r.ev >= P.out_begin && r.nodes >= P.out_begin);
    CHECK(r.nodes + np * 4 <= P.out_begin + P.out_bytes);
    CHECK(r.T + pp <= P.src_begin && P.src_begin + P.src_bytes == P.out_begin);
  }
  if (!with_src) CHECK(P.src_bytes == 0);
  CHECK(P.out_begin + P.out_bytes == P.bytes);
  size_t total = 0;
  for (const auto& r : regions) {
    CHECK(r.first % 8 == 0 && r.second % 8 == 0);
    CHECK(r.first + r.second <= P.bytes);
    total += r.second;
  }
  CHECK(total == P.bytes);  // no gaps: with disjointness below, the regions tile the slab
  std::sort(regions.begin(), regions.end());
  for (size_t k = 1; k < regions.size(); ++k) CHECK(regions[k - 1].first + regions[k - 1].second <= regions[k].first);
  // the work list: a permutation, n descending, ties by index
  std::vector<int32_t> seen(P.order);
  std::sort(seen.begin(), seen.end());
  for (size_t i = 0; i < count; ++i) CHECK(seen[i] == static_cast<int32_t>(i));
  for (size_t k = 1; k < count; ++k) {
    const int32_t a = P.order[k - 1], b = P.order[k];
    CHECK(n[a] > n[b] || (n[a] == n[b] && a < b));
  }
}

int main() {
  std::mt19937 rng(20240607);
  for (int trial = 0; trial < 60; ++trial) {
    const int count = trial == 0 ? 1 : (trial == 1 ? 1000 : 1 + static_cast<int>(rng() % 1000));
    std::vector<int32_t> n(static_cast<size_t>(count));
    for (auto& v : n) v = 1 + static_cast<int32_t>(rng() % 128);
    if (trial == 2) std::fill(n.begin(), n.end(), 128);
    if (trial == 3) std::fill(n.begin(), n.end(), 1);
    check_plan(n, true);
    check_plan(n, false);

    // compaction: rounds of random finishes keep exactly the unfinished problems, in their order
    const sp::Plan P = sp::make_plan(n, false);
    std::vector<char> done(n.size(), 0);
    std::vector<int32_t> list = P.order;
    CHECK(sp::launch_lds_bytes(list, n) == static_cast<size_t>(sp::padded(n[list[0]])) * sp::padded(n[list[0]]) * 8);
    while (!list.empty()) {
      for (int32_t i : list)
        if (rng() % 3 == 0) done[static_cast<size_t>(i)] = 1;
      std::vector<int32_t> expect;
      for (int32_t i : list)
        if (!done[static_cast<size_t>(i)]) expect.push_back(i);
      const std::vector<int32_t> next = sp::compact(list, [&](int32_t i) { return done[static_cast<size_t>(i)] != 0; });
      CHECK(next == expect);
      for (size_t k = 1; k < next.size(); ++k) CHECK(n[next[k - 1]] >= n[next[k]]);
      // the LDS of a launch: its largest active problem
      int32_t big = 0;
      for (int32_t i : next) big = std::max(big, n[i]);
      const size_t np = static_cast<size_t>(big + (big & 1));
      CHECK(sp::launch_lds_bytes(next, n) == np * np * 8);
      CHECK(sp::launch_lds_bytes(next, n) <= 128 * 128 * 8);
      list = next;
    }
    CHECK(sp::launch_lds_bytes(list, n) == 0);
  }
  // an unordered list: the figure is still the maximum
  const std::vector<int32_t> n = {3, 128, 64, 7};
  CHECK(sp::launch_lds_bytes({0, 3}, n) == 8 * 8 * 8);
  CHECK(sp::launch_lds_bytes({0, 2, 3}, n) == 64 * 64 * 8);
  CHECK(sp::launch_lds_bytes({3, 1}, n) == 128 * 128 * 8);
  const sp::Plan P = sp::make_plan(n, true);
  CHECK((P.order == std::vector<int32_t>{1, 2, 3, 0}));
  CHECK((sp::make_plan({5, 9, 5, 9}, false).order == std::vector<int32_t>{1, 3, 0, 2}));
  std::printf("sdp batch plan ok\n");
  return 0;
}
