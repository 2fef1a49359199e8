// test_mc_batch_plan.cpp — the plan of a batched maximum-clique call (csrc/host_mcplan.hpp; host only, g++): slab regions
// disjoint, 8-byte aligned and inside the slab, the slots dealt, the launch tables' rows, the compaction, the two vertex
// orders. Built and run by tests/test_batch_maxclique_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "host_mcplan.hpp"

namespace mp = clipper_mc_plan;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)

constexpr size_t PROB = 136, CTL = 64, SLOT = 24, SRC = 112;  // stand-ins for the kernels' struct sizes (multiples of 8)

static void check_plan(const std::vector<mp::Size>& sz, int64_t cap, size_t room) {
  const mp::Plan P = mp::make_plan(sz, cap, room, PROB, CTL, SLOT, SRC);
  const size_t count = sz.size();
  CHECK(P.at.size() == count);
  std::vector<std::pair<size_t, size_t>> regions;  // (begin, bytes)
  regions.push_back({P.probs, count * PROB});
  regions.push_back({P.src, count * SRC});
  regions.push_back({P.ctl, count * CTL});
  int64_t total = 0;
  size_t nsl = 0, nrow = 0, arena = 0;
  int64_t nwmax = 0;
  for (size_t i = 0; i < count; ++i) {
    const mp::Regions& r = P.at[i];
    const size_t m = static_cast<size_t>(sz[i].m), nw = (m + 63) / 64, mpad = m + (m & 1), ns = static_cast<size_t>(r.nslots);
    CHECK(r.nw == static_cast<int64_t>(nw) && r.mp == static_cast<int32_t>(mpad));
    CHECK(r.nslots >= 1 && r.nslots <= sz[i].m);  // at least one slot per problem, never more than seeds
    total += r.nslots;
    nsl += static_cast<size_t>(sz[i].nslices);
    nrow += m;
    nwmax = std::max<int64_t>(nwmax, r.nw);
    arena += ns * m * nw * 8;
    for (auto pr : {std::make_pair(r.G, m * nw * 8), std::make_pair(r.alive, nw * 8), std::make_pair(r.degw, mpad * 4),
                    std::make_pair(r.arena, ns * m * nw * 8), std::make_pair(r.paths, ns * (m + 1) * 4),
                    std::make_pair(r.recs, ns * (m + 1) * 4), std::make_pair(r.list, mpad * 4),
                    std::make_pair(r.pos, mpad * 4), std::make_pair(r.slots, ns * SLOT), std::make_pair(r.out, (m + 2) * 4),
                    std::make_pair(r.deg, mpad * 4), std::make_pair(r.core, mpad * 4)})
      regions.push_back(pr);
    // what the host reads or writes lies behind host_begin, what one copy moves inside its range
    CHECK(r.G < P.host_begin && r.arena < P.host_begin && r.recs < P.host_begin);
    CHECK(r.list >= P.up_begin && r.slots + ns * SLOT <= P.up_end && r.pos >= P.up_begin);
    CHECK(r.out >= P.out_begin && r.out + (m + 2) * 4 <= P.out_begin + P.out_bytes + 8);
    CHECK(r.deg >= P.deg_begin && r.deg < P.core_begin && r.core >= P.core_begin);
    CHECK(r.G >= P.G_begin && r.G + m * nw * 8 <= P.G_begin + P.G_bytes);
    CHECK(r.alive >= P.alive_begin && r.alive + nw * 8 <= P.alive_begin + P.alive_bytes);
    // deg and degw are laid out alike: one device copy moves all of them
    CHECK(r.deg - P.deg_begin == r.degw - P.degw_begin);
  }
  CHECK(P.core_begin - P.deg_begin == P.deg_bytes);
  CHECK(P.total_slots == total && P.nslice_rows == nsl && P.nrow_rows == nrow && P.nw_max == nwmax);
  CHECK(total <= std::max<int64_t>(cap, static_cast<int64_t>(count)));  // the cap, or one slot each
  CHECK(arena <= room || total == static_cast<int64_t>(count) || cap <= static_cast<int64_t>(count));
  regions.push_back({P.slice_tab, nsl * sizeof(mp::Item)});
  regions.push_back({P.row_tab, nrow * sizeof(mp::Item)});
  regions.push_back({P.work, count * 4});
  regions.push_back({P.slot_tab, static_cast<size_t>(total) * sizeof(mp::Item)});
  CHECK(P.probs >= P.up_begin && P.ctl + count * CTL <= P.up_end && P.up_begin == P.host_begin);
  CHECK(P.slice_tab >= P.up_end && P.row_tab + nrow * sizeof(mp::Item) <= P.adj_end && P.work >= P.adj_end);
  for (const auto& r : regions) {
    CHECK(r.first % 8 == 0);
    CHECK(r.first + r.second <= P.bytes);
  }
  std::sort(regions.begin(), regions.end());
  for (size_t k = 1; k < regions.size(); ++k) CHECK(regions[k - 1].first + regions[k - 1].second <= regions[k].first);

  // the tables: every (problem, slice) and (problem, row) once
  std::vector<mp::Item> srows(nsl), rrows(nrow);
  mp::adjacency_rows(sz, srows.data(), rrows.data());
  std::set<std::pair<int32_t, int32_t>> seen;
  for (const mp::Item& it : srows) {
    CHECK(it.prob >= 0 && static_cast<size_t>(it.prob) < count && it.idx >= 0 && it.idx < sz[static_cast<size_t>(it.prob)].nslices);
    CHECK(seen.insert({it.prob, it.idx}).second);
  }
  CHECK(seen.size() == nsl);
  seen.clear();
  for (const mp::Item& it : rrows) {
    CHECK(it.prob >= 0 && static_cast<size_t>(it.prob) < count && it.idx >= 0 && it.idx < sz[static_cast<size_t>(it.prob)].m);
    CHECK(seen.insert({it.prob, it.idx}).second);
  }
  CHECK(seen.size() == nrow);
  for (size_t k = 1; k < rrows.size(); ++k)  // problem after problem, rows ascending (adjacent threads, adjacent columns)
    CHECK(rrows[k - 1].prob < rrows[k].prob || (rrows[k - 1].prob == rrows[k].prob && rrows[k - 1].idx + 1 == rrows[k].idx));
}

int main() {
  std::mt19937 rng(20240917);
  const std::vector<int32_t> edge = {1, 64, 65, 2048, 2, 63, 128, 129, 2047, 1000};
  // an empty batch
  {
    const mp::Plan P = mp::make_plan({}, 2048, size_t(1) << 30, PROB, CTL, SLOT, SRC);
    CHECK(P.at.empty() && P.total_slots == 0 && P.bytes == 0 && P.nrow_rows == 0 && P.nslice_rows == 0);
    CHECK(mp::deal_slots({}, 2048).empty());
    CHECK(mp::slot_rows({}, {}).empty());
    CHECK(mp::compact({}, [](int32_t) { return false; }).empty());
  }
  for (int trial = 0; trial < 40; ++trial) {
    const int count = trial == 0 ? 1 : (trial == 1 ? static_cast<int>(edge.size()) : 1 + static_cast<int>(rng() % 300));
    std::vector<mp::Size> sz(static_cast<size_t>(count));
    for (size_t i = 0; i < sz.size(); ++i) {
      const int32_t m = trial == 1 ? edge[i] : (rng() % 4 == 0 ? edge[rng() % edge.size()] : 1 + static_cast<int32_t>(rng() % 2048));
      const int32_t ncg = (m + 63) / 64, nchunks = (m + 255) / 256;
      sz[i] = mp::Size{m, trial % 3 == 2 ? 0 : ncg * nchunks};  // (every third batch: dense stores)
    }
    if (trial == 0) sz[0].m = 2048;
    check_plan(sz, 2048, size_t(4) << 30);
    check_plan(sz, 2048, size_t(64) << 20);  // little room: fewer slots
    check_plan(sz, 8, size_t(4) << 30);      // fewer slots than problems: one each
    check_plan(sz, 2048, 0);

    // compaction and the slot table of what is left
    std::vector<int32_t> nslots(sz.size());
    const mp::Plan P = mp::make_plan(sz, 2048, size_t(4) << 30, PROB, CTL, SLOT, SRC);
    for (size_t i = 0; i < sz.size(); ++i) nslots[i] = P.at[i].nslots;
    std::vector<int32_t> list(sz.size());
    for (size_t i = 0; i < list.size(); ++i) list[i] = static_cast<int32_t>(i);
    std::vector<char> done(sz.size(), 0);
    while (!list.empty()) {
      const std::vector<mp::Item> rows = mp::slot_rows(list, nslots);
      size_t k = 0;
      for (int32_t i : list)
        for (int32_t s = 0; s < nslots[static_cast<size_t>(i)]; ++s, ++k) CHECK(rows[k].prob == i && rows[k].idx == s);
      CHECK(k == rows.size() && static_cast<int64_t>(k) <= P.total_slots);
      for (int32_t i : list)
        if (rng() % 3 == 0) done[static_cast<size_t>(i)] = 1;
      std::vector<int32_t> expect;
      for (int32_t i : list)
        if (!done[static_cast<size_t>(i)]) expect.push_back(i);
      const std::vector<int32_t> next = mp::compact(list, [&](int32_t i) { return done[static_cast<size_t>(i)] != 0; });
      CHECK(next == expect);  // order kept, exactly the finished ones dropped
      list = next;
    }
  }
  // dealing: proportional, at least one for a positive weight, none for weight 0, never more than the weight
  {
    const std::vector<int32_t> s = mp::deal_slots({1000, 0, 1, 3000, 2}, 2048);
    CHECK(s[1] == 0 && s[2] == 1 && s[0] >= 1 && s[3] >= 1 && s[4] >= 1 && s[4] <= 2);
    CHECK(s[0] + s[2] + s[3] + s[4] <= 2048 && s[3] > 2 * s[0] && s[0] > 400);
    const std::vector<int32_t> one = mp::deal_slots({5, 5, 5}, 1);
    CHECK((one == std::vector<int32_t>{1, 1, 1}));
    const std::vector<int32_t> lone = mp::deal_slots({2048}, 2048);
    CHECK((lone == std::vector<int32_t>{2048}));
    const std::vector<int32_t> few = mp::deal_slots({3}, 2048);
    CHECK((few == std::vector<int32_t>{3}));
  }
  // the vertex orders
  {
    const std::vector<int32_t> core = {1, 3, 2, 3, 0, 2}, deg = {1, 4, 2, 3, 0, 5};
    std::vector<int32_t> seeds(6), pos(6), roots;
    mp::seed_order(core.data(), 6, seeds.data());
    CHECK((seeds == std::vector<int32_t>{1, 3, 2, 5, 0, 4}));
    mp::root_order(core.data(), deg.data(), 6, 2, pos.data(), roots);
    // (core, degree, index) ascending: 4, 0, 2, 5, 3, 1
    CHECK((pos == std::vector<int32_t>{1, 5, 2, 4, 0, 3}));
    CHECK((roots == std::vector<int32_t>{1, 3, 5, 2}));
  }
  CHECK(mp::BATCH_MAX_M == 2048);
  std::printf("mc batch plan ok\n");
  return 0;
}
