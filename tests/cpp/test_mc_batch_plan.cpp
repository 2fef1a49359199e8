// test_mc_batch_plan.cpp — the plan of a maximum-clique call (csrc/host_mcplan.hpp; host only, g++): the regions of
// the graph part and of the search part disjoint, 8-byte aligned and inside their slab, the slots dealt, the slot
// tables' rows, the compaction, the two vertex orders. Built and run by tests/test_batch_maxclique_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
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

using Regions = std::vector<std::pair<size_t, size_t>>;  // (begin, bytes)

static void check_regions(Regions regions, size_t bytes) {
  for (const auto& r : regions) {
    CHECK(r.first % 8 == 0);
    CHECK(r.first + r.second <= bytes);
  }
  std::sort(regions.begin(), regions.end());
  for (size_t k = 1; k < regions.size(); ++k) CHECK(regions[k - 1].first + regions[k - 1].second <= regions[k].first);
}

static void check_graph(const std::vector<int32_t>& ms, int64_t cap) {
  const mp::GraphPlan P = mp::make_graph_plan(ms, cap, PROB, CTL, SRC);
  const size_t count = ms.size();
  CHECK(P.at.size() == count);
  const size_t rows = count ? static_cast<size_t>(std::max<int64_t>(cap, static_cast<int64_t>(count))) : 0;
  CHECK(P.slot_rows == static_cast<int64_t>(rows));
  Regions regions = {{P.probs, count * PROB}, {P.src, count * SRC}, {P.ctl, count * CTL}, {P.work, count * 4},
                     {P.slot_tab, rows * sizeof(mp::Item)}};
  int64_t nwmax = 0;
  int32_t mmax = 0;
  for (size_t i = 0; i < count; ++i) {
    const mp::GraphRegions& r = P.at[i];
    const size_t m = static_cast<size_t>(ms[i]), nw = (m + 63) / 64, mpad = m + (m & 1);
    CHECK(r.nw == static_cast<int64_t>(nw) && r.mp == static_cast<int32_t>(mpad));
    nwmax = std::max<int64_t>(nwmax, r.nw);
    mmax = std::max(mmax, ms[i]);
    for (auto pr : {std::make_pair(r.G, m * nw * 8), std::make_pair(r.alive, nw * 8), std::make_pair(r.degw, mpad * 4),
                    std::make_pair(r.list, mpad * 4), std::make_pair(r.pos, mpad * 4), std::make_pair(r.out, (m + 2) * 4),
                    std::make_pair(r.deg, mpad * 4), std::make_pair(r.core, mpad * 4)})
      regions.push_back(pr);
    for (size_t at : {r.G, r.alive, r.degw, r.list, r.pos, r.out, r.deg, r.core}) CHECK(at % mp::ARRAY_ALIGN == 0);
    // what the host reads or writes lies behind host_begin, what one copy moves inside its range
    CHECK(r.G < P.host_begin && r.alive < P.host_begin && r.degw + mpad * 4 <= P.host_begin);
    CHECK(r.list >= P.up_begin && r.pos >= P.up_begin && r.pos + mpad * 4 <= P.up_end && r.list + mpad * 4 <= P.up_end);
    CHECK(r.out >= P.out_begin && r.out + (m + 2) * 4 <= P.out_begin + P.out_bytes);
    CHECK(r.deg >= P.deg_begin && r.deg < P.core_begin && r.core >= P.core_begin);
    CHECK(r.G >= P.G_begin && r.G + m * nw * 8 <= P.G_begin + P.G_bytes);
    CHECK(r.alive >= P.alive_begin && r.alive + nw * 8 <= P.alive_begin + P.alive_bytes);
    // deg and degw are laid out alike: one device copy moves all of them
    CHECK(r.deg - P.deg_begin == r.degw - P.degw_begin);
  }
  CHECK(P.core_begin - P.deg_begin == P.deg_bytes);
  CHECK(P.nw_max == nwmax && P.m_max == mmax);
  // HEU's deal (by m): at least one slot per problem, never more than its seeds, and the table holds all of them
  const std::vector<int32_t> hs = mp::deal_slots(std::vector<int64_t>(ms.begin(), ms.end()), cap);
  int64_t htotal = 0;
  for (size_t i = 0; i < count; ++i) {
    CHECK(hs[i] >= 1 && hs[i] <= ms[i]);
    htotal += hs[i];
  }
  CHECK(htotal <= P.slot_rows);
  CHECK(P.probs >= P.up_begin && P.ctl + count * CTL <= P.up_end && P.up_begin == P.host_begin);
  CHECK(P.work >= P.up_end && P.slot_tab >= P.up_end && P.out_begin >= P.up_end && P.deg_begin >= P.host_begin);
  check_regions(regions, P.bytes);
}

// K of each problem is drawn below m; `searching` of them have roots
static void check_search(const std::vector<mp::Search>& sr, int64_t cap, size_t room) {
  const mp::SearchPlan P = mp::make_search_plan(sr, cap, room, SLOT);
  const size_t count = sr.size();
  CHECK(P.at.size() == count);
  Regions regions;
  int64_t total = 0, searching = 0;
  size_t arena = 0, host = 0;
  for (size_t i = 0; i < count; ++i) {
    const mp::SearchRegions& r = P.at[i];
    const size_t nw = (static_cast<size_t>(sr[i].m) + 63) / 64, D = static_cast<size_t>(sr[i].K) + 1;
    const size_t ns = static_cast<size_t>(r.nslots);
    CHECK(r.D == sr[i].K + 1);  // a stack has K + 1 levels, whatever m is
    CHECK(mp::slot_bytes(sr[i], SLOT) == D * nw * 8 + 2 * (D + 1) * 4 + SLOT);
    if (sr[i].roots > 0) {
      ++searching;
      CHECK(r.nslots >= 1 && r.nslots <= sr[i].roots);  // at least one slot per searching problem, never more than roots
    } else {
      CHECK(r.nslots == 0);
    }
    total += r.nslots;
    arena += ns * mp::slot_bytes(sr[i], SLOT);
    host += ns * SLOT;
    for (auto pr : {std::make_pair(r.arena, ns * D * nw * 8), std::make_pair(r.paths, ns * (D + 1) * 4),
                    std::make_pair(r.recs, ns * (D + 1) * 4), std::make_pair(r.slots, ns * SLOT)})
      regions.push_back(pr);
    CHECK(r.arena % mp::ARRAY_ALIGN == 0 && r.paths % mp::ARRAY_ALIGN == 0 && r.recs % mp::ARRAY_ALIGN == 0);
    CHECK(r.arena + ns * D * nw * 8 <= P.host_begin && r.recs + ns * (D + 1) * 4 <= P.host_begin);
    CHECK(r.slots >= P.host_begin && r.slots + ns * SLOT <= P.slot_tab);
  }
  regions.push_back({P.slot_tab, static_cast<size_t>(total) * sizeof(mp::Item)});
  CHECK(P.total_slots == total && P.arena_bytes == arena && P.fits == (arena <= room));
  CHECK(total <= std::max<int64_t>(cap, searching));  // the cap, or one slot each
  CHECK(arena <= room || total == searching);         // within the room, or one slot each
  CHECK(P.slot_tab >= P.host_begin);
  // the mirrored range is within what the staging buffer was given before K was known
  CHECK(P.bytes - P.host_begin == host + static_cast<size_t>(total) * sizeof(mp::Item));
  CHECK(P.bytes - P.host_begin <= mp::search_host_bound(cap, count, SLOT));
  check_regions(regions, P.bytes);
}

// the slot rule of a call of one problem: min(cap, roots, room / bytes per slot)
static void check_one(int32_t m, int32_t K, int64_t roots, int64_t cap, size_t room) {
  const mp::Search s{m, K, roots};
  const size_t per = mp::slot_bytes(s, SLOT);
  const mp::SearchPlan P = mp::make_search_plan({s}, cap, room, SLOT);
  const int64_t want = std::min<int64_t>(std::min<int64_t>(cap, roots), static_cast<int64_t>(room / per));
  if (want < 1) {
    CHECK(!P.fits && P.at[0].nslots == 1);  // below a single slot: the caller refuses
  } else {
    CHECK(P.fits && P.at[0].nslots == want);
  }
  check_search({s}, cap, room);
}

int main() {
  std::mt19937 rng(20240917);
  const std::vector<int32_t> edge = {1, 64, 65, 2048, 2, 63, 128, 129, 2047, 1000};
  // an empty call
  {
    const mp::GraphPlan P = mp::make_graph_plan({}, 2048, PROB, CTL, SRC);
    CHECK(P.at.empty() && P.bytes == 0 && P.slot_rows == 0 && P.nw_max == 0 && P.m_max == 0);
    const mp::SearchPlan X = mp::make_search_plan({}, 2048, size_t(1) << 30, SLOT);
    CHECK(X.at.empty() && X.total_slots == 0 && X.bytes == 0 && X.fits);
    CHECK(mp::deal_slots({}, 2048).empty());
    CHECK(mp::slot_rows({}, {}).empty());
    CHECK(mp::compact({}, [](int32_t) { return false; }).empty());
  }
  for (int trial = 0; trial < 40; ++trial) {
    const int count = trial == 0 ? 1 : (trial == 1 ? static_cast<int>(edge.size()) : 1 + static_cast<int>(rng() % 300));
    std::vector<int32_t> ms(static_cast<size_t>(count));
    for (size_t i = 0; i < ms.size(); ++i) {
      // (every fifth batch: sizes past the batched route's limit)
      const int32_t top = trial % 5 == 4 ? 20000 : 2048;
      ms[i] = trial == 1 ? edge[i] : (rng() % 4 == 0 ? edge[rng() % edge.size()] : 1 + static_cast<int32_t>(rng() % top));
    }
    if (trial == 0) ms[0] = 2048;
    check_graph(ms, 2048);
    check_graph(ms, 8);  // fewer slots than problems: a table row each

    // the search part: K = 0, K = m - 1 and random K; some problems do not search
    std::vector<mp::Search> sr(ms.size());
    for (size_t i = 0; i < ms.size(); ++i) {
      const int32_t m = ms[i];
      const int32_t K = i % 3 == 0 ? 0 : (i % 3 == 1 ? m - 1 : static_cast<int32_t>(rng() % m));
      sr[i] = mp::Search{m, K, trial > 1 && rng() % 4 == 0 ? 0 : 1 + static_cast<int64_t>(rng() % m)};
    }
    check_search(sr, 2048, size_t(4) << 30);
    check_search(sr, 2048, size_t(64) << 20);  // little room: fewer slots
    check_search(sr, 8, size_t(4) << 30);      // fewer slots than problems: one each
    check_search(sr, 2048, 0);

    // compaction and the slot table of what is left
    const mp::SearchPlan P = mp::make_search_plan(sr, 2048, size_t(4) << 30, SLOT);
    std::vector<int32_t> nslots(sr.size()), list;
    for (size_t i = 0; i < sr.size(); ++i) {
      nslots[i] = P.at[i].nslots;
      if (nslots[i] > 0) list.push_back(static_cast<int32_t>(i));
    }
    std::vector<char> done(sr.size(), 0);
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
  // one problem: the bench problem's sizes (m = 10 000, nw = 157, K = 849: 1.07 MB per slot) and the edge sizes
  {
    const size_t per = mp::slot_bytes(mp::Search{10000, 849, 1}, SLOT);
    CHECK(per == size_t(850) * 157 * 8 + 2 * 851 * 4 + SLOT);
    check_one(10000, 849, 9000, 2048, size_t(4) << 30);  // the room does not bind: the cap
    check_one(10000, 849, 300, 2048, size_t(4) << 30);   // ... the roots
    check_one(10000, 849, 9000, 2048, 100 * per + 5);    // the room binds: 100 slots
    check_one(10000, 849, 9000, 2048, 100 * per);
    check_one(10000, 849, 9000, 2048, 100 * per - 1);    // 99
    check_one(10000, 849, 300, 2048, 299 * per);         // the room binds below the roots
    check_one(10000, 849, 9000, 2048, per);              // exactly one
    check_one(10000, 849, 9000, 2048, per - 1);          // below a single slot
    check_one(10000, 849, 9000, 2048, 0);
    for (int32_t m : edge)
      for (int32_t K : {0, m - 1, m / 2})
        for (size_t room : {size_t(0), size_t(1) << 16, size_t(1) << 22, size_t(4) << 30})
          check_one(m, K, 1 + m / 2, 2048, room);
  }
  // the size arithmetic past 2^32 (size_t only; nothing is allocated): m = 100 000 and the largest m there is
  for (int32_t m : {100000, 655360}) {
    const size_t nw = (static_cast<size_t>(m) + 63) / 64;
    check_graph({m}, 2048);
    const mp::GraphPlan G = mp::make_graph_plan({m}, 2048, PROB, CTL, SRC);
    CHECK(G.G_bytes == static_cast<size_t>(m) * nw * 8 && G.bytes > G.G_bytes);
    for (int32_t K : {0, m - 1, 849}) {
      const size_t D = static_cast<size_t>(K) + 1;
      CHECK(mp::slot_bytes(mp::Search{m, K, 1}, SLOT) == D * nw * 8 + 2 * (D + 1) * 4 + SLOT);
      check_one(m, K, m, 2048, size_t(4) << 30);
      check_one(m, K, m, 2048, size_t(1) << 20);
    }
  }
  CHECK(mp::make_graph_plan({655360}, 2048, PROB, CTL, SRC).G_bytes == size_t(655360) * 10240 * 8);  // 53.7 GB
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
