// host_mcplan.hpp — the plan of a maximum-clique call (host_maxclique.hpp): where every problem's buffers
// sit in the call's two device slabs, how the search slots are dealt, the rows of the slot tables, the compaction of
// the work list between launches, and the two vertex orders of the search.
// Host-only (no HIP): tests/cpp/test_mc_batch_plan.cpp builds it with g++.
//
// The graph part is planned before anything runs, from the problems' m alone. Byte offsets, every table a multiple
// of 8 bytes, every array of a problem starting on a 256-byte boundary. First what only the device works on, each kind contiguous over the problems (one memset or copy serves
// all of them): G (m rows of nw = ceil(m / 64) words), alive (nw words), degw (mp = m rounded up to even int32). From
// `host_begin` on what the host reads or writes, mirrored at the same relative offsets by the caller's pinned staging
// buffer:
//   up    [up_begin, up_end): the descriptor table, the adjacency sources, the McCtl array, the vertex lists of a
//         seeded call (none otherwise: the offsets after them are those of an unseeded call), every problem's list
//         and pos — written by the host before a phase, ONE copy
//   tab   the work list (one int32 per problem) and HEU's slot table ((problem, slot) per dealt slot)
//   out   per problem m + 2 int32 (count, then the clique), ONE copy back
//   deg, core   (mp int32 each per problem; deg of all problems, then core of all), ONE copy back
// The search part is planned after HEU, for the problems that run EXACT, from each one's K and root count: per slot a
// stack of D = K + 1 levels of nw words (a clique has at most K + 1 vertices), a path and a record of D + 1 int32
// (device only), then, from its own `host_begin` on, the slots' states and EXACT's slot table. Its mirror follows the
// graph part's in the staging buffer; search_host_bound() says how much it can take before K is known.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace clipper_mc_plan {

constexpr int32_t BATCH_MAX_M = 2048;  // problems up to this size share a call: the batch's resident limit

struct Item {  // a row of a slot table
  int32_t prob, idx;
};

struct GraphRegions {  // byte offsets into the graph slab
  size_t G, alive, degw, list, pos, out, deg, core;
  int64_t nw;
  int32_t mp;  // m rounded up to even
  size_t given = 0;  // a seeded call: the caller's vertex list
};

struct GraphPlan {
  std::vector<GraphRegions> at;
  size_t bytes = 0, host_begin = 0;
  size_t G_begin = 0, G_bytes = 0, alive_begin = 0, alive_bytes = 0, degw_begin = 0, deg_bytes = 0;
  size_t probs = 0, src = 0, ctl = 0, up_begin = 0, up_end = 0;
  size_t given_end = 0;  // the end of the seeded problems' vertex lists (no list: the end of the McCtl array)
  size_t work = 0, slot_tab = 0;
  size_t out_begin = 0, out_bytes = 0, deg_begin = 0, core_begin = 0;
  int64_t slot_rows = 0;  // rows HEU's slot table has room for: max(slot_cap, problems)
  int64_t nw_max = 0;
  int32_t m_max = 0;
};

struct Search {  // what the search part needs to know of a problem
  int32_t m, K;
  int64_t roots;  // EXACT's roots; 0: the problem does not search
};

struct SearchRegions {  // byte offsets into the search slab
  size_t arena, paths, recs, slots;
  int32_t nslots, D;
};

struct SearchPlan {
  std::vector<SearchRegions> at;
  size_t bytes = 0, host_begin = 0, slot_tab = 0;
  size_t arena_bytes = 0;  // nslots x slot_bytes() over the problems: what `room` is compared with
  int64_t total_slots = 0;
  bool fits = true;  // arena_bytes <= room (if not: one slot per searching problem)
};

inline size_t up8(size_t b) { return (b + 7) & ~static_cast<size_t>(7); }
// Every array a kernel scans starts on a 256-byte boundary, as an allocation of its own would: a wave's 256-byte
// load of int32 then touches two 128-byte lines, not three (the peel scans degw once per round).
constexpr size_t ARRAY_ALIGN = 256;
inline size_t up_array(size_t b) { return (b + ARRAY_ALIGN - 1) & ~(ARRAY_ALIGN - 1); }

// Slots in proportion to the weights (seeds or roots), at least one per problem of positive weight, never more than
// its weight, none for weight 0; the total is at most max(cap, problems of positive weight).
inline std::vector<int32_t> deal_slots(const std::vector<int64_t>& weight, int64_t cap) {
  std::vector<int32_t> out(weight.size(), 0);
  int64_t npos = 0, W = 0;
  for (int64_t w : weight)
    if (w > 0) {
      ++npos;
      W += w;
    }
  if (npos == 0) return out;
  const int64_t spare = std::max<int64_t>(cap, npos) - npos;
  for (size_t i = 0; i < weight.size(); ++i)
    if (weight[i] > 0) {
      const int64_t s = 1 + static_cast<int64_t>(static_cast<long double>(spare) * weight[i] / W);
      out[i] = static_cast<int32_t>(std::min<int64_t>(s, weight[i]));
    }
  return out;
}

// prob_bytes, ctl_bytes, src_bytes: sizeof(McProb), McCtl, McAdjSrc (multiples of 8). slot_cap: slots of the whole
// call at most (the chip's waves). ngiven: the length of each problem's vertex list in a seeded call (empty: no
// problem has one).
inline GraphPlan make_graph_plan(const std::vector<int32_t>& m, int64_t slot_cap, size_t prob_bytes, size_t ctl_bytes,
                                 size_t src_bytes, const std::vector<int32_t>& ngiven = {}) {
  GraphPlan P;
  const size_t count = m.size();
  P.at.resize(count);
  P.slot_rows = count ? std::max<int64_t>(slot_cap, static_cast<int64_t>(count)) : 0;
  size_t o = 0;
  auto take = [&o](size_t bytes) {  // a table
    const size_t at = o;
    o += up8(bytes);
    return at;
  };
  auto array = [&o](size_t bytes) {  // a problem's array
    const size_t at = o;
    o += up_array(bytes);
    return at;
  };
  for (size_t i = 0; i < count; ++i) {
    GraphRegions& r = P.at[i];
    r.nw = (m[i] + 63) / 64;
    r.mp = m[i] + (m[i] & 1);
    P.nw_max = std::max(P.nw_max, r.nw);
    P.m_max = std::max(P.m_max, m[i]);
  }
  P.G_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].G = array(static_cast<size_t>(m[i]) * P.at[i].nw * 8);
  P.G_bytes = o - P.G_begin;
  P.alive_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].alive = array(static_cast<size_t>(P.at[i].nw) * 8);
  P.alive_bytes = o - P.alive_begin;
  P.degw_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].degw = array(static_cast<size_t>(P.at[i].mp) * 4);
  P.deg_bytes = o - P.degw_begin;
  P.host_begin = P.up_begin = o;
  P.probs = take(count * prob_bytes);
  P.src = take(count * src_bytes);
  P.ctl = take(count * ctl_bytes);
  P.given_end = o;
  for (size_t i = 0; i < ngiven.size() && i < count; ++i)
    if (ngiven[i] > 0) {
      o = up_array(o);
      P.at[i].given = array(static_cast<size_t>(ngiven[i]) * 4);
      P.given_end = o;
    }
  o = up_array(o);
  for (size_t i = 0; i < count; ++i) {
    P.at[i].list = array(static_cast<size_t>(P.at[i].mp) * 4);
    P.at[i].pos = array(static_cast<size_t>(P.at[i].mp) * 4);
  }
  P.up_end = o;
  P.work = take(count * 4);
  P.slot_tab = take(static_cast<size_t>(P.slot_rows) * sizeof(Item));
  P.out_begin = o = up_array(o);
  for (size_t i = 0; i < count; ++i) P.at[i].out = array((static_cast<size_t>(m[i]) + 2) * 4);
  P.out_bytes = o - P.out_begin;
  P.deg_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].deg = array(static_cast<size_t>(P.at[i].mp) * 4);
  P.core_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].core = array(static_cast<size_t>(P.at[i].mp) * 4);
  P.bytes = o;
  return P;
}

// what one search slot of a problem costs: its stack, path, record and state (slot_bytes: sizeof(McSlot))
inline size_t slot_bytes(const Search& s, size_t state_bytes) {
  const size_t D = static_cast<size_t>(s.K) + 1, nw = (static_cast<size_t>(s.m) + 63) / 64;
  return D * nw * 8 + 2 * (D + 1) * 4 + state_bytes;
}

// the host-visible bytes of any search part of `count` problems under `slot_cap`
inline size_t search_host_bound(int64_t slot_cap, size_t count, size_t state_bytes) {
  return static_cast<size_t>(std::max<int64_t>(slot_cap, static_cast<int64_t>(count))) * (state_bytes + sizeof(Item));
}

// Slots dealt by roots under slot_cap. While they cost more than `room` bytes (at most 4 GiB) the cap is lowered in
// proportion, down to one slot per searching problem; for one problem that is min(slot_cap, roots, room / slot_bytes).
inline SearchPlan make_search_plan(const std::vector<Search>& sr, int64_t slot_cap, size_t room, size_t state_bytes) {
  SearchPlan P;
  const size_t count = sr.size();
  P.at.resize(count);
  std::vector<int64_t> weight(count);
  int64_t npos = 0;
  for (size_t i = 0; i < count; ++i) {
    weight[i] = sr[i].roots;
    npos += sr[i].roots > 0;
  }
  std::vector<int32_t> slots;
  for (int64_t cap = std::max<int64_t>(slot_cap, 1);;) {
    slots = deal_slots(weight, cap);
    P.total_slots = 0;
    P.arena_bytes = 0;
    for (size_t i = 0; i < count; ++i) {
      P.total_slots += slots[i];
      P.arena_bytes += static_cast<size_t>(slots[i]) * slot_bytes(sr[i], state_bytes);
    }
    P.fits = P.arena_bytes <= room;
    if (P.fits || P.total_slots <= npos) break;
    const size_t share = static_cast<size_t>(P.total_slots) * room / P.arena_bytes;  // (< total_slots)
    cap = std::max<int64_t>(npos, std::min<int64_t>(P.total_slots - 1, static_cast<int64_t>(share)));
  }
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += up8(bytes);
    return at;
  };
  auto array = [&o](size_t bytes) {
    const size_t at = o;
    o += up_array(bytes);
    return at;
  };
  for (size_t i = 0; i < count; ++i) {
    SearchRegions& r = P.at[i];
    r.nslots = slots[i];
    r.D = sr[i].K + 1;
    const size_t ns = static_cast<size_t>(slots[i]), D = static_cast<size_t>(r.D);
    r.arena = array(ns * D * ((static_cast<size_t>(sr[i].m) + 63) / 64) * 8);
    r.paths = array(ns * (D + 1) * 4);
    r.recs = array(ns * (D + 1) * 4);
  }
  P.host_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].slots = take(static_cast<size_t>(slots[i]) * state_bytes);
  P.slot_tab = take(static_cast<size_t>(P.total_slots) * sizeof(Item));
  P.bytes = o;
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

// The slot table of a launch over `list`: (problem, slot) for each of the problem's nslots[problem] slots.
inline std::vector<Item> slot_rows(const std::vector<int32_t>& list, const std::vector<int32_t>& nslots) {
  std::vector<Item> rows;
  for (int32_t i : list)
    for (int32_t s = 0; s < nslots[static_cast<size_t>(i)]; ++s) rows.push_back(Item{i, s});
  return rows;
}

// ---- the two vertex orders of the search ------------------------------------------------------------
// HEU's seeds: core number descending, index ascending.
inline void seed_order(const int32_t* core, int64_t m, int32_t* seeds) {
  std::iota(seeds, seeds + m, 0);
  std::stable_sort(seeds, seeds + m, [&](int32_t a, int32_t c) { return core[a] > core[c]; });
}

// EXACT's order by (core, degree, index): pos[v] = v's place in it; roots = the vertices with core >= heu, taken from
// the end of that order (the largest bound first).
inline void root_order(const int32_t* core, const int32_t* deg, int64_t m, int heu, int32_t* pos,
                       std::vector<int32_t>& roots) {
  std::vector<int32_t> order(static_cast<size_t>(m));
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t c2) {
    if (core[a] != core[c2]) return core[a] < core[c2];
    if (deg[a] != deg[c2]) return deg[a] < deg[c2];
    return a < c2;
  });
  for (int64_t i = 0; i < m; ++i) pos[order[static_cast<size_t>(i)]] = static_cast<int32_t>(i);
  roots.clear();
  for (int64_t i = m - 1; i >= 0; --i)
    if (core[order[static_cast<size_t>(i)]] >= heu) roots.push_back(order[static_cast<size_t>(i)]);
}

// ---- seeded calls (DESIGN.md 9 "Seeded calls") ----------------------------------------------------------------------
// The position of the first entry of a caller's vertex list that is out of range or repeats an earlier one, -1 when
// the list is a set of vertices of 0..m-1.
inline int64_t first_bad_seed(const int32_t* seed, int64_t n, int32_t m) {
  std::vector<uint8_t> seen(static_cast<size_t>(std::max<int32_t>(m, 0)), 0);
  for (int64_t i = 0; i < n; ++i) {
    if (seed[i] < 0 || seed[i] >= m || seen[static_cast<size_t>(seed[i])]) return i;
    seen[static_cast<size_t>(seed[i])] = 1;
  }
  return -1;
}

// Whose clique a seeded call returns (clipper_maxclique_seed_info_t::winner): the search's (0) when it raised the
// incumbent above b = max(s, HEU); else the seed clique's (2) when HEU did not beat its s vertices (ties go to the
// seed clique; s < 2: the call ran unseeded), else HEU's (1). `found` is the incumbent's size at the end, b for a
// call that did not search.
inline int seeded_winner(int s, int b, int found) {
  if (found > b) return 0;
  return s >= 2 && b == s ? 2 : 1;
}

}  // namespace clipper_mc_plan
