// host_mcplan.hpp — the plan of a batched maximum-clique call (host_mcbatch.hpp, DESIGN.md 9 "Batches"): where every
// problem's buffers sit in the call's one device slab, how the search slots are dealt, the rows of the launch tables and
// their compaction between launches; and the two vertex orders of the search, which the lone call
// (host_maxclique.hpp) takes from here too, so that both sort the same way.
// Host-only (no HIP): tests/cpp/test_mc_batch_plan.cpp builds it with g++.
//
// Slab layout, byte offsets, every region a multiple of 8 bytes. First what only the device works on, each kind
// contiguous over the problems (one memset or copy serves all of them): G (m rows of nw = ceil(m / 64) words), alive
// (nw words), degw (mp = m rounded up to even int32), the slots' arenas (nslots x m x nw words: a stack has at most
// m levels), paths and recs (nslots x (m + 1) int32, rounded up to even). From `host_begin` on what the host reads or
// writes, mirrored at the same relative offsets by ONE pinned staging buffer:
//   up    [up_begin, up_end): the descriptor table, the adjacency sources, the McCtl array, every problem's list, pos and slot states —
//         written by the host before a phase, ONE copy
//   adj   [up_end, adj_end): the (problem, slice) and (problem, row) tables of the adjacency and degree launches
//   tab   the work list (one int32 per problem) and the slot table ((problem, slot) per dealt slot) of a launch
//   out   per problem m + 2 int32 (count, then the clique), ONE copy back
//   deg, core   (mp int32 each per problem; deg of all problems, then core of all), ONE copy back
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

namespace clipper_mc_plan {

constexpr int32_t BATCH_MAX_M = 2048;  // problems up to this size run in the batched launches: the batch's resident limit

struct Size {
  int32_t m;
  int32_t nslices;  // slices of its store (column groups x chunks), 0: a dense store
};

struct Item {  // a row of a launch table
  int32_t prob, idx;
};

struct Regions {  // byte offsets into the slab
  size_t G, alive, degw, arena, paths, recs, list, pos, slots, out, deg, core;
  int64_t nw;
  int32_t mp;      // m rounded up to even
  int32_t nslots;  // search slots dealt to the problem (HEU's waves, the capacity of EXACT's)
};

struct Plan {
  std::vector<Regions> at;
  size_t bytes = 0, host_begin = 0;
  size_t G_begin = 0, G_bytes = 0, alive_begin = 0, alive_bytes = 0, degw_begin = 0, deg_bytes = 0;
  size_t probs = 0, src = 0, ctl = 0, up_begin = 0, up_end = 0;
  size_t slice_tab = 0, row_tab = 0, adj_end = 0;
  size_t nslice_rows = 0, nrow_rows = 0;
  size_t work = 0, slot_tab = 0;
  size_t out_begin = 0, out_bytes = 0, deg_begin = 0, core_begin = 0;
  int64_t total_slots = 0;
  int64_t nw_max = 0;
};

inline size_t up8(size_t b) { return (b + 7) & ~static_cast<size_t>(7); }

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

// prob_bytes, ctl_bytes, slot_bytes, src_bytes: sizeof(McProb), McCtl, McSlot, McAdjSrc (multiples of 8). slot_cap: slots
// of the whole call at most (the chip's waves); halved, down to one slot per problem, while the arenas exceed
// arena_room bytes.
inline Plan make_plan(const std::vector<Size>& sz, int64_t slot_cap, size_t arena_room, size_t prob_bytes,
                      size_t ctl_bytes, size_t slot_bytes, size_t src_bytes) {
  Plan P;
  const size_t count = sz.size();
  P.at.resize(count);
  std::vector<int64_t> weight(count);
  for (size_t i = 0; i < count; ++i) weight[i] = sz[i].m;
  std::vector<int32_t> slots;
  auto arena_bytes = [&] {
    size_t b = 0;
    for (size_t i = 0; i < count; ++i)
      b += static_cast<size_t>(slots[i]) * static_cast<size_t>(sz[i].m) * static_cast<size_t>((sz[i].m + 63) / 64) * 8;
    return b;
  };
  for (int64_t cap = std::max<int64_t>(slot_cap, 1);; cap /= 2) {
    slots = deal_slots(weight, cap);
    if (arena_bytes() <= arena_room || cap <= static_cast<int64_t>(count)) break;
  }
  size_t o = 0;
  auto take = [&o](size_t bytes) {
    const size_t at = o;
    o += up8(bytes);
    return at;
  };
  for (size_t i = 0; i < count; ++i) {
    Regions& r = P.at[i];
    r.nw = (sz[i].m + 63) / 64;
    r.mp = sz[i].m + (sz[i].m & 1);
    r.nslots = slots[i];
    P.total_slots += slots[i];
    P.nw_max = std::max(P.nw_max, r.nw);
    P.nslice_rows += static_cast<size_t>(sz[i].nslices);
    P.nrow_rows += static_cast<size_t>(sz[i].m);
  }
  P.G_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].G = take(static_cast<size_t>(sz[i].m) * P.at[i].nw * 8);
  P.G_bytes = o - P.G_begin;
  P.alive_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].alive = take(static_cast<size_t>(P.at[i].nw) * 8);
  P.alive_bytes = o - P.alive_begin;
  P.degw_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].degw = take(static_cast<size_t>(P.at[i].mp) * 4);
  P.deg_bytes = o - P.degw_begin;
  for (size_t i = 0; i < count; ++i) P.at[i].arena = take(static_cast<size_t>(slots[i]) * sz[i].m * P.at[i].nw * 8);
  for (size_t i = 0; i < count; ++i) {
    P.at[i].paths = take(static_cast<size_t>(slots[i]) * (sz[i].m + 1) * 4);
    P.at[i].recs = take(static_cast<size_t>(slots[i]) * (sz[i].m + 1) * 4);
  }
  P.host_begin = P.up_begin = o;
  P.probs = take(count * prob_bytes);
  P.src = take(count * src_bytes);
  P.ctl = take(count * ctl_bytes);
  for (size_t i = 0; i < count; ++i) {
    P.at[i].list = take(static_cast<size_t>(P.at[i].mp) * 4);
    P.at[i].pos = take(static_cast<size_t>(P.at[i].mp) * 4);
    P.at[i].slots = take(static_cast<size_t>(slots[i]) * slot_bytes);
  }
  P.up_end = o;
  P.slice_tab = take(P.nslice_rows * sizeof(Item));
  P.row_tab = take(P.nrow_rows * sizeof(Item));
  P.adj_end = o;
  P.work = take(count * 4);
  P.slot_tab = take(static_cast<size_t>(P.total_slots) * sizeof(Item));
  P.out_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].out = take((static_cast<size_t>(sz[i].m) + 2) * 4);
  P.out_bytes = o - P.out_begin;
  P.deg_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].deg = take(static_cast<size_t>(P.at[i].mp) * 4);
  P.core_begin = o;
  for (size_t i = 0; i < count; ++i) P.at[i].core = take(static_cast<size_t>(P.at[i].mp) * 4);
  P.bytes = o;
  return P;
}

// The (problem, slice) rows of the adjacency launch on slices and the (problem, row) rows of the dense adjacency and
// the degree launches: problem after problem, every pair once.
inline void adjacency_rows(const std::vector<Size>& sz, Item* slice_rows, Item* row_rows) {
  size_t a = 0, b = 0;
  for (size_t i = 0; i < sz.size(); ++i) {
    for (int32_t s = 0; s < sz[i].nslices; ++s) slice_rows[a++] = Item{static_cast<int32_t>(i), s};
    for (int32_t v = 0; v < sz[i].m; ++v) row_rows[b++] = Item{static_cast<int32_t>(i), v};
  }
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

}  // namespace clipper_mc_plan
