// host_batchpack.hpp — how the resident solves of a batch are packed into launches (host_batchsolve.hpp).
// Host-only (no HIP): tests/cpp/test_batch_pack.cpp builds it with g++.
//
// Every problem the batch solves resident brings its own plan: `units` workgroups of one instantiation
// k_solve_resident_batch<VT, V, E> (key). A launch runs one instantiation, so problems are grouped by key
// (ascending); inside a group they are taken in their order in the batch, and a launch is closed when the
// next problem's units would take it past `cap` workgroups (cus - 8: one workgroup per CU, the LDS allows no
// second, and a margin for whatever else runs). A problem is never split over two launches: its units wait
// for each other's sums, and only workgroups of the same launch are sure to be resident together.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace clipper_batch {

struct PackItem {
  int key;    // instantiation (VT, V, E), any ordering the caller chooses
  int units;  // workgroups of the problem's plan, 1 <= units <= cap
};

struct PackLaunch {
  int key = 0;
  int workgroups = 0;
  std::vector<int> items;  // indices into the item list, in batch order
};

// Deterministic: the same items give the same launches. Items with units < 1 or > cap are left out
// (returned in `rejected`: the caller solves them alone).
inline std::vector<PackLaunch> pack_launches(const std::vector<PackItem>& items, int cap, std::vector<int>* rejected = nullptr) {
  std::vector<int> order;
  order.reserve(items.size());
  for (int i = 0; i < static_cast<int>(items.size()); ++i) {
    if (items[i].units >= 1 && items[i].units <= cap) order.push_back(i);
    else if (rejected) rejected->push_back(i);
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return items[a].key < items[b].key; });
  std::vector<PackLaunch> out;
  for (int i : order) {
    const PackItem& it = items[i];
    if (out.empty() || out.back().key != it.key || out.back().workgroups + it.units > cap) {
      out.emplace_back();
      out.back().key = it.key;
    }
    out.back().workgroups += it.units;
    out.back().items.push_back(i);
  }
  return out;
}

}  // namespace clipper_batch
