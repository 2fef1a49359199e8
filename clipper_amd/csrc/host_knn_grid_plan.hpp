// host_knn_grid_plan.hpp — the dimensions of the uniform grid of the nearest-neighbour search's grid route, from the
// bounding box of the searched cloud and its size ("The grid route of the search"). Pure host
// arithmetic over knn_grid_rules.hpp's KnnGrid: no HIP, builds with g++ (tests/cpp/test_knn_grid_rules.cpp).
//
// The grid aims at KNN_GRID_POINTS_PER_CELL points per cell with cubic cells, over the axes that have an extent: an
// axis of zero extent (a planar cloud, a collinear one, identical points), one whose bounds are not finite and one
// thinner than a cell have dim = 1. The cell count never exceeds max(1, n1), so the tables never outgrow the cloud.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "knn_grid_rules.hpp"

#ifndef KNN_GRID_POINTS_PER_CELL
#define KNN_GRID_POINTS_PER_CELL 4.0  // measured on the MI355X: DESIGN.md section 9 (profiles/knn_grid_probe.json)
#endif

namespace clipper_hip {

constexpr int64_t KNN_GRID_MAX_CELLS = int64_t(1) << 27;  // cell numbers and the tables' offsets are int32

inline int64_t knn_grid_cells(const KnnGrid& g) {
  return static_cast<int64_t>(g.dim[0]) * g.dim[1] * g.dim[2];
}

inline KnnGrid knn_grid_plan(const double (&lo)[3], const double (&hi)[3], int64_t n1,
                             double points_per_cell = KNN_GRID_POINTS_PER_CELL) {
  KnnGrid g{};
  const int64_t cap = std::min<int64_t>(std::max<int64_t>(1, n1), KNN_GRID_MAX_CELLS);
  const double want = std::min(static_cast<double>(cap), std::max(1.0, static_cast<double>(n1) / points_per_cell));
  double ext[3];
  bool live[3];
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = std::isfinite(lo[a]) ? lo[a] : 0.0;
    g.inv[a] = 0.0;
    g.dim[a] = 1;
    ext[a] = hi[a] - lo[a];
    live[a] = std::isfinite(lo[a]) && std::isfinite(hi[a]) && std::isfinite(ext[a]) && ext[a] > 0.0;
  }
  // cubic cells of edge s over the live axes: prod(ext / s) = want; an axis thinner than s leaves the product
  double logs = 0.0;
  for (int pass = 0; pass < 3; ++pass) {
    int k = 0;
    double sum = 0.0;
    for (int a = 0; a < 3; ++a)
      if (live[a]) {
        ++k;
        sum += std::log(ext[a]);
      }
    if (k == 0) break;
    logs = (sum - std::log(want)) / k;
    bool dropped = false;
    for (int a = 0; a < 3; ++a)
      if (live[a] && !(std::log(ext[a]) - logs >= 0.0)) {
        live[a] = false;
        dropped = true;
      }
    if (!dropped) break;
  }
  for (int a = 0; a < 3; ++a)
    if (live[a]) {
      const double cells = std::floor(std::exp(std::log(ext[a]) - logs));
      g.dim[a] = static_cast<int32_t>(std::min(std::max(cells, 1.0), static_cast<double>(cap)));
    }
  // the rounding of exp / log may leave the product one step above the cap: take it from the longest axis
  while (knn_grid_cells(g) > cap) {
    int a = 0;
    for (int b = 1; b < 3; ++b)
      if (g.dim[b] > g.dim[a]) a = b;
    g.dim[a] = static_cast<int32_t>(std::max<int64_t>(1, std::min<int64_t>(g.dim[a] - 1, cap / std::max<int64_t>(1, knn_grid_cells(g) / g.dim[a]))));
  }
  for (int a = 0; a < 3; ++a) {
    if (g.dim[a] > 1) {
      g.inv[a] = static_cast<double>(g.dim[a]) / ext[a];
      if (!std::isfinite(g.inv[a]) || !(g.inv[a] > 0.0)) {  // an extent so small that the factor overflows
        g.inv[a] = 0.0;
        g.dim[a] = 1;
      }
    }
  }
  g.off[0] = 0;
  g.off[1] = g.dim[0];
  g.off[2] = g.dim[0] + g.dim[1];
  return g;
}

}  // namespace clipper_hip
