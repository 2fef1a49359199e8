// The plan of the semidefinite relaxation's wide route (clipper_amd/csrc/host_sdpwide_plan.hpp), host only: the
// geometry of the launch that runs one Jacobi step, the circle order, the slab of one problem and the split of a batch.
// Built with g++ by tests/test_sdp_wide_cpu.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_sdpwide_plan.hpp"

namespace plan = clipper_sdpw_plan;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// every 2 x 2 block (k, l), k <= l, once; every (row, pair) of Q once; for a few steps: every entry of A and Q is
// written exactly once by the launch (the blocks, their transposes, the diagonal blocks' four entries)
static void check_step_geometry(int np) {
  const plan::StepGeom g = plan::step_geom(np);
  CHECK(g.h == np / 2 && g.a_tiles == g.ht * (g.ht + 1) / 2 && g.q_tiles == g.q_row_tiles * g.ht);
  CHECK(g.ht * plan::TILE >= g.h && (g.ht - 1) * plan::TILE < g.h);
  std::vector<int> block(static_cast<size_t>(g.h) * g.h, 0), rowpair(static_cast<size_t>(np) * g.h, 0);
  for (int wg = 0; wg < g.a_tiles; ++wg) {
    int kt, lt;
    plan::a_tile(g, wg, kt, lt);
    CHECK(0 <= kt && kt <= lt && lt < g.ht);
    for (int tid = 0; tid < plan::STEP_THREADS; ++tid) {
      int k, l;
      if (!plan::a_item(g, wg, tid, k, l)) continue;
      CHECK(0 <= k && k <= l && l < g.h);
      ++block[static_cast<size_t>(k) * g.h + l];
    }
  }
  for (int k = 0; k < g.h; ++k)
    for (int l = 0; l < g.h; ++l) CHECK(block[static_cast<size_t>(k) * g.h + l] == (k <= l ? 1 : 0));
  for (int wg = 0; wg < g.q_tiles; ++wg)
    for (int tid = 0; tid < plan::STEP_THREADS; ++tid) {
      int row, k;
      if (!plan::q_item(g, wg, tid, row, k)) continue;
      CHECK(0 <= row && row < np && 0 <= k && k < g.h);
      ++rowpair[static_cast<size_t>(row) * g.h + k];
    }
  for (int v : rowpair) CHECK(v == 1);
  const int steps[] = {0, 1, np / 2, np - 2};
  for (int t : steps) {
    if (t < 0 || t > np - 2) continue;
    std::vector<int> a(static_cast<size_t>(np) * np, 0), q(static_cast<size_t>(np) * np, 0);
    for (int k = 0; k < g.h; ++k) {
      int p, qq;
      plan::circle_pair(k, t, np, p, qq);
      for (int l = k; l < g.h; ++l) {
        int r, s;
        plan::circle_pair(l, t, np, r, s);
        const int rows[2] = {p, qq}, cols[2] = {r, s};
        for (int x : rows)
          for (int y : cols) {
            ++a[static_cast<size_t>(x) * np + y];
            if (k != l) ++a[static_cast<size_t>(y) * np + x];
          }
      }
      for (int row = 0; row < np; ++row) {
        ++q[static_cast<size_t>(row) * np + p];
        ++q[static_cast<size_t>(row) * np + qq];
      }
    }
    for (int v : a) CHECK(v == 1);
    for (int v : q) CHECK(v == 1);
  }
}

// the pairs of a step partition the indices; over the np - 1 steps every unordered pair occurs exactly once
static void check_circle_order(int np) {
  std::vector<int> met(static_cast<size_t>(np) * np, 0);
  for (int t = 0; t < np - 1; ++t) {
    std::vector<int> seen(static_cast<size_t>(np), 0);
    for (int k = 0; k < np / 2; ++k) {
      int p, q;
      plan::circle_pair(k, t, np, p, q);
      CHECK(0 <= p && p < np && 0 <= q && q < np && p != q);
      ++seen[static_cast<size_t>(p)];
      ++seen[static_cast<size_t>(q)];
      ++met[static_cast<size_t>(std::min(p, q)) * np + std::max(p, q)];
    }
    for (int v : seen) CHECK(v == 1);
  }
  for (int i = 0; i < np; ++i)
    for (int j = 0; j < np; ++j) CHECK(met[static_cast<size_t>(i) * np + j] == (i < j ? 1 : 0));
}

static void check_slab(int n) {
  const plan::Regions r = plan::make_regions(n);
  const auto s = plan::spans(n);
  const size_t np = static_cast<size_t>(plan::padded(n)), nn = static_cast<size_t>(n) * n;
  const size_t tiles = static_cast<size_t>((n + 15) / 16) * static_cast<size_t>((n + 15) / 16);
  CHECK(static_cast<size_t>(plan::update_tiles(n)) == tiles);
  const size_t formula = 8 * (5 * nn + 5 * np * np + np + 6 * tiles) + 4 * np + plan::STATE_BYTES;
  CHECK(r.bytes == formula);
  size_t end = 0, sum = 0;
  for (const auto& sp : s) {  // (in slab order: disjoint when each begins where the last ended)
    CHECK(sp.first % 8 == 0 && sp.second % 8 == 0 && sp.second > 0);
    CHECK(sp.first == end);
    end = sp.first + sp.second;
    sum += sp.second;
  }
  CHECK(end == r.bytes && sum == r.bytes);
  CHECK(r.Q[1] == r.work_begin && r.mu < r.work_begin && r.A[0] > r.work_begin);
  CHECK(r.Q[1] - r.Q[0] >= 8 * np * np && r.A[1] - r.A[0] == 8 * np * np && r.T - r.Q[0] == 8 * np * np);
  CHECK(r.mask - r.M == 8 * nn && r.X - r.mask == 8 * nn && r.Z - r.X == 8 * nn && r.U - r.Z == 8 * nn);
}

int main() {
  const int nps[] = {2, 4, 130, 192, 1024};
  for (int np : nps) {
    check_step_geometry(np);
    check_circle_order(np);
    check_slab(np);
    check_slab(np - 1);  // the odd n below it: the same np
    CHECK(plan::padded(np - 1) == np && plan::padded(np) == np);
  }
  CHECK(plan::make_regions(1024).bytes == 8u * 10u * 1024u * 1024u + 8u * (1024u + 6u * 4096u) + 4096u + plan::STATE_BYTES);
  CHECK(plan::make_regions(1024).bytes < (81u << 20));  // "80 MB at n = 1024"

  // routes and the split of a batch, both lists in the caller's order
  CHECK(plan::route_limit(plan::ROUTE_WORKGROUP) == 128 && plan::route_limit(plan::ROUTE_AUTO) == 1024 &&
        plan::route_limit(plan::ROUTE_WIDE) == 1024);
  CHECK(plan::route_of(plan::ROUTE_WORKGROUP, 128) == plan::ROUTE_WORKGROUP);
  CHECK(plan::route_of(plan::ROUTE_AUTO, 128) == plan::ROUTE_WORKGROUP && plan::route_of(plan::ROUTE_AUTO, 129) == plan::ROUTE_WIDE);
  CHECK(plan::route_of(plan::ROUTE_WIDE, 1) == plan::ROUTE_WIDE);
  const std::vector<int32_t> n = {40, 129, 128, 200, 7, 1024, 1};
  plan::Split s = plan::split(n, plan::ROUTE_AUTO);
  CHECK((s.workgroup == std::vector<int32_t>{0, 2, 4, 6}) && (s.wide == std::vector<int32_t>{1, 3, 5}));
  s = plan::split(n, plan::ROUTE_WIDE);
  CHECK(s.workgroup.empty() && (s.wide == std::vector<int32_t>{0, 1, 2, 3, 4, 5, 6}));
  s = plan::split({40, 128, 7}, plan::ROUTE_WORKGROUP);
  CHECK((s.workgroup == std::vector<int32_t>{0, 1, 2}) && s.wide.empty());
  CHECK(plan::split({}, plan::ROUTE_AUTO).wide.empty());
  std::printf("sdp wide plan ok\n");
  return 0;
}
