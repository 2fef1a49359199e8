// CPU test of the grid route's rules (clipper_amd/csrc/knn_grid_rules.hpp) and of its plan function
// (host_knn_grid_plan.hpp), g++ only. A host restatement of build + query — bin the searched cloud, reduce the slab
// tables, walk the rings of every query with knn_grid_query — is compared with a direct brute force, entry for entry
// and bit for bit, for K in {1, 4, 32} on clouds chosen for what can go wrong: exact ties, repeated points, degenerate
// boxes, coordinates far from the origin, queries outside the box, fewer points than K, and clusters the grid cannot
// separate. `plan` as the first argument runs the plan function's checks alone.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "host_knn_grid_plan.hpp"

using namespace clipper_hip;

namespace {

typedef std::vector<double> Cloud;  // n x 3 row-major

struct Rng {
  std::mt19937_64 g;
  explicit Rng(uint64_t s) : g(s) {}
  double uni() { return static_cast<double>(g() >> 11) * (1.0 / 9007199254740992.0); }  // [0, 1)
  size_t below(size_t n) { return static_cast<size_t>(g() % n); }
};

Cloud uniform_cloud(Rng& r, int n, double scale = 1.0) {
  Cloud c(static_cast<size_t>(n) * 3);
  for (double& v : c) v = r.uni() * scale;
  return c;
}

Cloud shifted(const Cloud& c, double by) {
  Cloud o(c);
  for (double& v : o) v = v + by;
  return o;
}

// the contract, written out on its own: fp64, coordinate order, nothing fused, ascending by (distance, index)
void brute(const Cloud& Q, const Cloud& P, int K, std::vector<double>& od, std::vector<int32_t>& oi) {
  const size_t n0 = Q.size() / 3, n1 = P.size() / 3;
  od.assign(n0 * K, 1.0e300);
  oi.assign(n0 * K, -1);
  std::vector<std::pair<double, int32_t>> all(n1);
  for (size_t i = 0; i < n0; ++i) {
    for (size_t j = 0; j < n1; ++j) {
      double dist = 0.0;
      for (int k = 0; k < 3; ++k) {
        const double df = Q[i * 3 + k] - P[j * 3 + k];
        dist = dist + df * df;
      }
      all[j] = {dist, static_cast<int32_t>(j)};
    }
    std::sort(all.begin(), all.end());
    for (size_t k = 0; k < static_cast<size_t>(K) && k < n1; ++k) {
      if (!(all[k].first < 1.0e300)) break;
      od[i * K + k] = all[k].first;
      oi[i * K + k] = all[k].second;
    }
  }
}

struct Built {
  KnnGrid g;
  std::vector<int32_t> start;               // cells + 1
  std::vector<double> xyz;                  // the cloud in cell order
  std::vector<int32_t> idx;                 // original indices, in cell order
  std::vector<double> smin, pmax;
};

// `reverse`: the points of a cell in descending index order instead of ascending (the device's order inside a cell is
// whatever the atomics give: the lists may not depend on it)
Built build(const Cloud& P, bool reverse) {
  const int64_t n1 = static_cast<int64_t>(P.size() / 3);
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = 0; i < n1; ++i)
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], P[i * 3 + a]);
      hi[a] = std::max(hi[a], P[i * 3 + a]);
    }
  Built b;
  b.g = knn_grid_plan(lo, hi, n1);
  const int64_t cells = knn_grid_cells(b.g);
  const int32_t nslab = b.g.dim[0] + b.g.dim[1] + b.g.dim[2];
  std::vector<int32_t> cell(n1);
  std::vector<double> rawmin(nslab, INFINITY), rawmax(nslab, -INFINITY);
  b.start.assign(cells + 1, 0);
  for (int64_t i = 0; i < n1; ++i) {
    const double p[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
    int32_t c[3];
    knn_grid_cell3(b.g, p, c);
    cell[i] = knn_grid_cell_number(b.g, c);
    ++b.start[cell[i] + 1];
    for (int a = 0; a < 3; ++a) {
      rawmin[b.g.off[a] + c[a]] = std::min(rawmin[b.g.off[a] + c[a]], p[a]);
      rawmax[b.g.off[a] + c[a]] = std::max(rawmax[b.g.off[a] + c[a]], p[a]);
    }
  }
  for (int64_t c = 0; c < cells; ++c) b.start[c + 1] += b.start[c];
  std::vector<int32_t> cursor(b.start.begin(), b.start.end() - 1);
  b.xyz.resize(n1 * 3);
  b.idx.resize(n1);
  for (int64_t s = 0; s < n1; ++s) {
    const int64_t i = reverse ? n1 - 1 - s : s;
    const int32_t at = cursor[cell[i]]++;
    for (int a = 0; a < 3; ++a) b.xyz[at * 3 + a] = P[i * 3 + a];
    b.idx[at] = static_cast<int32_t>(i);
  }
  b.smin = rawmin;
  b.pmax = rawmax;
  for (int a = 0; a < 3; ++a) {
    const int32_t o = b.g.off[a], d = b.g.dim[a];
    for (int32_t c = d - 2; c >= 0; --c) b.smin[o + c] = std::min(b.smin[o + c], b.smin[o + c + 1]);
    for (int32_t c = 1; c < d; ++c) b.pmax[o + c] = std::max(b.pmax[o + c], b.pmax[o + c - 1]);
  }
  return b;
}

template <int K>
int64_t grid_search(const Cloud& Q, const Built& b, std::vector<double>& od, std::vector<int32_t>& oi) {
  const size_t n0 = Q.size() / 3;
  od.assign(n0 * K, 0.0);
  oi.assign(n0 * K, 0);
  int64_t seen = 0;
  for (size_t i = 0; i < n0; ++i) {
    const double q[3] = {Q[i * 3], Q[i * 3 + 1], Q[i * 3 + 2]};
    double bd[K];
    int32_t bi[K];
    knn_grid_clear(bd, bi);
    seen += knn_grid_query<K>(
        b.g, q, static_cast<int64_t>(b.idx.size()), b.smin.data(), b.pmax.data(), bd, bi,
        [&](int32_t first, int32_t last, int32_t& t, int32_t& e) {
          t = b.start[first];
          e = b.start[last + 1];
        },
        [&](int32_t t) {
          const double p[3] = {b.xyz[t * 3], b.xyz[t * 3 + 1], b.xyz[t * 3 + 2]};
          knn_grid_insert<K>(bd, bi, knn_grid_sqdist(q, p), b.idx[t]);
        });
    for (int k = 0; k < K; ++k) {
      od[i * K + k] = bd[k];
      oi[i * K + k] = bi[k];
    }
  }
  return seen;
}

int failures = 0;

template <int K>
void check_k(const char* name, const Cloud& Q, const Cloud& P, double max_visit_share) {
  std::vector<double> rd, gd;
  std::vector<int32_t> ri, gi;
  brute(Q, P, K, rd, ri);
  for (int rev = 0; rev < 2; ++rev) {
    const Built b = build(P, rev != 0);
    const int64_t seen = grid_search<K>(Q, b, gd, gi);
    const bool same = ri == gi && std::memcmp(rd.data(), gd.data(), rd.size() * sizeof(double)) == 0;
    const double share = static_cast<double>(seen) / (static_cast<double>(Q.size() / 3) * static_cast<double>(P.size() / 3));
    std::printf("%-28s K=%-2d order=%d grid=%dx%dx%d visited %.3f of n0*n1 %s\n", name, K, rev, b.g.dim[0], b.g.dim[1],
                b.g.dim[2], share, same ? "equal" : "DIFFERENT");
    if (!same) {
      ++failures;
      for (size_t e = 0; e < ri.size(); ++e)
        if (ri[e] != gi[e] || std::memcmp(&rd[e], &gd[e], 8) != 0) {
          std::printf("  first difference at query %zu entry %zu: brute (%d, %.17g) grid (%d, %.17g)\n", e / K, e % K, ri[e],
                      rd[e], gi[e], gd[e]);
          break;
        }
    }
    if (share > max_visit_share) {
      std::printf("  visited share %.3f above %.3f\n", share, max_visit_share);
      ++failures;
    }
  }
}

// max_visit_share: 1 where nothing is promised. 0.5 on the evenly filled clouds at K <= 4: the plan gives 700 points
// 5 x 5 x 5 cells of about 5.6 points; a query whose K <= 4 neighbours lie within ring 1 visits at most 27 of the 125
// cells (0.22 of the cloud; fewer in the planar and collinear grids), and 0.5 leaves room for the queries that need
// ring 2 while still failing a walk that visits everything.
void check(const char* name, const Cloud& Q, const Cloud& P, double max_visit_share = 1.0) {
  check_k<1>(name, Q, P, max_visit_share);
  check_k<4>(name, Q, P, max_visit_share);
  check_k<32>(name, Q, P, 1.0);
}

// The brute-force rule (strict <, the earlier index stays in front) and the lexicographic rule leave the same list when
// the candidates arrive in ascending index order: streams with exact ties (distances drawn from `levels` values) and
// with fewer than K candidates, compared after every candidate.
template <int K>
void check_insert_rules(Rng& r, int n, size_t levels) {
  double fd[K], gd[K];
  int32_t fi[K], gi[K];
  knn_grid_clear(fd, fi);
  knn_grid_clear(gd, gi);
  bool same = true;
  for (int32_t j = 0; j < n && same; ++j) {
    const double d = 0.25 * static_cast<double>(r.below(levels));
    knn_insert_first<K>(fd, fi, d, j);
    knn_grid_insert<K>(gd, gi, d, j);
    same = std::memcmp(fd, gd, sizeof(fd)) == 0 && std::memcmp(fi, gi, sizeof(fi)) == 0;
  }
  std::printf("insertion rules K=%-2d %3d candidates, %zu distinct distances %s\n", K, n, levels, same ? "equal" : "DIFFERENT");
  if (!same) ++failures;
}

int run_rules() {
  Rng rules_rng(20250117);  // (its own stream: the clouds below keep theirs)
  for (int n : {0, 1, 5, 64})             // fewer than K = 8 candidates, and many
    for (size_t levels : {1, 3, 1000}) {  // every distance tied, ties in runs, hardly any
      check_insert_rules<1>(rules_rng, n, levels);
      check_insert_rules<2>(rules_rng, n, levels);
      check_insert_rules<8>(rules_rng, n, levels);
    }
  Rng r(20240611);
  const Cloud P = uniform_cloud(r, 700), Q = uniform_cloud(r, 150);
  check("uniform 150 x 700", Q, P, 0.5);
  check("self-search 700", P, P, 0.5);
  check("uniform shifted by 1e6", shifted(Q, 1.0e6), shifted(P, 1.0e6), 0.5);
  check("self-search shifted by 1e6", shifted(P, 1.0e6), shifted(P, 1.0e6), 0.5);
  {  // exact ties everywhere
    Cloud L;
    std::vector<int> order(512);
    for (int i = 0; i < 512; ++i) order[i] = i;
    for (int i = 511; i > 0; --i) std::swap(order[i], order[r.below(static_cast<size_t>(i) + 1)]);
    for (int o : order) {
      L.push_back(o % 8);
      L.push_back((o / 8) % 8);
      L.push_back(o / 64);
    }
    check("lattice 8x8x8 shuffled", L, L);
    Cloud T;  // every point three times
    for (int rep = 0; rep < 3; ++rep) T.insert(T.end(), P.begin(), P.begin() + 200 * 3);
    check("every point three times", T, T);
  }
  {
    Cloud F(P), Qf(Q);
    for (size_t i = 2; i < F.size(); i += 3) F[i] = 0.0;
    for (size_t i = 2; i < Qf.size(); i += 3) Qf[i] = 0.0;
    check("planar z = 0", Qf, F, 0.5);
    check("planar, queries off the plane", Q, F);
    Cloud C(P), Qc(Q);
    for (size_t i = 0; i < C.size(); i += 3) C[i + 1] = C[i + 2] = 0.5;
    for (size_t i = 0; i < Qc.size(); i += 3) Qc[i + 1] = Qc[i + 2] = 0.5;
    check("collinear", Qc, C, 0.5);
    Cloud D;  // a diagonal line: collinear, no axis of zero extent
    for (int i = 0; i < 300; ++i) {
      const double t = r.uni();
      D.push_back(t);
      D.push_back(2.0 * t);
      D.push_back(-t);
    }
    check("collinear, diagonal", D, D);
  }
  {
    Cloud I(40 * 3, 0.5);
    check("40 identical points", I, I);
    check("40 identical, other queries", Q, I);
  }
  {
    Cloud far(Q);
    for (size_t i = 0; i < far.size(); ++i) far[i] = (i % 2 ? -1.0 : 1.0) * (5.0 + 100.0 * far[i]);
    check("queries well outside the box", far, P);
  }
  {
    const Cloud three(P.begin(), P.begin() + 9);
    check("3 points, K larger", Q, three);
    const Cloud one(P.begin(), P.begin() + 3);
    check("1 point", Q, one);
  }
  {  // two clusters of width 1e-3 a unit apart: the grid cannot separate them; slow there, never wrong
    Cloud W;
    for (int i = 0; i < 400; ++i) {
      const double base = i % 2 ? 1.0 : 0.0;
      for (int a = 0; a < 3; ++a) W.push_back(base + 1.0e-3 * r.uni());
    }
    check("two clusters of width 1e-3", W, W);
  }
  std::printf(failures ? "knn grid rules FAILED (%d)\n" : "knn grid rules ok\n", failures);
  return failures ? 1 : 0;
}

int run_plan() {
  int bad = 0;
  auto expect = [&](bool ok, const std::string& what) {
    if (!ok) {
      std::printf("plan: %s\n", what.c_str());
      ++bad;
    }
  };
  {  // zero-extent axes have dim 1 (planar, collinear, identical), whatever n1
    const double lo[3] = {0.0, -1.0, 2.0};
    for (int64_t n1 : {1, 2, 40, 1000, 100000, 10000000}) {
      const double planar[3] = {1.0, 3.0, 2.0}, line[3] = {0.0, 3.0, 2.0}, point[3] = {0.0, -1.0, 2.0};
      KnnGrid g = knn_grid_plan(lo, planar, n1);
      expect(g.dim[2] == 1 && g.inv[2] == 0.0, "planar cloud: dim[2] != 1 at n1 = " + std::to_string(n1));
      if (n1 >= 1000) expect(g.dim[0] > 1 && g.dim[1] > 1, "planar cloud: no cells in the plane at n1 = " + std::to_string(n1));
      g = knn_grid_plan(lo, line, n1);
      expect(g.dim[0] == 1 && g.dim[2] == 1, "collinear cloud: dims at n1 = " + std::to_string(n1));
      if (n1 >= 1000) expect(g.dim[1] > 1, "collinear cloud: one slab at n1 = " + std::to_string(n1));
      g = knn_grid_plan(lo, point, n1);
      expect(g.dim[0] == 1 && g.dim[1] == 1 && g.dim[2] == 1, "identical points: dims at n1 = " + std::to_string(n1));
    }
  }
  {  // cells <= max(1, n1), n1 from 1 to 10^7, over boxes of every shape; factors finite and non-negative
    Rng r(7);
    int64_t n1 = 1;
    while (n1 <= 10000000) {
      for (int t = 0; t < 40; ++t) {
        double lo[3], hi[3];
        for (int a = 0; a < 3; ++a) {
          lo[a] = (r.uni() - 0.5) * std::pow(10.0, 12.0 * r.uni() - 6.0);
          const double e = (t % 5 == a) ? 0.0 : std::pow(10.0, 18.0 * r.uni() - 12.0);
          hi[a] = lo[a] + e;
        }
        const KnnGrid g = knn_grid_plan(lo, hi, n1);
        const int64_t cells = knn_grid_cells(g);
        expect(cells >= 1 && cells <= std::max<int64_t>(1, n1), "cells " + std::to_string(cells) + " at n1 = " + std::to_string(n1));
        for (int a = 0; a < 3; ++a) {
          expect(g.dim[a] >= 1 && std::isfinite(g.inv[a]) && g.inv[a] >= 0.0, "dim / factor at n1 = " + std::to_string(n1));
          expect(!(hi[a] == lo[a]) || g.dim[a] == 1, "zero extent with dim > 1 at n1 = " + std::to_string(n1));
          expect(knn_grid_cell(hi[a], g.lo[a], g.inv[a], g.dim[a]) <= g.dim[a] - 1, "cell of the maximum");
          expect(knn_grid_cell(lo[a], g.lo[a], g.inv[a], g.dim[a]) == 0, "cell of the minimum");
        }
        expect(g.off[0] == 0 && g.off[1] == g.dim[0] && g.off[2] == g.dim[0] + g.dim[1], "offsets");
      }
      n1 = n1 < 64 ? n1 + 1 : n1 * 3 + 1;
    }
    const double lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};
    expect(knn_grid_cells(knn_grid_plan(lo, hi, 10000000)) <= 10000000, "cells at 10^7");
    expect(knn_grid_cells(knn_grid_plan(lo, hi, 10000000)) >= 1000000, "a 10^7 cube gets a real grid");
    const double huge_lo[3] = {-1.0e308, 0, 0}, huge_hi[3] = {1.0e308, 1, 1}, tiny_hi[3] = {4.9e-324, 1, 1};
    expect(knn_grid_plan(huge_lo, huge_hi, 1000).dim[0] == 1, "an extent that overflows");
    const KnnGrid t = knn_grid_plan(lo, tiny_hi, 1000);
    expect(std::isfinite(t.inv[0]) && t.dim[0] >= 1, "an extent of one denormal");
  }
  {  // the cell of a coordinate is monotone, clamping included
    const double lo[3] = {1.0e6, 1.0e6, 1.0e6}, hi[3] = {1.0e6 + 1.0, 1.0e6 + 1.0, 1.0e6 + 1.0};
    const KnnGrid g = knn_grid_plan(lo, hi, 5000);
    int32_t prev = 0;
    for (int i = -2000; i <= 12000; ++i) {
      const double x = 1.0e6 + 1.0e-4 * i;
      const int32_t c = knn_grid_cell(x, g.lo[0], g.inv[0], g.dim[0]);
      expect(c >= prev && c >= 0 && c < g.dim[0], "cell not monotone at " + std::to_string(i));
      prev = c;
    }
    expect(knn_grid_cell(-INFINITY, g.lo[0], g.inv[0], g.dim[0]) == 0, "cell of -inf");
    expect(knn_grid_cell(INFINITY, g.lo[0], g.inv[0], g.dim[0]) == g.dim[0] - 1, "cell of +inf");
    expect(knn_grid_cell(NAN, g.lo[0], g.inv[0], g.dim[0]) == 0, "cell of NaN");
  }
  std::printf(bad ? "knn grid plan FAILED (%d)\n" : "knn grid plan ok\n", bad);
  return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "plan") return run_plan();
  return run_rules() | run_plan();
}
