// CPU test of the host side of descriptor matching (clipper_amd/csrc/host_match_select.hpp): the filters on lists
// written by hand — each alone and all together, the ratio test without a second neighbour, equality at the max_sqdist
// bound (kept) and in the ratio comparison (dropped), a mutual hit at the last position of the backward list, the row
// order — the column-major output with its capacity check, the zero padding, and every refusal with its message.
//   g++ -std=c++17 -O1 -I clipper_amd/csrc tests/cpp/test_match_select.cpp -o /tmp/t && /tmp/t
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "host_match_select.hpp"

using namespace clipper_match;

#define REQUIRE(c)                                          \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED %s at line %d\n", #c, __LINE__); \
      std::exit(1);                                         \
    }                                                       \
  } while (0)

typedef std::vector<std::pair<int, int>> Pairs;

static Pairs pairs(const Rows& r) {
  Pairs p;
  for (size_t k = 0; k < r.i.size(); ++k) p.emplace_back(r.i[k], r.j[k]);
  return p;
}

// 4 queries against 3 points, lists of 2. Query 3 has no second neighbour.
static const int32_t FI[8] = {0, 1, 0, 2, 1, 2, 2, -1};
static const double FD[8] = {0.1, 0.5, 0.2, 0.3, 0.4, 0.4, 0.05, 1e300};
// the backward lists of the 3 points: query 0 is the LAST entry of point 1's, query 1 of point 0's
static const int32_t BI[6] = {0, 1, 2, 0, 3, 2};
static const double BD[6] = {0.1, 0.2, 0.4, 0.5, 0.05, 0.4};
static const Lists FWD{FI, FD, 4, 2}, BWD{BI, BD, 3, 2};

static void test_filters_knn2() {
  Rows r = select(Params{2, 0, 0.0, 0.0}, FWD, BWD);  // nothing but the missing neighbour is dropped; i, then k ascending
  REQUIRE(pairs(r) == (Pairs{{0, 0}, {0, 1}, {1, 0}, {1, 2}, {2, 1}, {2, 2}, {3, 2}}));
  REQUIRE(r.sqd == (std::vector<double>{0.1, 0.5, 0.2, 0.3, 0.4, 0.4, 0.05}));
  r = select(Params{2, 0, 0.0, 0.4}, FWD, BWD);  // the bound itself is kept (0.4 <= 0.4), 0.5 is not
  REQUIRE(pairs(r) == (Pairs{{0, 0}, {1, 0}, {1, 2}, {2, 1}, {2, 2}, {3, 2}}));
  r = select(Params{2, 0, 0.0, -1.0}, FWD, BWD);  // <= 0: off
  REQUIRE(r.i.size() == 7);
  r = select(Params{2, 1, 0.0, 0.0}, FWD, BWD);  // (0,1) and (1,0) are hits at the last position; (1,2) is no hit
  REQUIRE(pairs(r) == (Pairs{{0, 0}, {0, 1}, {1, 0}, {2, 1}, {2, 2}, {3, 2}}));
  r = select(Params{2, 1, 0.0, 0.4}, FWD, BWD);
  REQUIRE(pairs(r) == (Pairs{{0, 0}, {1, 0}, {2, 1}, {2, 2}, {3, 2}}));
  REQUIRE(r.sqd == (std::vector<double>{0.1, 0.2, 0.4, 0.4, 0.05}));
}

static void test_filters_knn1() {
  // knn = 1 on the same lists: the second entries are read by the ratio test only
  Rows r = select(Params{1, 0, 0.0, 0.0}, FWD, BWD);
  REQUIRE(pairs(r) == (Pairs{{0, 0}, {1, 0}, {2, 1}, {3, 2}}));
  // 0.1 < 0.25 * 0.5; 0.2 >= 0.25 * 0.3; 0.4 >= 0.25 * 0.4; no second neighbour: passes
  r = select(Params{1, 0, 0.5, 0.0}, FWD, BWD);
  REQUIRE(pairs(r) == (Pairs{{0, 0}, {3, 2}}));
  // mutual with knn = 1 reads the FIRST backward entry only: query 1 is second in point 0's list
  r = select(Params{1, 1, 0.0, 0.0}, FWD, BWD);
  REQUIRE(pairs(r) == (Pairs{{0, 0}, {2, 1}, {3, 2}}));
  r = select(Params{1, 1, 0.5, 0.08}, FWD, BWD);  // all together
  REQUIRE(pairs(r) == (Pairs{{3, 2}}));
  REQUIRE(r.sqd == (std::vector<double>{0.05}));
  REQUIRE(forward_len(Params{1, 1, 0.5, 0.0}) == 2 && forward_len(Params{1, 1, 0.0, 0.0}) == 1);
  REQUIRE(forward_len(Params{8, 0, 0.0, 0.0}) == 8);
}

static void test_ratio_equality_is_dropped() {
  // ratio 0.5: (ratio * ratio) * 1.0 == 0.25 exactly. 0.25 < 0.25 is false: dropped; the next smaller double passes.
  const int32_t fi[4] = {0, 1, 1, 0};
  const double fd[4] = {0.25, 1.0, std::nextafter(0.25, 0.0), 1.0};
  const Lists fwd{fi, fd, 2, 2}, none{nullptr, nullptr, 0, 0};
  Rows r = select(Params{1, 0, 0.5, 0.0}, fwd, none);
  REQUIRE(pairs(r) == (Pairs{{1, 1}}));
  // the comparison is the one written in the contract, in fp64: sqd_0 < (ratio * ratio) * sqd_1
  const double ratio = 0.8, s1 = 0.3;
  const double edge = (ratio * ratio) * s1;
  const double gd[4] = {edge, s1, std::nextafter(edge, 0.0), s1};
  r = select(Params{1, 0, ratio, 0.0}, Lists{fi, gd, 2, 2}, none);
  REQUIRE(pairs(r) == (Pairs{{1, 1}}));
}

static void test_emit() {
  const Rows r = select(Params{2, 0, 0.0, 0.0}, FWD, BWD);
  std::vector<int32_t> A(14, -7);
  std::vector<double> sq(7, -1.0);
  REQUIRE(emit(r, A.data(), sq.data(), 7).empty());
  REQUIRE(A == (std::vector<int32_t>{0, 0, 1, 1, 2, 2, 3, 0, 1, 0, 2, 1, 2, 2}));  // column-major 7 x 2
  REQUIRE(sq == r.sqd);
  REQUIRE(emit(r, A.data(), nullptr, 8).empty());  // no distances wanted; spare capacity
  REQUIRE(emit(r, A.data(), sq.data(), 6) == "capacity 6 < 7 associations");
  REQUIRE(emit(r, A.data(), sq.data(), -1) == "capacity -1 < 7 associations");
  REQUIRE(emit(r, nullptr, nullptr, 7) == "null association buffer");
  REQUIRE(emit(Rows{}, nullptr, nullptr, 0).empty());  // nothing kept: nothing written
}

static void test_refusals() {
  const double F[6] = {0, 1, 2, 3, 4, 5};
  const Params ok{1, 1, 0.0, 0.0};
  REQUIRE(check_args(F, 2, F, 3, 2, &ok).empty());
  REQUIRE(check_args(nullptr, 2, F, 3, 2, &ok) == "null descriptor array");
  REQUIRE(check_args(F, 2, nullptr, 3, 2, &ok) == "null descriptor array");
  REQUIRE(check_args(F, 2, F, 3, 2, nullptr) == "null match parameters");
  REQUIRE(check_args(F, 0, F, 3, 2, &ok) == "both descriptor sets need at least one point (n0 = 0, n1 = 3)");
  REQUIRE(check_args(F, 2, F, -1, 2, &ok) == "both descriptor sets need at least one point (n0 = 2, n1 = -1)");
  REQUIRE(check_args(F, int64_t(1) << 31, F, 3, 2, &ok) == "more than 2^31 - 1 points in a descriptor set");
  REQUIRE(check_args(F, 2, F, 3, 0, &ok) == "descriptors must have 1..64 coordinates (d = 0)");
  REQUIRE(check_args(F, 2, F, 3, 65, &ok) == "descriptors must have 1..64 coordinates (d = 65)");
  REQUIRE(check_args(F, 1, F, 1, 1, &ok).empty() && check_args(F, 1, F, 1, 64, &ok).empty());
  Params p = ok;
  p.knn = 0;
  REQUIRE(check_args(F, 2, F, 3, 2, &p) == "knn must be in 1..8 (knn = 0)");
  p.knn = 9;
  REQUIRE(check_args(F, 2, F, 3, 2, &p) == "knn must be in 1..8 (knn = 9)");
  p.knn = 8;
  REQUIRE(check_args(F, 2, F, 3, 2, &p).empty());
  p = ok;
  p.ratio = -0.1;
  REQUIRE(check_args(F, 2, F, 3, 2, &p) == "ratio must be 0 (off) or in (0, 1) (ratio = -0.1)");
  p.ratio = 1.0;
  REQUIRE(check_args(F, 2, F, 3, 2, &p) == "ratio must be 0 (off) or in (0, 1) (ratio = 1)");
  p.ratio = std::numeric_limits<double>::quiet_NaN();
  REQUIRE(check_args(F, 2, F, 3, 2, &p) == "ratio must be 0 (off) or in (0, 1) (ratio = nan)");
  p.ratio = 0.8;
  REQUIRE(check_args(F, 2, F, 3, 2, &p).empty());
  p.knn = 2;
  REQUIRE(check_args(F, 2, F, 3, 2, &p) == "the ratio test needs knn == 1 (knn = 2)");
  p = ok;
  p.max_sqdist = std::numeric_limits<double>::quiet_NaN();
  REQUIRE(check_args(F, 2, F, 3, 2, &p) == "max_sqdist is not a number");

  REQUIRE(check_finite("F0", F, 3, 2).empty());
  double G[6] = {0, 1, 2, 3, 4, 5};
  G[3] = std::numeric_limits<double>::quiet_NaN();
  REQUIRE(check_finite("F0", G, 3, 2) == "F0: non-finite value at coordinate 1 of descriptor 1");
  G[3] = 3;
  G[4] = -std::numeric_limits<double>::infinity();
  REQUIRE(check_finite("F1", G, 2, 3) == "F1: non-finite value at coordinate 1 of descriptor 1");
  REQUIRE(check_finite("F1", G, 2, 2).empty());  // (only the first n * d values are read)
}

static void test_padding() {
  const double F[6] = {1, 2, 3, 4, 5, 6};
  REQUIRE(pad_rows(F, 2, 3, 8) == (std::vector<double>{1, 2, 3, 0, 0, 0, 0, 0, 4, 5, 6, 0, 0, 0, 0, 0}));
  REQUIRE(pad_rows(F, 3, 2, 2) == (std::vector<double>{1, 2, 3, 4, 5, 6}));
}

int main() {
  test_filters_knn2();
  test_filters_knn1();
  test_ratio_equality_is_dropped();
  test_emit();
  test_refusals();
  test_padding();
  std::printf("match select ok\n");
  return 0;
}
