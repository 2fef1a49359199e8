// CPU test of the matcher's shared filter rules (clipper_amd/csrc/match_rules.hpp): the header the device's
// k_match_select and the host's clipper_match::select both read compiles with g++ alone, and, driven by a plain loop
// in the shape of the kernel's two passes (count per query, exclusive scan, rows written at the offsets), it reproduces
// clipper_match::select row for row and bit for bit: on lists written by hand (the single-point rule, a bound landing
// exactly on a distance, equality in the ratio test, a mutual hit at the last position, every row dropped, none
// dropped) and on random lists with ties over every knn, with and without each filter.
//   g++ -std=c++17 -O1 -I clipper_amd/csrc tests/cpp/test_match_rules.cpp -o /tmp/t && /tmp/t
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "match_rules.hpp"  // first, alone: it must stand without the host header

#include "host_match_select.hpp"

using namespace clipper_match;

#define REQUIRE(c)                                          \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED %s at line %d\n", #c, __LINE__); \
      std::exit(1);                                         \
    }                                                       \
  } while (0)

// the device's order of work on the host: pass 1 counts, the scan gives each query its first row, pass 2 writes
static Rows by_the_rules(const Params& prm, const Lists& fwd, const Lists& bwd) {
  std::vector<int32_t> cnt(static_cast<size_t>(fwd.n)), off(static_cast<size_t>(fwd.n) + 1);
  for (int pass = 0; pass < 2; ++pass) {
    Rows out;
    if (pass == 1) {
      out.i.resize(static_cast<size_t>(off[fwd.n]));
      out.j.resize(out.i.size());
      out.sqd.resize(out.i.size());
    }
    for (int64_t i = fwd.n - 1; i >= 0; --i) {  // (any order of the queries: the offsets place the rows)
      const int32_t* nn = fwd.idx + i * fwd.stride;
      const double* sd = fwd.sqd + i * fwd.stride;
      int32_t kept = 0;
      if (query_passes(prm, nn, sd))
        for (int k = 0; k < prm.knn; ++k) {
          if (!entry_kept(prm, i, k, nn, sd, bwd.idx, bwd.stride)) continue;
          if (pass == 1) {
            const size_t r = static_cast<size_t>(off[i] + kept);
            out.i[r] = static_cast<int32_t>(i), out.j[r] = nn[k], out.sqd[r] = sd[k];
          }
          ++kept;
        }
      if (pass == 0) cnt[i] = kept;
    }
    if (pass == 1) return out;
    off[0] = 0;
    for (int64_t i = 0; i < fwd.n; ++i) off[i + 1] = off[i] + cnt[i];
  }
  return {};
}

static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) {
  if (a.size() != b.size()) return false;
  for (size_t k = 0; k < a.size(); ++k) {
    uint64_t x, y;
    std::memcpy(&x, &a[k], 8), std::memcpy(&y, &b[k], 8);
    if (x != y) return false;
  }
  return true;
}

static size_t check(const Params& prm, const Lists& fwd, const Lists& bwd) {
  const Rows want = select(prm, fwd, bwd), got = by_the_rules(prm, fwd, bwd);
  REQUIRE(got.i == want.i && got.j == want.j && same_bits(got.sqd, want.sqd));
  return want.i.size();
}

// 4 queries against 3 points, lists of 2 (tests/cpp/test_match_select.cpp's). Query 3 has no second neighbour.
static const int32_t FI[8] = {0, 1, 0, 2, 1, 2, 2, -1};
static const double FD[8] = {0.1, 0.5, 0.2, 0.3, 0.4, 0.4, 0.05, 1e300};
static const int32_t BI[6] = {0, 1, 2, 0, 3, 2};
static const double BD[6] = {0.1, 0.2, 0.4, 0.5, 0.05, 0.4};
static const Lists FWD{FI, FD, 4, 2}, BWD{BI, BD, 3, 2};

static void test_by_hand() {
  REQUIRE(check(Params{2, 0, 0.0, 0.0}, FWD, BWD) == 7);   // nothing but the missing neighbour is dropped
  REQUIRE(check(Params{2, 0, 0.0, 0.4}, FWD, BWD) == 6);   // the bound lands exactly on two distances: kept
  REQUIRE(check(Params{2, 0, 0.0, std::nextafter(0.4, 0.0)}, FWD, BWD) == 4);
  REQUIRE(check(Params{2, 1, 0.0, 0.0}, FWD, BWD) == 6);   // mutual hits at the last position of a backward list
  REQUIRE(check(Params{1, 0, 0.5, 0.0}, FWD, BWD) == 2);   // ratio; the query without a second neighbour passes
  REQUIRE(check(Params{1, 1, 0.5, 0.08}, FWD, BWD) == 1);  // all together
  REQUIRE(check(Params{1, 0, 0.0, 0.01}, FWD, BWD) == 0);  // every row filtered out
  // ratio 0.5: 0.25 < (0.5 * 0.5) * 1.0 is false (dropped); the next smaller double passes
  const int32_t fi[4] = {0, 1, 1, 0};
  const double fd[4] = {0.25, 1.0, std::nextafter(0.25, 0.0), 1.0};
  const Lists fwd{fi, fd, 2, 2}, none{nullptr, nullptr, 0, 0};
  REQUIRE(check(Params{1, 0, 0.5, 0.0}, fwd, none) == 1);
  // the single-point rule: the other set has one point, every second entry is -1
  const int32_t si[6] = {0, -1, 0, -1, 0, -1};
  const double sdq[6] = {3.0, 1e300, 0.0, 1e300, 7.5, 1e300};
  const int32_t sb[2] = {1, 0};
  const double sbd[2] = {0.0, 3.0};
  const Lists sf{si, sdq, 3, 2}, sbw{sb, sbd, 1, 2};
  REQUIRE(check(Params{1, 0, 0.8, 0.0}, sf, sbw) == 3);
  REQUIRE(check(Params{1, 1, 0.8, 0.0}, sf, sbw) == 1);    // knn = 1: only query 1 is the point's nearest
  REQUIRE(check(Params{1, 0, 0.8, 3.0}, sf, sbw) == 2);
}

// random lists: distances drawn from a few values so that they tie, indices any; the rules do not care whether the
// lists could have come from a search
static void test_random() {
  uint64_t s = 12345;
  auto next = [&]() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(s >> 33);
  };
  size_t total = 0;
  for (int64_t n0 : {1, 63, 64, 65, 257})
    for (int64_t n1 : {1, 7, 64})
      for (int knn : {1, 2, 8}) {
        const int stride = knn == 1 ? 2 : knn;
        std::vector<int32_t> fi(static_cast<size_t>(n0 * stride)), bi(static_cast<size_t>(n1 * knn));
        std::vector<double> fd(fi.size()), bd(bi.size());
        for (int64_t i = 0; i < n0; ++i)
          for (int k = 0; k < stride; ++k) {
            const bool have = k < n1;
            fi[static_cast<size_t>(i * stride + k)] = have ? static_cast<int32_t>(next() % n1) : -1;
            fd[static_cast<size_t>(i * stride + k)] = have ? 0.125 * static_cast<double>(next() % 5 + k) : 1e300;
          }
        for (size_t e = 0; e < bi.size(); ++e) bi[e] = (next() % 4 == 0) ? -1 : static_cast<int32_t>(next() % n0);
        const Lists fwd{fi.data(), fd.data(), n0, stride}, bwd{bi.data(), bd.data(), n1, knn};
        for (int mutual : {0, 1})
          for (double ratio : {0.0, 0.8})
            for (double bound : {0.0, 0.25}) {
              if (ratio > 0.0 && knn != 1) continue;
              total += check(Params{knn, mutual, ratio, bound}, fwd, bwd);
            }
      }
  REQUIRE(total > 1000);
}

int main() {
  test_by_hand();
  test_random();
  std::printf("match rules ok\n");
  return 0;
}
