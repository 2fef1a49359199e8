// CPU test of the sparse input checks (clipper_amd/csrc/host_csc_input.hpp): every refusal of check_csc / upper_only /
// symmetric_lists with its message, the count of entries below the diagonal, the strictly upper input that is not
// copied, the C == pattern(M) test, the symmetric lists of small matrices against answers written by hand, and the
// value checks of both setters (non-finite values, values that round to fp32 infinity).
//   g++ -std=c++17 -O1 -I clipper_amd/csrc tests/cpp/test_csc_input.cpp -o /tmp/t && /tmp/t
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "host_csc_input.hpp"

using namespace clipper_csc;

#define REQUIRE(c)                                          \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED %s at line %d\n", #c, __LINE__); \
      std::exit(1);                                         \
    }                                                       \
  } while (0)

struct Mat {  // a matrix written out by hand, CSC
  std::vector<int64_t> cp;
  std::vector<int32_t> ri;
  std::vector<double> va;
  CscRef ref() const { return CscRef{cp.data(), ri.data(), va.data()}; }
};

static void test_check_csc() {
  const int64_t m = 3;
  Mat ok{{0, 0, 1, 3}, {0, 0, 1}, {0.5, 0.25, 0.75}};
  REQUIRE(check_csc("M", m, ok.ref()).empty());
  Mat first = ok;
  first.cp[0] = 1;
  REQUIRE(check_csc("M", m, first.ref()) == "M: colptr[0] must be 0");
  Mat dec = ok;
  dec.cp[1] = 1;
  dec.cp[2] = 0;
  REQUIRE(check_csc("C", m, dec.ref()) == "C: colptr decreases at column 1");
  Mat null_rows = ok;
  REQUIRE(check_csc("M", m, CscRef{null_rows.cp.data(), nullptr, null_rows.va.data()}) == "M: null CSC arrays");
  REQUIRE(check_csc("M", m, CscRef{null_rows.cp.data(), null_rows.ri.data(), nullptr}) == "M: null CSC arrays");
  Mat empty{{0, 0, 0, 0}, {}, {}};
  REQUIRE(check_csc("M", m, CscRef{empty.cp.data(), nullptr, nullptr}).empty());  // (no entries: no arrays needed)
  Mat high = ok;
  high.ri[2] = 3;
  REQUIRE(check_csc("M", m, high.ref()) == "M: row index 3 out of range at entry 2");
  Mat neg = ok;
  neg.ri[0] = -1;
  REQUIRE(check_csc("C", m, neg.ref()) == "C: row index -1 out of range at entry 0");
}

static void test_upper_only() {
  const int64_t m = 3;
  // strictly upper (what Eigen hands over): left as it is, nothing copied
  Mat up{{0, 0, 1, 3}, {0, 0, 1}, {0.5, 0.25, 0.75}};
  CscRef a = up.ref();
  CscLists out;
  int64_t dropped = 0;
  REQUIRE(upper_only("M", m, a, out, dropped).empty());
  REQUIRE(a.cp == up.cp.data() && a.ri == up.ri.data() && a.va == up.va.data());
  REQUIRE(out.cp.empty() && dropped == 0);
  // both triangles, a zero diagonal: the lower copies dropped and counted, the diagonal left out
  //   column 0: rows 0 (0.0), 1 (0.5), 2 (0.25); column 1: rows 0 (0.5), 2 (0.75); column 2: rows 0, 1
  Mat full{{0, 3, 5, 7}, {0, 1, 2, 0, 2, 0, 1}, {0.0, 0.5, 0.25, 0.5, 0.75, 0.25, 0.75}};
  a = full.ref();
  REQUIRE(upper_only("M", m, a, out, dropped).empty());
  REQUIRE(dropped == 3);
  REQUIRE(a.cp == out.cp.data() && a.ri == out.ri.data() && a.va == out.va.data());
  REQUIRE((out.cp == std::vector<int64_t>{0, 0, 1, 3}));
  REQUIRE((out.ri == std::vector<int32_t>{0, 0, 1}));
  REQUIRE((out.va == std::vector<double>{0.5, 0.25, 0.75}));
  // the count adds up over M and C
  Mat lower{{0, 2, 3, 3}, {1, 2, 2}, {1.0, 1.0, 1.0}};
  CscRef b = lower.ref();
  CscLists out2;
  REQUIRE(upper_only("C", m, b, out2, dropped).empty());
  REQUIRE(dropped == 6);
  REQUIRE((out2.cp == std::vector<int64_t>{0, 0, 0, 0}) && out2.ri.empty());
  // a stored non-zero diagonal is refused
  Mat diag{{0, 0, 2, 3}, {0, 1, 1}, {0.5, 2.0, 0.75}};
  CscRef c = diag.ref();
  CscLists out3;
  int64_t d3 = 0;
  REQUIRE(upper_only("M", m, c, out3, d3) ==
          "M: a stored diagonal entry (1,1) — the matrices must not have diagonal values set");
}

static void test_is_pattern() {
  const int64_t m = 3;
  Mat M{{0, 0, 1, 3}, {0, 0, 1}, {0.5, 0.25, 0.75}};
  Mat C{{0, 0, 1, 3}, {0, 0, 1}, {1.0, 1.0, 1.0}};
  REQUIRE(is_pattern(m, M.ref(), C.ref()));
  Mat C2 = C;
  C2.va[1] = 0.5;  // a weight other than 1
  REQUIRE(!is_pattern(m, M.ref(), C2.ref()));
  Mat M0 = M;
  M0.va[2] = 0.0;  // a stored zero in M: C holds a constraint M does not
  REQUIRE(!is_pattern(m, M0.ref(), C.ref()));
  Mat C3{{0, 0, 1, 2}, {0, 0}, {1.0, 1.0}};  // another structure
  REQUIRE(!is_pattern(m, M.ref(), C3.ref()));
  Mat C4{{0, 0, 1, 3}, {0, 1, 0}, {1.0, 1.0, 1.0}};  // same counts, other rows
  REQUIRE(!is_pattern(m, M.ref(), C4.ref()));
  Mat e{{0, 0, 0, 0}, {}, {}};
  REQUIRE(is_pattern(m, CscRef{e.cp.data(), nullptr, nullptr}, CscRef{e.cp.data(), nullptr, nullptr}));
}

static void test_symmetric_lists() {
  // 4 x 4, strictly upper with ascending rows: (0,1) 1, (0,2) 2, (1,2) 3, (0,3) 4, (2,3) 5
  const int64_t m = 4;
  Mat U{{0, 0, 1, 3, 5}, {0, 0, 1, 0, 2}, {1, 2, 3, 4, 5}};
  CscLists L;
  REQUIRE(symmetric_lists(m, U.ref(), L).empty());
  REQUIRE((L.cp == std::vector<int64_t>{0, 3, 5, 8, 10}));
  REQUIRE((L.ri == std::vector<int32_t>{1, 2, 3, 0, 2, 0, 1, 3, 0, 2}));
  REQUIRE((L.va == std::vector<double>{1, 2, 4, 1, 3, 2, 3, 5, 4, 5}));
  // the same entries with unsorted rows inside the columns: the same lists
  Mat V{{0, 0, 1, 3, 5}, {0, 1, 0, 2, 0}, {1, 3, 2, 5, 4}};
  CscLists L2;
  REQUIRE(symmetric_lists(m, V.ref(), L2).empty());
  REQUIRE(L2.cp == L.cp && L2.ri == L.ri && L2.va == L.va);
  // an empty matrix
  Mat E{{0, 0, 0, 0, 0}, {}, {}};
  CscLists L3;
  REQUIRE(symmetric_lists(m, CscRef{E.cp.data(), nullptr, nullptr}, L3).empty());
  REQUIRE((L3.cp == std::vector<int64_t>{0, 0, 0, 0, 0}) && L3.ri.empty() && L3.va.empty());
  // (0,1) stored twice in column 1: refused, found in column 0 (its mirror, the first column sorted)
  Mat D{{0, 0, 2, 2, 2}, {0, 0}, {1, 1}};
  CscLists L4;
  REQUIRE(symmetric_lists(m, D.ref(), L4) == "entry (1,0) is stored more than once");
}

static void test_check_values() {
  const int64_t m = 3;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double first_inf = 0x1.ffffffp+127;  // FLT_MAX plus half its last place: the tie goes to even, which is infinity
  const double last_finite = std::nextafter(first_inf, 0.0);
  REQUIRE(std::isinf(static_cast<float>(first_inf)) && static_cast<float>(last_finite) == std::numeric_limits<float>::max());
  // CSC, strictly upper: (0,1) (0,2) (1,2)
  Mat ok{{0, 0, 1, 3}, {0, 0, 1}, {5e-324, -1e-50, last_finite}};
  for (bool f32 : {false, true}) REQUIRE(check_values_csc("M", m, ok.ref(), f32).empty());
  Mat a = ok;
  a.va[1] = nan;
  for (bool f32 : {false, true}) REQUIRE(check_values_csc("M", m, a.ref(), f32) == "M: entry (0,2) is not finite (nan)");
  a.va[1] = inf;
  REQUIRE(check_values_csc("C", m, a.ref(), false) == "C: entry (0,2) is not finite (inf)");
  a.va[1] = -inf;
  REQUIRE(check_values_csc("M", m, a.ref(), true) == "M: entry (0,2) is not finite (-inf)");
  a = ok;
  a.va[2] = first_inf;
  REQUIRE(check_values_csc("M", m, a.ref(), false).empty());  // an fp64 storage holds it
  REQUIRE(check_values_csc("M", m, a.ref(), true) ==
          "M: entry (1,2) = 3.4028235677973366e+38 rounds to infinity in fp32 storage");
  a.va[2] = -first_inf;
  REQUIRE(check_values_csc("M", m, a.ref(), true) ==
          "M: entry (1,2) = -3.4028235677973366e+38 rounds to infinity in fp32 storage");
  a.va[2] = -last_finite;
  REQUIRE(check_values_csc("M", m, a.ref(), true).empty());
  // entries on and below the diagonal are never read: whatever they hold (column 0: rows 1, 2; column 1: row 1)
  Mat low{{0, 2, 4, 4}, {1, 2, 0, 1}, {nan, inf, 0.5, nan}};
  REQUIRE(check_values_csc("M", m, low.ref(), true).empty());
  // dense, column-major 3 x 3: A[i + j * m] is read for i < j only
  std::vector<double> D{nan, nan, inf, 5e-324, nan, -inf, -1e-50, last_finite, nan};
  for (bool f32 : {false, true}) REQUIRE(check_values_dense_upper("M", m, D.data(), f32).empty());
  std::vector<double> E = D;
  E[0 + 2 * 3] = nan;
  REQUIRE(check_values_dense_upper("M", m, E.data(), true) == "M: entry (0,2) is not finite (nan)");
  E[0 + 2 * 3] = -inf;
  REQUIRE(check_values_dense_upper("C", m, E.data(), false) == "C: entry (0,2) is not finite (-inf)");
  E = D;
  E[0 + 1 * 3] = inf;
  REQUIRE(check_values_dense_upper("M", m, E.data(), false) == "M: entry (0,1) is not finite (inf)");
  E = D;
  E[1 + 2 * 3] = first_inf;
  REQUIRE(check_values_dense_upper("M", m, E.data(), false).empty());
  REQUIRE(check_values_dense_upper("M", m, E.data(), true) ==
          "M: entry (1,2) = 3.4028235677973366e+38 rounds to infinity in fp32 storage");
  const double one = 1.0;
  REQUIRE(check_values_dense_upper("M", 1, &one, true).empty());  // m = 1: no pair
}

int main() {
  test_check_values();
  test_check_csc();
  test_upper_only();
  test_is_pattern();
  test_symmetric_lists();
  std::printf("csc input ok\n");
  return 0;
}
