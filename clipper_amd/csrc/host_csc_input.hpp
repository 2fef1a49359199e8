// host_csc_input.hpp — the caller's sparse (M, C) as clipper_hip_set_sparse reads them: the structure checks, the upper
// triangle, the C == pattern(M) test and the symmetric lists the slices are packed from; and the value check of both
// setters (check_values_csc, check_values_dense_upper). Pure host code (no HIP):
// tests/cpp/test_csc_input.cpp compiles it with g++ alone. A refusal comes back as its message (empty: accepted); the
// caller hands it to fail(). Nothing here catches std::bad_alloc: it reaches the entry point's guard.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

namespace clipper_csc {

// m columns in compressed sparse columns, as handed over: colptr[m + 1], rows and values [colptr[m]]
struct CscRef {
  const int64_t* cp;
  const int32_t* ri;
  const double* va;
};

// the same, held here (a filtered copy, or the symmetric lists)
struct CscLists {
  std::vector<int64_t> cp;
  std::vector<int32_t> ri;
  std::vector<double> va;
};

template <typename... Args>
std::string format(const char* fmt, Args... args) {
  char buf[512];
  std::snprintf(buf, sizeof(buf), fmt, args...);
  return buf;
}

// the caller's arrays are not trusted: colptr starts at 0 and never decreases, every row is in range
std::string check_csc(const char* what, int64_t m, const CscRef& a) {
  if (a.cp[0] != 0) return format("%s: colptr[0] must be 0", what);
  for (int64_t c = 0; c < m; ++c)
    if (a.cp[c + 1] < a.cp[c]) return format("%s: colptr decreases at column %lld", what, static_cast<long long>(c));
  const int64_t nnz = a.cp[m];
  if (nnz > 0 && (!a.ri || !a.va)) return format("%s: null CSC arrays", what);
  for (int64_t p = 0; p < nnz; ++p)
    if (a.ri[p] < 0 || a.ri[p] >= m)
      return format("%s: row index %d out of range at entry %lld", what, a.ri[p], static_cast<long long>(p));
  return {};
}

// The reference keeps what it is handed (clipper.cpp:162-166) and reads it through selfadjointView<Eigen::Upper>
// (clipper.cpp:194-271): an entry BELOW the diagonal is never read — a full symmetric SpAffinity counts through its
// upper half, a lower-triangular one is an empty matrix — and a stored diagonal would count once on top of the
// implicit identity. Same here for the lower triangle (dropped, whatever it holds, and counted in `dropped_below`);
// the diagonal is implicit in every storage of this library, so a stored non-zero diagonal — outside the reference's
// own contract, clipper.h:137-138 — is refused rather than silently dropped. A strictly upper matrix (what Eigen hands
// over) is left as it is; anything else is copied to `out` without those entries and `a` is pointed at the copy.
std::string upper_only(const char* what, int64_t m, CscRef& a, CscLists& out, int64_t& dropped_below) {
  bool strict = true;
  for (int64_t j = 0; j < m && strict; ++j)
    for (int64_t p = a.cp[j]; p < a.cp[j + 1]; ++p)
      if (a.ri[p] >= j) {
        strict = false;
        break;
      }
  if (strict) return {};
  out.cp.assign(static_cast<size_t>(m) + 1, 0);
  for (int64_t j = 0; j < m; ++j) {
    for (int64_t p = a.cp[j]; p < a.cp[j + 1]; ++p) {
      const int64_t i = a.ri[p];
      if (i > j) {
        ++dropped_below;
        continue;
      }
      if (i == j) {
        if (a.va[p] != 0.0)
          return format("%s: a stored diagonal entry (%lld,%lld) — the matrices must not have diagonal values set", what,
                        static_cast<long long>(i), static_cast<long long>(j));
        continue;
      }
      out.ri.push_back(static_cast<int32_t>(i));
      out.va.push_back(a.va[p]);
    }
    out.cp[static_cast<size_t>(j) + 1] = static_cast<int64_t>(out.ri.size());
  }
  a = CscRef{out.cp.data(), out.ri.data(), out.va.data()};
  return {};
}

// The values of a handed-over matrix, refused before anything is touched: a non-finite value anywhere in the strict
// upper triangle (every later product would be NaN), and — when the storage asked for holds fp32 values (`f32`) — a
// finite value whose float cast is infinite. The round-to-nearest-even cast gives infinity from FLT_MAX plus half its
// last place on: 0x1.ffffffp+127. Entries on or below the diagonal are never read, so they are not looked at.
std::string check_value(const char* what, int64_t i, int64_t j, double v, bool f32) {
  if (!std::isfinite(v))
    return format("%s: entry (%lld,%lld) is not finite (%g)", what, static_cast<long long>(i), static_cast<long long>(j), v);
  if (f32 && std::fabs(v) >= 0x1.ffffffp+127)
    return format("%s: entry (%lld,%lld) = %.17g rounds to infinity in fp32 storage", what, static_cast<long long>(i),
                  static_cast<long long>(j), v);
  return {};
}

// a CSC matrix whose structure check_csc has accepted
std::string check_values_csc(const char* what, int64_t m, const CscRef& a, bool f32) {
  for (int64_t j = 0; j < m; ++j)
    for (int64_t p = a.cp[j]; p < a.cp[j + 1]; ++p) {
      if (a.ri[p] >= j) continue;
      std::string err = check_value(what, a.ri[p], j, a.va[p], f32);
      if (!err.empty()) return err;
    }
  return {};
}

// a dense column-major m x m matrix, read as the dense setter reads it: A[i + j * m] for i < j
std::string check_values_dense_upper(const char* what, int64_t m, const double* A, bool f32) {
  for (int64_t j = 1; j < m; ++j)
    for (int64_t i = 0; i < j; ++i) {
      const double v = A[i + j * m];
      if (std::isfinite(v) && !(f32 && std::fabs(v) >= 0x1.ffffffp+127)) continue;
      return check_value(what, i, j, v, f32);
    }
  return {};
}

// C == pattern(M)?  (same structure, every stored C equal to 1, every stored M non-zero)
bool is_pattern(int64_t m, const CscRef& M, const CscRef& C) {
  const int64_t nnzM = M.cp[m], nnzC = C.cp[m];
  bool pattern = (nnzM == nnzC) && std::equal(M.cp, M.cp + m + 1, C.cp) && (nnzM == 0 || std::equal(M.ri, M.ri + nnzM, C.ri));
  for (int64_t p = 0; pattern && p < nnzM; ++p) pattern = (C.va[p] == 1.0) && (M.va[p] != 0.0);
  return pattern;
}

// The full symmetric lists of an upper-triangle matrix (both triangles, the diagonal left out), rows ascending in every
// column. Strictly-upper input with ascending rows comes out sorted; anything else is sorted here; an entry given
// twice (e.g. in both triangles) is refused.
std::string symmetric_lists(int64_t m, const CscRef& M, CscLists& out) {
  std::vector<int64_t>& cp = out.cp;
  cp.assign(static_cast<size_t>(m) + 1, 0);
  for (int64_t j = 0; j < m; ++j)
    for (int64_t p = M.cp[j]; p < M.cp[j + 1]; ++p) {
      const int64_t i = M.ri[p];
      if (i == j) continue;
      ++cp[static_cast<size_t>(i) + 1];
      ++cp[static_cast<size_t>(j) + 1];
    }
  for (int64_t c = 0; c < m; ++c) cp[static_cast<size_t>(c) + 1] += cp[static_cast<size_t>(c)];
  const int64_t nnz2 = cp[static_cast<size_t>(m)];
  std::vector<int32_t>& ri = out.ri;
  std::vector<double>& va = out.va;
  ri.assign(static_cast<size_t>(nnz2), 0);
  va.assign(static_cast<size_t>(nnz2), 0.0);
  {
    std::vector<int64_t> cur(cp.begin(), cp.end() - 1);
    for (int64_t j = 0; j < m; ++j)
      for (int64_t p = M.cp[j]; p < M.cp[j + 1]; ++p) {
        const int64_t i = M.ri[p];
        if (i == j) continue;
        int64_t& a = cur[static_cast<size_t>(j)];
        ri[static_cast<size_t>(a)] = static_cast<int32_t>(i);
        va[static_cast<size_t>(a)] = M.va[p];
        ++a;
        int64_t& b = cur[static_cast<size_t>(i)];
        ri[static_cast<size_t>(b)] = static_cast<int32_t>(j);
        va[static_cast<size_t>(b)] = M.va[p];
        ++b;
      }
  }
  std::vector<std::pair<int32_t, double>> buf;
  for (int64_t c = 0; c < m; ++c) {
    const int64_t a = cp[static_cast<size_t>(c)], b = cp[static_cast<size_t>(c) + 1];
    bool sorted = true;
    for (int64_t p = a + 1; p < b && sorted; ++p) sorted = ri[static_cast<size_t>(p - 1)] < ri[static_cast<size_t>(p)];
    if (sorted) continue;
    buf.clear();
    for (int64_t p = a; p < b; ++p) buf.emplace_back(ri[static_cast<size_t>(p)], va[static_cast<size_t>(p)]);
    std::sort(buf.begin(), buf.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    for (size_t q = 1; q < buf.size(); ++q)
      if (buf[q - 1].first == buf[q].first)
        return format("entry (%d,%lld) is stored more than once", buf[q].first, static_cast<long long>(c));
    for (int64_t p = a; p < b; ++p) {
      ri[static_cast<size_t>(p)] = buf[static_cast<size_t>(p - a)].first;
      va[static_cast<size_t>(p)] = buf[static_cast<size_t>(p - a)].second;
    }
  }
  return {};
}

}  // namespace clipper_csc
