// device_invariant_hostloop.cpp — the host loop a user-defined C++ invariant takes (CLIPPER::scoreCustomInvariantOnHost:
// one virtual call per pair, OpenMP, then the dense M and C uploaded), timed on EuclideanDistance restated as a
// PairwiseInvariant subclass. Reads D1, D2 (3 x n, column-major fp64) and A (m x 2, column-major int32) from the raw
// files tools/device_invariant_probe.py writes; prints one JSON line. Built and run by that probe.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <vector>

#include <clipper/clipper.h>

namespace {
class HostEuclid : public clipper::invariants::PairwiseInvariant {
 public:
  double operator()(const clipper::invariants::Datum& ai, const clipper::invariants::Datum& aj,
                    const clipper::invariants::Datum& bi, const clipper::invariants::Datum& bj) override {
    double s1 = 0.0, s2 = 0.0;
    for (std::ptrdiff_t k = 0; k < ai.size(); ++k) {
      const double t1 = ai(k) - aj(k), t2 = bi(k) - bj(k);
      s1 = std::fma(t1, t1, s1);
      s2 = std::fma(t2, t2, s2);
    }
    const double c = std::abs(std::sqrt(s1) - std::sqrt(s2));
    return c < 0.05 ? std::exp(-0.5 * c * c / (0.015 * 0.015)) : 0.0;
  }
};

template <typename T>
std::vector<T> load(const char* path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  const size_t n = static_cast<size_t>(f.tellg()) / sizeof(T);
  std::vector<T> v(n);
  f.seekg(0);
  f.read(reinterpret_cast<char*>(v.data()), static_cast<std::streamsize>(n * sizeof(T)));
  return v;
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s D1.f64 D2.f64 A.i32\n", argv[0]);
    return 2;
  }
  const auto d1 = load<double>(argv[1]), d2 = load<double>(argv[2]);
  const auto a = load<int32_t>(argv[3]);
  const std::ptrdiff_t n1 = static_cast<std::ptrdiff_t>(d1.size() / 3), n2 = static_cast<std::ptrdiff_t>(d2.size() / 3);
  const std::ptrdiff_t m = static_cast<std::ptrdiff_t>(a.size() / 2);
  clipper::invariants::Data D1(3, n1), D2(3, n2);
  for (std::ptrdiff_t c = 0; c < n1; ++c)
    for (int r = 0; r < 3; ++r) D1(r, c) = d1[static_cast<size_t>(c * 3 + r)];
  for (std::ptrdiff_t c = 0; c < n2; ++c)
    for (int r = 0; r < 3; ++r) D2(r, c) = d2[static_cast<size_t>(c * 3 + r)];
  clipper::Association A(m, 2);
  for (std::ptrdiff_t i = 0; i < m; ++i) {
    A(i, 0) = a[static_cast<size_t>(i)];
    A(i, 1) = a[static_cast<size_t>(m + i)];
  }
  clipper::CLIPPER c(std::make_shared<HostEuclid>(), clipper::Params());
  const auto t0 = std::chrono::steady_clock::now();
  c.scorePairwiseConsistency(D1, D2, A);
  const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  std::printf("{\"m\": %td, \"host_loop_s\": %.6f}\n", m, s);
  return 0;
}
