// test_ransac_rules.cpp — clipper_amd/csrc/ransac_rules.hpp on the host (g++ -ffp-contract=off, no HIP): whole RANSAC
// calls from the header, with the fold as the kernels run it, printed as bit patterns for tests/test_ransac_rules.py to
// compare with tests/ransac_model.py. Run without arguments it checks the argument checks of host_ransac_check.hpp.
//   test_ransac_rules                      the checks
//   test_ransac_rules table case.bin       per hypothesis of round 0: number, pass flag, count, sample
//   test_ransac_rules run case.bin [thr]   a whole call on thr host threads (default 1)
//   test_ransac_rules time case.bin thr    the same, timed: milliseconds of the call (tools/ransac_probe.py)
// case.bin: 3 doubles (max_distance, edge_similarity, confidence), int64 max_hypotheses, 4 int32 (hypotheses_per_round,
// n_sample, refine_iterations, m), uint64 seed, then the gathered pairs P and B (3 x m doubles each).
#include <chrono>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "host_ransac_check.hpp"
#include "ransac_rules.hpp"

using namespace clipper_hip;

static int failures = 0;

static void expect(const std::string& got, const char* want, const char* what) {
  const bool ok = want[0] ? got.find(want) != std::string::npos : got.empty();
  if (!ok) {
    std::printf("FAILED %s: got \"%s\", want \"%s\"\n", what, got.c_str(), want);
    ++failures;
  }
}

static int run_checks() {
  namespace cr = clipper_ransac;
  const cr::Params good{0.02, 0.9, 0.999, 100000, 4096, 3, 1, 0};
  expect(cr::check_params(&good), "", "good params");
  expect(cr::check_params(nullptr), "null params", "null params");
  cr::Params p = good;
  p.max_distance = 0.0;
  expect(cr::check_params(&p), "max_distance = 0", "max_distance 0");
  p.max_distance = std::numeric_limits<double>::infinity();
  expect(cr::check_params(&p), "max_distance = inf", "max_distance inf");
  p = good, p.edge_similarity = 1.0;
  expect(cr::check_params(&p), "edge_similarity = 1", "edge_similarity 1");
  p = good, p.edge_similarity = -0.5;
  expect(cr::check_params(&p), "edge_similarity = -0.5", "edge_similarity < 0");
  p = good, p.edge_similarity = 0.0;
  expect(cr::check_params(&p), "", "edge_similarity 0");
  p = good, p.confidence = 1.0;
  expect(cr::check_params(&p), "confidence = 1", "confidence 1");
  p = good, p.confidence = 0.0;
  expect(cr::check_params(&p), "confidence = 0", "confidence 0");
  p = good, p.max_hypotheses = 0;
  expect(cr::check_params(&p), "max_hypotheses = 0", "max_hypotheses 0");
  p = good, p.max_hypotheses = int64_t(1) << 31;
  expect(cr::check_params(&p), "max_hypotheses = 2147483648", "max_hypotheses 2^31");
  p = good, p.hypotheses_per_round = 255;
  expect(cr::check_params(&p), "hypotheses_per_round = 255", "round 255");
  p = good, p.hypotheses_per_round = 300;
  expect(cr::check_params(&p), "hypotheses_per_round = 300", "round 300");
  p = good, p.hypotheses_per_round = 65536 + 256;
  expect(cr::check_params(&p), "hypotheses_per_round = 65792", "round too long");
  p = good, p.hypotheses_per_round = 65536;
  expect(cr::check_params(&p), "", "round 65536");
  p = good, p.n_sample = 2;
  expect(cr::check_params(&p), "n_sample = 2", "n_sample 2");
  p = good, p.n_sample = 9;
  expect(cr::check_params(&p), "n_sample = 9", "n_sample 9");
  p = good, p.refine_iterations = -1;
  expect(cr::check_params(&p), "refine_iterations = -1", "refine -1");
  p = good, p.refine_iterations = 11;
  expect(cr::check_params(&p), "refine_iterations = 11", "refine 11");
  p = good, p.reserved = 7;
  expect(cr::check_params(&p), "reserved = 7", "reserved");

  double D1[12] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1}, D2[15] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 5, 6, 7};
  int32_t A[8] = {0, 1, 2, 3, 0, 1, 2, 4};  // column-major 4 x 2
  double lo[3], hi[3];
  expect(cr::check_cloud_size("D1", nullptr, 4), "null D1", "null cloud");
  expect(cr::check_cloud_size("D2", D2, 0), "D2: a cloud needs at least one point (n = 0)", "empty cloud");
  expect(cr::check_associations(D1, 4, D2, 5, A, 4, 3, lo, hi), "", "good associations");
  if (!(lo[0] == 0 && lo[1] == 0 && lo[2] == 0 && hi[0] == 5 && hi[1] == 6 && hi[2] == 7)) {
    std::printf("FAILED box of the gathered targets\n");
    ++failures;
  }
  expect(cr::check_associations(D1, 4, D2, 5, nullptr, 4, 3, lo, hi), "null association", "null A");
  expect(cr::check_associations(D1, 4, D2, 5, A, 2, 3, lo, hi), "m = 2, n_sample = 3", "m < n_sample");
  expect(cr::check_associations(D1, 4, D2, 4, A, 4, 3, lo, hi), "association row 3 out of range (3, 4)", "row out of range");
  A[1] = -1;
  expect(cr::check_associations(D1, 4, D2, 5, A, 4, 3, lo, hi), "association row 1 out of range (-1, 1)", "negative row");
  A[1] = 1;
  D1[7] = std::numeric_limits<double>::quiet_NaN();
  expect(cr::check_associations(D1, 4, D2, 5, A, 4, 3, lo, hi), "D1: non-finite value at coordinate 1 of point 2", "NaN in D1");
  D1[7] = 1;
  D2[12] = std::numeric_limits<double>::infinity();
  expect(cr::check_associations(D1, 4, D2, 5, A, 4, 3, lo, hi), "D2: non-finite value at coordinate 0 of point 4", "inf in D2");
  A[7] = 3;  // (the non-finite point is no longer referred to)
  expect(cr::check_associations(D1, 4, D2, 5, A, 4, 3, lo, hi), "", "an unreferenced non-finite point");

  if (ransac_needed(10, 10, 3, 0.999) != 1) std::printf("FAILED needed at w = 1\n"), ++failures;
  if (ransac_needed(3, 2000000000, 3, 0.999) != INT64_MAX) std::printf("FAILED needed at a vanishing w\n"), ++failures;
  if (failures == 0) std::printf("ransac checks ok\n");
  return failures ? 1 : 0;
}

struct Case {
  RansacCall c;
  int32_t m;
  std::vector<double> P, B;
};

static bool read_case(const char* path, Case& k) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return false;
  double d[3];
  int64_t mh;
  int32_t i[4];
  uint64_t seed;
  bool ok = std::fread(d, 8, 3, f) == 3 && std::fread(&mh, 8, 1, f) == 1 && std::fread(i, 4, 4, f) == 4 && std::fread(&seed, 8, 1, f) == 1;
  if (ok) {
    k.c = RansacCall{d[0], d[1], d[2], mh, i[0], i[1], i[2], seed};
    k.m = i[3];
    k.P.resize(static_cast<size_t>(k.m) * 3);
    k.B.resize(static_cast<size_t>(k.m) * 3);
    ok = std::fread(k.P.data(), 8, k.P.size(), f) == k.P.size() && std::fread(k.B.data(), 8, k.B.size(), f) == k.B.size();
  }
  std::fclose(f);
  return ok;
}

static uint64_t bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}

template <int N>
static void table(const Case& k) {
  const double s2 = k.c.edge_similarity * k.c.edge_similarity, d2 = k.c.max_distance * k.c.max_distance;
  for (int g = 0; g < k.c.hypotheses_per_round; ++g) {
    int32_t s[N];
    double T[16];
    int64_t cnt = 0;
    const bool pass = ransac_host_score<N>(k.c, static_cast<uint64_t>(g), k.P.data(), k.B.data(), k.m, s2, d2, s, T, cnt);
    std::printf("%d %d %" PRId64, g, pass ? 1 : 0, cnt);
    for (int a = 0; a < N; ++a) std::printf(" %d", s[a]);
    std::printf("\n");
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return run_checks();
  if (argc < 3) return 2;
  Case k;
  if (!read_case(argv[2], k)) {
    std::printf("cannot read %s\n", argv[2]);
    return 2;
  }
  const std::string mode = argv[1];
  if (mode == "table") {
    switch (k.c.n_sample) {
      case 3: table<3>(k); break;
      case 4: table<4>(k); break;
      case 5: table<5>(k); break;
      case 6: table<6>(k); break;
      case 7: table<7>(k); break;
      default: table<8>(k); break;
    }
    return 0;
  }
  const int threads = argc > 3 ? std::atoi(argv[3]) : 1;
  RansacOutcome out;
  std::vector<uint8_t> mask(static_cast<size_t>(k.m));
  const auto t0 = std::chrono::steady_clock::now();
  ransac_host_call(k.c, k.P.data(), k.B.data(), k.m, threads, out, mask.data());
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (mode == "time") {
    std::printf("ms %.6f evaluated %" PRId64 " checked %" PRId64 " count %" PRId64 "\n", ms, out.evaluated, out.checked, out.count);
    return 0;
  }
  std::printf("status %d refined %d evaluated %" PRId64 " checked %" PRId64 " best_hypothesis %" PRId64 " best_count %" PRId64
              " count %" PRId64 "\n", out.status, out.refined, out.evaluated, out.checked, out.best_hypothesis, out.best_count, out.count);
  std::printf("fitness %016" PRIx64 " rmse %016" PRIx64 "\n", bits(out.fitness), bits(out.inlier_rmse));
  std::printf("sample");
  for (int a = 0; a < RANSAC_MAX_SAMPLE; ++a) std::printf(" %d", out.sample[a]);
  std::printf("\nT");
  for (int a = 0; a < 16; ++a) std::printf(" %016" PRIx64, bits(out.T[a]));
  std::printf("\nmask ");
  for (uint8_t b : mask) std::putchar(b ? '1' : '0');
  std::printf("\n");
  return 0;
}
