// test_gicp_rules.cpp — the generalized part of clipper_amd/csrc/icp_rules.hpp on the host (g++ only,
// -ffp-contract=off): whole generalized ICPs (the transform, a brute-force K = 1 search in the contract's arithmetic,
// icp_generalized_terms, the addition tree as the kernels run it, icp_iterate<ICP_GENERALIZED>) and the covariance rule
// over brute-force neighbour lists. Prints bit patterns; tests/test_gicp_rules.py compares them with
// tests/gicp_model.py bit for bit.
//   usage: test_gicp_rules icp <case file>   (binary: int32 max_iterations, n_src, n_tgt, 0; double max_distance,
//          rel_fitness, rel_rmse; T_init 16 column-major; src n_src x 3; C_src n_src x 6; tgt n_tgt x 3; C_tgt n_tgt x 6)
//          test_gicp_rules cov <case file>   (binary: int32 n, knn; double radius, epsilon; P n x 3)
// Without an argument: the checks of host_icp_check.hpp that the generalized calls add, and a pair with a singular
// C_b + R C_a R^T fed to the terms past those checks.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host_icp_check.hpp"
#include "knn_grid_rules.hpp"

using namespace clipper_hip;

static int failures = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                              \
    }                                                          \
  } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

constexpr int TERMS = ICP_GENERALIZED_TERMS;

// the sums of n rows of TERMS terms in the kernels' order: 256 per partial, partials t, t + 256, ... per lane, the tree
static void fold(const std::vector<double>& terms, int n, double* S) {
  const int nb = (n + ICP_BLOCK - 1) / ICP_BLOCK;
  std::vector<double> part(static_cast<size_t>(nb) * TERMS), v(static_cast<size_t>(ICP_BLOCK) * TERMS);
  for (int b = 0; b < nb; ++b) {
    for (int i = 0; i < ICP_BLOCK; ++i)
      for (int a = 0; a < TERMS; ++a) {
        const int p = b * ICP_BLOCK + i;
        v[static_cast<size_t>(i) * TERMS + a] = p < n ? terms[static_cast<size_t>(p) * TERMS + a] : 0.0;
      }
    for (int a = 0; a < TERMS; ++a) {
      icp_tree(v.data() + a, TERMS);
      part[static_cast<size_t>(b) * TERMS + a] = v[a];
    }
  }
  for (int i = 0; i < ICP_BLOCK; ++i)
    for (int a = 0; a < TERMS; ++a) {
      double acc = 0.0;
      for (int b = i; b < nb; b += ICP_BLOCK) acc = acc + part[static_cast<size_t>(b) * TERMS + a];
      v[static_cast<size_t>(i) * TERMS + a] = acc;
    }
  for (int a = 0; a < TERMS; ++a) {
    icp_tree(v.data() + a, TERMS);
    S[a] = v[a];
  }
}

static void print_result(const IcpRecord& rec, const double* T, const std::vector<double>& hist) {
  std::printf("status %d iterations %d count %" PRId64 "\nT", rec.status, rec.iterations, rec.count);
  for (int i = 0; i < 16; ++i) std::printf(" %016" PRIx64, bits(T[i]));
  std::printf("\nhistory");
  for (double h : hist) std::printf(" %016" PRIx64, bits(h));
  std::printf("\n");
}

static int run_icp(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  int32_t h[4];
  double d[3], T[16];
  if (std::fread(h, 4, 4, f) != 4 || std::fread(d, 8, 3, f) != 3 || std::fread(T, 8, 16, f) != 16) return 3;
  const int iters = h[0], ns = h[1], nt = h[2];
  std::vector<double> src(static_cast<size_t>(ns) * 3), cs(static_cast<size_t>(ns) * 6), tgt(static_cast<size_t>(nt) * 3),
      ct(static_cast<size_t>(nt) * 6);
  if (std::fread(src.data(), 8, src.size(), f) != src.size() || std::fread(cs.data(), 8, cs.size(), f) != cs.size() ||
      std::fread(tgt.data(), 8, tgt.size(), f) != tgt.size() || std::fread(ct.data(), 8, ct.size(), f) != ct.size())
    return 4;
  std::fclose(f);
  const clipper_icp::Params prm{ICP_GENERALIZED, iters, d[0], d[1], d[2]};
  if (!clipper_icp::check_generalized_params(&prm).empty() || !clipper_icp::check_covariances("source", cs.data(), ns).empty() ||
      !clipper_icp::check_covariances("target", ct.data(), nt).empty())
    return 5;
  double lo[3], hi[3], o[3];
  for (int a = 0; a < 3; ++a) lo[a] = hi[a] = tgt[a];
  for (int j = 0; j < nt; ++j)
    for (int a = 0; a < 3; ++a) {
      lo[a] = tgt[j * 3 + a] < lo[a] ? tgt[j * 3 + a] : lo[a];
      hi[a] = tgt[j * 3 + a] > hi[a] ? tgt[j * 3 + a] : hi[a];
    }
  icp_origin(lo, hi, o);
  const double d2 = prm.max_distance * prm.max_distance;
  const IcpStop stop{prm.max_iterations, ns, prm.rel_fitness, prm.rel_rmse};
  std::vector<double> hist(static_cast<size_t>(prm.max_iterations + 1) * 3, 0.0), terms(static_cast<size_t>(ns) * TERMS);
  IcpRecord rec{};
  rec.status = ICP_RUNNING;
  for (int k = 0; rec.status == ICP_RUNNING; ++k) {
    for (int i = 0; i < ns; ++i) {
      const double p[3] = {src[i * 3], src[i * 3 + 1], src[i * 3 + 2]};
      double q[3], t[TERMS];
      icp_transform_point(T, p, q);
      double bd[1];
      int32_t bi[1];
      knn_grid_clear(bd, bi);
      for (int j = 0; j < nt; ++j) {
        const double b[3] = {tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2]};
        knn_grid_insert<1>(bd, bi, knn_grid_sqdist(q, b), j);
      }
      for (int a = 0; a < TERMS; ++a) t[a] = 0.0;
      if (icp_inlier(bi[0], bd[0], d2)) {
        const int j = bi[0];
        const double b[3] = {tgt[j * 3], tgt[j * 3 + 1], tgt[j * 3 + 2]};
        double ca[6], cb[6];
        for (int a = 0; a < 6; ++a) {
          ca[a] = cs[static_cast<size_t>(i) * 6 + a];
          cb[a] = ct[static_cast<size_t>(j) * 6 + a];
        }
        icp_generalized_terms(q, b, ca, cb, T, bd[0], o, t);
      }
      for (int a = 0; a < TERMS; ++a) terms[static_cast<size_t>(i) * TERMS + a] = t[a];
    }
    double S[TERMS];
    fold(terms, ns, S);
    icp_iterate<ICP_GENERALIZED>(stop, k, S, o, T, rec, hist.data() + static_cast<size_t>(k) * 3);
  }
  print_result(rec, T, hist);
  return 0;
}

static int run_cov(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  int32_t h[2];
  double d[2];
  if (std::fread(h, 4, 2, f) != 2 || std::fread(d, 8, 2, f) != 2) return 3;
  const int n = h[0], knn = h[1];
  const double radius = d[0], epsilon = d[1];
  std::vector<double> P(static_cast<size_t>(n) * 3);
  if (std::fread(P.data(), 8, P.size(), f) != P.size()) return 4;
  std::fclose(f);
  const clipper_features::Neighborhood nb{knn, radius};
  if (!clipper_features::check_neighborhood("neighbourhood", &nb).empty() || !clipper_icp::check_epsilon(epsilon).empty()) return 5;
  const bool use_r = radius > 0.0;
  const double r2 = radius * radius, w = 1.0 - epsilon;
  std::printf("C");
  std::vector<int> cnts;
  for (int i = 0; i < n; ++i) {
    const double p[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
    double bd[FEAT_MAX_KNN];
    int32_t bi[FEAT_MAX_KNN];
    knn_grid_clear(bd, bi);
    for (int j = 0; j < n; ++j) {
      const double b[3] = {P[j * 3], P[j * 3 + 1], P[j * 3 + 2]};
      knn_grid_insert<FEAT_MAX_KNN>(bd, bi, knn_grid_sqdist(p, b), j);
    }
    int cnt = 0;
    while (cnt < knn && feat_kept(bi[cnt], bd[cnt], use_r, r2)) ++cnt;
    double c[6];
    icp_point_covariance(
        cnt,
        [&](int k, double (&x)[3]) {
          for (int a = 0; a < 3; ++a) x[a] = P[static_cast<size_t>(bi[k]) * 3 + a];
        },
        w, c);
    for (int a = 0; a < 6; ++a) std::printf(" %016" PRIx64, bits(c[a]));
    cnts.push_back(cnt);
  }
  std::printf("\ncount");
  for (int c : cnts) std::printf(" %d", c);
  std::printf("\n");
  return 0;
}

static int checks() {
  namespace ci = clipper_icp;
  ci::Params p{2, 30, 0.1, 1e-6, 1e-6};
  EXPECT(ci::check_generalized_params(&p).empty() && ci::check_generalized_params(nullptr) == "null params");
  EXPECT(ci::check_not_generalized(&p) == "method 2 (generalized) takes per-point covariances: call clipper_hip_icp_generalized");
  EXPECT(ci::check_params(&p) == "unknown method 2");  // (the check of the other call, as it was)
  p.method = 1;
  EXPECT(ci::check_generalized_params(&p) == "method must be CLIPPER_ICP_GENERALIZED (2) (method = 1)");
  EXPECT(ci::check_not_generalized(&p).empty() && ci::check_not_generalized(nullptr).empty());
  p.method = 2;
  p.max_distance = -1.0;
  EXPECT(ci::check_generalized_params(&p) == "max_distance must be positive and finite (max_distance = -1)");
  p.max_distance = 0.1;
  p.max_iterations = 1001;
  EXPECT(ci::check_generalized_params(&p) == "max_iterations must be in 0..1000 (max_iterations = 1001)");
  EXPECT(ci::check_epsilon(1e-3).empty() && ci::check_epsilon(1.0).empty());
  EXPECT(ci::check_epsilon(0.0) == "epsilon must be in (0, 1] (epsilon = 0)");
  EXPECT(ci::check_epsilon(1.5) == "epsilon must be in (0, 1] (epsilon = 1.5)");
  EXPECT(ci::check_epsilon(NAN).find("epsilon must be in (0, 1]") == 0);
  double C[12] = {1, 0, 0, 1, 0, 1, 2, 0.5, 0, 2, 0, 1e-3};
  EXPECT(ci::check_covariances("source", C, 2).empty());
  EXPECT(ci::check_covariances("source", nullptr, 2) == "null source covariance array");
  C[10] = INFINITY;
  EXPECT(ci::check_covariances("target", C, 2) == "target covariances: non-finite value at entry 4 of point 1");
  C[10] = 0.0;
  C[6] = -2.0;
  EXPECT(ci::check_covariances("target", C, 2).find("the matrix of point 1 is not positive definite (leading minor 1 = -2)") !=
         std::string::npos);
  C[6] = 2.0;
  C[7] = 2.0;  // xx yy - xy^2 = 0
  EXPECT(ci::check_covariances("target", C, 2).find("point 1 is not positive definite (leading minor 2 = 0)") != std::string::npos);
  C[7] = 0.5;
  C[11] = 0.0;  // zz = 0: the determinant
  EXPECT(ci::check_covariances("target", C, 2).find("point 1 is not positive definite (leading minor 3 = 0)") != std::string::npos);

  // the rule of a covariance: eigenvalue epsilon along nv, 1 across it; symmetric in the sign of nv
  const double nv[3] = {0.6, 0.0, 0.8}, mv[3] = {-0.6, -0.0, -0.8};
  double c[6], c2[6];
  icp_covariance_of_normal(nv, 1.0 - 1e-3, c);
  icp_covariance_of_normal(mv, 1.0 - 1e-3, c2);
  for (int a = 0; a < 6; ++a) EXPECT(bits(c[a]) == bits(c2[a]));
  const double Cn[3] = {(c[0] * nv[0] + c[1] * nv[1]) + c[2] * nv[2], (c[1] * nv[0] + c[3] * nv[1]) + c[4] * nv[2],
                        (c[2] * nv[0] + c[4] * nv[1]) + c[5] * nv[2]};
  for (int a = 0; a < 3; ++a) EXPECT(std::fabs(Cn[a] - 1e-3 * nv[a]) < 1e-15);
  EXPECT(c[3] == 1.0 && c[1] == 0.0 && c[4] == 0.0);

  // with identity covariances and T = I the metric is point-to-point's up to the factor 1 / 2: M = I / 2 exactly
  const double I6[6] = {1, 0, 0, 1, 0, 1}, Z6[6] = {0, 0, 0, 0, 0, 0};
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const double o[3] = {0.0, 0.0, 0.0};
  {
    const double q[3] = {1.0, 2.0, 3.0}, b[3] = {0.5, 2.0, 3.25};
    double t[TERMS];
    icp_generalized_terms(q, b, I6, I6, T, 0.3125, o, t);
    EXPECT(t[0] == 1.0 && t[29] == 0.3125 && t[28] == 0.5 * 0.3125);             // d^T M d = |d|^2 / 2
    EXPECT(t[16] == 0.5 && t[19] == 0.5 && t[21] == 0.5 && t[17] == 0.0);         // the lower-right block: M
    EXPECT(t[25] == 0.25 && t[26] == 0.0 && t[27] == -0.125);                     // M d
  }
  // a singular C_b + R C_a R^T, past check_covariances: both matrices zero. det == 0, the divisions give non-numbers,
  // the pivot test refuses them: DEGENERATE, T untouched, the history row still finite
  {
    std::vector<double> terms(static_cast<size_t>(4) * TERMS);
    for (int i = 0; i < 4; ++i) {
      const double q[3] = {0.1 * i, 0.2, 0.3 + 0.05 * i}, b[3] = {0.1 * i + 0.01, 0.21, 0.3};
      double t[TERMS];
      icp_generalized_terms(q, b, i == 2 ? Z6 : I6, i == 2 ? Z6 : I6, T, 0.0625, o, t);
      EXPECT((i == 2) == (t[1] != t[1]));  // a non-number from the singular pair alone
      for (int a = 0; a < TERMS; ++a) terms[static_cast<size_t>(i) * TERMS + a] = t[a];
    }
    double S[TERMS], row[3], T1[16];
    fold(terms, 4, S);
    for (int i = 0; i < 16; ++i) T1[i] = T[i] + (i == 12 ? 0.25 : 0.0);
    double keep[16];
    std::memcpy(keep, T1, sizeof(keep));
    IcpRecord rec{};
    rec.status = ICP_RUNNING;
    const IcpStop stop{30, 4, 1e-6, 1e-6};
    icp_iterate<ICP_GENERALIZED>(stop, 0, S, o, T1, rec, row);
    EXPECT(rec.status == ICP_DEGENERATE && rec.count == 4 && rec.iterations == 0);
    EXPECT(std::memcmp(keep, T1, sizeof(keep)) == 0);
    EXPECT(row[0] == 4.0 && row[1] == 1.0 && row[2] == 0.25);
  }
  std::puts(failures ? "gicp checks FAILED" : "gicp checks ok");
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return checks();
  if (std::string(argv[1]) == "icp") return run_icp(argv[2]);
  if (std::string(argv[1]) == "cov") return run_cov(argv[2]);
  return 1;
}
