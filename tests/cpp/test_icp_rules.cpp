// test_icp_rules.cpp — whole ICPs on the host over clipper_amd/csrc/icp_rules.hpp (g++ only, -ffp-contract=off): the
// transform, a brute-force K = 1 search in the contract's arithmetic, the terms, the addition tree as the kernels run
// it (256 per partial, partials t, t + 256, ... per lane, the tree again), icp_iterate. Prints T and the history as
// hexadecimal bit patterns; tests/test_icp_rules.py compares them with tests/icp_model.py bit for bit.
//   usage: test_icp_rules <case file>    (binary: int32 method, max_iterations, n_src, n_tgt; double max_distance,
//          rel_fitness, rel_rmse; T_init 16 column-major; src n_src x 3; tgt n_tgt x 3; normals n_tgt x 3 iff method 1)
// Without an argument: the checks of host_icp_check.hpp.
#include <cinttypes>
#include <cstdio>
#include <cstring>
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

template <int METHOD>
static void fold(const std::vector<double>& terms, int n, double* S) {
  constexpr int T = icp_terms(METHOD);
  const int nb = (n + ICP_BLOCK - 1) / ICP_BLOCK;
  std::vector<double> part(static_cast<size_t>(nb) * T), v(static_cast<size_t>(ICP_BLOCK) * T);
  for (int b = 0; b < nb; ++b) {
    for (int i = 0; i < ICP_BLOCK; ++i)
      for (int a = 0; a < T; ++a) {
        const int p = b * ICP_BLOCK + i;
        v[static_cast<size_t>(i) * T + a] = p < n ? terms[static_cast<size_t>(p) * T + a] : 0.0;
      }
    for (int a = 0; a < T; ++a) {
      icp_tree(v.data() + a, T);
      part[static_cast<size_t>(b) * T + a] = v[a];
    }
  }
  for (int i = 0; i < ICP_BLOCK; ++i)
    for (int a = 0; a < T; ++a) {
      double acc = 0.0;
      for (int b = i; b < nb; b += ICP_BLOCK) acc = acc + part[static_cast<size_t>(b) * T + a];
      v[static_cast<size_t>(i) * T + a] = acc;
    }
  for (int a = 0; a < T; ++a) {
    icp_tree(v.data() + a, T);
    S[a] = v[a];
  }
}

template <int METHOD>
static void run(const std::vector<double>& src, const std::vector<double>& tgt, const std::vector<double>& nrm, int ns, int nt,
                const clipper_icp::Params& prm, double* T) {
  constexpr int TERMS = icp_terms(METHOD);
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
        if constexpr (METHOD == ICP_POINT_TO_PLANE) {
          const double n[3] = {nrm[j * 3], nrm[j * 3 + 1], nrm[j * 3 + 2]};
          icp_plane_terms(q, b, n, bd[0], o, t);
        } else {
          icp_point_terms(q, b, bd[0], o, t);
        }
      }
      for (int a = 0; a < TERMS; ++a) terms[static_cast<size_t>(i) * TERMS + a] = t[a];
    }
    double S[TERMS];
    fold<METHOD>(terms, ns, S);
    icp_iterate<METHOD>(stop, k, S, o, T, rec, hist.data() + static_cast<size_t>(k) * 3);
  }
  std::printf("status %d iterations %d count %" PRId64 "\nT", rec.status, rec.iterations, rec.count);
  for (int i = 0; i < 16; ++i) std::printf(" %016" PRIx64, bits(T[i]));
  std::printf("\nhistory");
  for (double h : hist) std::printf(" %016" PRIx64, bits(h));
  std::printf("\n");
}

static int checks() {
  namespace ci = clipper_icp;
  const double P[6] = {0, 0, 0, 1, 2, 3};
  double bad[6] = {0, 0, 0, 1, NAN, 3};
  EXPECT(ci::check_cloud("source", P, 2).empty());
  EXPECT(ci::check_cloud("source", nullptr, 2) == "null source point array");
  EXPECT(ci::check_cloud("target", P, 0) == "target: a cloud needs at least one point (n = 0)");
  EXPECT(ci::check_cloud("target", P, int64_t(1) << 31).find("n = 2147483648") != std::string::npos);
  EXPECT(ci::check_cloud("source", bad, 2) == "source: non-finite value at coordinate 1 of point 1");
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  EXPECT(ci::check_transform("T_init", T).empty() && ci::check_transform("T_init", nullptr).empty());
  T[7] = 0.5;
  EXPECT(ci::check_transform("T_init", T) == "T_init: the bottom row must be 0 0 0 1 (entry (3, 1) = 0.5)");
  T[7] = 0.0;
  T[13] = INFINITY;
  EXPECT(ci::check_transform("T_init", T) == "T_init: non-finite value at entry (1, 3)");
  ci::Params p{0, 30, 0.1, 1e-6, 1e-6};
  EXPECT(ci::check_params(&p).empty() && ci::check_params(nullptr) == "null params");
  p.method = 2;
  EXPECT(ci::check_params(&p) == "unknown method 2");
  p.method = 1;
  p.max_distance = 0.0;
  EXPECT(ci::check_params(&p) == "max_distance must be positive and finite (max_distance = 0)");
  p.max_distance = 0.1;
  p.max_iterations = 1001;
  EXPECT(ci::check_params(&p) == "max_iterations must be in 0..1000 (max_iterations = 1001)");
  p.max_iterations = 0;
  p.rel_rmse = -1.0;
  EXPECT(ci::check_params(&p) == "rel_rmse must be at least 0 (rel_rmse = -1)");
  EXPECT(ci::check_target_normals(0, nullptr, 2).empty());
  EXPECT(ci::check_target_normals(1, nullptr, 2) == "point-to-plane needs the target's normals (N_tgt is null)");
  const double N[6] = {0, 0, 1, 0, 0, 2};
  EXPECT(ci::check_target_normals(1, N, 2).find("normal 1 is not of unit length") != std::string::npos);
  // the Cayley map is a rotation, and the rotation of a cross-covariance reproduces a known one
  const double w[3] = {0.3, -0.2, 0.5};
  double R[9], RtR = 0.0;
  icp_cayley(w, R);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += R[k * 3 + i] * R[k * 3 + j];
      RtR = std::fmax(RtR, std::fabs(s - (i == j ? 1.0 : 0.0)));
    }
  EXPECT(RtR < 1e-15 && std::fabs(icp_det3(R) - 1.0) < 1e-15);
  double R2[9];
  rotation_from_cross_covariance(R, R2);  // (H = R: the closest rotation to a rotation is itself)
  for (int i = 0; i < 9; ++i) EXPECT(std::fabs(R2[i] - R[i]) < 1e-14);
  std::puts(failures ? "icp checks FAILED" : "icp checks ok");
  return failures ? 1 : 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return checks();
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[4];
  double d[3], T[16];
  if (std::fread(h, 4, 4, f) != 4 || std::fread(d, 8, 3, f) != 3 || std::fread(T, 8, 16, f) != 16) return 3;
  const int method = h[0], ns = h[2], nt = h[3];
  std::vector<double> src(static_cast<size_t>(ns) * 3), tgt(static_cast<size_t>(nt) * 3), nrm(method == 1 ? tgt.size() : 0);
  if (std::fread(src.data(), 8, src.size(), f) != src.size() || std::fread(tgt.data(), 8, tgt.size(), f) != tgt.size() ||
      std::fread(nrm.data(), 8, nrm.size(), f) != nrm.size())
    return 4;
  std::fclose(f);
  const clipper_icp::Params prm{method, h[1], d[0], d[1], d[2]};
  if (method == 1)
    run<ICP_POINT_TO_PLANE>(src, tgt, nrm, ns, nt, prm, T);
  else
    run<ICP_POINT_TO_POINT>(src, tgt, nrm, ns, nt, prm, T);
  return 0;
}
