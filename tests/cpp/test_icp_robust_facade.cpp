// test_icp_robust_facade.cpp — clipper::registration::icp_robust / icp_generalized_robust through the clipper:: facade:
// the clouds, the target's normals and the covariances come from files (column-major 3 x n and 6 x n doubles); the
// refined transform and (count, within, trim_sqd, weight_sum) of a Huber loss with trimming go to files for
// tests/test_gpu_icp_robust.py to compare with the model's bits; the defaults equal the plain calls; a refusal arrives as
// std::invalid_argument with the library's message. Plain asserts (no gtest in the image). Built and run on the GPU box
// by tests/test_gpu_icp_robust.py.
//   test_icp_robust_facade n_src n_tgt src.f64 tgt.f64 nrm.f64 cs.f64 ct.f64 out_plane.f64 out_gen.f64
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include <clipper/registration.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static clipper::invariants::Data read(const char* path, long rows, long n) {
  clipper::invariants::Data M(rows, n);
  FILE* f = std::fopen(path, "rb");
  EXPECT(f != nullptr);
  EXPECT(std::fread(M.data(), sizeof(double), static_cast<size_t>(rows * n), f) == static_cast<size_t>(rows * n));
  std::fclose(f);
  return M;
}

static void write(const char* path, const clipper::registration::IcpRobustResult& r) {
  double v[20];
  for (int i = 0; i < 16; ++i) v[i] = r.T[i];
  v[16] = static_cast<double>(r.count);
  v[17] = static_cast<double>(r.within);
  v[18] = r.trim_sqd;
  v[19] = r.weight_sum;
  FILE* f = std::fopen(path, "wb");
  EXPECT(f != nullptr);
  EXPECT(std::fwrite(v, sizeof(double), 20, f) == 20);
  std::fclose(f);
}

int main(int argc, char** argv) {
  EXPECT(argc == 10);
  const long ns = std::atol(argv[1]), nt = std::atol(argv[2]);
  namespace reg = clipper::registration;
  const clipper::invariants::Data src = read(argv[3], 3, ns), tgt = read(argv[4], 3, nt), nrm = read(argv[5], 3, nt);
  const clipper::invariants::Data cs = read(argv[6], 6, ns), ct = read(argv[7], 6, nt);

  reg::IcpParams prm;
  prm.method = reg::IcpMethod::PointToPlane;
  prm.max_distance = 0.1;
  prm.max_iterations = 40;
  reg::IcpRobust rb;
  EXPECT(rb.loss == reg::IcpLoss::None && rb.scale == 0.0 && rb.trim == 1.0);
  reg::setKnnSearch(reg::KnnSearch::Grid);

  // the defaults: the plain call's bits
  const reg::IcpResult plain = reg::icp(src, tgt, prm, nullptr, nrm);
  const reg::IcpRobustResult same = reg::icp_robust(src, tgt, prm, rb, nullptr, nrm);
  for (int i = 0; i < 16; ++i) EXPECT(plain.T[i] == same.T[i]);
  EXPECT(plain.iterations == same.iterations && plain.status == same.status && plain.count == same.count);
  EXPECT(plain.inlier_rmse == same.inlier_rmse && same.within == same.count && same.trim_sqd == 0.1 * 0.1);

  rb.loss = reg::IcpLoss::Huber;
  rb.scale = 0.01;
  rb.trim = 0.6;
  const reg::IcpRobustResult a = reg::icp_robust(src, tgt, prm, rb, nullptr, nrm);
  EXPECT(a.count < a.within && a.within <= ns && a.trim_sqd > 0.0 && a.trim_sqd < 0.1 * 0.1 && a.weight_sum == 0.0);
  EXPECT(static_cast<int>(a.history.size()) == a.iterations + 1 && a.history.back()[0] == static_cast<double>(a.count));
  write(argv[8], a);
  prm.method = reg::IcpMethod::Generalized;
  const reg::IcpRobustResult g = reg::icp_generalized_robust(src, cs, tgt, ct, prm, rb);
  EXPECT(g.count < g.within);
  write(argv[9], g);
  reg::setKnnSearch(reg::KnnSearch::Brute);
  const reg::IcpRobustResult b = reg::icp_generalized_robust(src, cs, tgt, ct, prm, rb);  // brute force: the same bits
  for (int i = 0; i < 16; ++i) EXPECT(g.T[i] == b.T[i]);
  EXPECT(b.route == reg::KnnSearch::Brute && b.trim_sqd == g.trim_sqd && b.within == g.within);

  std::string said;
  rb.trim = 1.5;
  try {
    reg::icp_generalized_robust(src, cs, tgt, ct, prm, rb);
  } catch (const std::invalid_argument& e) {
    said = e.what();
  }
  EXPECT(said == "icp_generalized_robust: trim must be in (0, 1] (trim = 1.5)");
  said.clear();
  rb.trim = 0.6;
  rb.scale = -2.0;
  prm.method = reg::IcpMethod::PointToPoint;
  try {
    reg::icp_robust(src, tgt, prm, rb);
  } catch (const std::invalid_argument& e) {
    said = e.what();
  }
  EXPECT(said == "icp_robust: scale must be positive and finite with a loss (scale = -2)");
  std::printf("ALL ROBUST ICP FACADE TESTS PASSED\n");
  return 0;
}
