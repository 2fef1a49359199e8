// test_gicp_facade.cpp — clipper::registration::estimate_covariances / icp_generalized through the clipper:: facade: the
// clouds come from files (column-major 3 x n doubles), the covariances of the target and the refined transform go to
// files (column-major 6 x n and 4 x 4) for tests/test_gpu_gicp.py to compare with the model's bits; a refusal arrives as
// std::invalid_argument with the library's message. Plain asserts (no gtest in the image). Built and run on the GPU
// box by tests/test_gpu_gicp.py.
//   test_gicp_facade n_src n_tgt src.f64 tgt.f64 C_tgt_out.f64 T_out.f64
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

static clipper::invariants::Data read(const char* path, long n) {
  clipper::invariants::Data M(3, n);
  FILE* f = std::fopen(path, "rb");
  EXPECT(f != nullptr);
  EXPECT(std::fread(M.data(), sizeof(double), static_cast<size_t>(3 * n), f) == static_cast<size_t>(3 * n));
  std::fclose(f);
  return M;
}

static void write(const char* path, const double* v, size_t count) {
  FILE* f = std::fopen(path, "wb");
  EXPECT(f != nullptr);
  EXPECT(std::fwrite(v, sizeof(double), count, f) == count);
  std::fclose(f);
}

int main(int argc, char** argv) {
  EXPECT(argc == 7);
  const long ns = std::atol(argv[1]), nt = std::atol(argv[2]);
  const clipper::invariants::Data src = read(argv[3], ns), tgt = read(argv[4], nt);
  namespace reg = clipper::registration;

  const clipper::invariants::Data cs = reg::estimate_covariances(src), ct = reg::estimate_covariances(tgt);  // knn 20, 1e-3
  EXPECT(cs.rows() == 6 && cs.cols() == ns && ct.rows() == 6 && ct.cols() == nt);
  write(argv[5], ct.data(), static_cast<size_t>(6 * nt));

  reg::IcpParams prm;
  prm.method = reg::IcpMethod::Generalized;
  prm.max_distance = 0.1;
  reg::setKnnSearch(reg::KnnSearch::Grid);
  const reg::IcpResult a = reg::icp_generalized(src, cs, tgt, ct, prm);
  reg::setKnnSearch(reg::KnnSearch::Brute);
  EXPECT(a.status == reg::IcpStatus::Converged && a.fitness == 1.0 && a.count == ns);
  EXPECT(static_cast<int>(a.history.size()) == a.iterations + 1 && a.history.back()[1] == a.fitness);
  EXPECT(a.route == reg::KnnSearch::Grid && a.candidates > 0);
  write(argv[6], a.T, 16);
  const reg::IcpResult b = reg::icp_generalized(src, cs, tgt, ct, prm);  // brute force: the same bits
  for (int i = 0; i < 16; ++i) EXPECT(a.T[i] == b.T[i]);
  EXPECT(b.route == reg::KnnSearch::Brute && b.iterations == a.iterations);

  std::string said;
  try {
    reg::icp(src, tgt, prm);  // the other call knows two methods
  } catch (const std::invalid_argument& e) {
    said = e.what();
  }
  EXPECT(said == "icp: method 2 (generalized) takes per-point covariances: call clipper_hip_icp_generalized");
  said.clear();
  prm.method = reg::IcpMethod::PointToPoint;
  try {
    reg::icp_generalized(src, cs, tgt, ct, prm);
  } catch (const std::invalid_argument& e) {
    said = e.what();
  }
  EXPECT(said == "icp_generalized: method must be CLIPPER_ICP_GENERALIZED (2) (method = 0)");
  said.clear();
  try {
    reg::estimate_covariances(src, reg::Neighborhood{20, 0.0}, 0.0);
  } catch (const std::invalid_argument& e) {
    said = e.what();
  }
  EXPECT(said == "estimate_covariances: epsilon must be in (0, 1] (epsilon = 0)");
  said.clear();
  try {
    reg::icp_generalized(src, ct, tgt, ct, prm);  // a covariance per point
  } catch (const std::invalid_argument& e) {
    said = e.what();
  }
  EXPECT(said == "covariances must be 6 x n, one column per point");
  said.clear();
  try {
    reg::estimate_covariances(src, reg::Neighborhood{20, 0.0}, 1e-3, 4096);
  } catch (const std::invalid_argument& e) {
    said = e.what();
  }
  EXPECT(said.find("device 4096 out of range") == 0);
  std::printf("ALL GICP FACADE TESTS PASSED\n");
  return 0;
}
