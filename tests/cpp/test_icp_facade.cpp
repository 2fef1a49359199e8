// test_icp_facade.cpp — clipper::registration::icp / evaluate_registration through the clipper:: facade: the clouds and
// the target's normals come from files (column-major 3 x n doubles), the refined transforms of both methods go to files
// (column-major 4 x 4) for tests/test_gpu_icp.py to compare with the model's bits; a refusal arrives as
// std::invalid_argument with the library's message. Plain asserts (no gtest in the image). Built and run on the GPU
// box by tests/test_gpu_icp.py.
//   test_icp_facade n_src n_tgt src.f64 tgt.f64 normals.f64 T_point_out.f64 T_plane_out.f64
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

static void write(const char* path, const double (&T)[16]) {
  FILE* f = std::fopen(path, "wb");
  EXPECT(f != nullptr);
  EXPECT(std::fwrite(T, sizeof(double), 16, f) == 16);
  std::fclose(f);
}

int main(int argc, char** argv) {
  EXPECT(argc == 8);
  const long ns = std::atol(argv[1]), nt = std::atol(argv[2]);
  const clipper::invariants::Data src = read(argv[3], ns), tgt = read(argv[4], nt), nrm = read(argv[5], nt);
  namespace reg = clipper::registration;

  reg::IcpParams prm;
  EXPECT(prm.max_iterations == 30 && prm.rel_fitness == 1e-6 && prm.rel_rmse == 1e-6 && prm.method == reg::IcpMethod::PointToPoint);
  prm.max_distance = 0.1;
  const reg::IcpResult a = reg::icp(src, tgt, prm);
  EXPECT(a.status == reg::IcpStatus::Converged && a.fitness == 1.0 && a.count == ns);
  EXPECT(static_cast<int>(a.history.size()) == a.iterations + 1 && a.history.back()[1] == a.fitness);
  EXPECT(a.route == reg::KnnSearch::Brute && a.candidates == 0);
  write(argv[6], a.T);

  prm.method = reg::IcpMethod::PointToPlane;
  reg::setKnnSearch(reg::KnnSearch::Grid);
  const reg::IcpResult b = reg::icp(src, tgt, prm, nullptr, nrm);
  reg::setKnnSearch(reg::KnnSearch::Brute);
  EXPECT(b.status == reg::IcpStatus::Converged && b.route == reg::KnnSearch::Grid && b.candidates > 0);
  write(argv[7], b.T);

  std::vector<int32_t> corr;
  const reg::RegistrationQuality q = reg::evaluate_registration(src, tgt, b.T, 0.1, &corr);
  EXPECT(q.fitness == b.fitness && q.inlier_rmse == b.inlier_rmse && q.count == b.count);
  EXPECT(static_cast<long>(corr.size()) == ns && corr[0] >= 0 && corr[0] < nt);

  bool thrown = false;
  try {
    reg::icp(src, tgt, prm);  // point-to-plane without normals
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "icp: point-to-plane needs the target's normals (N_tgt is null)";
  }
  EXPECT(thrown);
  thrown = false;
  try {
    reg::evaluate_registration(src, tgt, nullptr, -1.0);
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "evaluate_registration: max_distance must be positive and finite (max_distance = -1)";
  }
  EXPECT(thrown);
  std::printf("ALL ICP FACADE TESTS PASSED\n");
  return 0;
}
