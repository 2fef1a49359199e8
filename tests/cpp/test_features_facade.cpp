// test_features_facade.cpp — clipper::registration::estimate_normals / compute_fpfh through the clipper:: facade: the
// cloud comes from a file (column-major 3 x n doubles), the normals (3 x n) and the descriptors of the two-call and
// the one-call route (33 x n each) go to files for tests/test_gpu_features.py to compare with the C ABI's bits; a
// refusal arrives as std::invalid_argument with the library's message. Plain asserts (no gtest in the image). Built
// and run on the GPU box by tests/test_gpu_features.py.
//   test_features_facade n P.f64 N_out.f64 F_out.f64 F1_out.f64
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

static void write(const char* path, const clipper::invariants::Data& M) {
  FILE* f = std::fopen(path, "wb");
  EXPECT(f != nullptr);
  const size_t count = static_cast<size_t>(M.rows()) * static_cast<size_t>(M.cols());
  EXPECT(std::fwrite(M.data(), sizeof(double), count, f) == count);
  std::fclose(f);
}

int main(int argc, char** argv) {
  EXPECT(argc == 6);
  const long n = std::atol(argv[1]);
  clipper::invariants::Data P(3, n);
  FILE* f = std::fopen(argv[2], "rb");
  EXPECT(f != nullptr);
  EXPECT(std::fread(P.data(), sizeof(double), static_cast<size_t>(3 * n), f) == static_cast<size_t>(3 * n));
  std::fclose(f);
  namespace reg = clipper::registration;

  const double view[3] = {0.0, 0.1, 1.0};
  const reg::Neighborhood nnb{12, 0.0}, fnb{20, 0.03};
  const clipper::invariants::Data N = reg::estimate_normals(P, nnb, view);
  EXPECT(N.rows() == 3 && N.cols() == n);
  const clipper::invariants::Data F = reg::compute_fpfh(P, N, fnb);
  EXPECT(F.rows() == 33 && F.cols() == n);
  const clipper::invariants::Data F1 = reg::compute_fpfh(P, nnb, view, fnb);
  EXPECT(F1.rows() == 33 && F1.cols() == n);
  write(argv[3], N);
  write(argv[4], F);
  write(argv[5], F1);
  EXPECT(reg::Neighborhood{}.knn == 16 && reg::Neighborhood{}.radius == 0.0);

  bool thrown = false;
  try {
    reg::estimate_normals(P, reg::Neighborhood{2, 0.0});
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "neighbourhood: knn must be in 3..32 (knn = 2)";
  }
  EXPECT(thrown);
  thrown = false;
  try {
    clipper::invariants::Data Z(3, n);
    for (long k = 0; k < 3 * n; ++k) Z.data()[k] = 0.0;
    reg::compute_fpfh(P, Z);
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "N: normal 0 is not of unit length (squared length = 0)";
  }
  EXPECT(thrown);
  std::printf("ALL FEATURES FACADE TESTS PASSED\n");
  return 0;
}
