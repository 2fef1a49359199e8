// test_ransac_facade.cpp — clipper::registration::ransac_correspondences through the clipper:: facade: the clouds
// (column-major 3 x n doubles) and the associations (column-major m x 2 int32) come from files, T (column-major 4 x 4),
// the integers of the info and the mask go to a file for tests/test_gpu_ransac.py to compare with the Python facade's
// bytes; a refusal arrives as std::invalid_argument with the library's message. Plain asserts (no gtest in the image).
// Built and run on the GPU box by tests/test_gpu_ransac.py.
//   test_ransac_facade n1 n2 m D1.f64 D2.f64 A.i32 out.bin
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

int main(int argc, char** argv) {
  EXPECT(argc == 8);
  const long n1 = std::atol(argv[1]), n2 = std::atol(argv[2]), m = std::atol(argv[3]);
  const clipper::invariants::Data D1 = read(argv[4], n1), D2 = read(argv[5], n2);
  clipper::Association A(m, 2);
  {
    FILE* f = std::fopen(argv[6], "rb");
    EXPECT(f != nullptr);
    EXPECT(std::fread(A.data(), sizeof(int32_t), static_cast<size_t>(2 * m), f) == static_cast<size_t>(2 * m));
    std::fclose(f);
  }
  namespace reg = clipper::registration;

  reg::RansacParams prm;
  EXPECT(prm.n_sample == 3 && prm.edge_similarity == 0.9 && prm.max_hypotheses == 100000 && prm.confidence == 0.999);
  EXPECT(prm.seed == 0 && prm.refine_iterations == 1 && prm.hypotheses_per_round == 4096);
  prm.max_distance = 0.02;
  prm.hypotheses_per_round = 256;
  prm.max_hypotheses = 1024;
  const reg::RansacInfo r = reg::ransac_correspondences(D1, D2, A, prm);
  EXPECT(r.status == reg::RansacStatus::Converged || r.status == reg::RansacStatus::MaxHypotheses);
  EXPECT(static_cast<long>(r.inliers.size()) == m && r.evaluated % 256 == 0 && r.best_hypothesis >= 0);
  int64_t in = 0;
  for (uint8_t b : r.inliers) in += b;
  EXPECT(in == r.count && r.fitness == static_cast<double>(r.count) / static_cast<double>(m));
  EXPECT(r.sample[2] >= 0 && r.sample[3] == -1);
  {
    FILE* f = std::fopen(argv[7], "wb");
    EXPECT(f != nullptr);
    const int64_t ints[7] = {static_cast<int64_t>(r.status), r.refined, r.evaluated, r.checked, r.best_hypothesis, r.best_count, r.count};
    EXPECT(std::fwrite(r.T, sizeof(double), 16, f) == 16);
    EXPECT(std::fwrite(ints, sizeof(int64_t), 7, f) == 7);
    EXPECT(std::fwrite(r.inliers.data(), 1, r.inliers.size(), f) == r.inliers.size());
    std::fclose(f);
  }

  bool thrown = false;
  try {
    prm.n_sample = 9;
    reg::ransac_correspondences(D1, D2, A, prm);
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "ransac_correspondences: n_sample must be in 3..8 (n_sample = 9)";
  }
  EXPECT(thrown);
  thrown = false;
  try {
    prm.n_sample = 3;
    reg::ransac_correspondences(D1, D2, A, prm, 12345);
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()).find("device 12345 out of range") != std::string::npos;
  }
  EXPECT(thrown);
  std::printf("ALL RANSAC FACADE TESTS PASSED\n");
  return 0;
}
