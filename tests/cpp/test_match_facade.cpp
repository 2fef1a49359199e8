// test_match_facade.cpp — clipper::registration::match_descriptors through the clipper:: facade: the descriptors of
// two views come from files (column-major d x n doubles), the associations of three filter settings go to stdout for
// tests/test_gpu_match.py to compare with the C ABI's rows; a refusal arrives as std::invalid_argument with the
// library's message. Plain asserts (no gtest in the image). Built and run on the GPU box by tests/test_gpu_match.py.
//   test_match_facade d n0 n1 F0.f64 F1.f64
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

static clipper::invariants::Data read(const char* path, long d, long n) {
  clipper::invariants::Data F(d, n);
  FILE* f = std::fopen(path, "rb");
  EXPECT(f != nullptr);
  EXPECT(std::fread(F.data(), sizeof(double), static_cast<size_t>(d * n), f) == static_cast<size_t>(d * n));
  std::fclose(f);
  return F;
}

static void print(const char* name, const clipper::Association& A) {
  EXPECT(A.cols() == 2 || A.rows() == 0);
  std::printf("%s %ld\n", name, static_cast<long>(A.rows()));
  for (long r = 0; r < static_cast<long>(A.rows()); ++r) std::printf("%d %d\n", A(r, 0), A(r, 1));
}

int main(int argc, char** argv) {
  EXPECT(argc == 6);
  const long d = std::atol(argv[1]), n0 = std::atol(argv[2]), n1 = std::atol(argv[3]);
  const clipper::invariants::Data F0 = read(argv[4], d, n0), F1 = read(argv[5], d, n1);
  namespace reg = clipper::registration;

  print("default", reg::match_descriptors(F0, F1));  // knn 1, mutual
  reg::MatchParams p;
  p.mutual = false;
  p.ratio = 0.8;
  print("ratio", reg::match_descriptors(F0, F1, p));
  p = reg::MatchParams{};
  p.knn = 2;
  p.max_sqdist = 0.12;
  print("knn2", reg::match_descriptors(F0, F1, p, 0));

  p.knn = 9;
  bool thrown = false;
  try {
    reg::match_descriptors(F0, F1, p);
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "knn must be in 1..8 (knn = 9)";
  }
  EXPECT(thrown);
  std::printf("ALL MATCH FACADE TESTS PASSED\n");
  return 0;
}
