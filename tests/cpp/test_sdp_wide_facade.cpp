// test_sdp_wide_facade.cpp — the route switch of the clipper:: facade (sdp::setRoute, include/clipper/sdp.h): under
// Route::Auto sdp::solve at 150 x 150 and CLIPPER::solveAsMSRCSDR with setDeviceSdp(true) at m = 200 take the wide
// route and return what the C ABI returns (tests/test_gpu_sdp_wide.py computes that and passes it in a file); under the
// default route both are refused as before. Plain asserts (no gtest in the image).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <clipper/clipper.h>
#include <clipper/sdp.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static clipper::MatrixXd read_matrix(const char* path, int n) {
  clipper::MatrixXd A = clipper::MatrixXd::Zero(n, n);
  FILE* f = std::fopen(path, "r");
  EXPECT(f != nullptr);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double v = 0;
      EXPECT(std::fscanf(f, "%lf", &v) == 1);
      A(i, j) = v;
    }
  std::fclose(f);
  return A;
}

static std::vector<int> read_nodes(FILE* f) {
  int k = 0;
  EXPECT(std::fscanf(f, "%d", &k) == 1 && k >= 0);
  std::vector<int> nodes(static_cast<size_t>(k));
  for (int& v : nodes) EXPECT(std::fscanf(f, "%d", &v) == 1);
  return nodes;
}

template <class F>
static bool refused(F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    return std::string(e.what()).find("limit of 128") != std::string::npos;
  }
  return false;
}

int main(int argc, char** argv) {
  EXPECT(argc == 6);
  namespace sdp = clipper::sdp;
  const clipper::MatrixXd M150 = read_matrix(argv[1], 150), C150 = read_matrix(argv[2], 150);
  const clipper::MatrixXd M200 = read_matrix(argv[3], 200), C200 = read_matrix(argv[4], 200);
  FILE* f = std::fopen(argv[5], "r");
  EXPECT(f != nullptr);
  double pobj = 0;
  EXPECT(std::fscanf(f, "%lf", &pobj) == 1);
  const std::vector<int> want150 = read_nodes(f), want200 = read_nodes(f);
  std::fclose(f);

  const sdp::Params p;
  EXPECT(sdp::route() == sdp::Route::Workgroup);
  EXPECT(refused([&] { sdp::solve(M150, C150, p); }));

  sdp::setRoute(sdp::Route::Auto);
  EXPECT(sdp::route() == sdp::Route::Auto);
  const sdp::Solution s = sdp::solve(M150, C150, p);
  EXPECT(s.nodes == want150 && !s.nodes.empty());
  EXPECT(s.pobj == static_cast<float>(pobj));
  EXPECT(s.X.rows() == 150 && s.lambdas.size() == 150 && s.evec1.size() == 150 && s.iters > 0);

  clipper::invariants::EuclideanDistance::Params iparams;
  auto invariant = std::make_shared<clipper::invariants::EuclideanDistance>(iparams);
  clipper::CLIPPER clipper(invariant, clipper::Params());
  clipper.setMatrixData(M200, C200);
  clipper.setDeviceSdp(true);
  clipper.solveAsMSRCSDR(p);
  std::vector<int> got(clipper.getSolution().nodes.begin(), clipper.getSolution().nodes.end());
  EXPECT(got == want200 && !got.empty());
  EXPECT(clipper.getSolution().score == -1);

  // both solve overloads follow the setting: a batch of one
  const std::vector<sdp::Solution> many = sdp::solve(std::vector<clipper::MatrixXd>{M150}, std::vector<clipper::MatrixXd>{C150}, p);
  EXPECT(many.size() == 1 && many[0].nodes == want150 && many[0].pobj == s.pobj);

  sdp::setRoute(sdp::Route::Workgroup);
  EXPECT(sdp::route() == sdp::Route::Workgroup);
  EXPECT(refused([&] { sdp::solve(M150, C150, p); }));
  std::printf("ALL SDP WIDE FACADE TESTS PASSED\n");
  return 0;
}
