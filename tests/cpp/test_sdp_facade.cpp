// test_sdp_facade.cpp — CLIPPER::solveAsMSRCSDR with setDeviceSdp and sdp::solve through the clipper:: facade on the
// reference's golden case (test/sdp_test.cpp: the 20 x 20 M, C = (M > 0)). The default stays the stub of a build
// without SCS; with the device on, the Solution fields are those of clipper.cpp:108-112. Plain asserts (no gtest in
// the image). Built and run on the GPU box by tests/test_gpu_sdp.py, which passes a file that holds M.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include <clipper/clipper.h>
#include <clipper/sdp.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

int main(int argc, char** argv) {
  EXPECT(argc == 2);
  const int n = 20;
  clipper::MatrixXd M = clipper::MatrixXd::Zero(n, n), C = clipper::MatrixXd::Zero(n, n);
  FILE* f = std::fopen(argv[1], "r");
  EXPECT(f != nullptr);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) {
      double v = 0;
      EXPECT(std::fscanf(f, "%lf", &v) == 1);
      M(i, j) = v;
      C(i, j) = v > 0 ? 1.0 : 0.0;
    }
  std::fclose(f);

  clipper::sdp::Params p;
  p.eps_abs = 1e-6f;
  p.eps_rel = 1e-6f;
  p.max_iters = 20000;
  const clipper::sdp::Solution s = clipper::sdp::solve(M, C, p);
  EXPECT(!s.nodes.empty() && s.iters > 0 && s.t > 0);
  EXPECT(s.X.rows() == n && s.lambdas.size() == n && s.evec1.size() == n);
  EXPECT(s.pobj <= s.dobj + 1e-4f);  // (SCS's sign: -<M, X> and the bound's negative)
  double tr = 0;
  for (int i = 0; i < n; ++i) tr += s.X(i, i);
  EXPECT(std::fabs(tr - 1.0) < 1e-9);
  for (int i = 1; i < n; ++i) EXPECT(s.lambdas(i - 1) <= s.lambdas(i));
  for (int i = 0; i < n; ++i) EXPECT((std::fabs(s.evec1(i)) > s.thr) == (std::find(s.nodes.begin(), s.nodes.end(), i) != s.nodes.end()));

  clipper::invariants::EuclideanDistance::Params iparams;
  auto invariant = std::make_shared<clipper::invariants::EuclideanDistance>(iparams);
  clipper::CLIPPER clipper(invariant, clipper::Params());
  clipper.setMatrixData(M, C);
  clipper.solveAsMSRCSDR(p);  // default: the stub
  EXPECT(clipper.getSolution().nodes.empty() && clipper.getSolution().score == -1);
  clipper.setDeviceSdp(true);
  clipper.solveAsMSRCSDR(p);
  const clipper::Solution& c = clipper.getSolution();
  EXPECT(c.nodes == s.nodes);
  EXPECT(c.score == -1 && c.ifinal == 0 && c.t > 0);
  EXPECT(c.u.size() == n);
  for (int i = 0; i < n; ++i) EXPECT(c.u(i) == 0);
  // a solve afterwards is an ordinary solve
  clipper.solve();
  EXPECT(clipper.getSolution().score > 0);
  clipper.setDeviceSdp(false);
  clipper.solveAsMSRCSDR(p);
  EXPECT(clipper.getSolution().nodes.empty());
  std::printf("ALL SDP FACADE TESTS PASSED\n");
  return 0;
}
