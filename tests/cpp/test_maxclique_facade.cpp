// test_maxclique_facade.cpp — CLIPPER::solveAsMaximumClique through the clipper::CLIPPER facade on the reference's
// golden case (test/affinity_test.cpp:33-48: 4 model points, 3 data points, all-to-all): every method returns the
// clique {0, 4, 8} with the reference's Solution fields (clipper.cpp:92-96). Plain asserts (no gtest in the image).
// Built and run on the GPU box by tests/test_gpu_maxclique.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>

#include <clipper/clipper.h>
#include <clipper/utils.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

int main() {
  clipper::invariants::EuclideanDistance::Params iparams;
  auto invariant = std::make_shared<clipper::invariants::EuclideanDistance>(iparams);
  clipper::invariants::Data model = clipper::invariants::Data::Zero(3, 4), data = clipper::invariants::Data::Zero(3, 3);
  const double pts[4][3] = {{0, 0, 0}, {2, 0, 0}, {0, 3, 0}, {2, 2, 0}};
  for (int c = 0; c < 4; ++c)
    for (int r = 0; r < 3; ++r) model(r, c) = pts[c][r];
  const double th = M_PI / 8, t[3] = {5, 3, 0};
  const double R[3][3] = {{std::cos(th), -std::sin(th), 0}, {std::sin(th), std::cos(th), 0}, {0, 0, 1}};
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < 3; ++r) {
      double acc = 0;
      for (int k = 0; k < 3; ++k) acc += R[k][r] * (model(k, c) - t[k]);
      data(r, c) = acc;
    }
  const clipper::maxclique::Method methods[3] = {clipper::maxclique::Method::EXACT, clipper::maxclique::Method::HEU,
                                                 clipper::maxclique::Method::KCORE};
  for (auto method : methods) {
    clipper::CLIPPER clipper(invariant, clipper::Params());
    clipper.scorePairwiseConsistency(model, data);  // all-to-all
    clipper::maxclique::Params p;
    p.method = method;
    p.verbose = true;
    clipper.solveAsMaximumClique(p);
    const clipper::Solution& s = clipper.getSolution();
    EXPECT(s.nodes.size() == 3 && s.nodes[0] == 0 && s.nodes[1] == 4 && s.nodes[2] == 8);
    EXPECT(s.score == -1 && s.ifinal == 0 && s.t > 0);
    EXPECT(s.u.size() == 12);
    for (int i = 0; i < 12; ++i) EXPECT(s.u(i) == 0);
    const clipper::Association Ain = clipper.getSelectedAssociations();
    EXPECT(Ain.rows() == 3);
    for (int i = 0; i < 3; ++i) EXPECT(Ain(i, 0) == Ain(i, 1));
    // a solve afterwards is an ordinary solve
    clipper.solve();
    EXPECT(clipper.getSolution().score > 0);
  }
  std::printf("ALL MAXCLIQUE FACADE TESTS PASSED\n");
  return 0;
}
