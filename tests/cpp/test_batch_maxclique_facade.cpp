// test_batch_maxclique_facade.cpp — the batched maximum-clique call through the clipper:: facade:
// CLIPPERBatch::solveAsMaximumClique gives per problem what CLIPPER::solveAsMaximumClique leaves on a lone CLIPPER
// (nodes ascending, u = 0, score = -1, ifinal = 0), getSelectedAssociations(i) follows it, and a later solve() is
// untouched. Plain asserts (no gtest in the image). Built and run on the GPU box by tests/test_gpu_batch_maxclique.py,
// which passes a file that holds the golden affinity_test points (4 model points, then 3 data points, x y z each).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <vector>

#include <clipper/batch.h>
#include <clipper/clipper.h>
#include <clipper/utils.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// n points in the unit cube, the same moved rigidly; m associations, the first m (1 - rho) true
static clipper::BatchProblem make_problem(int n, int m, double rho, unsigned seed) {
  std::mt19937 g(seed);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  clipper::BatchProblem p;
  p.D1 = clipper::invariants::Data::Zero(3, n);
  p.D2 = clipper::invariants::Data::Zero(3, n);
  const double th = 0.3, c = std::cos(th), s = std::sin(th);
  for (int k = 0; k < n; ++k) {
    for (int r = 0; r < 3; ++r) p.D1(r, k) = U(g);
    p.D2(0, k) = c * p.D1(0, k) - s * p.D1(1, k) + 0.5;
    p.D2(1, k) = s * p.D1(0, k) + c * p.D1(1, k) - 0.3;
    p.D2(2, k) = p.D1(2, k) + 0.8;
  }
  p.A = clipper::Association(m, 2);
  const int good = static_cast<int>(m * (1.0 - rho));
  for (int i = 0; i < m; ++i) {
    p.A(i, 0) = i % n;
    p.A(i, 1) = i < good ? i % n : static_cast<int>(g() % n);
  }
  p.u0 = clipper::utils::randvec(static_cast<size_t>(m));
  return p;
}

int main(int argc, char** argv) {
  EXPECT(argc == 2);
  FILE* f = std::fopen(argv[1], "r");
  EXPECT(f != nullptr);
  clipper::BatchProblem gold;
  gold.D1 = clipper::invariants::Data::Zero(3, 4);
  gold.D2 = clipper::invariants::Data::Zero(3, 3);
  for (int k = 0; k < 4; ++k)
    for (int r = 0; r < 3; ++r) EXPECT(std::fscanf(f, "%lf", &gold.D1(r, k)) == 1);
  for (int k = 0; k < 3; ++k)
    for (int r = 0; r < 3; ++r) EXPECT(std::fscanf(f, "%lf", &gold.D2(r, k)) == 1);
  std::fclose(f);
  gold.A = clipper::utils::createAllToAll(4, 3);
  gold.u0 = clipper::VectorXd::Zero(12);
  for (int k = 0; k < 12; ++k) gold.u0(k) = 0.5;

  auto inv = std::make_shared<clipper::invariants::EuclideanDistance>(clipper::invariants::EuclideanDistance::Params{});
  std::vector<clipper::BatchProblem> probs = {gold, make_problem(60, 200, 0.8, 7u), make_problem(40, 65, 0.5, 8u)};
  clipper::CLIPPERBatch batch(inv, clipper::Params());
  bool threw = false;
  try {
    batch.solveAsMaximumClique();
  } catch (const std::logic_error&) {
    threw = true;
  }
  EXPECT(threw);
  const std::vector<clipper::Solution> first = batch.solve(probs);

  const clipper::maxclique::Method methods[] = {clipper::maxclique::Method::EXACT, clipper::maxclique::Method::HEU,
                                                clipper::maxclique::Method::KCORE};
  for (clipper::maxclique::Method meth : methods) {
    clipper::maxclique::Params prm;
    prm.method = meth;
    prm.threads = 3;  // (ignored)
    const std::vector<clipper::Solution> out = batch.solveAsMaximumClique(prm);
    EXPECT(out.size() == probs.size());
    EXPECT((out[0].nodes == std::vector<int>{0, 4, 8}));
    for (size_t i = 0; i < probs.size(); ++i) {
      clipper::CLIPPER lone(inv, clipper::Params());
      lone.scorePairwiseConsistency(probs[i].D1, probs[i].D2, probs[i].A);
      lone.solveAsMaximumClique(prm);
      const clipper::Solution& c = lone.getSolution();
      EXPECT(c.nodes == out[i].nodes && !out[i].nodes.empty());
      EXPECT(out[i].score == -1 && out[i].ifinal == 0 && out[i].t > 0);
      EXPECT(out[i].u.size() == c.u.size() && out[i].u.size() == probs[i].u0.size());
      for (int k = 0; k < out[i].u.size(); ++k) EXPECT(out[i].u(k) == 0.0);
      const clipper::Association sa = lone.getSelectedAssociations(), sb = batch.getSelectedAssociations(static_cast<int>(i));
      EXPECT(sa.rows() == sb.rows() && sb.rows() == static_cast<int>(out[i].nodes.size()));
      for (int r = 0; r < sa.rows(); ++r) EXPECT(sa(r, 0) == sb(r, 0) && sa(r, 1) == sb(r, 1));
    }
  }
  // the golden answer's associations pair point k with point k
  {
    const clipper::Association sel = batch.getSelectedAssociations(0);
    EXPECT(sel.rows() == 3);
    for (int r = 0; r < 3; ++r) EXPECT(sel(r, 0) == sel(r, 1));
  }
  // the solver state is untouched
  const std::vector<clipper::Solution> again = batch.solve(probs);
  for (size_t i = 0; i < probs.size(); ++i) {
    EXPECT(again[i].nodes == first[i].nodes && again[i].u.size() == first[i].u.size());
    EXPECT(std::memcmp(again[i].u.data(), first[i].u.data(), sizeof(double) * static_cast<size_t>(first[i].u.size())) == 0);
  }
  std::printf("ALL BATCH MAXCLIQUE FACADE TESTS PASSED\n");
  return 0;
}
