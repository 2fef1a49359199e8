// test_batch_facade.cpp — clipper::CLIPPERBatch (include/clipper/batch.h): a batch of random registration problems
// gives per problem what a lone clipper::CLIPPER gives with the same inputs and u0 (nodes, score, ifinal, u bit for
// bit, selected associations); an empty u0 draws utils::randvec; a user-defined invariant is refused.
// Plain asserts (no gtest in the image). Built and run on the GPU box by tests/test_gpu_batch.py.
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

#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

struct Custom : clipper::invariants::PairwiseInvariant {
  double operator()(const clipper::invariants::Datum&, const clipper::invariants::Datum&,
                    const clipper::invariants::Datum&, const clipper::invariants::Datum&) override {
    return 1.0;
  }
};

// n points in the unit cube, the same moved by a rotation about z and a translation; m associations of which the first
// m * (1 - rho) are the true ones
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

int main() {
  clipper::invariants::EuclideanDistance::Params ip;
  ip.sigma = 0.015;
  ip.epsilon = 0.05;
  auto inv = std::make_shared<clipper::invariants::EuclideanDistance>(ip);
  bool threw = false;
  try {
    clipper::CLIPPERBatch bad(std::make_shared<Custom>(), clipper::Params());
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);

  std::vector<clipper::BatchProblem> probs;
  const int ms[] = {40, 200, 700, 1300};
  for (int k = 0; k < 4; ++k) probs.push_back(make_problem(ms[k] / 2 + 10, ms[k], 0.5, 100u + k));
  probs.push_back(make_problem(50, 100, 0.5, 200u));
  probs.back().u0 = clipper::VectorXd();  // drawn by the batch
  clipper::CLIPPERBatch batch(inv, clipper::Params());
  const std::vector<clipper::Solution> sols = batch.solve(probs);
  EXPECT(sols.size() == probs.size());
  for (size_t i = 0; i < probs.size(); ++i) {
    clipper::CLIPPER lone(inv, clipper::Params());
    lone.scorePairwiseConsistency(probs[i].D1, probs[i].D2, probs[i].A);
    lone.solve(sols[i].u0);  // (the u0 the batch used, drawn or given)
    const clipper::Solution& s = lone.getSolution();
    const bool same_route = batch.solvedBatched(static_cast<int>(i)) == lone.lastSolveWasResident();
    EXPECT(same_route);
    EXPECT(s.nodes == sols[i].nodes);
    EXPECT(s.score == sols[i].score && s.ifinal == sols[i].ifinal);
    EXPECT(s.u.size() == sols[i].u.size());
    EXPECT(std::memcmp(s.u.data(), sols[i].u.data(), sizeof(double) * static_cast<size_t>(s.u.size())) == 0);
    const clipper::Association a = lone.getSelectedAssociations(), b = batch.getSelectedAssociations(static_cast<int>(i));
    EXPECT(a.rows() == b.rows());
    for (int r = 0; r < a.rows(); ++r) EXPECT(a(r, 0) == b(r, 0) && a(r, 1) == b(r, 1));
  }
  EXPECT(batch.solve({}).empty());
  std::printf("batch facade ok (%zu problems)\n", probs.size());
  return 0;
}
