// test_batch_custom_facade.cpp — clipper::CLIPPERBatch::withDeviceInvariant (include/clipper/batch.h): a batch scored
// by a DeviceInvariant gives per problem what a lone clipper::CLIPPER with the same DeviceInvariant gives with the same
// inputs and u0 (nodes, score, ifinal, u bit for bit, selected associations); problems of another dimension are
// refused; the public constructor still refuses the DeviceInvariant. Plain asserts (no gtest in the image). Compiled
// by tests/test_batch_custom_cpu.py, built and run on the GPU box by tests/test_gpu_batch_custom.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include <clipper/batch.h>
#include <clipper/clipper.h>
#include <clipper/invariants/device.h>
#include <clipper/utils.h>

#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

// EuclideanDistance restated; params = {sigma, epsilon, mindist}
static const char* kEuclid = R"(
__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi, const double* bj,
                                    const double* params) {
  double s1 = 0.0, s2 = 0.0;
  for (int k = 0; k < CLIPPER_D; ++k) {
    const double t1 = ai[k] - aj[k];
    const double t2 = bi[k] - bj[k];
    s1 = fma(t1, t1, s1);
    s2 = fma(t2, t2, s2);
  }
  const double l1 = sqrt(s1), l2 = sqrt(s2);
  if (params[2] > 0 && (l1 < params[2] || l2 < params[2])) return 0.0;
  const double c = fabs(l1 - l2);
  return (c < params[1]) ? exp(-0.5 * c * c / (params[0] * params[0])) : 0.0;
}
)";

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
  auto inv = std::make_shared<clipper::invariants::DeviceInvariant>(kEuclid, std::vector<double>{0.015, 0.05, 0.0});
  bool threw = false;
  try {
    clipper::CLIPPERBatch bad(inv, clipper::Params());  // the constructor: built-ins only
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);

  std::vector<clipper::BatchProblem> probs;
  const int ms[] = {40, 200, 700, 1300};
  for (int k = 0; k < 4; ++k) probs.push_back(make_problem(ms[k] / 2 + 10, ms[k], 0.5, 300u + k));
  probs.push_back(make_problem(50, 100, 0.5, 400u));
  probs.back().u0 = clipper::VectorXd();  // drawn by the batch
  std::unique_ptr<clipper::CLIPPERBatch> batch = clipper::CLIPPERBatch::withDeviceInvariant(inv, clipper::Params());
  const std::vector<clipper::Solution> sols = batch->solve(probs);
  EXPECT(sols.size() == probs.size());
  int batched = 0;
  for (size_t i = 0; i < probs.size(); ++i) {
    clipper::CLIPPER lone(inv, clipper::Params());
    lone.scorePairwiseConsistency(probs[i].D1, probs[i].D2, probs[i].A);
    lone.solve(sols[i].u0);  // (the u0 the batch used, drawn or given)
    const clipper::Solution& s = lone.getSolution();
    const bool same_route = batch->solvedBatched(static_cast<int>(i)) == lone.lastSolveWasResident();
    EXPECT(same_route);
    batched += batch->solvedBatched(static_cast<int>(i)) ? 1 : 0;
    EXPECT(s.nodes == sols[i].nodes);
    EXPECT(s.score == sols[i].score && s.ifinal == sols[i].ifinal);
    EXPECT(s.u.size() == sols[i].u.size());
    EXPECT(std::memcmp(s.u.data(), sols[i].u.data(), sizeof(double) * static_cast<size_t>(s.u.size())) == 0);
    const clipper::Association a = lone.getSelectedAssociations(), b = batch->getSelectedAssociations(static_cast<int>(i));
    EXPECT(a.rows() == b.rows());
    for (int r = 0; r < a.rows(); ++r) EXPECT(a(r, 0) == b(r, 0) && a(r, 1) == b(r, 1));
  }
  EXPECT(batched >= 1);

  // every problem has the invariant's rows
  std::vector<clipper::BatchProblem> mixed = {probs[0], probs[1]};
  mixed[1].D1 = clipper::invariants::Data::Zero(2, mixed[1].D1.cols());
  threw = false;
  try {
    batch->solve(mixed);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);
  EXPECT(batch->solve({probs[2]}).size() == 1);  // the batch goes on working
  EXPECT(batch->solve({}).empty());
  std::printf("batch custom facade ok (%zu problems, %d batched)\n", probs.size(), batched);
  return 0;
}
