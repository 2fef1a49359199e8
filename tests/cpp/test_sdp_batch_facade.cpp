// test_sdp_batch_facade.cpp — the batched semidefinite relaxation through the clipper:: facade: sdp::solve on lists of
// M and C gives per problem what sdp::solve gives on it alone (bit for bit), and CLIPPERBatch::solveAsMSRCSDR gives per
// problem what CLIPPER::solveAsMSRCSDR with setDeviceSdp gives on a lone CLIPPER; sdpSolutions() carries the bounds.
// Plain asserts (no gtest in the image). Built and run on the GPU box by tests/test_gpu_sdp_batch.py, which passes a
// file that holds the golden 20 x 20 M.
#include <algorithm>
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
#include <clipper/sdp.h>
#include <clipper/utils.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static bool same_bits(const double* a, const double* b, size_t n) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

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

  // ---- sdp::solve on lists: the golden problem, a clique of 3 among 9 nodes, a lone node
  clipper::MatrixXd K = clipper::MatrixXd::Zero(9, 9);
  for (int i = 0; i < 9; ++i) K(i, i) = 1.0;
  for (int i : {1, 4, 7})
    for (int j : {1, 4, 7}) K(i, j) = 1.0;
  K(2, 3) = K(3, 2) = 1.0;
  clipper::MatrixXd one = clipper::MatrixXd::Zero(1, 1);
  one(0, 0) = 1.0;
  const std::vector<clipper::MatrixXd> Ms = {M, K, one, M}, Cs = {C, K, one, C};
  const std::vector<clipper::sdp::Solution> sols = clipper::sdp::solve(Ms, Cs, p);
  EXPECT(sols.size() == Ms.size());
  for (size_t i = 0; i < Ms.size(); ++i) {
    const clipper::sdp::Solution lone = clipper::sdp::solve(Ms[i], Cs[i], p);
    const clipper::sdp::Solution& s = sols[i];
    const size_t m = static_cast<size_t>(Ms[i].rows());
    EXPECT(s.nodes == lone.nodes && s.iters == lone.iters && s.thr == lone.thr);
    EXPECT(s.pobj == lone.pobj && s.dobj == lone.dobj && s.t > 0);
    EXPECT(static_cast<size_t>(s.X.rows()) == m && static_cast<size_t>(s.lambdas.size()) == m);
    EXPECT(same_bits(s.X.data(), lone.X.data(), m * m));
    EXPECT(same_bits(s.evec1.data(), lone.evec1.data(), m) && same_bits(s.lambdas.data(), lone.lambdas.data(), m));
  }
  EXPECT((sols[1].nodes == std::vector<int>{1, 4, 7}) && std::fabs(sols[1].pobj + 3.0f) < 1e-3f);
  EXPECT((sols[2].nodes == std::vector<int>{0}));
  EXPECT(clipper::sdp::solve(std::vector<clipper::MatrixXd>{}, std::vector<clipper::MatrixXd>{}, p).empty());
  bool threw = false;
  try {
    clipper::sdp::solve(std::vector<clipper::MatrixXd>{M, clipper::MatrixXd::Zero(129, 129)},
                        std::vector<clipper::MatrixXd>{C, clipper::MatrixXd::Zero(129, 129)}, p);
  } catch (const std::runtime_error& e) {
    threw = std::strstr(e.what(), "problem 1") != nullptr && std::strstr(e.what(), "limit of 128") != nullptr;
  }
  EXPECT(threw);

  // ---- CLIPPERBatch::solveAsMSRCSDR against lone CLIPPERs
  clipper::invariants::EuclideanDistance::Params ip;
  ip.sigma = 0.015;
  ip.epsilon = 0.05;
  auto inv = std::make_shared<clipper::invariants::EuclideanDistance>(ip);
  std::vector<clipper::BatchProblem> probs;
  const int ms[] = {30, 64, 101, 128};
  for (int k = 0; k < 4; ++k) probs.push_back(make_problem(ms[k] / 2 + 10, ms[k], 0.5, 100u + k));
  clipper::CLIPPERBatch batch(inv, clipper::Params());
  threw = false;
  try {
    batch.solveAsMSRCSDR(p);
  } catch (const std::logic_error&) {
    threw = true;
  }
  EXPECT(threw);
  const std::vector<clipper::Solution> first = batch.solve(probs);
  p.eps_abs = 1e-5f;
  p.eps_rel = 1e-5f;
  const std::vector<clipper::Solution> out = batch.solveAsMSRCSDR(p);
  const std::vector<clipper::sdp::Solution>& full = batch.sdpSolutions();
  EXPECT(out.size() == probs.size() && full.size() == probs.size());
  for (size_t i = 0; i < probs.size(); ++i) {
    clipper::CLIPPER lone(inv, clipper::Params());
    lone.scorePairwiseConsistency(probs[i].D1, probs[i].D2, probs[i].A);
    lone.setDeviceSdp(true);
    lone.solveAsMSRCSDR(p);
    const clipper::Solution& c = lone.getSolution();
    EXPECT(c.nodes == out[i].nodes && !out[i].nodes.empty());
    EXPECT(out[i].score == -1 && out[i].ifinal == 0 && out[i].t > 0);
    EXPECT(out[i].u.size() == c.u.size());
    for (int k = 0; k < out[i].u.size(); ++k) EXPECT(out[i].u(k) == 0.0);
    EXPECT(full[i].nodes == out[i].nodes && full[i].iters > 0);
    // the bound certifies the dense-cluster answer: -dobj >= u^T (M + I) u for the unit, non-negative u of solve()
    // (sdp::Solution::dobj is a float: the last term covers its rounding)
    const clipper::Affinity A = lone.getAffinityMatrix();
    const clipper::VectorXd& u = first[i].u;
    double val = 0;
    for (int a = 0; a < u.size(); ++a)
      for (int b = 0; b < u.size(); ++b) val += u(a) * A(a, b) * u(b);
    EXPECT(-static_cast<double>(full[i].dobj) >= val - (1e-5 + 1e-5 * std::fabs(full[i].dobj) + 1e-6) - 1e-5 * std::fabs(val));
    const clipper::Association sa = lone.getSelectedAssociations(), sb = batch.getSelectedAssociations(static_cast<int>(i));
    EXPECT(sa.rows() == sb.rows());
    for (int r = 0; r < sa.rows(); ++r) EXPECT(sa(r, 0) == sb(r, 0) && sa(r, 1) == sb(r, 1));
  }
  // the solver state is untouched
  const std::vector<clipper::Solution> again = batch.solve(probs);
  for (size_t i = 0; i < probs.size(); ++i) {
    EXPECT(again[i].nodes == first[i].nodes && again[i].u.size() == first[i].u.size());
    EXPECT(same_bits(again[i].u.data(), first[i].u.data(), static_cast<size_t>(first[i].u.size())));
  }
  EXPECT(batch.sdpSolutions().empty());  // (dropped with the solve they belonged to)
  std::printf("ALL SDP BATCH FACADE TESTS PASSED\n");
  return 0;
}
