// test_device_invariant_facade.cpp — clipper::invariants::DeviceInvariant through the clipper::CLIPPER facade: the
// reference's golden case (test/affinity_test.cpp:33-48: 4 model points, 3 data points, all-to-all) scored by
// EuclideanDistance restated as device source gives the built-in's matrix and solution, on one device and on two column
// shards (setDevices); the host call throws; CLIPPERBatch refuses it; a source that does not compile throws with the
// compiler's message. Plain asserts (no gtest in the image). Built and run on the GPU box by
// tests/test_gpu_device_invariant.py.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <clipper/batch.h>
#include <clipper/clipper.h>
#include <clipper/invariants/device.h>
#include <clipper/utils.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

// EuclideanDistance (euclidean_distance.cpp:13-31) as device source: params = {sigma, epsilon, mindist}
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

int main() {
  using namespace clipper;
  invariants::Data model = invariants::Data::Zero(3, 4), data = invariants::Data::Zero(3, 3);
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
  invariants::EuclideanDistance::Params ip;
  auto builtin = std::make_shared<invariants::EuclideanDistance>(ip);
  auto device = std::make_shared<invariants::DeviceInvariant>(kEuclid, std::vector<double>{ip.sigma, ip.epsilon, ip.mindist});
  EXPECT(device->params().size() == 3 && device->source() == kEuclid);

  CLIPPER ref(builtin, Params());
  ref.scorePairwiseConsistency(model, data);
  ref.solve();
  const Affinity Mref = ref.getAffinityMatrix();
  for (int shards = 1; shards <= 2; ++shards) {
    CLIPPER c(device, Params());
    if (shards == 2) c.setDevices({0, 0});
    c.scorePairwiseConsistency(model, data);  // all-to-all
    const Affinity M = c.getAffinityMatrix();
    EXPECT(M.rows() == 12 && M.cols() == 12);
    for (int j = 0; j < 12; ++j)
      for (int i = 0; i < 12; ++i) EXPECT(M(i, j) == Mref(i, j));
    VectorXd u0(12);
    for (int i = 0; i < 12; ++i) u0(i) = 1.0 / std::sqrt(12.0);
    c.solve(u0);
    ref.solve(u0);
    const Solution& s = c.getSolution();
    EXPECT(s.nodes == ref.getSolution().nodes);
    std::vector<int> sorted(s.nodes.begin(), s.nodes.end());
    std::sort(sorted.begin(), sorted.end());
    for (int v : sorted) std::printf("%d ", v);
    std::printf("<- nodes (%d shard(s))\n", shards);
    EXPECT(sorted == std::vector<int>({0, 4, 8}));
    EXPECT(s.score == ref.getSolution().score && s.ifinal == ref.getSolution().ifinal);
    std::printf("DeviceInvariant, %d shard(s): nodes {0, 4, 8}, score %.12f\n", shards, s.score);
  }

  bool threw = false;
  try {
    (*device)(VectorXd::Zero(3), VectorXd::Zero(3), VectorXd::Zero(3), VectorXd::Zero(3));
  } catch (const std::logic_error&) {
    threw = true;
  }
  EXPECT(threw);

  threw = false;
  try {
    CLIPPERBatch b(device, Params());
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  EXPECT(threw);

  threw = false;
  try {
    CLIPPER c(std::make_shared<invariants::DeviceInvariant>("__device__ double clipper_invariant(;"), Params());
    c.scorePairwiseConsistency(model, data);
  } catch (const std::runtime_error& e) {
    threw = std::string(e.what()).find("invariant:1:") != std::string::npos;
    std::printf("compile error: %.120s...\n", e.what());
  }
  EXPECT(threw);

  std::printf("ALL DEVICE INVARIANT FACADE TESTS PASSED\n");
  return 0;
}
