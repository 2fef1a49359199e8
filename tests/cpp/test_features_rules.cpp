// test_features_rules.cpp — features_rules.hpp and host_features_check.hpp on the host (g++ only, no HIP): the pair
// feature's bins of the pairs in a file and the normals of the neighbourhoods in a file go to stdout for
// tests/test_features_model.py to compare with the numpy model; the Jacobi is checked here against matrices whose
// eigenvectors are known; every refusal of the argument checks is checked with its message. Plain asserts.
//   test_features_rules pairs.f64 m nbrs.f64 g k
// pairs.f64: m rows of p1 n1 p2 n2 (12 doubles); nbrs.f64: g neighbourhoods of k points (3 doubles each), the first
// point of each being the point the normal belongs to. Normals are printed twice: largest component positive, and
// towards the viewpoint (0.5, 0.5, 3).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "host_features_check.hpp"

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

using namespace clipper_hip;
namespace cf = clipper_features;

static std::vector<double> read(const char* path, size_t count) {
  std::vector<double> v(count);
  FILE* f = std::fopen(path, "rb");
  EXPECT(f != nullptr);
  EXPECT(std::fread(v.data(), sizeof(double), count, f) == count);
  std::fclose(f);
  return v;
}

static void known_eigenvectors() {
  double nv[3], ev[3];
  // diagonal: no rotation at all, the smallest entry's axis; ties keep the first
  const double d0[6] = {3.0, 0.0, 0.0, 1.0, 0.0, 2.0};
  feat_smallest_eigenvector(d0, nv, ev);
  EXPECT(nv[0] == 0.0 && nv[1] == 1.0 && nv[2] == 0.0 && ev[1] == 1.0);
  const double d1[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 2.0};
  feat_smallest_eigenvector(d1, nv, nullptr);
  EXPECT(nv[0] == 1.0 && nv[1] == 0.0 && nv[2] == 0.0);
  // the plane x + y + z = 0 seen as the covariance I - (1/3) 1 1^T: smallest eigenvector (1, 1, 1) / sqrt(3)
  const double t = 1.0 / 3.0;
  const double pl[6] = {1.0 - t, -t, -t, 1.0 - t, -t, 1.0 - t};
  feat_smallest_eigenvector(pl, nv, ev);
  const double r = 1.0 / std::sqrt(3.0);
  for (int k = 0; k < 3; ++k) EXPECT(std::fabs(std::fabs(nv[k]) - r) < 1e-14);
  EXPECT(nv[0] * nv[1] > 0 && nv[0] * nv[2] > 0);
  // a line (rank one): the normal is orthogonal to it and of unit length; all zeros: still a unit vector
  const double ln[6] = {1.0, 2.0, 3.0, 4.0, 6.0, 9.0};
  feat_smallest_eigenvector(ln, nv, nullptr);
  EXPECT(std::fabs(nv[0] + 2.0 * nv[1] + 3.0 * nv[2]) < 1e-13);
  EXPECT(std::fabs(feat_dot(nv, nv) - 1.0) < 1e-15);
  const double z[6] = {0, 0, 0, 0, 0, 0};
  feat_smallest_eigenvector(z, nv, nullptr);
  EXPECT(feat_dot(nv, nv) == 1.0);
  // the sign rule: first of the largest components on ties; towards the viewpoint
  double a[3] = {-0.6, 0.6, 0.52915026221291817};
  const double p[3] = {0, 0, 0}, view[3] = {0, -1, 0};
  feat_orient(a, p, nullptr);
  EXPECT(a[0] == 0.6 && a[1] == -0.6);
  feat_orient(a, p, view);
  EXPECT(a[0] == 0.6 && a[1] == -0.6);
  const double view2[3] = {0, 1, 0};
  feat_orient(a, p, view2);
  EXPECT(a[0] == -0.6 && a[1] == 0.6);
}

static void bins_at_the_edges() {
  EXPECT(feat_bin(-0.5) == 0 && feat_bin(0.0) == 0 && feat_bin(0.999) == 0 && feat_bin(1.0) == 1);
  EXPECT(feat_bin(10.999) == 10 && feat_bin(11.0) == 10 && feat_bin(12.5) == 10);
  const double zero[3] = {0.0, 0.0, 0.0};
  int b[3];
  feat_bins(zero, b);  // the degenerate pair's feature
  EXPECT(b[0] == 5 && b[1] == 16 && b[2] == 27);
  EXPECT(feat_spfh_scale(1) == 0.0 && feat_spfh_scale(2) == 100.0 && feat_spfh_scale(5) == 25.0);
  EXPECT(feat_kept(3, 4.0, true, 4.0) && !feat_kept(3, std::nextafter(4.0, 5.0), true, 4.0));  // on the radius: kept
  EXPECT(feat_kept(3, 1e9, false, 4.0) && !feat_kept(-1, 0.0, false, 4.0));
  EXPECT(!feat_weighs(2, 2, 1.0) && !feat_weighs(3, 2, 0.0) && feat_weighs(3, 2, 1.0));
  EXPECT(feat_fpfh_bin(3.0, 0.0, 1.0) == 4.0 && feat_fpfh_bin(3.0, 50.0, 1.0) == 7.0);
}

static void refusals() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  cf::Neighborhood nb{16, 0.0};
  EXPECT(cf::check_neighborhood("neighbourhood", &nb).empty());
  EXPECT(cf::check_neighborhood("neighbourhood", nullptr) == "null neighbourhood");
  nb.knn = 2;
  EXPECT(cf::check_neighborhood("neighbourhood", &nb) == "neighbourhood: knn must be in 3..32 (knn = 2)");
  nb.knn = 33;
  EXPECT(cf::check_neighborhood("feature neighbourhood", &nb) == "feature neighbourhood: knn must be in 3..32 (knn = 33)");
  nb.knn = 3;
  EXPECT(cf::check_neighborhood("neighbourhood", &nb).empty());
  nb.knn = 32;
  nb.radius = -1.0;  // off
  EXPECT(cf::check_neighborhood("neighbourhood", &nb).empty());
  nb.radius = inf;
  EXPECT(cf::check_neighborhood("neighbourhood", &nb) == "neighbourhood: radius must be finite (radius = inf)");
  nb.radius = nan;
  EXPECT(cf::check_neighborhood("neighbourhood", &nb).find("radius must be finite") != std::string::npos);
  EXPECT(cf::check_count(0) == "a cloud needs at least one point (n = 0)");
  EXPECT(cf::check_count(-3) == "a cloud needs at least one point (n = -3)");
  EXPECT(cf::check_count(1).empty());
  double P[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
  EXPECT(cf::check_points(P, 3).empty());
  P[7] = nan;
  EXPECT(cf::check_points(P, 3) == "P: non-finite value at coordinate 1 of point 2");
  P[7] = 1.0;
  P[3] = -inf;
  EXPECT(cf::check_points(P, 3) == "P: non-finite value at coordinate 0 of point 1");
  double N[6] = {0, 0, 1, 0.6, 0.8, 0};
  EXPECT(cf::check_normals(N, 2).empty());
  N[5] = 0.2;
  EXPECT(cf::check_normals(N, 2).find("N: normal 1 is not of unit length (squared length = 1.04") == 0);
  N[5] = 0.09;  // 1.0081: inside
  EXPECT(cf::check_normals(N, 2).empty());
  N[3] = N[4] = N[5] = 0.0;
  EXPECT(cf::check_normals(N, 2) == "N: normal 1 is not of unit length (squared length = 0)");
  N[2] = nan;
  EXPECT(cf::check_normals(N, 2) == "N: non-finite value at coordinate 2 of normal 0");
  const double v[3] = {0, inf, 0};
  EXPECT(cf::check_viewpoint(nullptr).empty() && cf::check_viewpoint(P + 6).empty());
  EXPECT(cf::check_viewpoint(v) == "viewpoint: non-finite value at coordinate 1");
  EXPECT(cf::list_k(3) == 4 && cf::list_k(4) == 4 && cf::list_k(5) == 8 && cf::list_k(16) == 16 && cf::list_k(17) == 32 &&
         cf::list_k(32) == 32);
}

int main(int argc, char** argv) {
  known_eigenvectors();
  bins_at_the_edges();
  refusals();
  EXPECT(argc == 6);
  const long m = std::atol(argv[2]), g = std::atol(argv[4]), k = std::atol(argv[5]);
  const std::vector<double> pairs = read(argv[1], static_cast<size_t>(m) * 12), nbrs = read(argv[3], static_cast<size_t>(g * k) * 3);
  for (long r = 0; r < m; ++r) {
    const double* q = pairs.data() + r * 12;
    const double p1[3] = {q[0], q[1], q[2]}, n1[3] = {q[3], q[4], q[5]}, p2[3] = {q[6], q[7], q[8]}, n2[3] = {q[9], q[10], q[11]};
    double f[3];
    int b[3];
    feat_pair(p1, n1, p2, n2, f);
    feat_bins(f, b);
    std::printf("%d %d %d\n", b[0], b[1], b[2]);
  }
  const double view[3] = {0.5, 0.5, 3.0};
  for (long r = 0; r < g; ++r) {
    const double* q = nbrs.data() + r * k * 3;
    const double p[3] = {q[0], q[1], q[2]};
    auto get = [&](int t, double (&x)[3]) {
      x[0] = q[t * 3];
      x[1] = q[t * 3 + 1];
      x[2] = q[t * 3 + 2];
    };
    double a[3], b[3];
    feat_normal(static_cast<int>(k), get, p, nullptr, a);
    feat_normal(static_cast<int>(k), get, p, view, b);
    std::printf("%.17g %.17g %.17g %.17g %.17g %.17g\n", a[0], a[1], a[2], b[0], b[1], b[2]);
  }
  std::printf("features rules ok\n");
  return 0;
}
