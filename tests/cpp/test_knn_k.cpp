// host_knn_k.hpp with g++ alone: the list-length rule against a plain loop, and the dispatcher over every list of
// instantiated values a launch site names (the body runs exactly once with the exact K, or not at all).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_knn_k.hpp"

using clipper_hip::dispatch_k;
using clipper_hip::knn_list_k;

static int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
      ++failures;                                                   \
    }                                                               \
  } while (0)

// the smallest power of two >= len, clamped to [kmin, kmax]
static int list_k_by_loop(int len, int kmin, int kmax) {
  int p = 1;
  while (p < len) p *= 2;
  return p < kmin ? kmin : (p > kmax ? kmax : p);
}

static void list_lengths() {
  const int clamps[3][2] = {{1, 16}, {1, 8}, {4, 32}};  // knn_search, match_descriptors, features_run
  for (const auto& c : clamps)
    for (int len = 0; len <= 40; ++len) EXPECT(knn_list_k(len, c[0], c[1]) == list_k_by_loop(len, c[0], c[1]));
}

// one list: every member runs the body once with itself; the K of `outside` run nothing and come back false
template <int... Ks>
static void one_list(const std::vector<int>& outside) {
  for (int K : {Ks...}) {
    int calls = 0, seen = -1;
    const bool found = dispatch_k<Ks...>(K, [&](auto k) {
      ++calls;
      seen = decltype(k)::value;
    });
    EXPECT(found && calls == 1 && seen == K);
  }
  for (int K : outside) {
    int calls = 0;
    EXPECT(!dispatch_k<Ks...>(K, [&](auto) { ++calls; }) && calls == 0);
  }
}

int main() {
  list_lengths();
  one_list<1, 2, 4, 8, 16, 32>({0, 3, 5, 64, -1});     // the grid query; brute force, d = 3
  one_list<1, 2, 4, 8, 16>({0, 3, 5, 64, 32});         // brute force, d = 2
  one_list<1, 2, 4, 8>({0, 3, 5, 64, 16, 32});         // match: K
  one_list<1, 2, 4, 5, 8>({0, 3, 6, 7, 64, 16});       // match: G
  one_list<4, 8, 16, 32>({0, 1, 2, 3, 5, 64});         // SPFH
  if (failures) return 1;
  std::printf("knn k ok\n");
  return 0;
}
