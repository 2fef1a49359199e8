// match_probe_kernels.hip — helper of tools/match_probe.py: the search kernels of descriptor matching alone, timed with
// hipEvents, and the same search by brute force on the host cores.
//   match_probe_kernels n d [reps]       (n0 = n1 = n, knn = 1; prints one JSON line)
// Device: k_match_partial<1, G> + k_knn_merge<1> with the geometry of host_match.hpp, forward and backward searches
// timed one by one and queued back to back as the driver queues them; at d = 3 also k_knn_partial<1, 3> on the same
// clouds (unpadded rows). Medians of `reps` after one warm-up.
// Host: C++, the direct form (dist = dist + (q[k] - p[k]) * (q[k] - p[k]) in coordinate order), 16 std::threads over
// the queries, four candidates at a time so that the additions of different candidates overlap; both directions. From
// n = 100 000 on only 10 000 queries per direction are searched and the time is scaled by n / 10 000 (the search is
// linear in the queries): "host_extrapolated" says so.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I clipper_amd/csrc tools/match_probe_kernels.hip -o tools/_bin/match_probe_kernels -lpthread
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "k_match.hip.h"

using namespace clipper_hip;

#define CK(e)                                                                              \
  do {                                                                                     \
    hipError_t e_ = (e);                                                                   \
    if (e_ != hipSuccess) {                                                                \
      std::fprintf(stderr, "%s failed: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__); \
      std::exit(2);                                                                        \
    }                                                                                      \
  } while (0)

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct Geom {
  int S;
  int64_t chunk;
};
static Geom geom(int64_t nq, int64_t nc) {  // host_knn.hpp: knn_geom
  const int64_t qblocks = ceil_div(nq, 256), tiles = ceil_div(nc, KNN_TILE);
  const int S = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(tiles, ceil_div(512, qblocks))));
  return {S, ceil_div(tiles, S) * KNN_TILE};
}

struct Bufs {
  double *pd, *od;
  int32_t *pi, *oi;
};

template <int G>
static void search(const double* Q, const double* C, int64_t n, const Geom& g, const Bufs& b) {
  const unsigned qb = static_cast<unsigned>(ceil_div(n, 256));
  hipLaunchKernelGGL((k_match_partial<1, G>), dim3(qb, static_cast<unsigned>(g.S)), dim3(256), 0, nullptr, Q, n, C, n,
                     g.chunk, b.pd, b.pi);
  hipLaunchKernelGGL((k_knn_merge<1>), dim3(qb), dim3(256), 0, nullptr, b.pd, b.pi, n, g.S, b.od, b.oi);
}
static void search_g(int G, const double* Q, const double* C, int64_t n, const Geom& g, const Bufs& b) {
  if (G == 1) search<1>(Q, C, n, g, b);
  else if (G == 5) search<5>(Q, C, n, g, b);
  else search<8>(Q, C, n, g, b);
}
static void search_knn3(const double* Q, const double* C, int64_t n, const Geom& g, const Bufs& b) {
  const unsigned qb = static_cast<unsigned>(ceil_div(n, 256));
  hipLaunchKernelGGL((k_knn_partial<1, 3>), dim3(qb, static_cast<unsigned>(g.S)), dim3(256), 0, nullptr, Q, n, C, n,
                     g.chunk, b.pd, b.pi);
  hipLaunchKernelGGL((k_knn_merge<1>), dim3(qb), dim3(256), 0, nullptr, b.pd, b.pi, n, g.S, b.od, b.oi);
}

template <typename F>
static double median_ms(int reps, F&& run) {
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  std::vector<float> ms;
  for (int r = 0; r <= reps; ++r) {
    CK(hipEventRecord(e0, nullptr));
    run();
    CK(hipEventRecord(e1, nullptr));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float t = 0.f;
    CK(hipEventElapsedTime(&t, e0, e1));
    if (r) ms.push_back(t);  // (the first run is the warm-up)
  }
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  std::sort(ms.begin(), ms.end());
  return ms[ms.size() / 2];
}

// the nearest row of C to each of the rows [q0, q1) of Q, direct form, ties to the lower index
static void host_search(const double* Q, const double* C, int64_t q0, int64_t q1, int64_t nc, int d, int32_t* out) {
  for (int64_t i = q0; i < q1; ++i) {
    const double* q = Q + i * d;
    double best = 1e300;
    int32_t bi = -1;
    int64_t t = 0;
    for (; t + 4 <= nc; t += 4) {
      double s[4] = {0.0, 0.0, 0.0, 0.0};
      for (int k = 0; k < d; ++k)
        for (int u = 0; u < 4; ++u) {
          const double df = q[k] - C[(t + u) * d + k];
          s[u] = s[u] + df * df;
        }
      for (int u = 0; u < 4; ++u)
        if (s[u] < best) {
          best = s[u];
          bi = static_cast<int32_t>(t + u);
        }
    }
    for (; t < nc; ++t) {
      double s = 0.0;
      for (int k = 0; k < d; ++k) {
        const double df = q[k] - C[t * d + k];
        s = s + df * df;
      }
      if (s < best) {
        best = s;
        bi = static_cast<int32_t>(t);
      }
    }
    out[i - q0] = bi;
  }
}

static double host_direction(const double* Q, const double* C, int64_t nq, int64_t nc, int d, int threads,
                             std::vector<int32_t>& out) {
  out.assign(static_cast<size_t>(nq), -1);
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> pool;
  const int64_t per = ceil_div(nq, threads);
  for (int w = 0; w < threads; ++w) {
    const int64_t a = std::min<int64_t>(nq, w * per), b = std::min<int64_t>(nq, a + per);
    if (a < b) pool.emplace_back(host_search, Q, C, a, b, nc, d, out.data() + a);
  }
  for (auto& th : pool) th.join();
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: match_probe_kernels n d [reps]\n");
    return 2;
  }
  const int64_t n = std::atoll(argv[1]);
  const int d = std::atoi(argv[2]);
  const int reps = argc > 3 ? std::atoi(argv[3]) : 5;
  if (n < 1 || n > (int64_t(1) << 24) || (d != 3 && d != 33 && d != 64) || reps < 1) {
    std::fprintf(stderr, "n in 1..2^24, d in {3, 33, 64}, reps >= 1\n");
    return 2;
  }
  const int G = d <= 8 ? 1 : (d <= 40 ? 5 : 8), dp = 8 * G;
  std::mt19937_64 rng(12345 + n + d);
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<double> F0(static_cast<size_t>(n) * d), F1(F0.size());
  for (auto& v : F0) v = uni(rng);
  for (auto& v : F1) v = uni(rng);
  std::vector<double> P0(static_cast<size_t>(n) * dp, 0.0), P1(P0.size(), 0.0);
  for (int64_t p = 0; p < n; ++p)
    for (int k = 0; k < d; ++k) {
      P0[p * dp + k] = F0[p * d + k];
      P1[p * dp + k] = F1[p * d + k];
    }

  const Geom g = geom(n, n);
  double *d0, *d1, *u0 = nullptr, *u1 = nullptr;
  Bufs f{}, b{};
  const size_t np = static_cast<size_t>(g.S) * n;
  CK(hipMalloc(&d0, P0.size() * sizeof(double)));
  CK(hipMalloc(&d1, P1.size() * sizeof(double)));
  CK(hipMemcpy(d0, P0.data(), P0.size() * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemcpy(d1, P1.data(), P1.size() * sizeof(double), hipMemcpyHostToDevice));
  for (Bufs* x : {&f, &b}) {
    CK(hipMalloc(&x->pd, np * sizeof(double)));
    CK(hipMalloc(&x->pi, np * sizeof(int32_t)));
    CK(hipMalloc(&x->od, n * sizeof(double)));
    CK(hipMalloc(&x->oi, n * sizeof(int32_t)));
  }
  const double fwd = median_ms(reps, [&] { search_g(G, d0, d1, n, g, f); });
  const double bwd = median_ms(reps, [&] { search_g(G, d1, d0, n, g, b); });
  const double both = median_ms(reps, [&] {
    search_g(G, d0, d1, n, g, f);
    search_g(G, d1, d0, n, g, b);
  });
  std::vector<int32_t> gi(static_cast<size_t>(n));
  CK(hipMemcpy(gi.data(), f.oi, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  double knn3 = -1.0;
  if (d == 3) {  // the coordinate kernel on the same clouds, rows of 3
    CK(hipMalloc(&u0, F0.size() * sizeof(double)));
    CK(hipMalloc(&u1, F1.size() * sizeof(double)));
    CK(hipMemcpy(u0, F0.data(), F0.size() * sizeof(double), hipMemcpyHostToDevice));
    CK(hipMemcpy(u1, F1.data(), F1.size() * sizeof(double), hipMemcpyHostToDevice));
    knn3 = median_ms(reps, [&] { search_knn3(u0, u1, n, g, b); });
    std::vector<int32_t> ki(static_cast<size_t>(n));
    CK(hipMemcpy(ki.data(), b.oi, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (ki != gi) {
      std::fprintf(stderr, "k_match and k_knn disagree at d = 3\n");
      return 1;
    }
  }

  const int threads = 16;
  const int64_t nq = n >= 100000 ? 10000 : n;  // queries searched on the host per direction
  std::vector<int32_t> hi, hb;
  double host = host_direction(F0.data(), F1.data(), nq, n, d, threads, hi);
  host += host_direction(F1.data(), F0.data(), nq, n, d, threads, hb);
  host *= static_cast<double>(n) / static_cast<double>(nq);
  for (int64_t i = 0; i < nq; ++i)
    if (hi[i] != gi[i]) {
      std::fprintf(stderr, "device and host disagree at query %lld\n", static_cast<long long>(i));
      return 1;
    }
  std::printf("{\"n\": %lld, \"d\": %d, \"groups\": %d, \"chunks\": %d, \"forward_ms\": %.4f, \"backward_ms\": %.4f, "
              "\"search_ms\": %.4f, \"knn_d3_forward_ms\": %s, \"host_ms\": %.2f, \"host_threads\": %d, "
              "\"host_extrapolated\": %s, \"host_queries\": %lld}\n",
              static_cast<long long>(n), d, G, g.S, fwd, bwd, both,
              knn3 < 0 ? "null" : std::to_string(knn3).c_str(), host, threads, nq < n ? "true" : "false",
              static_cast<long long>(nq));
  return 0;
}
