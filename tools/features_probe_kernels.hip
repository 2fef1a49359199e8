// features_probe_kernels.hip — helper of tools/features_probe.py: the stages of raw cloud -> normals -> FPFH alone,
// timed with hipEvents, and the same stages by brute force on the host cores.
//   features_probe_kernels n [reps]       (normals knn = 16, features knn = 32, no radius; prints one JSON line)
// Device: the stages as host_features.hpp queues them for clipper_hip_fpfh_from_points: the search of the cloud in
// itself at K = 32 (k_knn_partial<32, 3> + k_knn_merge<32>), k_feat_normals over the first 16 entries, k_feat_spfh<32>,
// k_feat_fpfh; each timed alone and all four queued back to back. Medians of `reps` after one warm-up.
// Host: C++ over features_rules.hpp, 16 std::threads over the points: the direct-form search (dist = dist + df * df in
// coordinate order, sorted insertion into 32 slots), the normals, SPFH and FPFH. From n = 100 000 on only 10 000
// queries are searched and the search time is scaled by n / 10 000 (it is linear in the queries; the lists of the
// other points come from the device): "host_extrapolated" says so.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -I clipper_amd/csrc tools/features_probe_kernels.hip -o tools/_bin/features_probe_kernels -lpthread
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "k_knn.hip.h"
#include "k_features.hip.h"

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
constexpr int K = 32, KN = 16, KF = 32, THREADS = 16;

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

template <typename F>
static double host_ms(int64_t n, F&& body) {  // body(i0, i1) on THREADS threads over [0, n)
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<std::thread> th;
  for (int t = 0; t < THREADS; ++t)
    th.emplace_back([&, t] { body(n * t / THREADS, n * (t + 1) / THREADS); });
  for (auto& x : th) x.join();
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  const int64_t n = std::atoll(argv[1]);
  const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
  std::mt19937_64 gen(static_cast<uint64_t>(n));
  std::uniform_real_distribution<double> uni(0.0, 1.0);
  std::vector<double> P(static_cast<size_t>(n) * 3);
  for (auto& x : P) x = uni(gen);

  const int64_t qblocks = ceil_div(n, 256), tiles = ceil_div(n, KNN_TILE);  // host_knn.hpp: knn_geom
  const int S = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(tiles, ceil_div(512, qblocks))));
  const int64_t chunk = ceil_div(tiles, S) * KNN_TILE;
  const size_t no = static_cast<size_t>(n) * K, np = static_cast<size_t>(S) * no, nf = static_cast<size_t>(n) * FEAT_DIM;
  double *dP, *dN, *pd, *od, *dS, *dF;
  int32_t *pi, *oi, *dc;
  CK(hipMalloc(&dP, P.size() * sizeof(double)));
  CK(hipMalloc(&dN, P.size() * sizeof(double)));
  CK(hipMalloc(&pd, np * sizeof(double)));
  CK(hipMalloc(&pi, np * sizeof(int32_t)));
  CK(hipMalloc(&od, no * sizeof(double)));
  CK(hipMalloc(&oi, no * sizeof(int32_t)));
  CK(hipMalloc(&dS, nf * sizeof(double)));
  CK(hipMalloc(&dF, nf * sizeof(double)));
  CK(hipMalloc(&dc, static_cast<size_t>(n) * sizeof(int32_t)));
  CK(hipMemcpy(dP, P.data(), P.size() * sizeof(double), hipMemcpyHostToDevice));
  const unsigned qb = static_cast<unsigned>(qblocks);
  auto search = [&] {
    hipLaunchKernelGGL((k_knn_partial<K, 3>), dim3(qb, static_cast<unsigned>(S)), dim3(256), 0, nullptr, dP, n, dP, n, chunk,
                       pd, pi);
    hipLaunchKernelGGL((k_knn_merge<K>), dim3(qb), dim3(256), 0, nullptr, pd, pi, n, S, od, oi);
  };
  auto normals = [&] {
    hipLaunchKernelGGL(k_feat_normals<>, dim3(qb), dim3(256), 0, nullptr, dP, n, oi, od, K, KN, 0, 0.0, nullptr, dN, dc);
  };
  auto spfh = [&] {
    hipLaunchKernelGGL((k_feat_spfh<KF>), dim3(static_cast<unsigned>(ceil_div(n, 256 / KF))), dim3(256), 0, nullptr, dP, dN,
                       n, oi, od, K, KF, 0, 0.0, dS, dc);
  };
  auto fpfh = [&] {
    hipLaunchKernelGGL(k_feat_fpfh<>, dim3(static_cast<unsigned>(ceil_div(n, FEAT_FPFH_POINTS))), dim3(256), 0, nullptr, dS, n,
                       oi, od, K, KF, 0, 0.0, dF);
  };
  const double search_ms = median_ms(reps, search), normals_ms = median_ms(reps, normals), spfh_ms = median_ms(reps, spfh),
               fpfh_ms = median_ms(reps, fpfh);
  const double all_ms = median_ms(reps, [&] {
    search();
    normals();
    spfh();
    fpfh();
  });
  std::vector<int32_t> li(no);
  std::vector<double> ld(no), dFh(nf);
  CK(hipMemcpy(li.data(), oi, no * sizeof(int32_t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(ld.data(), od, no * sizeof(double), hipMemcpyDeviceToHost));
  CK(hipMemcpy(dFh.data(), dF, nf * sizeof(double), hipMemcpyDeviceToHost));

  // ---- the host: search (its lists must be the device's), normals, SPFH, FPFH ----
  const bool extrapolated = n >= 100000;
  const int64_t nq = extrapolated ? 10000 : n;
  long wrong = 0;
  double host_search_ms = host_ms(nq, [&](int64_t i0, int64_t i1) {
    long bad = 0;
    for (int64_t i = i0; i < i1; ++i) {
      double bd[K];
      int32_t bi[K];
      for (int k = 0; k < K; ++k) bd[k] = KNN_INF, bi[k] = -1;
      const double q0 = P[i * 3], q1 = P[i * 3 + 1], q2 = P[i * 3 + 2];
      for (int64_t j = 0; j < n; ++j) {
        double dist = 0.0, df = q0 - P[j * 3];
        dist = dist + df * df;
        df = q1 - P[j * 3 + 1];
        dist = dist + df * df;
        df = q2 - P[j * 3 + 2];
        dist = dist + df * df;
        if (dist < bd[K - 1]) {
          int k = K - 1;
          for (; k > 0 && dist < bd[k - 1]; --k) bd[k] = bd[k - 1], bi[k] = bi[k - 1];
          bd[k] = dist;
          bi[k] = static_cast<int32_t>(j);
        }
      }
      for (int k = 0; k < K; ++k) bad += bi[k] != li[i * K + k] || bd[k] != ld[i * K + k];
    }
    __atomic_fetch_add(&wrong, bad, __ATOMIC_RELAXED);
  });
  if (extrapolated) host_search_ms *= static_cast<double>(n) / static_cast<double>(nq);
  std::vector<double> N(P.size()), Sh(nf), Fh(nf);
  const double host_normals_ms = host_ms(n, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      const int32_t* row = li.data() + i * K;
      int cnt = 0;
      while (cnt < KN && feat_kept(row[cnt], ld[i * K + cnt], false, 0.0)) ++cnt;
      const double p[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]};
      double nv[3];
      feat_normal(
          cnt,
          [&](int k, double (&q)[3]) {
            const int64_t j = row[k];
            q[0] = P[j * 3], q[1] = P[j * 3 + 1], q[2] = P[j * 3 + 2];
          },
          p, nullptr, nv);
      N[i * 3] = nv[0], N[i * 3 + 1] = nv[1], N[i * 3 + 2] = nv[2];
    }
  });
  const double host_spfh_ms = host_ms(n, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      int hist[FEAT_DIM] = {0}, cnt = 0;
      const double p1[3] = {P[i * 3], P[i * 3 + 1], P[i * 3 + 2]}, n1[3] = {N[i * 3], N[i * 3 + 1], N[i * 3 + 2]};
      for (int k = 0; k < KF && feat_kept(li[i * K + k], ld[i * K + k], false, 0.0); ++k) {
        ++cnt;
        const int64_t j = li[i * K + k];
        if (j == i) continue;
        const double p2[3] = {P[j * 3], P[j * 3 + 1], P[j * 3 + 2]}, n2[3] = {N[j * 3], N[j * 3 + 1], N[j * 3 + 2]};
        double f[3];
        int b[3];
        feat_pair(p1, n1, p2, n2, f);
        feat_bins(f, b);
        ++hist[b[0]], ++hist[b[1]], ++hist[b[2]];
      }
      for (int b = 0; b < FEAT_DIM; ++b) Sh[i * FEAT_DIM + b] = static_cast<double>(hist[b]) * feat_spfh_scale(cnt);
    }
  });
  const double host_fpfh_ms = host_ms(n, [&](int64_t i0, int64_t i1) {
    for (int64_t i = i0; i < i1; ++i) {
      double f[FEAT_DIM] = {0.0};
      for (int k = 0; k < KF && feat_kept(li[i * K + k], ld[i * K + k], false, 0.0); ++k) {
        const int32_t j = li[i * K + k];
        const double sqd = ld[i * K + k];
        if (!feat_weighs(j, static_cast<int32_t>(i), sqd)) continue;
        for (int b = 0; b < FEAT_DIM; ++b) f[b] = feat_fpfh_add(f[b], Sh[static_cast<int64_t>(j) * FEAT_DIM + b], sqd);
      }
      for (int g = 0; g < FEAT_DIM; g += FEAT_BINS) {
        double s = 0.0;
        for (int c = 0; c < FEAT_BINS; ++c) s = s + f[g + c];
        for (int c = 0; c < FEAT_BINS; ++c) Fh[i * FEAT_DIM + g + c] = feat_fpfh_bin(f[g + c], s, Sh[i * FEAT_DIM + g + c]);
      }
    }
  });
  // how many of the host's descriptors are the device's bit for bit (the operations are the same; atan2 alone may differ
  // by ulps, which matters only to a pair within that of a bin edge)
  long rows_equal = 0;
  for (int64_t i = 0; i < n; ++i) rows_equal += std::equal(Fh.begin() + i * FEAT_DIM, Fh.begin() + (i + 1) * FEAT_DIM, dFh.begin() + i * FEAT_DIM);
  std::printf(
      "{\"n\": %lld, \"chunks\": %d, \"search_ms\": %.4f, \"normals_ms\": %.4f, \"spfh_ms\": %.4f, \"fpfh_ms\": %.4f, "
      "\"stages_ms\": %.4f, \"host_search_ms\": %.3f, \"host_normals_ms\": %.3f, \"host_spfh_ms\": %.3f, "
      "\"host_fpfh_ms\": %.3f, \"host_threads\": %d, \"host_extrapolated\": %s, \"host_list_mismatches\": %ld, "
      "\"descriptor_rows_equal\": %ld}\n",
      static_cast<long long>(n), S, search_ms, normals_ms, spfh_ms, fpfh_ms, all_ms, host_search_ms, host_normals_ms,
      host_spfh_ms, host_fpfh_ms, THREADS, extrapolated ? "true" : "false", wrong, rows_equal);
  return 0;
}
