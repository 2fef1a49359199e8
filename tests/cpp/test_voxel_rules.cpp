// test_voxel_rules.cpp — the whole of clipper_hip_voxel_downsample restated on the host from voxel_rules.hpp and
// host_voxel_check.hpp, with g++ alone (no HIP): checks, plan, keys, the order of the pairs found twice (once with
// std::stable_sort, once with a host LSD radix sort over the header's digits and passes: the two must agree), segments,
// chunked sums, centroid and normal. The result goes to a file that tests/test_voxel_model.py compares with the numpy
// model bit for bit. Plain asserts (no gtest in the image).
//   test_voxel_rules n P.f64 N.f64|- voxel_size out.bin
// out.bin: int64 n_out, dim[3], passes; then n_out x 3 doubles (points), n_out x 3 doubles (normals, only with N),
// n_out int32 (counts), n int32 (trace), n_out uint64 (the rows' keys).
// The last line but one is "host_ms <t>": the single-thread time of the call as restated here with std::stable_sort (checks,
// keys, sort, segments, sums; neither the radix sort nor the files), which tools/voxel_probe.py reports.
// A refused call prints "refused: <message>" and exits 2.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <string>
#include <vector>

#include "host_voxel_check.hpp"

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

using namespace clipper_hip;

static std::vector<double> read(const char* path, size_t count) {
  std::vector<double> v(count);
  FILE* f = std::fopen(path, "rb");
  EXPECT(f != nullptr);
  EXPECT(std::fread(v.data(), sizeof(double), count, f) == count);
  std::fclose(f);
  return v;
}

template <class T>
static void put(FILE* f, const T* p, size_t count) {
  EXPECT(std::fwrite(p, sizeof(T), count, f) == count);
}

int main(int argc, char** argv) {
  EXPECT(argc == 6);
  const int64_t n = std::atoll(argv[1]);
  const std::vector<double> P = read(argv[2], static_cast<size_t>(3 * n));
  const bool has_n = std::string(argv[3]) != "-";
  const std::vector<double> N = has_n ? read(argv[3], static_cast<size_t>(3 * n)) : std::vector<double>();
  const double voxel_size = std::atof(argv[4]);

  using clk = std::chrono::steady_clock;
  const clk::time_point t0 = clk::now();
  clipper_voxel::Plan plan{};
  int64_t n_out = 0;
  const std::string why = clipper_voxel::check_all(P.data(), has_n ? N.data() : nullptr, n, voxel_size, &n_out, nullptr, plan);
  if (!why.empty()) {
    std::printf("refused: %s\n", why.c_str());
    return 2;
  }
  const VoxelGrid& g = plan.g;
  EXPECT(plan.passes == sort_passes(voxel_cells(g)) && plan.passes >= 0 && plan.passes <= 8);

  // keys
  std::vector<uint64_t> key(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    const double p[3] = {P[3 * i], P[3 * i + 1], P[3 * i + 2]};
    key[i] = voxel_key(g, p);
    EXPECT(key[i] < voxel_cells(g));
  }
  // the order, twice
  std::vector<int32_t> by_std(static_cast<size_t>(n));
  std::iota(by_std.begin(), by_std.end(), 0);
  std::stable_sort(by_std.begin(), by_std.end(), [&](int32_t a, int32_t b) { return key[a] < key[b]; });
  const clk::time_point t1 = clk::now();
  std::vector<int32_t> idx(static_cast<size_t>(n)), tmp(static_cast<size_t>(n));
  std::iota(idx.begin(), idx.end(), 0);
  for (int pass = 0; pass < plan.passes; ++pass) {
    std::vector<int64_t> first(SORT_RADIX + 1, 0);
    for (int64_t i = 0; i < n; ++i) ++first[sort_digit(key[idx[i]], pass) + 1];
    for (int d = 0; d < SORT_RADIX; ++d) first[d + 1] += first[d];
    for (int64_t i = 0; i < n; ++i) tmp[first[sort_digit(key[idx[i]], pass)]++] = idx[i];
    idx.swap(tmp);
  }
  EXPECT(idx == by_std);
  const clk::time_point t2 = clk::now();

  // segments
  std::vector<int64_t> start;
  std::vector<int32_t> trace(static_cast<size_t>(n));
  for (int64_t i = 0; i < n; ++i) {
    if (i == 0 || key[idx[i]] != key[idx[i - 1]]) start.push_back(i);
    trace[idx[i]] = static_cast<int32_t>(start.size() - 1);
  }
  n_out = static_cast<int64_t>(start.size());
  start.push_back(n);

  // sums
  std::vector<double> pts(static_cast<size_t>(3 * n_out)), nrm(has_n ? static_cast<size_t>(3 * n_out) : 0);
  std::vector<int32_t> counts(static_cast<size_t>(n_out));
  std::vector<uint64_t> rowkey(static_cast<size_t>(n_out));
  for (int64_t r = 0; r < n_out; ++r) {
    const int64_t s = start[r], cnt = start[r + 1] - s;
    double tot[3], c[3];
    voxel_sum(cnt, [&](int64_t k, double(&v)[3]) {
      for (int a = 0; a < 3; ++a) v[a] = P[3 * idx[s + k] + a] - g.lo[a];
    }, tot);
    voxel_centroid(g, tot, static_cast<int32_t>(cnt), c);
    for (int a = 0; a < 3; ++a) pts[3 * r + a] = c[a];
    if (has_n) {
      double nv[3];
      voxel_sum(cnt, [&](int64_t k, double(&v)[3]) {
        for (int a = 0; a < 3; ++a) v[a] = N[3 * idx[s + k] + a];
      }, tot);
      voxel_normal(tot, nv);
      for (int a = 0; a < 3; ++a) nrm[3 * r + a] = nv[a];
    }
    counts[r] = static_cast<int32_t>(cnt);
    rowkey[r] = key[idx[s]];
    EXPECT(r == 0 || rowkey[r] > rowkey[r - 1]);
  }

  const clk::time_point t3 = clk::now();
  const double host_ms = std::chrono::duration<double, std::milli>((t1 - t0) + (t3 - t2)).count();

  FILE* f = std::fopen(argv[5], "wb");
  EXPECT(f != nullptr);
  const int64_t head[5] = {n_out, g.dim[0], g.dim[1], g.dim[2], plan.passes};
  put(f, head, 5);
  put(f, pts.data(), pts.size());
  put(f, nrm.data(), nrm.size());
  put(f, counts.data(), counts.size());
  put(f, trace.data(), trace.size());
  put(f, rowkey.data(), rowkey.size());
  std::fclose(f);
  std::printf("host_ms %.3f\nvoxel rules ok\n", host_ms);
  return 0;
}
