// wave_check.hip — the integer folds and scans of k_wave.hip.h on the device against plain host loops, bit for bit.
// A stand-alone program (its own main, no library linked, nothing added to the ABI), built by clipper_amd/build.py
// next to the library with the library's flags and run once by tests/test_gpu_wave_primitives.py.
//
//   wave_check --list     the case names, one per line; no HIP call
//   wave_check            one line per case: "PASS <name>" or "FAIL <name>: first mismatch at index i, got .., want .."
// Exit status: 0 every case passed, 1 mismatches, 2 a HIP call returned an error (nothing is launched after it).
//
// Group A: the primitives through thin kernels that only declare the LDS and call the function, at every instantiation
// a kernel of the tree uses (tests/test_wave_check_build.py reads the call sites and asks for a case per N).
// Group B: the project's own scan kernels, launched as the host code launches them.
// Every comparison is exact equality with a host loop in the output type. Every output buffer has guard words in
// front of and behind the part the kernel may write ([n] belongs to it only where a total is asked for); the guards
// are checked after every launch. Inputs come from one fixed-seed generator.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "kernels.hip.h"

using namespace clipper_hip;

#define CK(e)                                                                                   \
  do {                                                                                          \
    hipError_t e_ = (e);                                                                        \
    if (e_ != hipSuccess) {                                                                     \
      std::fflush(stdout);                                                                      \
      std::fprintf(stderr, "HIP error: %s: %s (line %d)\n", #e, hipGetErrorString(e_), __LINE__); \
      std::_Exit(2);                                                                            \
    }                                                                                           \
  } while (0)

#define TRY(e)                    \
  do {                            \
    std::string m_ = (e);         \
    if (!m_.empty()) return m_;   \
  } while (0)

using ull = unsigned long long;

// ---- thin kernels over the primitives (group A) ---------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void t_wave(const T* in, T* sum, T* mx, T* scan) {
  const int t = static_cast<int>(threadIdx.x);
  const T v = in[t];
  sum[t] = wave_sum(v);
  mx[t] = wave_max(v);
  scan[t] = wave_scan_incl(v);
}

// OP 0: WaveAdd with the default unit; OP 1: minimum (suffix) or maximum over `unit`, the lambda of k_kg_slabs.
// `calls` scans in a row over the same wsum, each on its own WAVES * 64 inputs, the documented barrier between them.
template <int WAVES, typename T, int OP>
__global__ __launch_bounds__(WAVES * 64) void t_scan_excl(const T* in, int calls, int suffix, T unit, T* out) {
  __shared__ T wsum[WAVES];
  const int t = static_cast<int>(threadIdx.x);
  for (int c = 0; c < calls; ++c) {
    const T v = in[c * WAVES * 64 + t];
    T r;
    if constexpr (OP == 0) {
      r = block_scan_excl<WAVES>(v, wsum);
    } else {
      auto op = [&](T x, T y) { return suffix ? (x < y ? x : y) : (x > y ? x : y); };
      r = block_scan_excl<WAVES>(v, wsum, op, unit);
    }
    out[c * WAVES * 64 + t] = r;
    __syncthreads();  // every thread is past its reads of wsum
  }
}

// in and out may be the same array (no __restrict__); every thread reports the total it got
template <int THREADS, typename TIn, typename TOut, typename I>
__global__ __launch_bounds__(THREADS) void t_scan_array(const TIn* in, I n, TOut* out, TOut* out2, TOut* totals) {
  __shared__ TOut wsum[THREADS / 64];
  __shared__ TOut carry;
  const TOut total = block_scan_array<THREADS>(in, n, out, wsum, &carry, out2);
  totals[threadIdx.x] = total;
}

// ---- host side ------------------------------------------------------------------------------------------------------
namespace {

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  uint64_t below(uint64_t m) { return next() % m; }
};

constexpr size_t GUARD = 64;
template <typename T>
constexpr T guard_word() { return static_cast<T>(0xA5A5A5A5A5A5A5A5ull); }
template <typename T>
constexpr T stale_word() { return static_cast<T>(0x5C5C5C5C5C5C5C5Cull); }  // an output word the kernel has not written

// n words the kernel may touch between two runs of guard words
template <typename T>
struct DevBuf {
  std::vector<T> h;
  T* d = nullptr;
  size_t n;
  explicit DevBuf(size_t n_) : h(n_ + 2 * GUARD, guard_word<T>()), n(n_) {
    std::fill(h.begin() + GUARD, h.begin() + GUARD + n, stale_word<T>());
    CK(hipMalloc(reinterpret_cast<void**>(&d), h.size() * sizeof(T)));
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)hipFree(d); }
  T* host() { return h.data() + GUARD; }
  T* dev() { return d + GUARD; }
  void set(const std::vector<T>& v) { std::copy(v.begin(), v.end(), host()); }
  void up() { CK(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice)); }
  void down() { CK(hipMemcpy(h.data(), d, h.size() * sizeof(T), hipMemcpyDeviceToHost)); }
  std::string guards(const char* what) const {
    for (size_t i = 0; i < GUARD; ++i) {
      if (h[i] != guard_word<T>())
        return std::string("guard word ") + std::to_string(GUARD - i) + " in front of " + what + " overwritten";
      if (h[GUARD + n + i] != guard_word<T>())
        return std::string("guard word ") + std::to_string(i) + " behind " + what + " overwritten";
    }
    return "";
  }
};

void sync() {
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
}

template <typename T>
std::string diff(const std::string& what, const T* got, const T* want, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (got[i] != want[i])
      return "first mismatch at index " + std::to_string(i) + ", got " + std::to_string(got[i]) + ", want " +
             std::to_string(want[i]) + " (" + what + ")";
  return "";
}

template <typename T>
std::string all_equal(const std::string& what, const T* got, T want, size_t n) {
  std::vector<T> w(n, want);
  return diff(what, got, w.data(), n);
}

// exclusive prefix sums in TOut; returns the total
template <typename TIn, typename TOut>
TOut host_scan(const std::vector<TIn>& in, std::vector<TOut>& out) {
  using U = typename std::make_unsigned<TOut>::type;  // (the sums of the signed cases stay far from overflow)
  U run = 0;
  out.resize(in.size());
  for (size_t i = 0; i < in.size(); ++i) {
    out[i] = static_cast<TOut>(run);
    run += static_cast<U>(static_cast<TOut>(in[i]));
  }
  return static_cast<TOut>(run);
}

struct Case {
  std::string name;
  std::function<std::string()> run;
};

// ---- group A: wave_sum, wave_max, wave_scan_incl --------------------------------------------------------------------
// four waves with different data: random, all negative (signed) or all large, one non-zero lane, random again
template <typename T>
std::string run_wave(uint64_t seed) {
  Rng rng{seed};
  constexpr int N = 256;
  std::vector<T> in(N);
  for (int t = 0; t < N; ++t) {
    const int w = t >> 6;
    uint64_t r = rng.next();
    if constexpr (sizeof(T) == 8) {
      r = (r & 0x3FFFFFFFFull) + (w == 1 ? (1ull << 33) : 0);  // a wave's sum passes 2^32
      in[t] = static_cast<T>(w == 2 ? ((t & 63) == 37 ? (1ull << 40) + 3 : 0) : r);
    } else if constexpr (std::is_signed<T>::value) {
      const int v = static_cast<int>(r % 2000001) - 1000000;
      in[t] = static_cast<T>(w == 1 ? -1 - static_cast<int>(r % 1000) : w == 2 ? ((t & 63) == 37 ? -5 : 0) : v);
    } else {
      in[t] = static_cast<T>(w == 1 ? 0xFFFFFFFFu - (r % 1000) : w == 2 ? ((t & 63) == 37 ? 9 : 0) : r % 1000000);
    }
  }
  DevBuf<T> din(N), dsum(N), dmax(N), dscan(N);
  din.set(in);
  din.up(); dsum.up(); dmax.up(); dscan.up();
  hipLaunchKernelGGL(t_wave<T>, dim3(1), dim3(N), 0, nullptr, din.dev(), dsum.dev(), dmax.dev(), dscan.dev());
  sync();
  dsum.down(); dmax.down(); dscan.down();
  using U = typename std::make_unsigned<T>::type;
  std::vector<T> wsum(N), wmax(N), wscan(N);
  for (int w = 0; w < N / 64; ++w) {
    U s = 0;
    T m = std::numeric_limits<T>::lowest();
    for (int l = 0; l < 64; ++l) {
      s += static_cast<U>(in[w * 64 + l]);
      m = std::max(m, in[w * 64 + l]);
      wscan[w * 64 + l] = static_cast<T>(s);
    }
    for (int l = 0; l < 64; ++l) {
      wsum[w * 64 + l] = static_cast<T>(s);
      wmax[w * 64 + l] = m;
    }
  }
  TRY(diff("wave_sum", dsum.host(), wsum.data(), N));
  TRY(diff("wave_max", dmax.host(), wmax.data(), N));
  TRY(diff("wave_scan_incl", dscan.host(), wscan.data(), N));
  TRY(dsum.guards("wave_sum's output"));
  TRY(dmax.guards("wave_max's output"));
  TRY(dscan.guards("wave_scan_incl's output"));
  return "";
}

// ---- group A: block_scan_excl ---------------------------------------------------------------------------------------
template <typename T>
T excl_random(Rng& rng, int op) {
  const uint64_t r = rng.next();
  if (op != 0) return static_cast<T>(r);                          // min / max: any key
  if constexpr (sizeof(T) == 8) return static_cast<T>(r & 0xFFFFFFFFFFull);  // sums pass 2^32, never 2^64
  if constexpr (std::is_signed<T>::value) return static_cast<T>(static_cast<int>(r % 2001) - 1000);
  return static_cast<T>(r);                                       // unsigned 32-bit sums wrap, on the host as well
}

// the input sets of one instantiation: all zero, all unit, one non-unit value at thread 0, 63, 64 and the last, random
template <int WAVES, typename T>
std::vector<std::pair<std::string, std::vector<T>>> excl_inputs(int op, T unit, Rng& rng) {
  constexpr int N = WAVES * 64;
  const T one = op == 0 ? static_cast<T>(sizeof(T) == 8 ? 0x100000007ull : 7) : static_cast<T>(0x123456789ull);
  std::vector<std::pair<std::string, std::vector<T>>> sets;
  sets.emplace_back("all zero", std::vector<T>(N, T(0)));
  sets.emplace_back("all unit", std::vector<T>(N, unit));
  for (int at : {0, 63, 64, N - 1}) {
    std::vector<T> v(N, unit);
    v[at] = one;
    sets.emplace_back("one value at thread " + std::to_string(at), v);
  }
  std::vector<T> v(N);
  for (auto& x : v) x = excl_random<T>(rng, op);
  sets.emplace_back("random", v);
  return sets;
}

template <typename T>
T excl_op(int op, int suffix, T a, T b) {
  using U = typename std::make_unsigned<T>::type;
  if (op == 0) return static_cast<T>(static_cast<U>(a) + static_cast<U>(b));
  return suffix ? std::min(a, b) : std::max(a, b);
}

// `in` holds calls * WAVES * 64 values: one launch, `calls` scans in a row
template <int WAVES, typename T, int OP>
std::string excl_launch(const std::string& what, const std::vector<T>& in, int calls, int suffix, T unit) {
  constexpr int N = WAVES * 64;
  DevBuf<T> din(in.size()), dout(in.size());
  din.set(in);
  din.up(); dout.up();
  hipLaunchKernelGGL((t_scan_excl<WAVES, T, OP>), dim3(1), dim3(N), 0, nullptr, din.dev(), calls, suffix, unit, dout.dev());
  sync();
  dout.down();
  std::vector<T> want(in.size());
  for (int c = 0; c < calls; ++c) {
    T run = unit;
    for (int t = 0; t < N; ++t) {
      want[c * N + t] = run;
      run = excl_op<T>(OP, suffix, run, in[c * N + t]);
    }
  }
  TRY(diff(what, dout.host(), want.data(), in.size()));
  return dout.guards(what.c_str());
}

template <int WAVES, typename T, int OP>
std::string run_excl(int suffix, T unit, bool back_to_back, uint64_t seed) {
  Rng rng{seed};
  const auto sets = excl_inputs<WAVES, T>(OP, unit, rng);
  if (!back_to_back) {
    for (const auto& s : sets) TRY((excl_launch<WAVES, T, OP>(s.first, s.second, 1, suffix, unit)));
    return "";
  }
  // two scans in a row: random then one value at the last thread, and random then random
  for (size_t second : {sets.size() - 2, sets.size() - 1}) {
    std::vector<T> in = sets.back().second;
    std::vector<T> b = sets[second].second;
    if (second == sets.size() - 1)
      for (auto& x : b) x = excl_random<T>(rng, OP);
    in.insert(in.end(), b.begin(), b.end());
    TRY((excl_launch<WAVES, T, OP>("random, then " + sets[second].first, in, 2, suffix, unit)));
  }
  return "";
}

// ---- group A: block_scan_array --------------------------------------------------------------------------------------
// KIND 0: block sums (64-bit, many above 2^32 / 3); 1: 32-bit sizes, every other one 0xFFFFFFFF; 2: counts 0..1024
template <typename TIn>
std::vector<TIn> array_input(int kind, size_t n, Rng& rng) {
  std::vector<TIn> in(n);
  for (size_t j = 0; j < n; ++j) {
    const uint64_t r = rng.next();
    in[j] = static_cast<TIn>(kind == 0 ? (j % 3 == 0 ? 0xFFFFFFFFull : r & 0xFFFFFFFFFFull)
                             : kind == 1 ? (j % 2 == 0 ? 0xFFFFFFFFull : r & 0xFFFFFFFFull)
                                         : r % 1025);
  }
  return in;
}

template <int THREADS, typename TIn, typename TOut, typename I>
std::string array_launch(const std::string& what, const std::vector<TIn>& in, bool in_place, bool with_out2,
                         std::vector<TOut>& out, std::vector<TOut>& totals) {
  const size_t n = in.size();
  DevBuf<TIn> din(n);
  DevBuf<TOut> dout(n), dout2(with_out2 ? n : 0), dtot(THREADS);
  din.set(in);
  din.up(); dout.up(); dout2.up(); dtot.up();
  TOut* o = dout.dev();
  if constexpr (std::is_same<TIn, TOut>::value) {
    if (in_place) o = din.dev();
  }
  hipLaunchKernelGGL((t_scan_array<THREADS, TIn, TOut, I>), dim3(1), dim3(THREADS), 0, nullptr, din.dev(), static_cast<I>(n), o,
                     with_out2 ? dout2.dev() : static_cast<TOut*>(nullptr), dtot.dev());
  sync();
  din.down(); dout.down(); dout2.down(); dtot.down();
  TRY(din.guards((what + ": the input").c_str()));
  TRY(dout.guards((what + ": out").c_str()));
  TRY(dout2.guards((what + ": out2").c_str()));
  TRY(dtot.guards((what + ": the totals").c_str()));
  if constexpr (std::is_same<TIn, TOut>::value) {
    if (in_place) {
      out.assign(din.host(), din.host() + n);
      TRY(all_equal(what + ": out, which an in-place scan must not touch", dout.host(), stale_word<TOut>(), n));
    } else {
      out.assign(dout.host(), dout.host() + n);
      TRY(diff(what + ": the input, which must stay", din.host(), in.data(), n));
    }
  } else {
    out.assign(dout.host(), dout.host() + n);
    TRY(diff(what + ": the input, which must stay", din.host(), in.data(), n));
  }
  if (with_out2) TRY(diff(what + ": out2 against out", dout2.host(), out.data(), n));
  totals.assign(dtot.host(), dtot.host() + THREADS);
  return "";
}

template <int THREADS, typename TIn, typename TOut, typename I>
std::string run_array(int kind, size_t n, bool in_place, bool with_out2, uint64_t seed) {
  Rng rng{seed + n};
  const std::vector<TIn> in = array_input<TIn>(kind, n, rng);
  std::vector<TOut> want, out, totals;
  const TOut total = host_scan(in, want);
  TRY((array_launch<THREADS, TIn, TOut, I>("out of place", in, false, with_out2, out, totals)));
  TRY(diff("out of place: prefix sums", out.data(), want.data(), n));
  TRY(all_equal("out of place: the total returned to thread [index]", totals.data(), total, THREADS));
  if (in_place) {
    std::vector<TOut> out_ip, totals_ip;
    TRY((array_launch<THREADS, TIn, TOut, I>("in place", in, true, with_out2, out_ip, totals_ip)));
    TRY(diff("in place: prefix sums", out_ip.data(), want.data(), n));
    TRY(all_equal("in place: the total returned to thread [index]", totals_ip.data(), total, THREADS));
    if (n && std::memcmp(out_ip.data(), out.data(), n * sizeof(TOut)) != 0) return "in place and out of place differ";
    if (std::memcmp(totals_ip.data(), totals.data(), THREADS * sizeof(TOut)) != 0) return "in place and out of place totals differ";
  }
  return "";
}

// ---- group B --------------------------------------------------------------------------------------------------------
std::string run_row_scan(int rows, int32_t n, bool with_out2, int with_total, uint64_t seed) {
  Rng rng{seed + static_cast<uint64_t>(n) * 1000 + rows};
  const size_t len = static_cast<size_t>(rows) * n, olen = len + (with_total ? 1 : 0);
  std::vector<int32_t> in(len);
  for (auto& x : in) x = static_cast<int32_t>(rng.below(1000));
  DevBuf<int32_t> din(len), dout(olen), dout2(with_out2 ? olen : 0);
  din.set(in);
  din.up(); dout.up(); dout2.up();
  hipLaunchKernelGGL(k_row_scan<>, dim3(rows), dim3(ROW_SCAN_THREADS), 0, nullptr, din.dev(), n, dout.dev(),
                     with_out2 ? dout2.dev() : static_cast<int32_t*>(nullptr), with_total);
  sync();
  din.down(); dout.down(); dout2.down();
  std::vector<int32_t> want(olen);
  for (int r = 0; r < rows; ++r) {
    int32_t run = 0;
    for (int32_t i = 0; i < n; ++i) {
      want[static_cast<size_t>(r) * n + i] = run;
      run += in[static_cast<size_t>(r) * n + i];
    }
    if (with_total) want[len] = run;  // (one row only)
  }
  TRY(diff("out", dout.host(), want.data(), olen));
  if (with_out2) TRY(diff("out2", dout2.host(), want.data(), olen));
  TRY(diff("the input, which must stay", din.host(), in.data(), len));
  TRY(din.guards("the input"));
  TRY(dout.guards("out"));
  return dout2.guards("out2");
}

std::vector<uint32_t> slice_sizes(int64_t n, Rng& rng) {  // the sum passes 2^32 from the third entry on
  return array_input<uint32_t>(1, static_cast<size_t>(n), rng);
}

// k_slice_scan_small as slices_enqueue launches it
std::string slice_scan_small(const std::vector<uint32_t>& sizes, std::vector<uint64_t>& pre, uint64_t& total) {
  const int64_t n = static_cast<int64_t>(sizes.size());
  DevBuf<uint32_t> dsz(sizes.size());
  DevBuf<uint64_t> dpre(sizes.size()), dtot(1);
  dsz.set(sizes);
  dsz.up(); dpre.up(); dtot.up();
  hipLaunchKernelGGL(k_slice_scan_small, dim3(1), dim3(1024), 0, nullptr, dsz.dev(), n, dpre.dev(), dtot.dev());
  sync();
  dsz.down(); dpre.down(); dtot.down();
  TRY(dsz.guards("one workgroup: sizes"));
  TRY(dpre.guards("one workgroup: Pre"));
  TRY(dtot.guards("one workgroup: total"));
  TRY(diff("one workgroup: sizes, which must stay", dsz.host(), sizes.data(), sizes.size()));
  pre.assign(dpre.host(), dpre.host() + sizes.size());
  total = dtot.host()[0];
  return "";
}

// k_slice_scan_local + _blocks + _add as slices_enqueue launches them; blocksum: nblk + 1 words
std::string slice_scan_two_level(const std::vector<uint32_t>& sizes, std::vector<uint64_t>& pre, std::vector<uint64_t>& blocksum) {
  const int64_t n = static_cast<int64_t>(sizes.size());
  const int64_t nblk = (n + SCAN_BLK - 1) / SCAN_BLK;
  DevBuf<uint32_t> dsz(sizes.size());
  DevBuf<uint64_t> dpre(sizes.size()), dblk(static_cast<size_t>(nblk) + 1);
  dsz.set(sizes);
  dsz.up(); dpre.up(); dblk.up();
  hipLaunchKernelGGL(k_slice_scan_local, dim3(static_cast<unsigned>(nblk)), dim3(256), 0, nullptr, dsz.dev(), n, dpre.dev(), dblk.dev());
  hipLaunchKernelGGL(k_slice_scan_blocks, dim3(1), dim3(256), 0, nullptr, dblk.dev(), nblk);
  hipLaunchKernelGGL(k_slice_scan_add, dim3(static_cast<unsigned>(nblk)), dim3(256), 0, nullptr, dpre.dev(), n, dblk.dev());
  sync();
  dsz.down(); dpre.down(); dblk.down();
  TRY(dsz.guards("two levels: sizes"));
  TRY(dpre.guards("two levels: Pre"));
  TRY(dblk.guards("two levels: the block sums"));
  TRY(diff("two levels: sizes, which must stay", dsz.host(), sizes.data(), sizes.size()));
  pre.assign(dpre.host(), dpre.host() + sizes.size());
  blocksum.assign(dblk.host(), dblk.host() + nblk + 1);
  return "";
}

// path 0: one workgroup, 1: two levels, 2: both on the same sizes, which must agree
std::string run_slice_scan(int64_t n, int path, uint64_t seed) {
  Rng rng{seed + static_cast<uint64_t>(n)};
  const std::vector<uint32_t> sizes = slice_sizes(n, rng);
  std::vector<uint64_t> want;
  const uint64_t total = host_scan(sizes, want);
  std::vector<uint64_t> pre1, pre2, blk;
  uint64_t tot1 = 0;
  if (path != 1) {
    TRY(slice_scan_small(sizes, pre1, tot1));
    TRY(diff("one workgroup: Pre", pre1.data(), want.data(), sizes.size()));
    TRY(diff("one workgroup: total", &tot1, &total, 1));
  }
  if (path != 0) {
    TRY(slice_scan_two_level(sizes, pre2, blk));
    std::vector<uint64_t> wblk(blk.size());
    for (size_t b = 0; b + 1 < blk.size(); ++b) wblk[b] = want[b * SCAN_BLK];
    wblk.back() = total;
    TRY(diff("two levels: the block sums and the total behind them", blk.data(), wblk.data(), blk.size()));
    TRY(diff("two levels: Pre", pre2.data(), want.data(), sizes.size()));
  }
  if (path == 2) {
    TRY(diff("Pre of the two levels against the one workgroup's", pre2.data(), pre1.data(), sizes.size()));
    TRY(diff("total of the two levels against the one workgroup's", &blk.back(), &tot1, 1));
  }
  return "";
}

std::string run_rv_scan(int nb, uint64_t seed) {
  Rng rng{seed + static_cast<uint64_t>(nb)};
  std::vector<uint32_t> in = array_input<uint32_t>(2, static_cast<size_t>(nb), rng);
  in[0] = 1024;  // both ends of the range are there
  if (nb > 1) in[nb - 1] = 0;
  std::vector<uint32_t> want;
  const uint32_t total = host_scan(in, want);
  want.push_back(total);
  DevBuf<uint32_t> dblk(static_cast<size_t>(nb) + 1);
  DevBuf<int32_t> dcount(1);
  dblk.set(in);
  dblk.up(); dcount.up();
  hipLaunchKernelGGL(k_rv_scan, dim3(1), dim3(1024), 0, nullptr, dblk.dev(), nb, dcount.dev());
  sync();
  dblk.down(); dcount.down();
  const int32_t wcount = static_cast<int32_t>(total);
  TRY(diff("blk, blk[nb] the total", dblk.host(), want.data(), want.size()));
  TRY(diff("count_out", dcount.host(), &wcount, 1));
  TRY(dblk.guards("blk"));
  return dcount.guards("count_out");
}

// order-preserving key of a double and its way back: the bit rule of kg_key / kg_unkey (k_knn_grid.hip.h)
ull host_key(double v) {
  ull b;
  std::memcpy(&b, &v, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
ull host_unkey_bits(ull k) { return (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k; }

std::string run_kg_slabs(int d0, int d1, int d2, uint64_t seed) {
  Rng rng{seed + static_cast<uint64_t>(d0) * 1000003 + static_cast<uint64_t>(d1) * 1009 + d2};
  KnnGrid g{};
  g.dim[0] = d0; g.dim[1] = d1; g.dim[2] = d2;
  g.off[0] = 0; g.off[1] = g.dim[0]; g.off[2] = g.dim[0] + g.dim[1];  // as knn_grid_plan sets them
  const size_t nslab = static_cast<size_t>(d0) + d1 + d2;
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<ull> kmin(nslab), kmax(nslab);
  for (size_t i = 0; i < nslab; ++i) {
    if (rng.below(4) == 0) {  // an empty slab: what k_kg_init wrote
      kmin[i] = host_key(inf);
      kmax[i] = host_key(-inf);
      continue;
    }
    double a = (static_cast<double>(rng.next() >> 11) * 0x1p-53 - 0.5) * 2000.0;
    double b = (static_cast<double>(rng.next() >> 11) * 0x1p-53 - 0.5) * 2000.0;
    if (rng.below(16) == 0) a = 0.0;
    if (rng.below(16) == 0) b = -0.0;
    kmin[i] = host_key(std::min(a, b));
    kmax[i] = host_key(std::max(a, b));
  }
  // the outputs as their bits: the comparison is of bits, and -0.0 is not 0.0 here
  DevBuf<ull> dmin(nslab), dmax(nslab), dsmin(nslab), dpmax(nslab);
  dmin.set(kmin); dmax.set(kmax);
  dmin.up(); dmax.up(); dsmin.up(); dpmax.up();
  hipLaunchKernelGGL(k_kg_slabs<>, dim3(6), dim3(256), 0, nullptr, g, dmin.dev(), dmax.dev(), reinterpret_cast<double*>(dsmin.dev()),
                     reinterpret_cast<double*>(dpmax.dev()));
  sync();
  dmin.down(); dmax.down(); dsmin.down(); dpmax.down();
  std::vector<ull> wsmin(nslab), wpmax(nslab);
  for (int a = 0; a < 3; ++a) {
    const int n = g.dim[a], off = g.off[a];
    ull run = ~0ull;
    for (int i = n - 1; i >= 0; --i) {
      run = std::min(run, kmin[off + i]);
      wsmin[off + i] = host_unkey_bits(run);
    }
    run = 0ull;
    for (int i = 0; i < n; ++i) {
      run = std::max(run, kmax[off + i]);
      wpmax[off + i] = host_unkey_bits(run);
    }
  }
  TRY(diff("smin, as the bits of the doubles", dsmin.host(), wsmin.data(), nslab));
  TRY(diff("pmax, as the bits of the doubles", dpmax.host(), wpmax.data(), nslab));
  TRY(diff("kmin, which must stay", dmin.host(), kmin.data(), nslab));
  TRY(diff("kmax, which must stay", dmax.host(), kmax.data(), nslab));
  TRY(dsmin.guards("smin"));
  return dpmax.guards("pmax");
}

std::string run_kg_sum(int32_t n0, uint64_t seed) {
  Rng rng{seed + static_cast<uint64_t>(n0)};
  std::vector<int32_t> v(static_cast<size_t>(n0));
  for (auto& x : v) x = static_cast<int32_t>(0x40000000u + rng.below(0x3FFFFFFFu));  // 256 of them pass 2^38
  const ull start = (1ull << 32) + 5;  // the kernel adds to what is there
  ull want = start;
  for (int32_t x : v) want += static_cast<ull>(x);
  DevBuf<int32_t> dv(v.size());
  DevBuf<ull> dsum(1);
  dv.set(v);
  dsum.host()[0] = start;
  dv.up(); dsum.up();
  const int64_t blocks = std::min<int64_t>(256, (static_cast<int64_t>(n0) + 255) / 256);  // knn_grid_sum_visited
  hipLaunchKernelGGL(k_kg_sum<>, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, nullptr, dv.dev(), static_cast<int64_t>(n0),
                     dsum.dev());
  sync();
  dv.down(); dsum.down();
  TRY(diff("sum", dsum.host(), &want, 1));
  TRY(diff("the values, which must stay", dv.host(), v.data(), v.size()));
  return dsum.guards("sum");
}

// ---- the table ------------------------------------------------------------------------------------------------------
template <int THREADS, typename TIn, typename TOut, typename I>
void add_array_cases(std::vector<Case>& cs, const std::string& tag, int kind, bool in_place, bool with_out2, uint64_t seed) {
  for (size_t n : {size_t(0), size_t(1), size_t(63), size_t(64), size_t(65), size_t(THREADS - 1), size_t(THREADS), size_t(THREADS + 1),
                   size_t(2 * THREADS + 1), size_t(3 * THREADS)})
    cs.push_back({"A.scan_array<" + std::to_string(THREADS) + ">." + tag + ".n" + std::to_string(n),
                  [=] { return run_array<THREADS, TIn, TOut, I>(kind, n, in_place, with_out2, seed); }});
}

template <int WAVES, typename T>
void add_excl_add_cases(std::vector<Case>& cs, const std::string& type, uint64_t seed) {
  const std::string base = "A.scan_excl<" + std::to_string(WAVES) + ">.add." + type;
  cs.push_back({base, [=] { return run_excl<WAVES, T, 0>(0, T(0), false, seed); }});
  cs.push_back({base + ".back_to_back", [=] { return run_excl<WAVES, T, 0>(0, T(0), true, seed + 1); }});
}

std::vector<Case> cases() {
  std::vector<Case> cs;
  // group A
  cs.push_back({"A.wave.i32", [] { return run_wave<int>(11); }});
  cs.push_back({"A.wave.u32", [] { return run_wave<uint32_t>(12); }});
  cs.push_back({"A.wave.u64", [] { return run_wave<uint64_t>(13); }});
  cs.push_back({"A.wave.ull", [] { return run_wave<ull>(14); }});
  add_excl_add_cases<4, uint32_t>(cs, "u32", 21);   // k_rv_scatter
  add_excl_add_cases<4, int32_t>(cs, "i32", 23);    // k_sort_scatter (SORT_WAVES = 4)
  add_excl_add_cases<4, uint64_t>(cs, "u64", 25);   // k_slice_scan_local, block_scan_array<256>
  add_excl_add_cases<16, uint32_t>(cs, "u32", 27);  // block_scan_array<1024>
  add_excl_add_cases<16, int32_t>(cs, "i32", 29);
  add_excl_add_cases<16, uint64_t>(cs, "u64", 31);
  cs.push_back({"A.scan_excl<4>.min.ull", [] { return run_excl<4, ull, 1>(1, ~0ull, false, 33); }});  // k_kg_slabs
  cs.push_back({"A.scan_excl<4>.min.ull.back_to_back", [] { return run_excl<4, ull, 1>(1, ~0ull, true, 34); }});
  cs.push_back({"A.scan_excl<4>.max.ull", [] { return run_excl<4, ull, 1>(0, 0ull, false, 35); }});
  cs.push_back({"A.scan_excl<4>.max.ull.back_to_back", [] { return run_excl<4, ull, 1>(0, 0ull, true, 36); }});
  add_array_cases<256, uint64_t, uint64_t, int64_t>(cs, "u64_u64.in_place", 0, true, false, 41);   // k_slice_scan_blocks
  add_array_cases<1024, uint32_t, uint32_t, int>(cs, "u32_u32.in_place", 2, true, false, 42);      // k_rv_scan
  add_array_cases<1024, uint32_t, uint64_t, int64_t>(cs, "u32_u64", 1, false, false, 43);          // k_slice_scan_small
  add_array_cases<1024, int32_t, int32_t, int32_t>(cs, "i32_i32", 2, false, false, 44);            // k_row_scan
  add_array_cases<1024, int32_t, int32_t, int32_t>(cs, "i32_i32.out2", 2, false, true, 45);
  // group B
  for (int rows : {1, 256})
    for (int32_t n : {1, 1023, 1024, 1025, 2049})
      for (int out2 : {0, 1})
        for (int with_total : {0, 1}) {
          if (with_total && rows != 1) continue;  // (documented: one row only)
          cs.push_back({"B.k_row_scan.rows" + std::to_string(rows) + ".n" + std::to_string(n) + (out2 ? ".out2" : ".no_out2") +
                            (with_total ? ".total" : ".no_total"),
                        [=] { return run_row_scan(rows, n, out2 != 0, with_total, 51); }});
        }
  for (int64_t n : {1, 1024, 1025, 32768})
    cs.push_back({"B.k_slice_scan_small.n" + std::to_string(n), [=] { return run_slice_scan(n, 0, 61); }});
  for (int64_t n : {32769, 262144, 262145, 2 * 262144 + 1025})
    cs.push_back({"B.k_slice_scan_two_level.n" + std::to_string(n), [=] { return run_slice_scan(n, 1, 62); }});
  for (int64_t n : {32768, 32769})
    cs.push_back({"B.k_slice_scan_both_paths.n" + std::to_string(n), [=] { return run_slice_scan(n, 2, 63); }});
  for (int nb : {1, 1023, 1024, 1025, 2049})
    cs.push_back({"B.k_rv_scan.nb" + std::to_string(nb), [=] { return run_rv_scan(nb, 71); }});
  const int dims[5][3] = {{1, 255, 256}, {257, 1000, 1}, {256, 257, 1000}, {1000, 1, 255}, {255, 256, 257}};
  for (const auto& d : dims) {
    const int d0 = d[0], d1 = d[1], d2 = d[2];
    cs.push_back({"B.k_kg_slabs.dim" + std::to_string(d0) + "x" + std::to_string(d1) + "x" + std::to_string(d2),
                  [=] { return run_kg_slabs(d0, d1, d2, 81); }});
  }
  for (int32_t n : {1, 255, 256, 257, 100000})
    cs.push_back({"B.k_kg_sum.n" + std::to_string(n), [=] { return run_kg_sum(n, 91); }});
  return cs;
}

}  // namespace

int main(int argc, char** argv) {
  const std::vector<Case> cs = cases();
  if (argc > 1 && std::strcmp(argv[1], "--list") == 0) {
    for (const auto& c : cs) std::printf("%s\n", c.name.c_str());
    return 0;
  }
  if (argc > 1) {
    std::fprintf(stderr, "usage: %s [--list]\n", argv[0]);
    return 2;
  }
  CK(hipSetDevice(0));
  int failed = 0;
  for (const auto& c : cs) {
    const std::string msg = c.run();
    if (msg.empty()) {
      std::printf("PASS %s\n", c.name.c_str());
    } else {
      std::printf("FAIL %s: %s\n", c.name.c_str(), msg.c_str());
      ++failed;
    }
    std::fflush(stdout);
  }
  return failed ? 1 : 0;
}
