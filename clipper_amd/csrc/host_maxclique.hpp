// host_maxclique.hpp — the maximum-clique solver (clipper_hip_max_clique, clipper_hip_core_numbers; kernels in
// k_maxclique.hip.h, semantics in DESIGN.md section 9): the source store of C, the buffers of one call, the launch
// loops with the time limit between launches, the node list.
// Part of clipper_hip.hip (one translation unit; included there, in order).
#pragma once

#include "host_mcplan.hpp"

namespace {

constexpr int64_t MC_MAX_M = 655360;           // the EXACT kernel's two LDS bitsets: 2 x 8 x ceil(m / 64) <= 160 KiB
constexpr long long MC_PEEL_BUDGET = 1ll << 24;  // row-word operations per peel launch (~ms)
constexpr long long MC_WAVE_BUDGET = 1ll << 18;  // row-word operations per wave and HEU / EXACT launch (~tens of ms)
constexpr int MC_WAVES_PER_CU = 8;

// Device buffers of one call (freed when it returns: the adjacency alone is m^2 / 8 bytes).
struct McBufs {
  uint64_t* G = nullptr;
  uint64_t* alive = nullptr;
  int32_t *deg = nullptr, *degw = nullptr, *core = nullptr, *pos = nullptr, *list = nullptr, *out = nullptr;
  McCtl* ctl = nullptr;
  McSlot* slots = nullptr;
  uint64_t* arena = nullptr;
  int32_t *paths = nullptr, *recs = nullptr;
  ~McBufs() {
    for (void* p : {static_cast<void*>(G), static_cast<void*>(alive), static_cast<void*>(deg), static_cast<void*>(degw),
                    static_cast<void*>(core), static_cast<void*>(pos), static_cast<void*>(list), static_cast<void*>(out),
                    static_cast<void*>(ctl), static_cast<void*>(slots), static_cast<void*>(arena),
                    static_cast<void*>(paths), static_cast<void*>(recs)})
      if (p) hipFree(p);
  }
};

// the one descriptor of a lone call (k_maxclique.hip.h): the buffers allocated so far
McProb mc_prob(const McBufs& b, int64_t nw, int64_t m) {
  McProb p{};
  p.G = b.G;
  p.nw = nw;
  p.m = static_cast<int32_t>(m);
  p.degw = b.degw;
  p.core = b.core;
  p.alive = b.alive;
  p.pos = b.pos;
  p.list = b.list;
  p.out = b.out;
  p.ctl = b.ctl;
  p.slots = b.slots;
  p.arena = b.arena;
  p.paths = b.paths;
  p.recs = b.recs;
  return p;
}

template <typename T>
int mc_alloc(T*& p, size_t count) {
  if (hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) {
    p = nullptr;
    (void)hipGetLastError();
    return fail(CLIPPER_HIP_E_NOMEM, "max clique: device allocation of %zu bytes failed", count * sizeof(T));
  }
  return 0;
}

int mc_check_scope(const Ctx* h) {
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (h->multiproc || h->world != 1 || h->sh.size() != 1)
    return fail(CLIPPER_HIP_E_SCOPE, "max clique: one-shard contexts only (this one holds column shards)");
  if (h->m > MC_MAX_M) return fail(CLIPPER_HIP_E_SCOPE, "max clique: m = %lld > %lld", (long long)h->m, (long long)MC_MAX_M);
  return 0;
}

// The adjacency bitsets from the store that holds C, the degrees, and the core numbers (device) of one call.
int mc_graph_and_cores(Ctx* h, McBufs& b, int64_t nw, std::vector<int32_t>& deg, std::vector<int32_t>& core) {
  Shard& s = h->sh[0];
  const int64_t m = h->m;
  HIPCHK(hipSetDevice(s.device));
  size_t freeb = 0, totalb = 0;
  HIPCHK(hipMemGetInfo(&freeb, &totalb));
  const size_t gbytes = static_cast<size_t>(m) * static_cast<size_t>(nw) * 8;
  if (gbytes + (64u << 20) > freeb)
    return fail(CLIPPER_HIP_E_NOMEM, "max clique: the adjacency bitsets need %zu bytes, %zu are free", gbytes, freeb);
  if (int rc = mc_alloc(b.G, static_cast<size_t>(m) * nw)) return rc;
  if (int rc = mc_alloc(b.alive, static_cast<size_t>(nw))) return rc;
  for (int32_t** p : {&b.deg, &b.degw, &b.core}) if (int rc = mc_alloc(*p, static_cast<size_t>(m))) return rc;
  if (int rc = mc_alloc(b.ctl, 1)) return rc;
  // C: the slices of M (pattern), else the explicit dense C, else the dense store of M (pattern)
  if (h->csc_valid && !h->explicitC) {
    HIPCHK(hipMemsetAsync(b.G, 0, gbytes, s.stream));
    const int64_t nsl = static_cast<int64_t>(s.s_ncg) * s.s_nchunks;
    dim3 grid(static_cast<unsigned>(ceil_div(nsl, 4))), block(256);
    dispatch_vt(h, [&](auto t) {  // (the value type; h->compressed says slices)
      hipLaunchKernelGGL((k_mc_adj_slices<decltype(t), SL_H>), grid, block, 0, s.stream, slice_view(h, s), b.G, nw, m);
    });
  } else {
    const void* src = h->explicitC ? s.Cs : s.S;
    if (!src) return fail(CLIPPER_HIP_E_STATE, "max clique: the store of C is not on the device");
    dim3 grid(static_cast<unsigned>(ceil_div(m, 256)), static_cast<unsigned>(std::min<int64_t>(nw, 65535))), block(256);
    dispatch_vt(h, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL(k_mc_adj_dense<T>, grid, block, 0, s.stream, static_cast<const T*>(src), h->W, m, nw, b.G);
    });
  }
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_mc_degree, dim3(static_cast<unsigned>(ceil_div(m, 4))), dim3(256), 0, s.stream, b.G, nw, m, b.deg);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(b.degw, b.deg, static_cast<size_t>(m) * 4, hipMemcpyDeviceToDevice, s.stream));
  HIPCHK(hipMemsetAsync(b.alive, 0xff, static_cast<size_t>(nw) * 8, s.stream));
  HIPCHK(hipMemsetAsync(b.ctl, 0, sizeof(McCtl), s.stream));
  const int lds = static_cast<int>(nw * 8);
  if (lds > 64 * 1024) raise_dynamic_lds(reinterpret_cast<const void*>(k_mc_core_peel), s.device, lds);
  McCtl c{};
  int64_t launches = 0;
  do {
    if (++launches > m + 1) return fail(CLIPPER_HIP_E_INTERNAL, "max clique: the core peel made no progress");
    hipLaunchKernelGGL(k_mc_core_peel, dim3(1), dim3(MC_PEEL_THREADS), lds, s.stream, mc_prob(b, nw, m), MC_PEEL_BUDGET);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&c, b.ctl, sizeof(McCtl), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
  } while (c.removed < m);
  deg.resize(static_cast<size_t>(m));
  core.resize(static_cast<size_t>(m));
  HIPCHK(hipMemcpy(deg.data(), b.deg, static_cast<size_t>(m) * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(core.data(), b.core, static_cast<size_t>(m) * 4, hipMemcpyDeviceToHost));
  return 0;
}

int max_clique_impl(Ctx* h, int method, double time_limit_s, clipper_maxclique_info_t* info) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto elapsed = [&] { return std::chrono::duration<double>(clk::now() - t0).count(); };
  auto out_of_time = [&] { return time_limit_s > 0 && elapsed() >= time_limit_s; };
  if (method != CLIPPER_HIP_MC_EXACT && method != CLIPPER_HIP_MC_HEU && method != CLIPPER_HIP_MC_KCORE)
    return fail(CLIPPER_HIP_E_INVALID, "max clique: unknown method %d", method);
  if (int rc = mc_check_scope(h)) return rc;
  Shard& s = h->sh[0];
  const int64_t m = h->m, nw = ceil_div(m, 64);
  clipper_maxclique_info_t I{};
  McBufs b;
  std::vector<int32_t> deg, core;
  if (int rc = mc_graph_and_cores(h, b, nw, deg, core)) return rc;
  int64_t dsum = 0;
  int K = 0;
  for (int64_t v = 0; v < m; ++v) {
    dsum += deg[static_cast<size_t>(v)];
    K = std::max(K, core[static_cast<size_t>(v)]);
  }
  I.edges = dsum / 2;
  I.max_core = K;
  std::vector<int32_t> nodes;
  const int lds1 = static_cast<int>(nw * 8);
  const int nwaves = std::max(1, h->cus) * MC_WAVES_PER_CU;
  if (method == CLIPPER_HIP_MC_KCORE) {
    // ROBIN: every vertex of core number K (an edgeless graph: all of them)
    for (int64_t v = 0; v < m; ++v)
      if (core[static_cast<size_t>(v)] == K) nodes.push_back(static_cast<int32_t>(v));
  } else if (I.edges > 0) {
    // ---- HEU: seeds by core descending, index ascending
    std::vector<int32_t> seeds(static_cast<size_t>(m));
    clipper_mc_plan::seed_order(core.data(), m, seeds.data());
    if (int rc = mc_alloc(b.list, static_cast<size_t>(m))) return rc;
    if (int rc = mc_alloc(b.out, static_cast<size_t>(K) + 2)) return rc;
    HIPCHK(hipMemcpy(b.list, seeds.data(), static_cast<size_t>(m) * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(b.ctl, 0, sizeof(McCtl)));
    if (lds1 > 64 * 1024) {
      raise_dynamic_lds(reinterpret_cast<const void*>(k_mc_heu), s.device, lds1);
      raise_dynamic_lds(reinterpret_cast<const void*>(k_mc_heu_one), s.device, lds1);
    }
    McCtl c{};
    McProb pr = mc_prob(b, nw, m);
    pr.nlist = static_cast<int32_t>(m);
    do {
      hipLaunchKernelGGL(k_mc_heu, dim3(static_cast<unsigned>(nwaves)), dim3(64), lds1, s.stream, pr, MC_WAVE_BUDGET);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(&c, b.ctl, sizeof(McCtl), hipMemcpyDeviceToHost, s.stream));
      HIPCHK(hipStreamSynchronize(s.stream));
      if (c.head < m && out_of_time()) {
        I.timed_out = 1;
        break;
      }
    } while (c.head < m);
    const int heu = static_cast<int>(c.key >> 32);
    const int seed = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(c.key & 0xFFFFFFFFull));
    if (heu < 2 || heu > K + 1 || seed < 0 || seed >= m)
      return fail(CLIPPER_HIP_E_INTERNAL, "max clique: HEU's record (size %d, seed %d) is not valid", heu, seed);
    pr.seed = seed;
    hipLaunchKernelGGL(k_mc_heu_one, dim3(1), dim3(64), lds1, s.stream, pr);
    HIPCHK(hipGetLastError());
    nodes.resize(static_cast<size_t>(heu));
    HIPCHK(hipMemcpyAsync(nodes.data(), b.out, static_cast<size_t>(heu) * 4, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    I.heuristic_size = heu;
    if (method == CLIPPER_HIP_MC_EXACT && heu < K + 1 && !I.timed_out) {
      // ---- EXACT: roots ordered by (core, degree, index); those that can hold a clique larger than HEU's,
      // taken from the end of that order (the largest bound first)
      std::vector<int32_t> pos(static_cast<size_t>(m)), roots;
      clipper_mc_plan::root_order(core.data(), deg.data(), m, heu, pos.data(), roots);
      I.roots_pruned = m - static_cast<int64_t>(roots.size());
      const int D = K + 1;  // stack levels: a clique has at most K + 1 vertices
      size_t freeb = 0, totalb = 0;
      HIPCHK(hipMemGetInfo(&freeb, &totalb));
      const size_t per_slot = static_cast<size_t>(D) * nw * 8 + 2 * static_cast<size_t>(D + 1) * 4 + sizeof(McSlot);
      const size_t room = std::min<size_t>(freeb / 4, size_t(4) << 30);
      const int nslots = static_cast<int>(std::min<size_t>(static_cast<size_t>(nwaves), room / per_slot));
      if (nslots < 1)
        return fail(CLIPPER_HIP_E_NOMEM, "max clique: one search stack needs %zu bytes, %zu are free", per_slot, freeb);
      if (int rc = mc_alloc(b.pos, static_cast<size_t>(m))) return rc;
      if (int rc = mc_alloc(b.slots, static_cast<size_t>(nslots))) return rc;
      if (int rc = mc_alloc(b.arena, static_cast<size_t>(nslots) * D * nw)) return rc;
      if (int rc = mc_alloc(b.paths, static_cast<size_t>(nslots) * (D + 1))) return rc;
      if (int rc = mc_alloc(b.recs, static_cast<size_t>(nslots) * (D + 1))) return rc;
      HIPCHK(hipMemcpy(b.pos, pos.data(), static_cast<size_t>(m) * 4, hipMemcpyHostToDevice));
      if (!roots.empty())
        HIPCHK(hipMemcpy(b.list, roots.data(), roots.size() * 4, hipMemcpyHostToDevice));
      std::vector<McSlot> hs(static_cast<size_t>(nslots));
      for (auto& x : hs) x = McSlot{-1, 0, 0, 0, 0ull};
      HIPCHK(hipMemcpy(b.slots, hs.data(), hs.size() * sizeof(McSlot), hipMemcpyHostToDevice));
      McCtl c0{};
      c0.key = (static_cast<unsigned long long>(heu) << 32) | 0xFFFFFFFFull;
      HIPCHK(hipMemcpy(b.ctl, &c0, sizeof(McCtl), hipMemcpyHostToDevice));
      const int lds2 = 2 * lds1;
      if (lds2 > 64 * 1024) raise_dynamic_lds(reinterpret_cast<const void*>(k_mc_exact), s.device, lds2);
      const int32_t nroots = static_cast<int32_t>(roots.size());
      pr = mc_prob(b, nw, m);
      pr.nlist = nroots;
      pr.heu = static_cast<int32_t>(heu);
      pr.D = static_cast<int32_t>(D);
      while (true) {
        HIPCHK(hipMemsetAsync(&b.ctl->active, 0, sizeof(int32_t), s.stream));
        hipLaunchKernelGGL(k_mc_exact, dim3(static_cast<unsigned>(nslots)), dim3(64), lds2, s.stream, pr, MC_WAVE_BUDGET);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&c, b.ctl, sizeof(McCtl), hipMemcpyDeviceToHost, s.stream));
        HIPCHK(hipStreamSynchronize(s.stream));
        if (c.head >= nroots && c.active == 0) break;
        if (out_of_time()) {
          I.timed_out = 1;
          break;
        }
      }
      if (c.overflow) return fail(CLIPPER_HIP_E_INTERNAL, "max clique: a branch went deeper than the core bound");
      I.roots_pruned += static_cast<int64_t>(c.roots_pruned);
      I.roots_searched = static_cast<int64_t>(c.roots_searched);
      I.bb_nodes = static_cast<int64_t>(c.bb_nodes);
      const int omega = static_cast<int>(c.key >> 32);
      if (omega > heu) {
        HIPCHK(hipMemcpy(hs.data(), b.slots, hs.size() * sizeof(McSlot), hipMemcpyDeviceToHost));
        int who = -1;
        for (int i = 0; i < nslots; ++i)
          if (hs[static_cast<size_t>(i)].rec_key == c.key) who = i;
        if (who < 0) return fail(CLIPPER_HIP_E_INTERNAL, "max clique: no record holds the incumbent");
        nodes.resize(static_cast<size_t>(omega));
        HIPCHK(hipMemcpy(nodes.data(), b.recs + static_cast<size_t>(who) * (D + 1), static_cast<size_t>(omega) * 4,
                         hipMemcpyDeviceToHost));
      }
    }
  }
  std::sort(nodes.begin(), nodes.end());
  h->nodes = nodes;
  I.num_nodes = static_cast<int32_t>(nodes.size());
  I.seconds = elapsed();
  if (info) *info = I;
  return 0;
}

int core_numbers_impl(Ctx* h, int32_t* core_out) {
  if (int rc = mc_check_scope(h)) return rc;
  McBufs b;
  std::vector<int32_t> deg, core;
  if (int rc = mc_graph_and_cores(h, b, ceil_div(h->m, 64), deg, core)) return rc;
  if (!core.empty()) std::memcpy(core_out, core.data(), core.size() * sizeof(int32_t));
  return 0;
}

}  // namespace
