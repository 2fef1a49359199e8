// host_maxclique.hpp — the maximum-clique solver (clipper_hip_max_clique, clipper_hip_core_numbers,
// clipper_hip_batch_max_clique; kernels in k_maxclique.hip.h, the plan in host_mcplan.hpp, semantics in DESIGN.md
// section 9). Part of clipper_hip.hip (one translation unit; included there, after host_batchsolve.hpp).
//
// mc_run is the one driver: a lone call is a call on one problem. It
//   1. plans the graph part for all its problems (G, alive, deg, degw, core, pos, lists, out, McCtl and the tables),
//      checks it against the free memory and allocates it as ONE slab; the host's side of it is the caller's pinned
//      staging buffer,
//   2. builds every adjacency from the store that holds C, the degrees, and peels: ONE workgroup per unfinished
//      problem and launch,
//   3. reads all deg and core back in ONE copy, sorts seeds and roots, writes all lists in ONE copy per phase,
//   4. runs HEU and the regeneration of the winning cliques; then, for the problems that go on to EXACT, plans and
//      allocates the search part from each one's K and roots, and runs EXACT over its slot table. After each launch
//      ONE copy of the McCtl array, the compaction of the work list to the unfinished problems, and the time limit.
// The number of copies and resets between launches does not depend on the number of problems, and per problem the
// results are a function of the graph alone.
// A seeded call (DESIGN.md 9 "Seeded calls") hands mc_run a vertex list per problem. The lists travel in the graph
// part's first copy; after step 3 ONE launch of k_mc_seed turns each into its seed clique Q0 in `out`, and ONE copy of
// the McCtl array brings the sizes s; HEU's and EXACT's incumbents start at s, and where Q0 wins it is taken from
// `out` as it lies. A problem without a list, and a call without lists, takes the steps above and no other.
#pragma once

#include "host_mcplan.hpp"

namespace {

constexpr int64_t MC_MAX_M = 655360;           // the EXACT kernel's two LDS bitsets: 2 x 8 x ceil(m / 64) <= 160 KiB
constexpr long long MC_PEEL_BUDGET = 1ll << 24;  // row-word operations per peel launch (~ms)
constexpr long long MC_WAVE_BUDGET = 1ll << 18;  // row-word operations per wave and HEU / EXACT launch (~tens of ms)
// Test infrastructure (clipper_hip_debug_mc_budgets): the budgets the launches are given, process-wide. A smaller budget
// cuts the same work into more launches and changes no result.
std::atomic<long long> g_mc_peel_budget{MC_PEEL_BUDGET}, g_mc_wave_budget{MC_WAVE_BUDGET};
constexpr int MC_WAVES_PER_CU = 8;
constexpr int MC_PEEL_ONLY = -1;  // mc_run's method for clipper_hip_core_numbers: stop after the peel, keep `core`
using McSeeds = std::vector<std::vector<int32_t>>;  // a seeded call's vertex list per problem (empty: not seeded)

static_assert(sizeof(McItem) == sizeof(clipper_mc_plan::Item), "the plan's table rows are the kernels'");
static_assert(sizeof(McProb) % 8 == 0 && sizeof(McCtl) % 8 == 0 && sizeof(McSlot) % 8 == 0 && sizeof(McAdjSrc) % 8 == 0,
              "8-byte tables");

// a device slab and the pinned mirror of its host-visible tail [host_begin, bytes)
struct McSlab {
  DevBuf<uint8_t> dev;
  uint8_t* host = nullptr;
  size_t host_begin = 0;
  int alloc(size_t bytes) {
    if (dev.alloc(std::max<size_t>(bytes, 8)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CLIPPER_HIP_E_NOMEM, "max clique: device allocation of %zu bytes failed", bytes);
    }
    return 0;
  }
  template <typename T>
  T* D(size_t off) const { return reinterpret_cast<T*>(dev + off); }
  template <typename T>
  T* H(size_t off) const { return reinterpret_cast<T*>(host + (off - host_begin)); }  // (off >= host_begin)
};

struct McResult {
  clipper_maxclique_info_t info{};
  clipper_maxclique_seed_info_t seed{};  // a seeded call
  std::vector<int32_t> nodes;  // ascending
  std::vector<int32_t> core;   // MC_PEEL_ONLY
};

// (a caller's method; the driver is also run with MC_PEEL_ONLY). seeded: an entry point that takes vertex lists
int mc_check_method(int method, bool seeded = false) {
  if (method != CLIPPER_HIP_MC_EXACT && method != CLIPPER_HIP_MC_HEU && method != CLIPPER_HIP_MC_KCORE &&
      !(seeded && method == CLIPPER_HIP_MC_SEED_ONLY))
    return fail(CLIPPER_HIP_E_INVALID, "max clique: unknown method %d", method);
  return 0;
}

// a caller's vertex list for a problem of m vertices: distinct and in range
int mc_check_seed(const int32_t* seed, int64_t n, int64_t m) {
  const int64_t bad = clipper_mc_plan::first_bad_seed(seed, n, static_cast<int32_t>(m));
  if (bad < 0) return 0;
  const int32_t v = seed[bad];
  if (v < 0 || v >= m)
    return fail(CLIPPER_HIP_E_INVALID, "max clique: seed[%lld] = %d is no vertex of 0..%lld", (long long)bad, v, (long long)m - 1);
  return fail(CLIPPER_HIP_E_INVALID, "max clique: seed[%lld] = %d repeats an earlier entry", (long long)bad, v);
}

int mc_check_scope(const Ctx* h) {
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (h->multiproc || h->world != 1 || h->sh.size() != 1)
    return fail(CLIPPER_HIP_E_SCOPE, "max clique: one-shard contexts only (this one holds column shards)");
  if (h->m > MC_MAX_M) return fail(CLIPPER_HIP_E_SCOPE, "max clique: m = %lld > %lld", (long long)h->m, (long long)MC_MAX_M);
  return 0;
}

// The maximum cliques (or, MC_PEEL_ONLY, the core numbers) of the problems of `cs`, which passed mc_check_scope (and
// `method` mc_check_method) and share a device, a value type and the stream `st`. R[k] is cs[k]'s result; `launches`
// counts the kernel launches. An error that is one problem's leaves its index in `fault`. seeds: null, or a checked
// vertex list per problem (mc_check_seed) and `method` may be CLIPPER_HIP_MC_SEED_ONLY.
int mc_run(const std::vector<Ctx*>& cs, int method, double time_limit_s, hipStream_t st, int device, PinnedBuf<uint8_t>& stage,
           int& launches, std::vector<McResult>& R, size_t& fault, const McSeeds* seeds = nullptr) {
  namespace plan = clipper_mc_plan;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto elapsed = [&] { return std::chrono::duration<double>(clk::now() - t0).count(); };
  auto out_of_time = [&] { return time_limit_s > 0 && elapsed() >= time_limit_s; };
  const size_t nb = cs.size();
  fault = nb;
  R.assign(nb, McResult{});
  if (nb == 0) return 0;
  HIPCHK(hipSetDevice(device));

  // ---- 1. the graph part -----------------------------------------------------------------------------------------
  std::vector<int32_t> ms(nb);
  for (size_t k = 0; k < nb; ++k) ms[k] = static_cast<int32_t>(cs[k]->m);
  const int64_t cap = static_cast<int64_t>(std::max(1, cs[0]->cus)) * MC_WAVES_PER_CU;
  std::vector<int32_t> ngiven;  // (stays empty in an unseeded call)
  for (size_t k = 0; seeds && k < nb; ++k)
    if (!(*seeds)[k].empty()) {
      ngiven.resize(nb, 0);
      ngiven[k] = static_cast<int32_t>((*seeds)[k].size());
      R[k].seed.seed_given = ngiven[k];
    }
  const plan::GraphPlan L = plan::make_graph_plan(ms, cap, sizeof(McProb), sizeof(McCtl), sizeof(McAdjSrc), ngiven);
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  if (L.bytes + (64u << 20) > free_b)
    return fail(CLIPPER_HIP_E_NOMEM, "max clique: %zu problems need a slab of %zu bytes, %zu are free", nb, L.bytes, free_b);
  McSlab g, x;  // the graph part, the search part
  if (int rc = g.alloc(L.bytes)) return rc;
  const size_t ghost = L.bytes - L.host_begin;
  HIPCHK(stage.grow(ghost + plan::search_host_bound(cap, nb, sizeof(McSlot))));
  g.host = stage.p;
  g.host_begin = L.host_begin;
  x.host = stage.p + ghost;
  auto up = [&](const McSlab& s, size_t begin, size_t end) -> int {    // host -> device, [begin, end)
    if (end > begin)
      HIPCHK(hipMemcpyAsync(s.D<uint8_t>(begin), s.H<uint8_t>(begin), end - begin, hipMemcpyHostToDevice, st));
    return 0;
  };
  auto down = [&](const McSlab& s, size_t begin, size_t end) -> int {  // device -> host, and wait
    if (end > begin)
      HIPCHK(hipMemcpyAsync(s.H<uint8_t>(begin), s.D<uint8_t>(begin), end - begin, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };
  McProb* probs = g.H<McProb>(L.probs);
  McCtl* ctl = g.H<McCtl>(L.ctl);
  const McProb* dprobs = g.D<McProb>(L.probs);
  McCtl* dctl = g.D<McCtl>(L.ctl);
  const McAdjSrc* dsrc = g.D<McAdjSrc>(L.src);
  const int32_t* dwork = g.D<int32_t>(L.work);
  const size_t ctl_end = L.ctl + nb * sizeof(McCtl);
  const int lds1 = static_cast<int>(L.nw_max * 8);
  if (lds1 > 64 * 1024)
    for (const void* f : {reinterpret_cast<const void*>(k_mc_core_peel), reinterpret_cast<const void*>(k_mc_heu),
                          reinterpret_cast<const void*>(k_mc_heu_one)})
      raise_dynamic_lds(f, device, lds1);
  if (2 * lds1 > 64 * 1024) raise_dynamic_lds(reinterpret_cast<const void*>(k_mc_exact), device, 2 * lds1);
  auto launched = [&]() -> int {
    HIPCHK(hipGetLastError());
    ++launches;
    return 0;
  };

  // ---- 2. descriptors (one copy), adjacency, degrees, the peel -------------------------------------------------------
  std::memset(g.H<uint8_t>(L.up_begin), 0, L.up_end - L.up_begin);
  int64_t nslices = 0;  // the most slices a problem has
  bool any_slices = false, any_dense = false;
  for (size_t k = 0; k < nb; ++k) {
    const Ctx* c = cs[k];
    const Shard& s = c->sh[0];
    const plan::GraphRegions& r = L.at[k];
    McProb p{};
    p.G = g.D<uint64_t>(r.G);
    p.nw = r.nw;
    p.m = ms[k];
    p.degw = g.D<int32_t>(r.degw);
    p.core = g.D<int32_t>(r.core);
    p.alive = g.D<uint64_t>(r.alive);
    p.pos = g.D<int32_t>(r.pos);
    p.list = g.D<int32_t>(r.list);
    p.out = g.D<int32_t>(r.out) + 1;  // (out[-1]: the count k_mc_collect leaves)
    p.ctl = dctl + k;
    if (!ngiven.empty() && ngiven[k] > 0) {
      p.given = g.D<int32_t>(r.given);
      p.ngiven = ngiven[k];
      std::memcpy(g.H<int32_t>(r.given), (*seeds)[k].data(), static_cast<size_t>(ngiven[k]) * sizeof(int32_t));
    }
    probs[k] = p;
    // C: the slices of M (pattern), else the explicit dense C, else the dense store of M (pattern)
    McAdjSrc a{};
    if (c->csc_valid && !c->explicitC) {
      a.M = slice_view(c, s);
      any_slices = true;
      nslices = std::max<int64_t>(nslices, static_cast<int64_t>(s.s_ncg) * s.s_nchunks);
    } else {
      a.S = c->explicitC ? s.Cs : s.S;
      any_dense = true;
      if (!a.S) {
        fault = k;
        return fail(CLIPPER_HIP_E_STATE, "max clique: the store of C is not on the device");
      }
    }
    a.ld = c->W;
    a.G = g.D<uint64_t>(r.G);
    a.nw = r.nw;
    a.m = ms[k];
    a.deg = g.D<int32_t>(r.deg);
    g.H<McAdjSrc>(L.src)[k] = a;
  }
  // (descriptors, sources, control words, a seeded call's vertex lists; HEU's and EXACT's lists come later)
  if (int rc = up(g, L.up_begin, ngiven.empty() ? ctl_end : L.given_end)) return rc;
  HIPCHK(hipMemsetAsync(g.D<uint8_t>(L.alive_begin), 0xff, L.alive_bytes, st));
  const int32_t np = static_cast<int32_t>(nb);
  const unsigned gp = static_cast<unsigned>(std::min<size_t>(nb, 65535));  // the grid's problem dimension
  if (any_slices) HIPCHK(hipMemsetAsync(g.D<uint8_t>(L.G_begin), 0, L.G_bytes, st));  // (the slices' ORs need it)
  if (nslices > 0) {
    dispatch_vt(cs[0], [&](auto t) {  // (the call's value type)
      hipLaunchKernelGGL((k_mc_adj_slices<decltype(t), SL_H>), dim3(static_cast<unsigned>(ceil_div(nslices, 4)), gp),
                         dim3(256), 0, st, dsrc, np);
    });
    if (int rc = launched()) return rc;
  }
  if (any_dense) {
    dim3 grid(static_cast<unsigned>(ceil_div(L.m_max, 256)), static_cast<unsigned>(std::min<int64_t>(L.nw_max, 65535)), gp);
    dispatch_vt(cs[0], [&](auto t) { hipLaunchKernelGGL(k_mc_adj_dense<decltype(t)>, grid, dim3(256), 0, st, dsrc, np); });
    if (int rc = launched()) return rc;
  }
  hipLaunchKernelGGL(k_mc_degree, dim3(static_cast<unsigned>(ceil_div(L.m_max, 4)), gp), dim3(256), 0, st, dsrc, np);
  if (int rc = launched()) return rc;
  HIPCHK(hipMemcpyAsync(g.D<uint8_t>(L.degw_begin), g.D<uint8_t>(L.deg_begin), L.deg_bytes, hipMemcpyDeviceToDevice, st));

  std::vector<int32_t> on_device;  // the work list the device holds
  auto put_work = [&](const std::vector<int32_t>& list) -> int {
    if (list == on_device) return 0;
    std::memcpy(g.H<int32_t>(L.work), list.data(), list.size() * sizeof(int32_t));
    on_device = list;
    return up(g, L.work, L.work + list.size() * sizeof(int32_t));
  };
  std::vector<int32_t> work(nb);
  std::iota(work.begin(), work.end(), 0);
  for (int64_t rounds = 0; !work.empty(); ++rounds) {
    if (rounds > L.m_max) return fail(CLIPPER_HIP_E_INTERNAL, "max clique: the core peel made no progress");
    if (int rc = put_work(work)) return rc;
    hipLaunchKernelGGL(k_mc_core_peel, dim3(static_cast<unsigned>(work.size())), dim3(MC_PEEL_THREADS), lds1, st, dprobs,
                       dwork, g_mc_peel_budget.load());
    if (int rc = launched()) return rc;
    if (int rc = down(g, L.ctl, ctl_end)) return rc;
    work = plan::compact(work, [&](int32_t k) { return ctl[k].removed >= ms[static_cast<size_t>(k)]; });
  }

  // ---- 3. deg and core in one copy; KCORE's lists, HEU's seeds ------------------------------------------------------
  if (int rc = down(g, L.deg_begin, L.bytes)) return rc;
  std::vector<int32_t> Kmax(nb, 0), heu(nb, 0), searching;
  std::vector<int64_t> weight(nb, 0);
  for (size_t k = 0; k < nb; ++k) {
    const int32_t m = ms[k];
    const int32_t* deg = g.H<int32_t>(L.at[k].deg);
    const int32_t* core = g.H<int32_t>(L.at[k].core);
    int64_t dsum = 0;
    int K = 0;
    for (int32_t v = 0; v < m; ++v) {
      dsum += deg[v];
      K = std::max(K, core[v]);
    }
    R[k].info.edges = dsum / 2;
    R[k].info.max_core = Kmax[k] = K;
    if (method == MC_PEEL_ONLY) {
      R[k].core.assign(core, core + m);
    } else if (method == CLIPPER_HIP_MC_KCORE) {
      // ROBIN: every vertex of core number K (an edgeless graph: all of them)
      for (int32_t v = 0; v < m; ++v)
        if (core[v] == K) R[k].nodes.push_back(v);
    } else if (dsum > 0) {
      // HEU's seeds: by core descending, index ascending
      plan::seed_order(core, m, g.H<int32_t>(L.at[k].list));
      probs[k].nlist = m;
      weight[k] = m;
      searching.push_back(static_cast<int32_t>(k));
    }
  }

  // ---- 3s. a seeded call: the seed cliques, one wave per seeded problem with an edge; their sizes with the McCtl copy -----
  std::vector<int32_t> seeded, s0(nb, 0);
  if (!ngiven.empty())
    for (int32_t k : searching)
      if (ngiven[static_cast<size_t>(k)] > 0) seeded.push_back(k);
  if (!seeded.empty()) {
    if (2 * lds1 > 64 * 1024) raise_dynamic_lds(reinterpret_cast<const void*>(k_mc_seed), device, 2 * lds1);
    if (int rc = put_work(seeded)) return rc;
    hipLaunchKernelGGL(k_mc_seed, dim3(static_cast<unsigned>(seeded.size())), dim3(64), 2 * lds1, st, dprobs, dwork);
    if (int rc = launched()) return rc;
    if (int rc = down(g, L.ctl, ctl_end)) return rc;
    for (int32_t k : seeded) {
      const size_t ku = static_cast<size_t>(k);
      const int32_t s = ctl[ku].seed_size, kept = ctl[ku].seed_kept;
      if (kept < 1 || kept > ngiven[ku] || s < kept || s > Kmax[ku] + 1) {
        fault = ku;
        return fail(CLIPPER_HIP_E_INTERNAL, "max clique: the seed clique's record (size %d, kept %d) is not valid", s, kept);
      }
      R[ku].seed.seed_kept = kept;
      R[ku].seed.seed_size = s0[ku] = s;
    }
  }

  // one launch over the slot table of `list` (kept in `s` at `tab`), then the copy of the control array
  std::vector<int32_t> tabled;  // the list whose slot table the device holds
  auto launch_slots = [&](const McSlab& s, size_t tab, const std::vector<int32_t>& list, const std::vector<int32_t>& ns,
                          bool exact) -> int {
    size_t rows = 0;
    for (int32_t k : list) rows += static_cast<size_t>(ns[static_cast<size_t>(k)]);
    if (list != tabled) {
      const std::vector<plan::Item> rws = plan::slot_rows(list, ns);
      std::memcpy(s.H<plan::Item>(tab), rws.data(), rws.size() * sizeof(plan::Item));
      tabled = list;
      if (int rc = up(s, tab, tab + rws.size() * sizeof(plan::Item))) return rc;
    }
    if (exact) {
      // `active` of every problem: one call
      HIPCHK(hipMemset2DAsync(&dctl[0].active, sizeof(McCtl), 0, sizeof(int32_t), nb, st));
      hipLaunchKernelGGL(k_mc_exact, dim3(static_cast<unsigned>(rows)), dim3(64), 2 * lds1, st, dprobs, s.D<McItem>(tab),
                         g_mc_wave_budget.load());
    } else {
      hipLaunchKernelGGL(k_mc_heu, dim3(static_cast<unsigned>(rows)), dim3(64), lds1, st, dprobs, s.D<McItem>(tab),
                         g_mc_wave_budget.load());
    }
    if (int rc = launched()) return rc;
    return down(g, L.ctl, ctl_end);
  };
  auto time_out = [&](const std::vector<int32_t>& list) {  // the time limit between launches
    if (list.empty() || !out_of_time()) return false;
    for (int32_t k : list) R[static_cast<size_t>(k)].info.timed_out = 1;
    return true;
  };
  // the cliques `out` holds after a launch over the work list `list`
  auto take_out = [&](const std::vector<int32_t>& list, const std::vector<int32_t>& size) -> int {
    if (int rc = down(g, L.out_begin, L.out_begin + L.out_bytes)) return rc;
    for (int32_t k : list) {
      const int32_t* out = g.H<int32_t>(L.at[static_cast<size_t>(k)].out) + 1;
      R[static_cast<size_t>(k)].nodes.assign(out, out + size[static_cast<size_t>(k)]);
    }
    return 0;
  };

  if (method == CLIPPER_HIP_MC_SEED_ONLY) {
    if (!seeded.empty())
      if (int rc = take_out(seeded, s0)) return rc;
    for (int32_t k : seeded) R[static_cast<size_t>(k)].seed.winner = 2;
  } else if (!searching.empty()) {
    // ---- 4a. HEU (a seed clique of two vertices or more is the incumbent it has to beat: ties go to the seed clique) ----
    std::memset(ctl, 0, nb * sizeof(McCtl));
    for (int32_t k : seeded)
      if (s0[static_cast<size_t>(k)] >= 2)
        ctl[k].key = (static_cast<unsigned long long>(s0[static_cast<size_t>(k)]) << 32) | 0xFFFFFFFFull;
    if (int rc = up(g, L.up_begin, L.up_end)) return rc;
    const std::vector<int32_t> hslots = plan::deal_slots(weight, cap);
    std::vector<int32_t> active = searching;
    while (!active.empty()) {
      if (int rc = launch_slots(g, L.slot_tab, active, hslots, false)) return rc;
      active = plan::compact(active, [&](int32_t k) { return ctl[k].head >= ms[static_cast<size_t>(k)]; });
      if (time_out(active)) break;
    }
    std::vector<int32_t> exact, heu_won;  // heu_won: the problems whose clique so far is HEU's, not the seed clique
    std::vector<plan::Search> sr(nb, plan::Search{0, 0, 0});
    std::vector<std::vector<int32_t>> roots(nb);
    const std::vector<McCtl> after_heu(ctl, ctl + nb);
    std::memset(ctl, 0, nb * sizeof(McCtl));
    for (int32_t k : searching) {
      const size_t ku = static_cast<size_t>(k);
      clipper_maxclique_info_t& Ik = R[ku].info;
      const int32_t m = ms[ku];
      const unsigned long long key = after_heu[ku].key;
      const int h = static_cast<int>(key >> 32);
      // (the size alone says whether HEU beat the seed clique: seed 0 leaves the tie field of the preload)
      const bool from_seed = s0[ku] >= 2 && h == s0[ku];
      const int seed = from_seed ? 0 : static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(key & 0xFFFFFFFFull));
      // (every launch finishes the seeds it takes, the first of which has the largest core number, so after one
      // launch the record holds a clique of two vertices or more, time limit or not)
      if (h < 2 || h < s0[ku] || h > Kmax[ku] + 1 || seed < 0 || seed >= m) {
        fault = ku;
        return fail(CLIPPER_HIP_E_INTERNAL, "max clique: HEU's record (size %d, seed %d) is not valid", h, seed);
      }
      heu[ku] = h;
      Ik.heuristic_size = h;
      probs[ku].seed = seed;
      if (!from_seed) heu_won.push_back(k);
      R[ku].seed.winner = plan::seeded_winner(s0[ku], h, h);
      if (method == CLIPPER_HIP_MC_EXACT && h < Kmax[ku] + 1 && !Ik.timed_out) {
        // EXACT: roots ordered by (core, degree, index); those that can hold a clique larger than HEU's, taken from
        // the end of that order (the largest bound first). They replace the seeds; the incumbent starts at HEU's clique.
        plan::root_order(g.H<int32_t>(L.at[ku].core), g.H<int32_t>(L.at[ku].deg), m, h, g.H<int32_t>(L.at[ku].pos), roots[ku]);
        std::memcpy(g.H<int32_t>(L.at[ku].list), roots[ku].data(), roots[ku].size() * sizeof(int32_t));
        Ik.roots_pruned = m - static_cast<int64_t>(roots[ku].size());
        probs[ku].nlist = static_cast<int32_t>(roots[ku].size());
        probs[ku].heu = h;
        ctl[ku].key = (static_cast<unsigned long long>(h) << 32) | 0xFFFFFFFFull;
        sr[ku] = plan::Search{m, Kmax[ku], static_cast<int64_t>(roots[ku].size())};
        if (!roots[ku].empty()) exact.push_back(k);
      }
    }

    // ---- 4b. the search part: slots dealt by roots, stacks of K + 1 levels ----------------------------------------------
    std::vector<int32_t> xslots(nb, 0);
    plan::SearchPlan X;
    if (!exact.empty()) {
      HIPCHK(hipMemGetInfo(&free_b, &total_b));
      X = plan::make_search_plan(sr, cap, std::min<size_t>(free_b / 4, size_t(4) << 30), sizeof(McSlot));
      if (!X.fits && nb == 1) {  // (several problems go on with one slot each)
        fault = static_cast<size_t>(exact[0]);
        return fail(CLIPPER_HIP_E_NOMEM, "max clique: one search stack needs %zu bytes, %zu are free",
                    plan::slot_bytes(sr[0], sizeof(McSlot)), free_b);
      }
      if (x.alloc(X.bytes))
        return fail(CLIPPER_HIP_E_NOMEM, "max clique: the search stacks of %zu problems need %zu bytes, %zu are free",
                    exact.size(), X.bytes, free_b);
      x.host_begin = X.host_begin;
      for (int32_t k : exact) {
        const size_t ku = static_cast<size_t>(k);
        const plan::SearchRegions& r = X.at[ku];
        probs[ku].D = r.D;
        probs[ku].nslots = xslots[ku] = r.nslots;
        probs[ku].slots = x.D<McSlot>(r.slots);
        probs[ku].arena = x.D<uint64_t>(r.arena);
        probs[ku].paths = x.D<int32_t>(r.paths);
        probs[ku].recs = x.D<int32_t>(r.recs);
        for (int32_t j = 0; j < r.nslots; ++j) x.H<McSlot>(r.slots)[j] = McSlot{-1, 0, 0, 0, 0ull};
      }
      if (int rc = up(x, X.host_begin, X.slot_tab)) return rc;
    }
    if (int rc = up(g, L.up_begin, L.up_end)) return rc;

    // ---- 4c. the winning cliques of HEU ---------------------------------------------------------------------------------
    // (a seed clique that HEU did not beat lies in `out` since k_mc_seed)
    if (!heu_won.empty()) {
      if (int rc = put_work(heu_won)) return rc;
      hipLaunchKernelGGL(k_mc_heu_one, dim3(static_cast<unsigned>(heu_won.size())), dim3(64), lds1, st, dprobs, dwork);
      if (int rc = launched()) return rc;
    }
    if (int rc = take_out(searching, heu)) return rc;

    // ---- 4d. EXACT -----------------------------------------------------------------------------------------------------
    if (!exact.empty()) {
      active = exact;
      tabled.clear();
      while (!active.empty()) {
        if (int rc = launch_slots(x, X.slot_tab, active, xslots, true)) return rc;
        active = plan::compact(active, [&](int32_t k) { return ctl[k].head >= probs[k].nlist && ctl[k].active == 0; });
        if (time_out(active)) break;
      }
      std::vector<int32_t> better, omega(nb, 0);
      for (int32_t k : exact) {
        const size_t ku = static_cast<size_t>(k);
        clipper_maxclique_info_t& Ik = R[ku].info;
        if (ctl[ku].overflow) {
          fault = ku;
          return fail(CLIPPER_HIP_E_INTERNAL, "max clique: a branch went deeper than the core bound");
        }
        Ik.roots_pruned += static_cast<int64_t>(ctl[ku].roots_pruned);
        Ik.roots_searched = static_cast<int64_t>(ctl[ku].roots_searched);
        Ik.bb_nodes = static_cast<int64_t>(ctl[ku].bb_nodes);
        omega[ku] = static_cast<int32_t>(ctl[ku].key >> 32);
        R[ku].seed.winner = plan::seeded_winner(s0[ku], heu[ku], omega[ku]);
        if (omega[ku] > heu[ku]) better.push_back(k);
      }
      if (!better.empty()) {
        if (int rc = put_work(better)) return rc;
        hipLaunchKernelGGL(k_mc_collect, dim3(static_cast<unsigned>(better.size())), dim3(64), 0, st, dprobs, dwork);
        if (int rc = launched()) return rc;
        if (int rc = take_out(better, omega)) return rc;
        for (int32_t k : better)
          if (g.H<int32_t>(L.at[static_cast<size_t>(k)].out)[0] != omega[static_cast<size_t>(k)]) {
            fault = static_cast<size_t>(k);
            return fail(CLIPPER_HIP_E_INTERNAL, "max clique: no record holds the incumbent");
          }
      }
    }
  }
  for (McResult& r : R) {
    std::sort(r.nodes.begin(), r.nodes.end());
    r.info.num_nodes = static_cast<int32_t>(r.nodes.size());
    r.info.seconds = elapsed();
  }
  return 0;
}

// a lone call: the driver on {h}, with h's stream, device and staging buffer; its launch count stays in the handle
int mc_run_one(Ctx* h, int method, double time_limit_s, McResult& r, const McSeeds* seeds = nullptr) {
  if (int rc = mc_check_scope(h)) return rc;
  if (seeds)
    if (int rc = mc_check_seed((*seeds)[0].data(), static_cast<int64_t>((*seeds)[0].size()), h->m)) return rc;
  std::vector<McResult> R;
  size_t fault = 0;
  h->mc_launches = 0;
  if (int rc = mc_run({h}, method, time_limit_s, h->sh[0].stream, h->sh[0].device, h->mc_stage, h->mc_launches, R, fault, seeds))
    return rc;
  r = std::move(R[0]);
  return 0;
}

int max_clique_impl(Ctx* h, int method, double time_limit_s, clipper_maxclique_info_t* info) {
  if (int rc = mc_check_method(method)) return rc;
  McResult r;
  if (int rc = mc_run_one(h, method, time_limit_s, r)) return rc;
  h->nodes = r.nodes;
  if (info) *info = r.info;
  return 0;
}

// the seeded call: seed == null and nseed == -1 stand for the context's node list
int max_clique_seeded_impl(Ctx* h, int method, double time_limit_s, const int32_t* seed, int32_t nseed,
                           clipper_maxclique_info_t* info, clipper_maxclique_seed_info_t* sinfo) {
  if (int rc = mc_check_method(method, true)) return rc;
  const bool own = !seed && nseed == -1;
  if (!own && (nseed < 0 || (nseed > 0 && !seed)))
    return fail(CLIPPER_HIP_E_INVALID, "max clique: a seed of %d entries at %s", nseed, seed ? "an address" : "NULL");
  const McSeeds seeds{own ? h->nodes : std::vector<int32_t>(seed, seed + nseed)};
  McResult r;
  if (int rc = mc_run_one(h, method, time_limit_s, r, &seeds)) return rc;
  h->nodes = r.nodes;
  if (info) *info = r.info;
  if (sinfo) *sinfo = r.seed;
  return 0;
}

// test infrastructure: values <= 0 restore the constants
int debug_mc_budgets(long long peel, long long wave) {
  g_mc_peel_budget.store(peel > 0 ? peel : MC_PEEL_BUDGET);
  g_mc_wave_budget.store(wave > 0 ? wave : MC_WAVE_BUDGET);
  return 0;
}

int core_numbers_impl(Ctx* h, int32_t* core_out) {
  McResult r;
  if (int rc = mc_run_one(h, MC_PEEL_ONLY, 0.0, r)) return rc;
  if (!r.core.empty()) std::memcpy(core_out, r.core.data(), r.core.size() * sizeof(int32_t));
  return 0;
}

// The maximum cliques of every problem of a batch's last solve: the problems up to BATCH_MAX_M in one driver call, then
// the larger ones one by one, each with the time that remains (a batch never holds several m^2 / 8 adjacencies at once).
// A seeded call hands in `seeds` and `offsets` (problem i's vertex list: seeds[offsets[i] .. offsets[i + 1])), or
// seeded = true and neither: every problem's own node list.
int batch_max_clique(Batch* b, int method, double time_limit_s, clipper_maxclique_info_t* infos, bool seeded = false,
                     const int32_t* seeds = nullptr, const int64_t* offsets = nullptr,
                     clipper_maxclique_seed_info_t* sinfos = nullptr) {
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto elapsed = [&] { return std::chrono::duration<double>(clk::now() - t0).count(); };
  if (!b->solved) return fail(CLIPPER_HIP_E_STATE, "max clique: no batch has been solved");
  if (int rc = mc_check_method(method, seeded)) return rc;
  if (seeded && ((seeds == nullptr) != (offsets == nullptr)))
    return fail(CLIPPER_HIP_E_INVALID, "max clique: seeds and offsets come together, or neither");
  b->mc_launches = b->mc_batched = b->mc_alone = 0;
  const size_t count = b->res.size();
  std::vector<std::vector<int32_t>> calls(1);  // the problems of each driver call: the batched route first
  for (size_t i = 0; i < count; ++i) {
    if (int rc = mc_check_scope(b->kids[i])) return fail(rc, "problem %zu: %s", i, std::string(g_err).c_str());
    if (b->kids[i]->m > clipper_mc_plan::BATCH_MAX_M) calls.push_back({static_cast<int32_t>(i)});
    else calls[0].push_back(static_cast<int32_t>(i));
  }
  McSeeds given(seeded ? count : 0);
  for (size_t i = 0; i < given.size(); ++i) {
    if (!offsets) {
      given[i] = b->res[i].nodes;
    } else {
      if (offsets[i] < 0 || offsets[i + 1] < offsets[i])
        return fail(CLIPPER_HIP_E_INVALID, "problem %zu: seed offsets %lld, %lld", i, (long long)offsets[i], (long long)offsets[i + 1]);
      given[i].assign(seeds + offsets[i], seeds + offsets[i + 1]);
    }
    if (int rc = mc_check_seed(given[i].data(), static_cast<int64_t>(given[i].size()), b->kids[i]->m))
      return fail(rc, "problem %zu: %s", i, std::string(g_err).c_str());
  }
  std::vector<McResult> all(count);
  for (size_t c = 0; c < calls.size(); ++c) {
    std::vector<Ctx*> cs;
    McSeeds sc;
    for (int32_t i : calls[c]) {
      cs.push_back(b->kids[static_cast<size_t>(i)]);
      if (seeded) sc.push_back(std::move(given[static_cast<size_t>(i)]));
    }
    // (no time left: the smallest positive limit, so that the call stops after its first launch)
    const double rem = time_limit_s > 0 ? std::max(time_limit_s - elapsed(), 1e-9) : 0.0;
    std::vector<McResult> R;
    int launches = 0;
    size_t fault = 0;
    if (int rc = mc_run(cs, method, rem, b->stream, b->device, b->hmc, launches, R, fault, seeded ? &sc : nullptr))
      return c > 0 || fault < cs.size()  // (a larger problem's call is all its own)
                 ? fail(rc, "problem %d: %s", calls[c][c > 0 ? 0 : fault], std::string(g_err).c_str()) : rc;
    for (size_t k = 0; k < cs.size(); ++k) all[static_cast<size_t>(calls[c][k])] = std::move(R[k]);
    if (c == 0) {
      b->mc_launches = launches;
      b->mc_batched = static_cast<int>(cs.size());
    } else {
      ++b->mc_alone;
    }
  }
  const double secs = elapsed();
  for (size_t i = 0; i < count; ++i) {
    Ctx* c = b->kids[i];
    Batch::Result& R = b->res[i];
    R.nodes = all[i].nodes;
    c->nodes = R.nodes;
    R.info.num_nodes = static_cast<int32_t>(R.nodes.size());  // (what the getters size their buffers by)
    R.sel.assign(2 * R.nodes.size(), 0);
    selected_associations(c, R.nodes, R.sel.data());
    all[i].info.seconds = secs;
    if (infos) infos[i] = all[i].info;
    if (sinfos) sinfos[i] = all[i].seed;
  }
  return 0;
}

}  // namespace
