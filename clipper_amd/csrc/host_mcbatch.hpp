// host_mcbatch.hpp — the maximum cliques of every problem of a batch's last solve in one call
// (clipper_hip_batch_max_clique; kernels in k_maxclique_batch.hip.h, the plan in host_mcplan.hpp, DESIGN.md section 9
// "Batches"). Part of clipper_hip.hip (one translation unit; included there, after host_batchsolve.hpp).
//
// A call
//   1. checks the batch and the method, splits the problems into the batched route (m <= BATCH_MAX_M) and the lone one,
//   2. plans ONE slab for the batched problems' G, alive, deg, degw, core, pos, lists, McCtl, slots, arenas, paths,
//      recs and the launch tables, checks it against the free memory and allocates it; the host's side of it is ONE
//      pinned staging buffer (kept by the batch from call to call),
//   3. builds every adjacency from the child's store (the slices where csc_valid, else the dense store: the rule of
//      mc_graph_and_cores), the degrees, and peels: ONE workgroup per unfinished problem and launch,
//   4. reads all deg and core back in ONE copy, sorts seeds and roots with the lone call's functions, writes all lists
//      in ONE copy per phase,
//   5. runs HEU, the regeneration of the winning cliques and EXACT over slot tables; after each launch ONE copy of the
//      McCtl array, the compaction of the work list to the unfinished problems, and the time limit,
//   6. runs the larger problems one by one through max_clique_impl on their child, with the time that remains.
// The number of copies and resets between launches does not depend on the number of problems. Per problem the node
// list, max_core, heuristic_size, edges and num_nodes are the lone call's: the device functions are the lone kernels'
// bodies, and their results are a function of the graph alone.
#pragma once

#include "host_mcplan.hpp"

namespace {

static_assert(sizeof(McItem) == sizeof(clipper_mc_plan::Item), "the plan's table rows are the kernels'");
static_assert(sizeof(McProb) % 8 == 0 && sizeof(McCtl) % 8 == 0 && sizeof(McSlot) % 8 == 0 && sizeof(McAdjSrc) % 8 == 0,
              "8-byte tables");

struct McSlab {
  uint8_t* p = nullptr;
  ~McSlab() {
    if (p) hipFree(p);
  }
};

int batch_max_clique(Batch* b, int method, double time_limit_s, clipper_maxclique_info_t* infos) {
  namespace plan = clipper_mc_plan;
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto elapsed = [&] { return std::chrono::duration<double>(clk::now() - t0).count(); };
  auto out_of_time = [&] { return time_limit_s > 0 && elapsed() >= time_limit_s; };
  if (!b->solved) return fail(CLIPPER_HIP_E_STATE, "max clique: no batch has been solved");
  if (method != CLIPPER_HIP_MC_EXACT && method != CLIPPER_HIP_MC_HEU && method != CLIPPER_HIP_MC_KCORE)
    return fail(CLIPPER_HIP_E_INVALID, "max clique: unknown method %d", method);
  b->mc_launches = b->mc_batched = b->mc_alone = 0;
  const size_t count = b->res.size();
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(b->device));
  hipStream_t st = b->stream;

  // ---- 1. the routes ---------------------------------------------------------------------------------------------
  std::vector<int32_t> ids, alone;  // problems of the batched route (k -> problem), of the lone route
  std::vector<plan::Size> sz;
  for (size_t i = 0; i < count; ++i) {
    const Ctx* c = b->kids[i];
    if (int rc = mc_check_scope(c)) return fail(rc, "problem %zu: %s", i, std::string(g_err).c_str());
    if (c->m > plan::BATCH_MAX_M) {
      alone.push_back(static_cast<int32_t>(i));
      continue;
    }
    const Shard& s = c->sh[0];
    if (!c->csc_valid && !s.S) return fail(CLIPPER_HIP_E_STATE, "problem %zu: max clique: the store of C is not on the device", i);
    ids.push_back(static_cast<int32_t>(i));
    sz.push_back(plan::Size{static_cast<int32_t>(c->m), c->csc_valid ? static_cast<int32_t>(s.s_ncg * s.s_nchunks) : 0});
  }
  const size_t nb = ids.size();
  std::vector<clipper_maxclique_info_t> I(count, clipper_maxclique_info_t{});
  std::vector<std::vector<int32_t>> nodes(count);

  // ---- 2. the slab -----------------------------------------------------------------------------------------------
  McSlab slab;
  plan::Plan L;
  if (nb) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    const int64_t cap = static_cast<int64_t>(std::max(1, b->kids[0]->cus)) * MC_WAVES_PER_CU;
    L = plan::make_plan(sz, cap, std::min<size_t>(free_b / 4, size_t(4) << 30), sizeof(McProb), sizeof(McCtl),
                        sizeof(McSlot), sizeof(McAdjSrc));
    if (L.bytes + (64u << 20) > free_b)
      return fail(CLIPPER_HIP_E_NOMEM, "max clique batch: %zu problems need a slab of %zu bytes, %zu are free", nb, L.bytes,
                  free_b);
    if (hipMalloc(reinterpret_cast<void**>(&slab.p), L.bytes) != hipSuccess) {
      slab.p = nullptr;
      (void)hipGetLastError();
      return fail(CLIPPER_HIP_E_NOMEM, "max clique batch: device allocation of %zu bytes failed", L.bytes);
    }
    const size_t hbytes = L.bytes - L.host_begin;
    if (hbytes > b->hmc_cap) {
      if (b->hmc) HIPCHK(hipHostFree(b->hmc));
      b->hmc = nullptr;
      b->hmc_cap = 0;
      HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&b->hmc), hbytes, hipHostMallocDefault));
      b->hmc_cap = hbytes;
    }
  }
  auto Dp = [&](size_t off) { return slab.p + off; };                        // on the device
  auto Hp = [&](size_t off) { return b->hmc + (off - L.host_begin); };       // its host copy (off >= host_begin)
  auto up = [&](size_t begin, size_t end) -> int {                           // host -> device, [begin, end)
    if (end > begin) HIPCHK(hipMemcpyAsync(Dp(begin), Hp(begin), end - begin, hipMemcpyHostToDevice, st));
    return 0;
  };
  auto down = [&](size_t begin, size_t end) -> int {                         // device -> host, and wait
    if (end > begin) HIPCHK(hipMemcpyAsync(Hp(begin), Dp(begin), end - begin, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  };

  if (nb) {
    McProb* probs = reinterpret_cast<McProb*>(Hp(L.probs));
    McCtl* ctl = reinterpret_cast<McCtl*>(Hp(L.ctl));
    McAdjSrc* src = reinterpret_cast<McAdjSrc*>(Hp(L.src));
    const McProb* dprobs = reinterpret_cast<const McProb*>(Dp(L.probs));
    McCtl* dctl = reinterpret_cast<McCtl*>(Dp(L.ctl));
    const McAdjSrc* dsrc = reinterpret_cast<const McAdjSrc*>(Dp(L.src));
    const int32_t* dwork = reinterpret_cast<const int32_t*>(Dp(L.work));
    const McItem* dslots = reinterpret_cast<const McItem*>(Dp(L.slot_tab));
    const size_t ctl_end = L.ctl + nb * sizeof(McCtl);
    const int lds1 = static_cast<int>(L.nw_max * 8);

    // ---- 3. descriptors and tables (one copy), adjacency, degrees, the peel ------------------------------------------
    std::memset(Hp(L.up_begin), 0, L.up_end - L.up_begin);
    bool any_dense = false;
    for (size_t k = 0; k < nb; ++k) {
      const Ctx* c = b->kids[static_cast<size_t>(ids[k])];
      const Shard& s = c->sh[0];
      const plan::Regions& r = L.at[k];
      McProb p{};
      p.G = reinterpret_cast<const uint64_t*>(Dp(r.G));
      p.nw = r.nw;
      p.m = sz[k].m;
      p.degw = reinterpret_cast<int32_t*>(Dp(r.degw));
      p.core = reinterpret_cast<int32_t*>(Dp(r.core));
      p.alive = reinterpret_cast<uint64_t*>(Dp(r.alive));
      p.pos = reinterpret_cast<const int32_t*>(Dp(r.pos));
      p.list = reinterpret_cast<const int32_t*>(Dp(r.list));
      p.out = reinterpret_cast<int32_t*>(Dp(r.out)) + 1;  // (out[-1]: the count k_mcb_collect leaves)
      p.ctl = dctl + k;
      p.slots = reinterpret_cast<McSlot*>(Dp(r.slots));
      p.arena = reinterpret_cast<uint64_t*>(Dp(r.arena));
      p.paths = reinterpret_cast<int32_t*>(Dp(r.paths));
      p.recs = reinterpret_cast<int32_t*>(Dp(r.recs));
      probs[k] = p;
      McAdjSrc a{};
      if (c->csc_valid) a.M = slice_view(c, s);
      else a.S = s.S;
      any_dense = any_dense || !c->csc_valid;
      a.ld = c->W;
      a.G = reinterpret_cast<uint64_t*>(Dp(r.G));
      a.nw = r.nw;
      a.m = sz[k].m;
      a.deg = reinterpret_cast<int32_t*>(Dp(r.deg));
      src[k] = a;
    }
    plan::adjacency_rows(sz, reinterpret_cast<plan::Item*>(Hp(L.slice_tab)), reinterpret_cast<plan::Item*>(Hp(L.row_tab)));
    if (int rc = up(L.up_begin, L.adj_end)) return rc;
    HIPCHK(hipMemsetAsync(Dp(L.G_begin), 0, L.G_bytes, st));
    HIPCHK(hipMemsetAsync(Dp(L.alive_begin), 0xff, L.alive_bytes, st));
    const McItem* dslice = reinterpret_cast<const McItem*>(Dp(L.slice_tab));
    const McItem* drow = reinterpret_cast<const McItem*>(Dp(L.row_tab));
    const int64_t nsr = static_cast<int64_t>(L.nslice_rows), nrr = static_cast<int64_t>(L.nrow_rows);
    if (nsr > 0) {
      dispatch_vt(b->kids[0], [&](auto t) {  // (the batch's value type)
        hipLaunchKernelGGL((k_mcb_adj_slices<decltype(t), SL_H>), dim3(static_cast<unsigned>(ceil_div(nsr, 4))), dim3(256),
                           0, st, dsrc, dslice, nsr);
      });
      HIPCHK(hipGetLastError());
      ++b->mc_launches;
    }
    if (any_dense) {
      dim3 grid(static_cast<unsigned>(ceil_div(nrr, 256)), static_cast<unsigned>(L.nw_max));
      dispatch_vt(b->kids[0], [&](auto t) {
        hipLaunchKernelGGL(k_mcb_adj_dense<decltype(t)>, grid, dim3(256), 0, st, dsrc, drow, nrr);
      });
      HIPCHK(hipGetLastError());
      ++b->mc_launches;
    }
    hipLaunchKernelGGL(k_mcb_degree, dim3(static_cast<unsigned>(ceil_div(nrr, 4))), dim3(256), 0, st, dsrc, drow, nrr);
    HIPCHK(hipGetLastError());
    ++b->mc_launches;
    HIPCHK(hipMemcpyAsync(Dp(L.degw_begin), Dp(L.deg_begin), L.deg_bytes, hipMemcpyDeviceToDevice, st));

    std::vector<int32_t> on_device;  // the work list the device holds
    auto put_work = [&](const std::vector<int32_t>& list) -> int {
      if (list == on_device) return 0;
      std::memcpy(Hp(L.work), list.data(), list.size() * sizeof(int32_t));
      on_device = list;
      return up(L.work, L.work + list.size() * sizeof(int32_t));
    };
    std::vector<int32_t> work(nb);
    std::iota(work.begin(), work.end(), 0);
    for (int64_t rounds = 0; !work.empty(); ++rounds) {
      if (rounds > plan::BATCH_MAX_M + 1) return fail(CLIPPER_HIP_E_INTERNAL, "max clique batch: the core peel made no progress");
      if (int rc = put_work(work)) return rc;
      hipLaunchKernelGGL(k_mcb_core_peel, dim3(static_cast<unsigned>(work.size())), dim3(MC_PEEL_THREADS), lds1, st, dprobs,
                         dwork, MC_PEEL_BUDGET);
      HIPCHK(hipGetLastError());
      ++b->mc_launches;
      if (int rc = down(L.ctl, ctl_end)) return rc;
      work = plan::compact(work, [&](int32_t k) { return ctl[k].removed >= sz[static_cast<size_t>(k)].m; });
    }

    // ---- 4. deg and core in one copy; KCORE's lists, HEU's seeds ----------------------------------------------------
    if (int rc = down(L.deg_begin, L.bytes)) return rc;
    std::vector<int32_t> Kmax(nb, 0), heu(nb, 0), nslots(nb, 0);
    std::vector<int32_t> searching;
    for (size_t k = 0; k < nb; ++k) {
      const int32_t m = sz[k].m;
      const int32_t* deg = reinterpret_cast<const int32_t*>(Hp(L.at[k].deg));
      const int32_t* core = reinterpret_cast<const int32_t*>(Hp(L.at[k].core));
      clipper_maxclique_info_t& Ik = I[static_cast<size_t>(ids[k])];
      int64_t dsum = 0;
      int K = 0;
      for (int32_t v = 0; v < m; ++v) {
        dsum += deg[v];
        K = std::max(K, core[v]);
      }
      Ik.edges = dsum / 2;
      Ik.max_core = K;
      Kmax[k] = K;
      nslots[k] = L.at[k].nslots;
      if (method == CLIPPER_HIP_MC_KCORE) {
        for (int32_t v = 0; v < m; ++v)
          if (core[v] == K) nodes[static_cast<size_t>(ids[k])].push_back(v);
      } else if (Ik.edges > 0) {
        plan::seed_order(core, m, reinterpret_cast<int32_t*>(Hp(L.at[k].list)));
        probs[k].nlist = m;
        searching.push_back(static_cast<int32_t>(k));
      }
    }

    // one launch over the slot table of `list`, then the copy of the control array
    std::vector<int32_t> tabled;  // the list whose slot table the device holds
    auto launch_slots = [&](const std::vector<int32_t>& list, const std::vector<int32_t>& ns, bool exact) -> int {
      size_t rows = 0;
      for (int32_t k : list) rows += static_cast<size_t>(ns[static_cast<size_t>(k)]);
      if (list != tabled) {
        const std::vector<plan::Item> tab = plan::slot_rows(list, ns);
        std::memcpy(Hp(L.slot_tab), tab.data(), tab.size() * sizeof(plan::Item));
        tabled = list;
        if (int rc = up(L.slot_tab, L.slot_tab + tab.size() * sizeof(plan::Item))) return rc;
      }
      if (exact) {
        // `active` of every problem: one call
        HIPCHK(hipMemset2DAsync(&dctl[0].active, sizeof(McCtl), 0, sizeof(int32_t), nb, st));
        hipLaunchKernelGGL(k_mcb_exact, dim3(static_cast<unsigned>(rows)), dim3(64), 2 * lds1, st, dprobs, dslots, MC_WAVE_BUDGET);
      } else {
        hipLaunchKernelGGL(k_mcb_heu, dim3(static_cast<unsigned>(rows)), dim3(64), lds1, st, dprobs, dslots, MC_WAVE_BUDGET);
      }
      HIPCHK(hipGetLastError());
      ++b->mc_launches;
      return down(L.ctl, ctl_end);
    };

    if (!searching.empty()) {
      // ---- 5a. HEU ------------------------------------------------------------------------------------------------
      std::memset(ctl, 0, nb * sizeof(McCtl));
      if (int rc = up(L.up_begin, L.up_end)) return rc;
      std::vector<int32_t> active = searching;
      while (!active.empty()) {
        if (int rc = launch_slots(active, nslots, false)) return rc;
        active = plan::compact(active, [&](int32_t k) { return ctl[k].head >= sz[static_cast<size_t>(k)].m; });
        if (!active.empty() && out_of_time()) {
          for (int32_t k : active) I[static_cast<size_t>(ids[static_cast<size_t>(k)])].timed_out = 1;
          break;
        }
      }
      std::vector<int32_t> regen, exact;
      std::vector<int64_t> weight(nb, 0);
      std::vector<std::vector<int32_t>> roots(nb);
      const std::vector<McCtl> after_heu(ctl, ctl + nb);
      std::memset(ctl, 0, nb * sizeof(McCtl));
      for (int32_t k : searching) {
        const size_t ku = static_cast<size_t>(k);
        clipper_maxclique_info_t& Ik = I[static_cast<size_t>(ids[ku])];
        const int32_t m = sz[ku].m;
        const unsigned long long key = after_heu[ku].key;
        const int h = static_cast<int>(key >> 32);
        const int seed = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(key & 0xFFFFFFFFull));
        // (as in the lone call: every launch finishes the seeds it takes, the first of which has the largest core
        // number, so after one launch the record holds a clique of two vertices or more, time limit or not)
        if (h < 2 || h > Kmax[ku] + 1 || seed < 0 || seed >= m)
          return fail(CLIPPER_HIP_E_INTERNAL, "problem %d: max clique: HEU's record (size %d, seed %d) is not valid", ids[ku], h, seed);
        heu[ku] = h;
        Ik.heuristic_size = h;
        probs[ku].seed = seed;
        regen.push_back(k);
        if (method == CLIPPER_HIP_MC_EXACT && h < Kmax[ku] + 1 && !Ik.timed_out) {
          // EXACT's order and roots replace the seeds; the incumbent starts at HEU's clique
          const int32_t* deg = reinterpret_cast<const int32_t*>(Hp(L.at[ku].deg));
          const int32_t* core = reinterpret_cast<const int32_t*>(Hp(L.at[ku].core));
          plan::root_order(core, deg, m, h, reinterpret_cast<int32_t*>(Hp(L.at[ku].pos)), roots[ku]);
          std::memcpy(Hp(L.at[ku].list), roots[ku].data(), roots[ku].size() * sizeof(int32_t));
          Ik.roots_pruned = m - static_cast<int64_t>(roots[ku].size());
          probs[ku].nlist = static_cast<int32_t>(roots[ku].size());
          probs[ku].heu = h;
          probs[ku].D = Kmax[ku] + 1;  // stack levels: a clique has at most K + 1 vertices (<= m, the arena's room)
          McSlot* hs = reinterpret_cast<McSlot*>(Hp(L.at[ku].slots));
          for (int32_t j = 0; j < L.at[ku].nslots; ++j) hs[j] = McSlot{-1, 0, 0, 0, 0ull};
          ctl[ku].key = (static_cast<unsigned long long>(h) << 32) | 0xFFFFFFFFull;
          weight[ku] = static_cast<int64_t>(roots[ku].size());
          if (!roots[ku].empty()) exact.push_back(k);
        }
      }
      // EXACT's slots: in proportion to the roots, within the slots the plan gave the problem room for
      std::vector<int32_t> xslots = plan::deal_slots(weight, static_cast<int64_t>(std::max(1, b->kids[0]->cus)) * MC_WAVES_PER_CU);
      for (size_t k = 0; k < nb; ++k) {
        xslots[k] = std::min(xslots[k], L.at[k].nslots);
        probs[k].nslots = xslots[k];
      }
      if (int rc = up(L.up_begin, L.up_end)) return rc;

      // ---- 5b. the winning cliques of HEU ----------------------------------------------------------------------------
      if (!regen.empty()) {
        if (int rc = put_work(regen)) return rc;
        hipLaunchKernelGGL(k_mcb_heu_one, dim3(static_cast<unsigned>(regen.size())), dim3(64), lds1, st, dprobs, dwork);
        HIPCHK(hipGetLastError());
        ++b->mc_launches;
        if (int rc = down(L.out_begin, L.out_begin + L.out_bytes)) return rc;
        for (int32_t k : regen) {
          const int32_t* out = reinterpret_cast<const int32_t*>(Hp(L.at[static_cast<size_t>(k)].out)) + 1;
          nodes[static_cast<size_t>(ids[static_cast<size_t>(k)])].assign(out, out + heu[static_cast<size_t>(k)]);
        }
      }

      // ---- 5c. EXACT ---------------------------------------------------------------------------------------------------
      if (!exact.empty()) {
        active = exact;
        tabled.clear();  // (the same problems may get other slot counts than in HEU)
        while (!active.empty()) {
          if (int rc = launch_slots(active, xslots, true)) return rc;
          active = plan::compact(active, [&](int32_t k) {
            return ctl[k].head >= probs[k].nlist && ctl[k].active == 0;
          });
          if (!active.empty() && out_of_time()) {
            for (int32_t k : active) I[static_cast<size_t>(ids[static_cast<size_t>(k)])].timed_out = 1;
            break;
          }
        }
        std::vector<int32_t> better;
        for (int32_t k : exact) {
          const size_t ku = static_cast<size_t>(k);
          clipper_maxclique_info_t& Ik = I[static_cast<size_t>(ids[ku])];
          if (ctl[ku].overflow)
            return fail(CLIPPER_HIP_E_INTERNAL, "problem %d: max clique: a branch went deeper than the core bound", ids[ku]);
          Ik.roots_pruned += static_cast<int64_t>(ctl[ku].roots_pruned);
          Ik.roots_searched = static_cast<int64_t>(ctl[ku].roots_searched);
          Ik.bb_nodes = static_cast<int64_t>(ctl[ku].bb_nodes);
          if (static_cast<int>(ctl[ku].key >> 32) > heu[ku]) better.push_back(k);
        }
        if (!better.empty()) {
          if (int rc = put_work(better)) return rc;
          hipLaunchKernelGGL(k_mcb_collect, dim3(static_cast<unsigned>(better.size())), dim3(64), 0, st, dprobs, dwork);
          HIPCHK(hipGetLastError());
          ++b->mc_launches;
          if (int rc = down(L.out_begin, L.out_begin + L.out_bytes)) return rc;
          for (int32_t k : better) {
            const size_t ku = static_cast<size_t>(k);
            const int32_t* out = reinterpret_cast<const int32_t*>(Hp(L.at[ku].out));
            const int omega = static_cast<int>(ctl[ku].key >> 32);
            if (out[0] != omega) return fail(CLIPPER_HIP_E_INTERNAL, "problem %d: max clique: no record holds the incumbent", ids[ku]);
            nodes[static_cast<size_t>(ids[ku])].assign(out + 1, out + 1 + omega);
          }
        }
      }
    }
    b->mc_batched = static_cast<int>(nb);
  }

  // ---- 6. the larger problems, one by one, with the time that remains -------------------------------------------------
  for (int32_t i : alone) {
    Ctx* c = b->kids[static_cast<size_t>(i)];
    // (no time left: the smallest positive limit, so that the call stops after its first launch)
    const double rem = time_limit_s > 0 ? std::max(time_limit_s - elapsed(), 1e-9) : 0.0;
    if (int rc = max_clique_impl(c, method, rem, &I[static_cast<size_t>(i)]))
      return fail(rc, "problem %d: %s", i, std::string(g_err).c_str());
    nodes[static_cast<size_t>(i)] = c->nodes;
    ++b->mc_alone;
  }

  const double secs = elapsed();
  for (size_t i = 0; i < count; ++i) {
    Ctx* c = b->kids[i];
    Batch::Result& R = b->res[i];
    std::sort(nodes[i].begin(), nodes[i].end());
    R.nodes = nodes[i];
    c->nodes = R.nodes;
    R.info.num_nodes = static_cast<int32_t>(R.nodes.size());  // (what the getters size their buffers by)
    R.sel.assign(2 * R.nodes.size(), 0);
    selected_associations(c, R.nodes, R.sel.data());
    I[i].num_nodes = R.info.num_nodes;
    I[i].seconds = secs;
    if (infos) infos[i] = I[i];
  }
  return 0;
}

}  // namespace
