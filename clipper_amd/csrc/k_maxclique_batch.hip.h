// k_maxclique_batch.hip.h — the maximum-clique solver on every problem of a batch ("Batches"):
// the launches of k_maxclique.hip.h with one more index. Every kernel here fetches its problem's descriptor from a
// device table and calls the device function the lone kernel calls, so per problem the arithmetic, the tie rules and
// hence the results are the lone call's. Host side: host_mcbatch.hpp, the tables' rows: host_mcplan.hpp.
// Part of kernels.hip.h (include that one).
//
// As in the lone kernels no workgroup waits for another (more workgroups than the chip holds is fine), no launch is
// cooperative, and the only words workgroups share are a problem's head, incumbent key and counters in its McCtl.
#pragma once

#include "k_maxclique.hip.h"

namespace clipper_hip {

struct McItem {  // a row of a launch table (= clipper_mc_plan::Item)
  int32_t prob, idx;
};

// where a problem's adjacency is read from and written to
struct McAdjSrc {
  SliceView M;     // the slices of its store (the slice storages)
  const void* S;   // its dense store S[j][c], row pitch ld (the dense storages)
  int64_t ld;
  uint64_t* G;
  int64_t nw, m;
  int32_t* deg;
};

// one wave per (problem, slice); G zeroed by the caller
template <typename VT, int H>
__global__ __launch_bounds__(256) void k_mcb_adj_slices(const McAdjSrc* __restrict__ src,
                                                        const McItem* __restrict__ rows, int64_t nrows) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (e >= nrows) return;
  const McItem it = rows[e];
  const McAdjSrc& a = src[it.prob];
  mc_adj_slice<VT, H>(a.M, a.G, a.nw, a.m, it.idx, threadIdx.x & 63);
}

// one thread per (problem, row, word): x = the (problem, row) table, y = the word (strided when nw > the grid's y).
// The table holds every problem's rows (the degree launch uses it too); the rows of a problem with no dense store
// (S == null: its slices are valid) are skipped, so a batch may hold both kinds.
template <typename T>
__global__ __launch_bounds__(256) void k_mcb_adj_dense(const McAdjSrc* __restrict__ src,
                                                       const McItem* __restrict__ rows, int64_t nrows) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (e >= nrows) return;
  const McItem it = rows[e];
  const McAdjSrc& a = src[it.prob];
  if (!a.S) return;  // (a problem whose graph comes from its slices: k_mcb_adj_slices has built its rows)
  const int64_t c = it.idx;
  for (int64_t w = blockIdx.y; w < a.nw; w += gridDim.y)
    a.G[c * a.nw + w] = mc_adj_dense_word(static_cast<const T*>(a.S), a.ld, a.m, c, w);
}

// one wave per (problem, row)
__global__ __launch_bounds__(256) void k_mcb_degree(const McAdjSrc* __restrict__ src, const McItem* __restrict__ rows,
                                                    int64_t nrows) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (e >= nrows) return;
  const McItem it = rows[e];
  const McAdjSrc& a = src[it.prob];
  mc_degree_row(a.G, a.nw, it.idx, a.deg, threadIdx.x & 63);
}

// one workgroup per unfinished problem (work[blockIdx.x]); dynamic LDS: the largest nw of the launch, in words
__global__ __launch_bounds__(MC_PEEL_THREADS) void k_mcb_core_peel(const McProb* __restrict__ probs,
                                                                   const int32_t* __restrict__ work, long long budget) {
  extern __shared__ uint64_t mc_alive[];
  __shared__ int32_t fr[MC_PEEL_FCAP];
  __shared__ int32_t sc[2];
  const McProb P = probs[work[blockIdx.x]];
  mc_peel(P, budget, mc_alive, fr, sc);
}

// one wave per slot; a slot takes its problem's seeds through that problem's head
__global__ __launch_bounds__(64) void k_mcb_heu(const McProb* __restrict__ probs, const McItem* __restrict__ slots,
                                                long long budget) {
  extern __shared__ uint64_t mc_cand[];
  const McProb P = probs[slots[blockIdx.x].prob];
  if (mc_load_i32(&P.ctl->head) >= P.nlist) return;  // (its problem is finished)
  mc_heu(P, budget, mc_cand);
}

// one wave per problem of the work list: the clique of its winning seed
__global__ __launch_bounds__(64) void k_mcb_heu_one(const McProb* __restrict__ probs, const int32_t* __restrict__ work) {
  extern __shared__ uint64_t mc_cand[];
  const McProb P = probs[work[blockIdx.x]];
  mc_heu_one(P, mc_cand);
}

// one wave per slot, with the stack, path and record the lone kernel keeps for it
__global__ __launch_bounds__(64) void k_mcb_exact(const McProb* __restrict__ probs, const McItem* __restrict__ slots,
                                                  long long budget) {
  extern __shared__ uint64_t mc_lds[];
  const McItem it = slots[blockIdx.x];
  const McProb P = probs[it.prob];
  if (P.slots[it.idx].root < 0 && mc_load_i32(&P.ctl->head) >= P.nlist) return;  // (nothing left for this slot)
  mc_exact(P, it.idx, budget, mc_lds);
}

// one wave per problem of the work list whose incumbent beat HEU's clique: the record of the slot that raised the
// final key goes to out[0 .. omega), its length to out[-1] (-1: no slot holds it)
__global__ __launch_bounds__(64) void k_mcb_collect(const McProb* __restrict__ probs, const int32_t* __restrict__ work) {
  const McProb P = probs[work[blockIdx.x]];
  const int lane = threadIdx.x;
  const unsigned long long key = P.ctl->key;
  int who = -1;
  for (int j = lane; j < P.nslots; j += 64)
    if (P.slots[j].rec_key == key) who = j;
  who = mc_wave_max(who);
  const int omega = static_cast<int>(key >> 32);
  if (who >= 0) {
    const int32_t* rec = P.recs + static_cast<int64_t>(who) * (P.D + 1);
    for (int i = lane; i < omega; i += 64) P.out[i] = rec[i];
  }
  if (lane == 0) P.out[-1] = who >= 0 ? omega : -1;
}

}  // namespace clipper_hip
