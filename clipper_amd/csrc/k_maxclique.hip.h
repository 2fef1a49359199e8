// k_maxclique.hip.h — the maximum-clique solver behind CLIPPER::solveAsMaximumClique:
// the adjacency of the consistency graph as row bitsets, its core numbers, the seed clique of a seeded call, the greedy
// clique (HEU) and the bitset branch and bound (EXACT), for every problem of a call. Host side: host_maxclique.hpp,
// host_mcplan.hpp.
// Part of kernels.hip.h (include that one): hand-written gfx950 device code of the CLIPPER hot path.
//
// The graph: vertices 0..m-1, edge (i, j), i != j, exactly when C(i, j) != 0. G[i][w] bit b = edge (i, 64 w + b),
// nw = ceil(m / 64) words per row, bits at or past m are zero.
//
// Every launch does a bounded amount of work (a budget in row-word operations per wave, or per workgroup for the
// peel) and leaves its state in device memory: the host loop resumes it with the next launch and checks the
// caller's time limit between launches. No workgroup ever waits for another: work is taken through an atomicAdd
// head, the incumbent is one atomicMax word.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_wave.hip.h"
#include "k_slices.hip.h"

namespace clipper_hip {

// device state of one max-clique call (zeroed by the host before each phase uses its fields)
struct McCtl {
  int32_t k;            // core peel: the current level
  int32_t removed;      // core peel: vertices peeled so far
  int32_t head;         // HEU seeds / EXACT roots taken
  int32_t active;       // EXACT: slots that left a root unfinished at the end of the launch
  unsigned long long key;  // incumbent: size << 32 | tie field (HEU: ~seed; EXACT: 0xFFFFFFFE - pos, HEU's clique 0xFFFFFFFF)
  unsigned long long roots_pruned, roots_searched, bb_nodes;
  int32_t overflow;     // EXACT: a branch deeper than the clique-size bound (cannot happen; checked, never silent)
  int32_t seed_size;    // a seeded call: the vertices of the seed clique Q0 ...
  int32_t seed_kept;    // ... and how many of them the caller's list gave (k_mc_seed writes both)
  int32_t pad;
};

// one EXACT wave's resumable state
struct McSlot {
  int32_t root;    // vertex being searched, -1 = none
  int32_t depth;   // top level of its stack
  int32_t pad0, pad1;
  unsigned long long rec_key;  // the key of the clique this slot recorded last (0: none)
};

// One problem as the device functions below see it. A call keeps a table of them on the device, one row per problem
// (a lone call: one row), and every kernel fetches its problem's row. The host fills the fields a phase reads: the
// peel G, nw, m, degw, core, alive, ctl; the seed clique of a seeded call also given, ngiven, out; HEU also list
// (seeds), nlist; the regeneration seed, out; EXACT list (roots), nlist, pos, heu, D and the slots' state.
struct McProb {
  const uint64_t* G;     // m rows of nw words
  int64_t nw;
  int32_t m;
  int32_t nlist;         // seeds (HEU) / roots (EXACT) in `list`
  int32_t* degw;         // the peel's working degrees
  int32_t* core;
  uint64_t* alive;       // nw words: the peel's alive set between launches
  const int32_t* pos;    // EXACT: the (core, degree, index) order
  const int32_t* list;
  int32_t heu;           // EXACT: HEU's size
  int32_t D;             // EXACT: stack levels of a slot
  int32_t seed;          // the regeneration of HEU's clique: its seed ...
  int32_t nslots;        // EXACT: the problem's slots (read by the collection of the record only)
  int32_t* out;          // ... and where it goes (out[-1]: the count k_mc_collect leaves)
  const int32_t* given;  // a seeded call: the caller's vertex list (distinct, in range) ...
  int32_t ngiven;        // ... and its length (0: the problem is not seeded)
  int32_t pad;
  McCtl* ctl;
  McSlot* slots;         // EXACT, per slot: state, D x nw words of stack, D + 1 path entries, D + 1 record entries
  uint64_t* arena;
  int32_t* paths;
  int32_t* recs;
};

struct McItem {  // a row of a launch table (= clipper_mc_plan::Item)
  int32_t prob, idx;
};

// where a problem's adjacency is read from and written to
struct McAdjSrc {
  SliceView M;     // the slices of its store (S == null)
  const void* S;   // else a dense store S[j][c], row pitch ld: the explicit C or M's values
  int64_t ld;
  uint64_t* G;
  int64_t nw, m;
  int32_t* deg;
};

constexpr int MC_PEEL_THREADS = 1024;
constexpr int MC_PEEL_FCAP = 2048;  // vertices peeled per round at most (the rest wait for the next round)

// ---- helpers (one wave = one workgroup of 64 lanes in the HEU / EXACT kernels; the folds are k_wave.hip.h's) ----
__device__ __forceinline__ unsigned long long mc_load_key(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int mc_load_i32(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// First non-zero word of X[lo, hi) (LDS, one wave), or -1. The word index is wave-uniform.
__device__ __forceinline__ int mc_first_word(const uint64_t* X, int lo, int hi, int lane) {
  for (int base = lo; base < hi; base += 64) {
    const int w = base + lane;
    const uint64_t x = (w < hi) ? X[w] : 0ull;
    const uint64_t msk = __ballot(x != 0ull);
    if (msk) return base + __ffsll(static_cast<unsigned long long>(msk)) - 1;
  }
  return -1;
}

// ---- adjacency ---------------------------------------------------------------------------------------------
// From the slices of a one-shard store (k_slices.hip.h): one wave per slice, lane = column c. Both triangles are
// stored, so column c's entries are row c of the graph. G is zeroed by the caller; a lane writes only words of
// its own row, the atomic OR keeps the chunks of one column group (other waves, other words) independent.
template <typename VT, int H>
__device__ __forceinline__ void mc_adj_slice(const SliceView& M, uint64_t* __restrict__ G, int64_t nw, int64_t m,
                                             int64_t s, int lane) {
  constexpr int QB = 4 * static_cast<int>(sizeof(VT));
  constexpr int R = SL_SUB * H;
  if (s >= static_cast<int64_t>(M.ncg) * M.nchunks) return;
  const int cg = static_cast<int>(s / M.nchunks), k = static_cast<int>(s - static_cast<int64_t>(cg) * M.nchunks);
  const int64_t c = static_cast<int64_t>(cg) * SL_W + lane;
  const int64_t r0 = static_cast<int64_t>(k) * R;
  SliceHead<H> hd;
  hd.load(static_cast<gbytes_t>((gbytes_t)M.data + 16 * M.Pre[s]), lane);
  const int maxq = __builtin_amdgcn_readfirstlane(hd.maxq);
  int tot = 0;
#pragma unroll
  for (int h = 0; h < H; ++h) tot += hd.nq[h];
  gbytes_t fbase = hd.sp + 16 + H * 64 + sl_so_bytes(maxq);
  for (int q = 0; q < maxq; ++q) {
    const bool active = q < tot;
    const uint64_t mask = __ballot(active);
    const int cnt = __popcll(mask);
    if (active && c < m) {
      const uint32_t rank = sl_lane_rank(mask);
      SliceQuad<VT> vq;
      vq.load(fbase + rank * QB);
      const uint32_t rq = *reinterpret_cast<const CLIPPER_GLOBAL uint32_t*>(fbase + cnt * QB + rank * 4);
      int rowbase = 0, edge = hd.nq[0];
#pragma unroll
      for (int h = 1; h < H; ++h) {
        rowbase = (q >= edge) ? h * SL_SUB : rowbase;
        edge += hd.nq[h];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (vq.v[e] != VT(0)) {
          const int64_t row = r0 + rowbase + ((rq >> (8 * e)) & 255u);
          if (row < m && row != c)
            atomicOr(reinterpret_cast<unsigned long long*>(G + c * nw + (row >> 6)), 1ull << (row & 63));
        }
    }
    fbase += cnt * QB + ((cnt * 4 + 15) & ~15);
  }
}

// From a dense one-shard store S[j][c] (row pitch ld; M's values or the explicit C): thread = (row c, word w),
// bit b set when S[64 w + b][c] != 0. The loads of one j are coalesced over c. Writes every word of G.
template <typename T>
__device__ __forceinline__ uint64_t mc_adj_dense_word(const T* __restrict__ S, int64_t ld, int64_t m, int64_t c,
                                                      int64_t w) {
  uint64_t word = 0;
  const int64_t j0 = w * 64;
  const int nb = static_cast<int>((m - j0) < 64 ? (m - j0) : 64);
  for (int b = 0; b < nb; ++b)
    if (S[(j0 + b) * ld + c] != T(0) && j0 + b != c) word |= 1ull << b;
  return word;
}

// degree of every vertex: one wave per row
__device__ __forceinline__ void mc_degree_row(const uint64_t* __restrict__ G, int64_t nw, int64_t v,
                                              int32_t* __restrict__ deg, int lane) {
  int d = 0;
  for (int64_t w = lane; w < nw; w += 64) d += __popcll(G[v * nw + w]);
  d = wave_sum(d);
  if (lane == 0) deg[v] = d;
}

// ---- core numbers: level-synchronous peeling (Batagelj-Zaversnik levels), one workgroup -------------------------
// Round: every alive vertex with degree <= k is peeled with core number k (at most MC_PEEL_FCAP of them; the rest
// in the next round), the degrees of its alive neighbours drop by one; a round that peels nothing raises k to the
// least alive degree. The result is the core number of every vertex, whatever the order within a round. The
// alive set lives in LDS for the launch and in `alive_g` between launches; `deg` is the working degree (updated
// by atomics, read with L1-bypassing loads); the launch returns after `budget` row-word operations at a round's end.
// The workgroup's LDS: mc_alive (nw words, dynamic), fr (MC_PEEL_FCAP entries), sc (nf, mindeg).
__device__ __forceinline__ void mc_peel(const McProb& P, long long budget, uint64_t* mc_alive, int32_t* fr, int32_t* sc) {
  const uint64_t* __restrict__ G = P.G;
  const int64_t nw = P.nw;
  const int32_t m = P.m;
  int32_t* deg = P.degw;
  int32_t* __restrict__ core = P.core;
  uint64_t* __restrict__ alive_g = P.alive;
  McCtl* ctl = P.ctl;
  int32_t& nf_s = sc[0];
  int32_t& mindeg_s = sc[1];
  const int tid = threadIdx.x;
  for (int64_t w = tid; w < nw; w += MC_PEEL_THREADS) mc_alive[w] = alive_g[w];
  int k = ctl->k, removed = ctl->removed;
  long long work = 0;
  __syncthreads();
  while (removed < m && work < budget) {
    if (tid == 0) {
      nf_s = 0;
      mindeg_s = 0x7fffffff;
    }
    __syncthreads();
    for (int v = tid; v < m; v += MC_PEEL_THREADS) {
      if (!((mc_alive[v >> 6] >> (v & 63)) & 1ull)) continue;
      const int d = mc_load_i32(deg + v);
      if (d <= k) {
        const int slot = atomicAdd(&nf_s, 1);
        if (slot < MC_PEEL_FCAP) {
          fr[slot] = v;
          core[v] = k;
          continue;
        }
      }
      atomicMin(&mindeg_s, d);
    }
    __syncthreads();
    const int n = nf_s < MC_PEEL_FCAP ? nf_s : MC_PEEL_FCAP;
    if (n == 0) {
      k = mindeg_s > k ? mindeg_s : k;  // (nothing alive at or below k)
      __syncthreads();
      continue;
    }
    for (int i = tid; i < n; i += MC_PEEL_THREADS)
      atomicAnd(reinterpret_cast<unsigned long long*>(&mc_alive[fr[i] >> 6]), ~(1ull << (fr[i] & 63)));
    __syncthreads();
    const int64_t items = static_cast<int64_t>(n) * nw;
    for (int64_t it = tid; it < items; it += MC_PEEL_THREADS) {
      const int f = fr[it / nw];
      const int64_t w = it - (it / nw) * nw;
      uint64_t bits = G[static_cast<int64_t>(f) * nw + w] & mc_alive[w];
      while (bits) {
        const int b = __ffsll(static_cast<unsigned long long>(bits)) - 1;
        bits &= bits - 1;
        atomicSub(deg + (w * 64 + b), 1);
      }
    }
    removed += n;
    work += items + n;
    __threadfence();  // the decrements (L2 atomics) complete before the next round reads the degrees
    __syncthreads();
  }
  for (int64_t w = tid; w < nw; w += MC_PEEL_THREADS) alive_g[w] = mc_alive[w];
  if (tid == 0) {
    ctl->k = k;
    ctl->removed = removed;
  }
}

// ---- HEU: the greedy clique of one seed (one wave; C = the candidate bitset in LDS) ------------------------------
// Candidates: N(v) minus the vertices with core + 1 < thr; step: take the candidate of largest core number (ties:
// smallest index), intersect with its row. Every pick's core is at most the previous one's, so with thr <= the
// final best size the clique of every seed that can reach that size is the one thr = 0 gives.
// Returns the size; `out` (may be null, lane 0 writes) receives the clique in pick order. Adds the row-word
// operations to `work`.
// The loop is entered after `size` picks, the last of which is u: with v = u = the seed and size = 1 by mc_greedy,
// where the candidates are the seed's row; with v = -1 by mc_seed_clique, where C already holds the common
// neighbourhood of the picks so far (the first intersection with u's row then changes nothing).
__device__ __forceinline__ int mc_greedy_loop(const uint64_t* __restrict__ G, int64_t nw,
                                              const int32_t* __restrict__ core, int v, int u, int size, int thr,
                                              uint64_t* C, int32_t* out, long long& work, int lane) {
  while (true) {
    unsigned long long bk = 0;
    const uint64_t* row = G + static_cast<int64_t>(u) * nw;
    for (int64_t w = lane; w < nw; w += 64) {
      uint64_t word = (u == v ? ~0ull : C[w]) & row[w];
      uint64_t bits = word;
      while (bits) {
        const int b = __ffsll(static_cast<unsigned long long>(bits)) - 1;
        bits &= bits - 1;
        const int x = static_cast<int>(w * 64 + b);
        const int cx = core[x];
        if (cx + 1 < thr) {
          word &= ~(1ull << b);
          continue;
        }
        const unsigned long long kx = (static_cast<unsigned long long>(cx + 1) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(x));
        bk = kx > bk ? kx : bk;
      }
      C[w] = word;
    }
    work += nw / 64 + 1;
    bk = wave_max(bk);
    __syncthreads();
    if (bk == 0) break;
    u = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(bk & 0xFFFFFFFFull));
    if (out && lane == 0) out[size] = u;
    ++size;
  }
  return size;
}

__device__ int mc_greedy(const uint64_t* __restrict__ G, int64_t nw, const int32_t* __restrict__ core, int v,
                         int thr, uint64_t* C, int32_t* out, long long& work, int lane) {
  if (out && lane == 0) out[0] = v;
  return mc_greedy_loop(G, nw, core, v, v, 1, thr, C, out, work, lane);
}

// ---- the seed clique Q0 of a seeded call (DESIGN.md 9 "Seeded calls"; one wave) --------------------------------------
// Reduce: degS(v) = |N(v) & S| for the vertices of the caller's list S, computed once; the candidates start as S;
// take the candidate of largest degS (ties: smallest index), intersect the candidates with its row, until none is
// left. Extend: the candidates become the common neighbourhood of the vertices taken, over all vertices, and
// mc_greedy's loop goes on from there (largest core number, ties smallest index, no threshold). Q0, in pick order,
// goes to P.out, its size to out[-1] and ctl->seed_size, the vertices the reduction took to ctl->seed_kept.
// LDS: S, C (nw words each). degS is kept by the position in the list, in P.degw (dead after the peel), so that a
// pick reads the list and its degS in order; it is written and read through L2 like the peel's degrees.
__device__ __forceinline__ void mc_seed_clique(const McProb& P, uint64_t* mc_lds) {
  const uint64_t* __restrict__ G = P.G;
  const int64_t nw = P.nw;
  const int32_t* __restrict__ given = P.given;
  const int32_t n = P.ngiven;
  int32_t* degS = P.degw;
  uint64_t* S = mc_lds;
  uint64_t* C = mc_lds + nw;
  const int lane = threadIdx.x;
  if (n <= 0) return;  // (the host lists seeded problems only; with a vertex in S the reduction takes one)
  for (int64_t w = lane; w < nw; w += 64) {
    S[w] = 0ull;
    C[w] = ~0ull;
  }
  __syncthreads();
  for (int i = lane; i < n; i += 64)
    atomicOr(reinterpret_cast<unsigned long long*>(&S[given[i] >> 6]), 1ull << (given[i] & 63));
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const uint64_t* row = G + static_cast<int64_t>(given[i]) * nw;
    int d = 0;
    for (int64_t w = lane; w < nw; w += 64) d += __popcll(row[w] & S[w]);
    d = wave_sum(d);
    if (lane == 0) __hip_atomic_store(degS + i, d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __threadfence();
  __syncthreads();
  int kept = 0, u = -1;
  while (true) {
    unsigned long long bk = 0;
    for (int i = lane; i < n; i += 64) {
      const int x = given[i];
      if (!((S[x >> 6] >> (x & 63)) & 1ull)) continue;
      const unsigned long long kx =
          (static_cast<unsigned long long>(mc_load_i32(degS + i) + 1) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(x));
      bk = kx > bk ? kx : bk;
    }
    bk = wave_max(bk);
    if (bk == 0) break;
    u = static_cast<int>(0xFFFFFFFFu - static_cast<uint32_t>(bk & 0xFFFFFFFFull));
    if (lane == 0) P.out[kept] = u;
    ++kept;
    const uint64_t* row = G + static_cast<int64_t>(u) * nw;
    __syncthreads();
    for (int64_t w = lane; w < nw; w += 64) {
      S[w] &= row[w];
      C[w] &= row[w];
    }
    __syncthreads();
  }
  long long work = 0;
  const int size = mc_greedy_loop(G, nw, P.core, -1, u, kept, 0, C, P.out, work, lane);
  if (lane == 0) {
    P.out[-1] = size;
    P.ctl->seed_size = size;
    P.ctl->seed_kept = kept;
  }
}

// Seeds (the host's order: core descending) taken through ctl->head; a seed whose core + 1 is below the best size
// so far is skipped. ctl->key = max over seeds of size << 32 | ~seed.
__device__ __forceinline__ void mc_heu(const McProb& P, long long budget, uint64_t* mc_cand) {
  const uint64_t* __restrict__ G = P.G;
  const int64_t nw = P.nw;
  const int32_t* __restrict__ core = P.core;
  const int32_t* __restrict__ seeds = P.list;
  const int32_t nseeds = P.nlist;
  McCtl* ctl = P.ctl;
  const int lane = threadIdx.x;
  long long work = 0;
  while (work < budget) {
    int idx = 0;
    if (lane == 0) idx = atomicAdd(&ctl->head, 1);
    idx = __shfl(idx, 0, 64);
    if (idx >= nseeds) break;
    const int v = seeds[idx];
    const int best = static_cast<int>(mc_load_key(&ctl->key) >> 32);
    if (core[v] + 1 < best) continue;
    const int size = mc_greedy(G, nw, core, v, best, mc_cand, nullptr, work, lane);
    if (lane == 0)
      atomicMax(&ctl->key, (static_cast<unsigned long long>(size) << 32) | (0xFFFFFFFFu - static_cast<uint32_t>(v)));
  }
}

// the clique of one seed (thr = 0), written to out[0..size)
__device__ __forceinline__ void mc_heu_one(const McProb& P, uint64_t* mc_cand) {
  long long work = 0;
  mc_greedy(P.G, P.nw, P.core, P.seed, 0, mc_cand, P.out, work, threadIdx.x);
}

// ---- EXACT: bitset branch and bound, one wave per root ----------------------------------------------------------
// Root r (vertices ordered by (core, degree, index): pos[]) searches the cliques {r} + K, K inside
// P0 = N(r) & {pos > pos[r]} & {core >= heu}. A stack level L holds the candidate bitset P_L of the clique
// {r, path[0..L-1]} (c = L + 1 vertices). A step at level L colours P_L greedily (vertices in index order, each
// colour class an independent set; BBMC): k colours bound the clique by c + k. If the key (c + k, rk) does not beat
// the incumbent the level is popped; else the LAST vertex coloured, v, is branched on: v leaves P_L, P_{L+1} =
// P_L & N(v). An empty P_{L+1} is a maximal clique of c + 1 vertices, offered to the incumbent. A level is
// coloured again every time the search returns to it (the bound of what is left, and no per-level list to keep:
// the stack is one bitset per level).
// Tie rule: rk = 0xFFFFFFFE - pos[r]; a branch is cut only when (bound, rk) <= the incumbent key, so the first
// clique of the final size in the DFS order of the first root (in pos order) that holds one is always found.
// The incumbent starts at (heu, 0xFFFFFFFF): only cliques larger than HEU's are searched for.
// A slot (= workgroup) keeps its root, depth, path and stack between launches; recs[slot] holds the clique of the
// last key it raised. LDS: Q, R (the colouring's bitsets).
// `slot` is the slot's index among its problem's; mc_lds holds 2 nw words.
__device__ __forceinline__ void mc_exact(const McProb& P_, int slot, long long budget, uint64_t* mc_lds) {
  const uint64_t* __restrict__ G = P_.G;
  const int64_t nw = P_.nw;
  const int32_t* __restrict__ core = P_.core;
  const int32_t* __restrict__ pos = P_.pos;
  const int32_t* __restrict__ roots = P_.list;
  const int32_t nroots = P_.nlist, heu = P_.heu, D = P_.D;
  McCtl* ctl = P_.ctl;
  uint64_t* __restrict__ arena = P_.arena;
  int32_t* __restrict__ paths = P_.paths;
  int32_t* __restrict__ recs = P_.recs;
  uint64_t* Q = mc_lds;
  uint64_t* R = mc_lds + nw;
  const int lane = threadIdx.x;
  McSlot* sl = P_.slots + slot;
  uint64_t* stk = arena + static_cast<int64_t>(slot) * D * nw;
  int32_t* path = paths + static_cast<int64_t>(slot) * (D + 1);  // path[0] = root, path[1 + L] = branch of level L
  int root = sl->root, L = sl->depth;
  unsigned long long rk = root >= 0 ? 0xFFFFFFFEull - static_cast<unsigned>(pos[root]) : 0;
  long long work = 0;
  unsigned long long nodes = 0, searched = 0, pruned = 0;
  while (work < budget) {
    if (root < 0) {
      int idx = 0;
      if (lane == 0) idx = atomicAdd(&ctl->head, 1);
      idx = __shfl(idx, 0, 64);
      if (idx >= nroots) break;
      const int r = roots[idx];
      rk = 0xFFFFFFFEull - static_cast<unsigned>(pos[r]);
      unsigned long long inc = mc_load_key(&ctl->key);
      if (((static_cast<unsigned long long>(core[r] + 1) << 32) | rk) <= inc) {
        ++pruned;
        continue;
      }
      const int pr = pos[r];
      int cnt = 0;
      for (int64_t w = lane; w < nw; w += 64) {
        uint64_t bits = G[static_cast<int64_t>(r) * nw + w], keep = 0;
        while (bits) {
          const int b = __ffsll(static_cast<unsigned long long>(bits)) - 1;
          bits &= bits - 1;
          const int x = static_cast<int>(w * 64 + b);
          if (pos[x] > pr && core[x] >= heu) keep |= 1ull << b;
        }
        stk[w] = keep;
        cnt += __popcll(keep);
      }
      cnt = wave_sum(cnt);
      work += nw / 64 + 1;
      inc = mc_load_key(&ctl->key);
      if (((static_cast<unsigned long long>(cnt + 1) << 32) | rk) <= inc) {
        ++pruned;
        continue;
      }
      ++searched;
      root = r;
      L = 0;
      if (lane == 0) path[0] = r;
      __threadfence_block();
    }
    // ---- one step at level L: colour P_L (stk + L * nw) into Q / R
    uint64_t* P = stk + static_cast<int64_t>(L) * nw;
    int hi = 0;
    for (int64_t w = lane; w < nw; w += 64) {
      const uint64_t x = P[w];
      Q[w] = x;
      if (x) hi = static_cast<int>(w) + 1;
    }
    hi = wave_max(hi);
    __syncthreads();
    int ncol = 0, last = -1, qlo = 0;
    ++nodes;
    while (true) {
      const int f = mc_first_word(Q, qlo, hi, lane);
      if (f < 0) break;
      qlo = f;
      ++ncol;
      for (int w = f + lane; w < hi; w += 64) R[w] = Q[w];
      __syncthreads();
      int rlo = f;
      while (true) {
        const int f2 = mc_first_word(R, rlo, hi, lane);
        if (f2 < 0) break;
        rlo = f2;
        const uint64_t word = R[f2];
        const int b = __ffsll(static_cast<unsigned long long>(word)) - 1;
        const int v = f2 * 64 + b;
        last = v;
        __syncthreads();
        const uint64_t* gv = G + static_cast<int64_t>(v) * nw;
        for (int w = f2 + lane; w < hi; w += 64) {
          uint64_t rw = R[w] & ~gv[w];
          uint64_t qw = Q[w];
          if (w == f2) {
            rw &= ~(1ull << b);
            qw &= ~(1ull << b);
          }
          R[w] = rw;
          Q[w] = qw;
        }
        work += (hi - f2) / 64 + 1;
        __syncthreads();
      }
    }
    const unsigned long long inc = mc_load_key(&ctl->key);
    if (ncol == 0 || ((static_cast<unsigned long long>(L + 1 + ncol) << 32) | rk) <= inc) {
      if (L == 0) root = -1;
      else --L;
      continue;
    }
    // branch on `last`: it leaves P_L; P_{L+1} = P_L & N(last)
    const uint64_t* gv = G + static_cast<int64_t>(last) * nw;
    int cnt = 0;
    const bool room = L + 1 < D;
    for (int64_t w = lane; w < hi; w += 64) {
      uint64_t x = P[w];
      if (w == (last >> 6)) x &= ~(1ull << (last & 63));
      P[w] = x;
      const uint64_t y = x & gv[w];
      if (room) P[nw + w] = y;
      cnt += __popcll(y);
    }
    if (room)
      for (int64_t w = hi + lane; w < nw; w += 64) P[nw + w] = 0;
    cnt = wave_sum(cnt);
    if (lane == 0) path[1 + L] = last;
    __threadfence_block();
    if (cnt == 0) {
      const unsigned long long key = (static_cast<unsigned long long>(L + 2) << 32) | rk;
      if (lane == 0) {
        // only the slot that raised the key to this value writes it: the record with the final key is its clique
        if (atomicMax(&ctl->key, key) < key) {
          int32_t* rec = recs + static_cast<int64_t>(slot) * (D + 1);
          for (int i = 0; i < L + 2; ++i) rec[i] = path[i];
          sl->rec_key = key;
        }
      }
    } else if (!room) {
      if (lane == 0) atomicAdd(&ctl->overflow, 1);
      root = -1;  // (not reachable: a clique of more than K + 1 vertices)
    } else {
      ++L;
    }
  }
  if (lane == 0) {
    sl->root = root;
    sl->depth = L;
    if (root >= 0) atomicAdd(&ctl->active, 1);
    atomicAdd(&ctl->bb_nodes, nodes);
    atomicAdd(&ctl->roots_searched, searched);
    atomicAdd(&ctl->roots_pruned, pruned);
  }
}

// ---- the launches -----------------------------------------------------------------------------------------------------
// Every kernel fetches its problem's row of the descriptor table, so a lone call and a batch run the same code. In the
// adjacency and degree launches the grid's last dimension is the problem (strided when the call holds more problems
// than a grid dimension does) and x the slice or row, up to the call's largest count: a wave or thread past its
// problem's count has nothing to do. No workgroup waits for another (more workgroups than the chip holds is fine), no
// launch is cooperative, and the only words workgroups share are a problem's head, incumbent key and counters.

// A pointer read from a device table is a generic one to the compiler, and every access through it a FLAT
// instruction, which also waits on the LDS counter. All buffers of a call are global memory: the fetches below say
// so, and the bodies get the global loads, stores and atomics that pointers passed as kernel arguments get.
template <typename T>
__device__ __forceinline__ T* mc_global(T* const& field) {  // the table's field, read as a pointer to global memory
  return (T*)(*static_cast<CLIPPER_GLOBAL T* const*>(static_cast<const void*>(&field)));
}
__device__ __forceinline__ McProb mc_fetch(const McProb* __restrict__ probs, int i) {
  const McProb& t = probs[i];
  McProb P = t;
  P.G = mc_global(t.G);
  P.degw = mc_global(t.degw);
  P.core = mc_global(t.core);
  P.alive = mc_global(t.alive);
  P.pos = mc_global(t.pos);
  P.list = mc_global(t.list);
  P.out = mc_global(t.out);
  P.given = mc_global(t.given);
  P.ctl = mc_global(t.ctl);
  P.slots = mc_global(t.slots);
  P.arena = mc_global(t.arena);
  P.paths = mc_global(t.paths);
  P.recs = mc_global(t.recs);
  return P;
}
__device__ __forceinline__ McAdjSrc mc_fetch(const McAdjSrc* __restrict__ src, int i) {
  const McAdjSrc& t = src[i];
  McAdjSrc a = t;
  a.S = mc_global(t.S);
  a.G = mc_global(t.G);
  a.deg = mc_global(t.deg);
  return a;
}

// one wave per (slice, problem); G zeroed by the caller. A problem read from a dense store is k_mc_adj_dense's.
template <typename VT, int H>
__global__ __launch_bounds__(256) void k_mc_adj_slices(const McAdjSrc* __restrict__ src, int32_t nprob) {
  const int64_t s = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  for (int32_t p = blockIdx.y; p < nprob; p += gridDim.y) {
    const McAdjSrc a = mc_fetch(src, p);
    if (!a.S) mc_adj_slice<VT, H>(a.M, a.G, a.nw, a.m, s, threadIdx.x & 63);  // (s past its slices: returns)
  }
}

// one thread per (row, word, problem): y = the word, z = the problem (both strided when the grid is smaller)
template <typename T>
__global__ __launch_bounds__(256) void k_mc_adj_dense(const McAdjSrc* __restrict__ src, int32_t nprob) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  for (int32_t p = blockIdx.z; p < nprob; p += gridDim.z) {
    const McAdjSrc a = mc_fetch(src, p);
    if (!a.S || c >= a.m) continue;
    for (int64_t w = blockIdx.y; w < a.nw; w += gridDim.y)
      a.G[c * a.nw + w] = mc_adj_dense_word(static_cast<const T*>(a.S), a.ld, a.m, c, w);
  }
}

// one wave per (row, problem)
__global__ __launch_bounds__(256) void k_mc_degree(const McAdjSrc* __restrict__ src, int32_t nprob) {
  const int64_t v = static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  for (int32_t p = blockIdx.y; p < nprob; p += gridDim.y) {
    const McAdjSrc a = mc_fetch(src, p);
    if (v < a.m) mc_degree_row(a.G, a.nw, v, a.deg, threadIdx.x & 63);
  }
}

// one workgroup per unfinished problem (work[blockIdx.x]); dynamic LDS: the largest nw of the call, in words
__global__ __launch_bounds__(MC_PEEL_THREADS) void k_mc_core_peel(const McProb* __restrict__ probs,
                                                                  const int32_t* __restrict__ work, long long budget) {
  extern __shared__ uint64_t mc_alive[];
  __shared__ int32_t fr[MC_PEEL_FCAP];
  __shared__ int32_t sc[2];
  const McProb P = mc_fetch(probs, work[blockIdx.x]);
  mc_peel(P, budget, mc_alive, fr, sc);
}

// one wave per slot; a slot takes its problem's seeds through that problem's head
__global__ __launch_bounds__(64) void k_mc_heu(const McProb* __restrict__ probs, const McItem* __restrict__ slots,
                                               long long budget) {
  extern __shared__ uint64_t mc_cand[];
  const McProb P = mc_fetch(probs, slots[blockIdx.x].prob);
  if (mc_load_i32(&P.ctl->head) >= P.nlist) return;  // (its problem is finished)
  mc_heu(P, budget, mc_cand);
}

// one wave per problem of the work list: the clique of its winning seed
__global__ __launch_bounds__(64) void k_mc_heu_one(const McProb* __restrict__ probs, const int32_t* __restrict__ work) {
  extern __shared__ uint64_t mc_cand[];
  const McProb P = mc_fetch(probs, work[blockIdx.x]);
  mc_heu_one(P, mc_cand);
}

// one wave per seeded problem of the work list: its seed clique; dynamic LDS: two bitsets of the call's largest nw
__global__ __launch_bounds__(64) void k_mc_seed(const McProb* __restrict__ probs, const int32_t* __restrict__ work) {
  extern __shared__ uint64_t mc_lds[];
  const McProb P = mc_fetch(probs, work[blockIdx.x]);
  mc_seed_clique(P, mc_lds);
}

// one wave per slot, with the stack, path and record it keeps between launches
__global__ __launch_bounds__(64) void k_mc_exact(const McProb* __restrict__ probs, const McItem* __restrict__ slots,
                                                 long long budget) {
  extern __shared__ uint64_t mc_lds[];
  const McItem it = slots[blockIdx.x];
  const McProb P = mc_fetch(probs, it.prob);
  if (P.slots[it.idx].root < 0 && mc_load_i32(&P.ctl->head) >= P.nlist) return;  // (nothing left for this slot)
  mc_exact(P, it.idx, budget, mc_lds);
}

// one wave per problem of the work list whose incumbent beat HEU's clique: the record of the slot that raised the
// final key goes to out[0 .. omega), its length to out[-1] (-1: no slot holds it)
__global__ __launch_bounds__(64) void k_mc_collect(const McProb* __restrict__ probs, const int32_t* __restrict__ work) {
  const McProb P = mc_fetch(probs, work[blockIdx.x]);
  const int lane = threadIdx.x;
  const unsigned long long key = P.ctl->key;
  int who = -1;
  for (int j = lane; j < P.nslots; j += 64)
    if (P.slots[j].rec_key == key) who = j;
  who = wave_max(who);
  const int omega = static_cast<int>(key >> 32);
  if (who >= 0) {
    const int32_t* rec = P.recs + static_cast<int64_t>(who) * (P.D + 1);
    for (int i = lane; i < omega; i += 64) P.out[i] = rec[i];
  }
  if (lane == 0) P.out[-1] = who >= 0 ? omega : -1;
}

}  // namespace clipper_hip
