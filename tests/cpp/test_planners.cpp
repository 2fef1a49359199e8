// CPU test of the host planners (clipper_amd/csrc/host_plan.hpp): on random slice directories —
// sizes on and off the edges, empty slices, dense blocks whose chunks must be cut by step range —
// every plan must cover every step of every slice exactly once.
//   plan_pass      work list of the streaming pass: per strip, the chunks are covered once by whole-range
//                  items or by step-range items that partition [0, maxq); every (strip, slot < nslots) is
//                  written by exactly one item; the stored-entry count is the directory's
//   plan_resident  units cover every (column group, chunk) once, slots are numbered 0..n-1 per group, a
//                  unit's slices fit its LDS share by the planner's own bound, the pieces of a unit
//                  partition the steps of each of its slices among waves mapped to that column group
//   plan_view_resident  (at check_view_resident)
//   plan identity  the plans of a fixed set of directories, folded into one hash per planner, are what they were
//                  (at check_identity)
//   plan image     every plan the test produces, packed (plan_pack) and read back through PlanLayout's accessors
//                  (at check_image)
//   g++ -std=c++17 -O1 -I clipper_amd/csrc tests/cpp/test_planners.cpp -o /tmp/t && /tmp/t
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>

#include "host_plan.hpp"

using namespace clipper_plan;

#define REQUIRE(c)                                                         \
  do {                                                                     \
    if (!(c)) {                                                            \
      std::printf("FAILED %s at line %d (case %s)\n", #c, __LINE__, g_case); \
      std::exit(1);                                                        \
    }                                                                      \
  } while (0)
static char g_case[128];

static std::vector<uint32_t> directory(std::mt19937& rng, int ncg, int nchunks, double density, double dense_frac) {
  // column lengths binomial-ish around density * 128 per slice; the last dense_frac of the matrix is a dense block
  std::vector<uint32_t> L(static_cast<size_t>(ncg) * nchunks);
  std::binomial_distribution<int> bin(128, density);
  for (int cg = 0; cg < ncg; ++cg)
    for (int k = 0; k < nchunks; ++k) {
      const bool dense = cg >= ncg * (1 - dense_frac) && k * 2 >= nchunks * 2 * (1 - dense_frac);
      int maxlen = 0, entries = 0;
      for (int l = 0; l < 64; ++l) {
        const int n = dense ? 128 - (rng() % 3) : bin(rng);
        maxlen = std::max(maxlen, n);
        entries += n;
      }
      if (density == 0.0 && !dense) maxlen = entries = 0;
      L[static_cast<size_t>(cg) * nchunks + k] = static_cast<uint32_t>((maxlen + 3) / 4) | (static_cast<uint32_t>(entries) << 8);
    }
  return L;
}

static size_t check_pass(const std::vector<uint32_t>& L, int ncg, int nchunks, int cus, double target,
                         const PassConsts K = PassConsts{4, 16}) {
  PassPlan P;
  plan_pass(L.data(), ncg, nchunks, K, cus, target, 2.0, P);
  const int nstrips = (ncg + K.nw - 1) / K.nw;
  uint64_t entries = 0;
  for (uint32_t v : L) entries += v >> 8;
  REQUIRE(P.entries == entries);
  std::map<std::pair<int, int>, int> slot_seen;
  std::vector<std::vector<std::vector<std::pair<int, int>>>> cover(nstrips, std::vector<std::vector<std::pair<int, int>>>(nchunks));
  for (const Work& w : P.work) {
    REQUIRE(w.strip >= 0 && w.strip < nstrips && w.slot >= 0 && w.slot < P.nslots);
    const int times = ++slot_seen[std::make_pair(w.strip, w.slot)];
    REQUIRE(times == 1);
    REQUIRE(w.t0 >= 0 && w.t0 <= w.t1 && w.t1 <= nchunks);
    for (int k = w.t0; k < w.t1; ++k) cover[w.strip][k].push_back(std::make_pair(w.q0, w.q1));
    if (w.t0 == w.t1) continue;  // a filler: writes the zeros of a (strip, slot) nobody else fills
    if (w.q0 != 0 || w.q1 != (1 << 30)) REQUIRE(w.t1 - w.t0 == 1 && w.q0 < w.q1 && w.q0 % K.so == 0);
  }
  REQUIRE(static_cast<int>(slot_seen.size()) == nstrips * P.nslots);  // every (strip, slot) written once
  for (int st = 0; st < nstrips; ++st)
    for (int k = 0; k < nchunks; ++k) {
      int mq = 0;
      for (int w = 0; w < K.nw && st * K.nw + w < ncg; ++w)
        mq = std::max(mq, static_cast<int>(L[static_cast<size_t>(st * K.nw + w) * nchunks + k] & 255u));
      auto& c = cover[st][k];
      REQUIRE(!c.empty());
      if (c.size() == 1 && c[0].first == 0 && c[0].second == (1 << 30)) continue;  // one whole-range item
      std::sort(c.begin(), c.end());
      int at = 0;
      for (auto& pr : c) {
        REQUIRE(pr.first == at);
        at = pr.second;
      }
      REQUIRE(at == mq);  // the step ranges partition [0, maxq of the strip's chunk)
    }
  return P.work.size();
}

// The plan image (PlanLayout, plan_pack): every offset is a multiple of 16, the arrays follow one another without
// overlap, the bytes asked for cover the last piece and the 64-byte tail, and nothing behind them is written; a plan
// packed into the buffer reads back through the accessors: units, slots, piece counts, wave map, the pieces in use.
// ONE buffer for every plan of the run, never cleared: a context packs plan after plan into the buffer it has.
template <class U>
static void check_image(const std::vector<U>& units, const std::vector<uint8_t>& slots, const std::vector<uint8_t>& npieces,
                        const std::vector<uint8_t>& wave_cg, const std::vector<uint32_t>& pieces, size_t pmax) {
  static std::vector<uint8_t> buf;
  if (npieces.empty()) return;  // (a directory turned down before any piece was dealt: there is no plan to pack)
  REQUIRE(!units.empty() && npieces.size() % units.size() == 0);
  REQUIRE(wave_cg.size() == npieces.size() && pieces.size() == npieces.size() * pmax);
  const PlanLayout A = plan_layout(units.size(), slots.size(), npieces.size(), pmax);
  REQUIRE(A.off_slots % 16 == 0 && A.off_np % 16 == 0 && A.off_wc % 16 == 0 && A.off_pc % 16 == 0);
  REQUIRE(A.off_slots >= units.size() * sizeof(U) && A.off_np >= A.off_slots + slots.size());
  REQUIRE(A.off_wc >= A.off_np + npieces.size() && A.off_pc >= A.off_wc + wave_cg.size());
  REQUIRE(A.bytes >= A.off_pc + pieces.size() * sizeof(uint32_t) + 64);
  constexpr size_t GUARD = 64;
  if (buf.size() < A.bytes + GUARD) buf.resize(A.bytes + GUARD);
  std::memset(buf.data() + A.bytes, 0xA5, GUARD);
  plan_pack(A, buf.data(), units.data(), slots.data(), npieces.data(), wave_cg.data(), pieces.data());
  for (size_t g = 0; g < GUARD; ++g) REQUIRE(buf[A.bytes + g] == 0xA5);
  const uint8_t* base = buf.data();
  REQUIRE(units.empty() || std::memcmp(A.units<U>(base), units.data(), units.size() * sizeof(U)) == 0);
  REQUIRE(slots.empty() || std::memcmp(A.slots(base), slots.data(), slots.size()) == 0);
  REQUIRE(npieces.empty() || std::memcmp(A.npieces(base), npieces.data(), npieces.size()) == 0);
  REQUIRE(wave_cg.empty() || std::memcmp(A.wave_cg(base), wave_cg.data(), wave_cg.size()) == 0);
  for (size_t wv = 0; wv < npieces.size(); ++wv)
    for (size_t j = 0; j < npieces[wv]; ++j) REQUIRE(A.pieces(base)[wv * pmax + j] == pieces[wv * pmax + j]);
}
static void check_image(const ResidentPlan& P, const ResidentConsts& K) {
  check_image(P.units, P.nsl, P.npieces, P.wave_cg, P.pieces, static_cast<size_t>(K.pmax));
}
static void check_image(const ViewResidentPlan& P, const ResidentConsts& K) {
  check_image(P.units, std::vector<uint8_t>(), P.npieces, P.wave_cg, P.pieces, static_cast<size_t>(K.pmax));
}

static const ResidentConsts K_RESIDENT{512, 8, 64, 12, 4, 159u * 1024u, 2 * 8 * 16 * 8, 64 * 4 + 64, 2048, 16};
static const ResidentConsts K_VIEW{512, 8, 64, 12, 2, 159u * 1024u, 2 * 8 * 16 * 8 + 64 * 8, 64 * 8 + 64, 2048, 16};

static bool check_resident(const std::vector<uint32_t>& L, int ncg, int nchunks, int64_t m, int esize, int max_units) {
  const ResidentConsts& K = K_RESIDENT;
  const int64_t mp = (m + 63) / 64 * 64;
  ResidentPlan P;
  plan_resident(L.data(), ncg, nchunks, m, mp, esize, max_units, 0, K, P);
  check_image(P, K);
  if (!P.ok) return false;
  REQUIRE(P.V == 1 && (P.E == 1 || P.E == 2 || P.E == 4) && static_cast<int64_t>(P.E) * K.nt >= mp);
  REQUIRE(static_cast<int>(P.units.size()) <= std::max(max_units, 1));
  // units cover every (cg, chunk) once; slots 0..n-1 per column group
  std::vector<std::vector<int>> seen(ncg, std::vector<int>(nchunks, 0));
  std::vector<std::set<int>> slots(ncg);
  for (size_t ui = 0; ui < P.units.size(); ++ui) {
    const Unit& U = P.units[ui];
    REQUIRE(U.ncgs >= 1 && U.ncgs <= K.nwv && U.cg0 >= 0 && U.cg0 + U.ncgs <= ncg && U.k0 >= 0 && U.k0 < U.k1 && U.k1 <= nchunks);
    REQUIRE(U.ncgs * (U.k1 - U.k0) <= K.tmax);
    uint64_t bytes = 0;
    for (int c = 0; c < U.ncgs; ++c) {
      const bool fresh = slots[U.cg0 + c].insert(U.slot).second;
      REQUIRE(fresh);
      for (int k = U.k0; k < U.k1; ++k) {
        ++seen[U.cg0 + c][k];
        bytes += slice_bound(L[static_cast<size_t>(U.cg0 + c) * nchunks + k], 4u * esize, K.so);
      }
    }
    REQUIRE(bytes + K.slice_pad <= P.lds_slices);
    // pieces: per column group of the unit, the steps of each slice are dealt out exactly once, to waves of that group
    std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> steps;  // (cgl, kl) -> ranges
    std::vector<int> waves_of(U.ncgs, 0);
    for (int w = 0; w < K.nwv; ++w) {
      const size_t wv = ui * K.nwv + w;
      const int cgl = P.wave_cg[wv];
      if (cgl == 255) {
        REQUIRE(P.npieces[wv] == 0);
        continue;
      }
      REQUIRE(cgl < U.ncgs);
      ++waves_of[cgl];
      REQUIRE(P.npieces[wv] <= K.pmax);
      for (int j = 0; j < P.npieces[wv]; ++j) {
        const uint32_t pc = P.pieces[wv * K.pmax + j];
        const int kl = pc & 255, q0 = (pc >> 8) & 255, q1 = (pc >> 16) & 255;
        REQUIRE(kl < U.k1 - U.k0 && q0 < q1);
        steps[std::make_pair(cgl, kl)].push_back(std::make_pair(q0, q1));
      }
    }
    for (int c = 0; c < U.ncgs; ++c) {
      REQUIRE(waves_of[c] >= 1);
      for (int k = U.k0; k < U.k1; ++k) {
        const int mq = static_cast<int>(L[static_cast<size_t>(U.cg0 + c) * nchunks + k] & 255u);
        auto it = steps.find(std::make_pair(c, k - U.k0));
        if (mq == 0) {
          REQUIRE(it == steps.end());
          continue;
        }
        REQUIRE(it != steps.end());
        std::sort(it->second.begin(), it->second.end());
        int at = 0;
        for (auto& pr : it->second) {
          REQUIRE(pr.first == at);
          at = pr.second;
        }
        REQUIRE(at == mq);
      }
    }
  }
  for (int cg = 0; cg < ncg; ++cg) {
    REQUIRE(static_cast<int>(slots[cg].size()) == P.nsl[cg] && P.nsl[cg] <= P.maxslots);
    REQUIRE(*slots[cg].begin() == 0 && *slots[cg].rbegin() == P.nsl[cg] - 1);
    for (int k = 0; k < nchunks; ++k) REQUIRE(seen[cg][k] == 1);
  }
  return true;
}

// plan_view_resident: the units partition every (column group, lane) — a group whole in one unit, or split
// into lane ranges that tile [0, 64) — and hold ALL chunks of their groups; a unit fits its LDS share by the
// planner's own bound (lane subsets: their share of the quads + every step's padding); the pieces of a unit
// partition the steps of each of its slices among waves mapped to that column group.
static bool check_view_resident(const std::vector<uint32_t>& L, int ncg, int nchunks, int esize, int target, int max_units,
                                uint32_t fixed) {
  const ResidentConsts& K = K_VIEW;
  ViewResidentPlan P;
  plan_view_resident(L.data(), ncg, nchunks, esize, target, max_units, fixed, K, P);
  check_image(P, K);
  if (!P.ok) return false;
  REQUIRE(static_cast<int>(P.units.size()) <= max_units && !P.units.empty());
  std::vector<std::vector<int>> lanes(ncg, std::vector<int>(64, 0));
  uint64_t entries = 0;
  for (uint32_t v : L) entries += v >> 8;
  REQUIRE(P.entries == entries);
  for (size_t ui = 0; ui < P.units.size(); ++ui) {
    const ViewUnit& U = P.units[ui];
    REQUIRE(U.ncgs >= 1 && U.ncgs <= K.nwv && U.cg0 >= 0 && U.cg0 + U.ncgs <= ncg);
    REQUIRE(U.l0 >= 0 && U.l0 < U.l1 && U.l1 <= 64);
    REQUIRE(U.ncgs == 1 || (U.l0 == 0 && U.l1 == 64));
    REQUIRE(U.ncgs * nchunks <= K.tmax);
    // a lane part is a PACKED unit: G = 64 / width chunks side by side per slice
    const int G = U.pack > 1 ? U.pack : 1;
    REQUIRE((U.l0 == 0 && U.l1 == 64) ? U.pack == 0 : (U.pack >= 2 && U.pack <= 8 && (U.l1 - U.l0) * U.pack == 64 && U.l0 % (U.l1 - U.l0) == 0));
    const int nsl = (nchunks + G - 1) / G;
    auto steps_of = [&](int c, int sidx) {
      int mq = 0;
      for (int g = 0; g < G && sidx * G + g < nchunks; ++g)
        mq = std::max(mq, static_cast<int>(L[static_cast<size_t>(U.cg0 + c) * nchunks + sidx * G + g] & 255u));
      return mq;
    };
    uint64_t bytes = 0;
    for (int c = 0; c < U.ncgs; ++c) {
      for (int l = U.l0; l < U.l1; ++l) ++lanes[U.cg0 + c][l];
      for (int k = 0; k < nchunks; ++k) {
        const uint32_t lq = L[static_cast<size_t>(U.cg0 + c) * nchunks + k];
        const uint64_t full = slice_bound(lq, 4u * esize, K.so);
        bytes += (U.l0 == 0 && U.l1 == 64) ? full : full * (U.l1 - U.l0) / 64 + 16 + 64 + 64 * 16;
      }
    }
    REQUIRE(bytes + K.slice_pad <= P.lds_slices + 8192);  // (the kernel checks the real sizes; the plan must be close)
    std::map<std::pair<int, int>, std::vector<std::pair<int, int>>> steps;
    std::vector<int> waves_of(U.ncgs, 0);
    for (int w = 0; w < K.nwv; ++w) {
      const size_t wv = ui * K.nwv + w;
      const int cgl = P.wave_cg[wv];
      if (cgl == 255) {
        REQUIRE(P.npieces[wv] == 0);
        continue;
      }
      REQUIRE(cgl < U.ncgs);
      ++waves_of[cgl];
      REQUIRE(P.npieces[wv] <= K.pmax);
      for (int j = 0; j < P.npieces[wv]; ++j) {
        const uint32_t pc = P.pieces[wv * K.pmax + j];
        const int kl = pc & 255, q0 = (pc >> 8) & 255, q1 = (pc >> 16) & 255;
        REQUIRE(kl < nsl && q0 < q1);
        steps[std::make_pair(cgl, kl)].push_back(std::make_pair(q0, q1));
      }
    }
    for (int c = 0; c < U.ncgs; ++c) {
      REQUIRE(waves_of[c] >= 1);
      for (int k = 0; k < nsl; ++k) {
        const int mq = steps_of(c, k);
        auto it = steps.find(std::make_pair(c, k));
        if (mq == 0) {
          REQUIRE(it == steps.end());
          continue;
        }
        REQUIRE(it != steps.end());
        std::sort(it->second.begin(), it->second.end());
        int at = 0;
        for (auto& pr : it->second) {
          REQUIRE(pr.first == at);
          at = pr.second;
        }
        REQUIRE(at == mq);
      }
    }
  }
  for (int cg = 0; cg < ncg; ++cg)
    for (int l = 0; l < 64; ++l) REQUIRE(lanes[cg][l] == 1);
  return true;
}

// ---- plan identity: the plans are, bit for bit, what they were ---------------------------------------------------------
// Every plan of a fixed set of directories is folded into one 64-bit FNV-1a value per planner and compared with a
// constant. The constants were printed by THIS code compiled against host_plan.hpp as it stood before the piece
// dealer was stated once (deal_pieces) — the commit before the one that added this check. They are never to be
// regenerated from the header under test: a change that moves them changes the association of every sum of the
// resident solvers, and has to say so.
// The directories come from raw std::mt19937 output (its sequence is fixed by the standard) and integer arithmetic only:
// std::binomial_distribution, which directory() uses, is not specified bit for bit across standard libraries.
struct Fnv {
  uint64_t h = 14695981039346656037ull;
  void bytes(const void* p, size_t n) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
  }
  template <class T>
  void value(T v) { bytes(&v, sizeof(v)); }
  template <class T>
  void array(const std::vector<T>& v) {
    value<uint64_t>(v.size());
    if (!v.empty()) bytes(v.data(), v.size() * sizeof(T));
  }
  // unit records, piece counts, wave map and the pieces in use
  template <class U>
  void tables(const std::vector<U>& units, const std::vector<uint8_t>& npieces, const std::vector<uint8_t>& wave_cg,
              const std::vector<uint32_t>& pieces, size_t pmax) {
    array(units);
    array(npieces);
    array(wave_cg);
    for (size_t wv = 0; wv < npieces.size() && (wv + 1) * pmax <= pieces.size(); ++wv)
      for (size_t j = 0; j < npieces[wv]; ++j) value<uint32_t>(pieces[wv * pmax + j]);
  }
};

// column lengths uniform in [0, 2 * mean] (mean <= 64); the slices of the last dense_cgs column groups from chunk
// dense_k0 on are a dense block (lengths 126 .. 128)
static std::vector<uint32_t> directory_raw(std::mt19937& rng, int ncg, int nchunks, uint32_t mean, int dense_cgs, int dense_k0) {
  std::vector<uint32_t> L(static_cast<size_t>(ncg) * nchunks);
  for (int cg = 0; cg < ncg; ++cg)
    for (int k = 0; k < nchunks; ++k) {
      const bool dense = cg >= ncg - dense_cgs && k >= dense_k0;
      uint32_t maxlen = 0, entries = 0;
      for (int l = 0; l < 64; ++l) {
        const uint32_t r = static_cast<uint32_t>(rng());
        const uint32_t n = dense ? 128u - r % 3u : r % (2u * mean + 1u);
        maxlen = std::max(maxlen, n);
        entries += n;
      }
      L[static_cast<size_t>(cg) * nchunks + k] = (maxlen + 3u) / 4u | (entries << 8);
    }
  return L;
}

static void check_identity() {
  std::mt19937 rng(950);
  Fnv res, view;
  int nres = 0, nres_ok = 0, nview = 0, nview_ok = 0;
  // resident plans: one unit (m <= 512 where the slices fit), the edge (512, 513), many units (up to 2048), both value sizes
  for (int m : {1, 64, 65, 300, 512, 513, 1000, 1500, 2047, 2048})
    for (uint32_t mean : {0u, 1u, 7u, 26u, 64u})
      for (int dense : {0, 1, 2}) {
        const int ncg = (m + 63) / 64, nchunks = (m + 127) / 128;
        const int dense_cgs = dense == 0 ? 0 : (dense == 1 ? std::max(1, ncg / 20) : (ncg + 1) / 2);
        const int dense_k0 = dense == 0 ? nchunks : (dense == 1 ? nchunks - std::max(1, nchunks / 20) : nchunks / 2);
        std::snprintf(g_case, sizeof(g_case), "identity m=%d mean=%u dense=%d", m, mean, dense);
        const auto L = directory_raw(rng, ncg, nchunks, mean, dense_cgs, dense_k0);
        for (int esize : {4, 8})
          for (int max_units : {64, 200}) {
            ResidentPlan P;
            plan_resident(L.data(), ncg, nchunks, m, (m + 63) / 64 * 64, esize, max_units, 0, K_RESIDENT, P);
            res.value<uint8_t>(P.ok ? 1 : 0);
            res.value<int32_t>(P.V);
            res.value<int32_t>(P.E);
            res.value<int32_t>(P.maxslots);
            res.value<uint32_t>(P.lds_slices);
            res.value<uint64_t>(P.total_bound);
            res.array(P.nsl);
            res.tables(P.units, P.npieces, P.wave_cg, P.pieces, static_cast<size_t>(K_RESIDENT.pmax));
            check_image(P, K_RESIDENT);
            ++nres;
            nres_ok += P.ok ? 1 : 0;
          }
      }
  // views of up to 1024 rows over thousands of columns, a dense inlier block in the last column groups
  auto plan_view = [&](const std::vector<uint32_t>& L, int ncg, int nchunks, int esize, int target) {
    const uint32_t fixed = std::max<uint32_t>(nchunks * 128 * 6 * 8, 8 * 7 * 64 * 8) + K_VIEW.red_bytes + K_VIEW.tab_bytes;
    ViewResidentPlan P;
    plan_view_resident(L.data(), ncg, nchunks, esize, target, 248, fixed, K_VIEW, P);
    view.value<uint8_t>(P.ok ? 1 : 0);
    view.value<uint32_t>(P.lds_slices);
    view.value<uint64_t>(P.entries);
    view.tables(P.units, P.npieces, P.wave_cg, P.pieces, static_cast<size_t>(K_VIEW.pmax));
    check_image(P, K_VIEW);
    ++nview;
    nview_ok += P.ok ? 1 : 0;
  };
  for (int ncg : {47, 79, 157, 196, 235})
    for (int nchunks : {1, 3, 5, 8})
      for (uint32_t mean : {1u, 10u, 32u}) {
        std::snprintf(g_case, sizeof(g_case), "identity view ncg=%d nchunks=%d mean=%u", ncg, nchunks, mean);
        const auto L = directory_raw(rng, ncg, nchunks, mean, std::max(1, ncg / 18), 0);
        for (int esize : {4, 8})
          for (int target : {40, 96, 170, 248}) plan_view(L, ncg, nchunks, esize, target);
      }
  std::snprintf(g_case, sizeof(g_case), "identity");
  std::printf("plan identity: resident %d plans (%d fit) 0x%016llxull, view %d plans (%d fit) 0x%016llxull\n", nres, nres_ok,
              static_cast<unsigned long long>(res.h), nview, nview_ok, static_cast<unsigned long long>(view.h));
  REQUIRE(nres >= 200 && nview >= 200 && 4 * nres_ok > nres && 2 * nview_ok > nview);
  REQUIRE(res.h == 0x1f15f6987c9eb4e7ull);
  REQUIRE(view.h == 0x94512d42459c111cull);
}

// A context that solves problems of changing size packs a large plan, then a small one, into the same buffer (check_image
// keeps one): the small one reads back right over what the large one left.
static void check_image_reuse() {
  std::mt19937 rng(951);
  std::snprintf(g_case, sizeof(g_case), "image reuse");
  ResidentPlan big, small;
  const auto Lb = directory_raw(rng, 32, 16, 7, 2, 8), Ls = directory_raw(rng, 2, 1, 7, 0, 1);
  plan_resident(Lb.data(), 32, 16, 2048, 2048, 4, 200, 0, K_RESIDENT, big);
  plan_resident(Ls.data(), 2, 1, 100, 128, 4, 200, 0, K_RESIDENT, small);
  REQUIRE(big.ok && small.ok && big.units.size() >= 32 && small.units.size() == 1);
  check_image(big, K_RESIDENT);
  check_image(small, K_RESIDENT);
}

int main() {
  check_identity();
  check_image_reuse();
  std::mt19937 rng(20260926);
  int npass = 0, nres = 0, nres_ok = 0;
  const int64_t sizes[] = {1, 2, 63, 64, 65, 100, 129, 300, 511, 512, 513, 777, 1000, 1500, 2047, 2048, 2500, 4000, 10000, 30000};
  for (int64_t m : sizes)
    for (double density : {0.0, 0.01, 0.11, 0.4, 1.0})
      for (double dense_frac : {0.0, 0.05, 0.5}) {
        const int ncg = static_cast<int>((m + 63) / 64), nchunks = static_cast<int>((m + 127) / 128);
        std::snprintf(g_case, sizeof(g_case), "m=%lld density=%.2f dense=%.2f", static_cast<long long>(m), density, dense_frac);
        const auto L = directory(rng, ncg, nchunks, density, dense_frac);
        for (double target : {0.0, 64.0, 1024.0, 5000.0}) {
          check_pass(L, ncg, nchunks, 256, target);
          ++npass;
        }
        if (m <= 4096)
          for (int esize : {4, 8})
            for (int max_units : {64, 200}) {
              ++nres;
              nres_ok += check_resident(L, ncg, nchunks, m, esize, max_units) ? 1 : 0;
            }
      }
  // large matrices and their row views: whole rounds of the workgroups the chip holds (6 per CU)
  for (int nchunks : {782, 41}) {
    std::snprintf(g_case, sizeof(g_case), "m=100000 nchunks=%d", nchunks);
    const auto L = directory(rng, 1563, nchunks, 0.11, 0.05);
    for (int per_strip : {12, 8}) {
      const size_t nw = check_pass(L, 1563, nchunks, 256, 0.0, PassConsts{4, 16, 6, per_strip});
      ++npass;
      REQUIRE(nw >= 1536 && nw <= 8 * 1536 + 391 * 40);  // (+ the fillers of strips with fewer items than the fullest)
    }
  }
  // row views of a few hundred rows over thousands of columns (the headline: 524 rows x 10 000 columns, a dense
  // inlier block in the last column groups): complete columns per unit, dense groups split by lanes
  int nview = 0, nview_ok = 0;
  for (int ncg : {47, 79, 157, 235})
    for (int nchunks : {1, 3, 5, 8})
      for (double density : {0.02, 0.16, 0.5})
        for (int esize : {4, 8})
          for (int target : {40, 96, 170, 248}) {
            std::snprintf(g_case, sizeof(g_case), "view ncg=%d nchunks=%d density=%.2f esize=%d target=%d", ncg, nchunks, density, esize, target);
            auto L = directory(rng, ncg, nchunks, density, 0.0);
            for (int cg = ncg - std::max(1, ncg / 18); cg < ncg; ++cg)  // the inlier block: every row of the view is stored
              for (int k = 0; k < nchunks; ++k) L[static_cast<size_t>(cg) * nchunks + k] = 32u | (uint32_t(128 * 64) << 8);
            const uint32_t fixed = std::max<uint32_t>(nchunks * 128 * 6 * 8, 8 * 7 * 64 * 8) + (2 * 8 * 16 * 8 + 64 * 8) + (64 * 8 + 64);
            ++nview;
            nview_ok += check_view_resident(L, ncg, nchunks, esize, target, 248, fixed) ? 1 : 0;
          }
  // a view with more column groups than the chip has places for units of one group each (600 rows x 12 500 columns:
  // 196 groups, ten of them dense): the planner packs more entries per unit until the units fit
  for (int ncg : {196, 223})
    for (int esize : {4, 8}) {
      std::snprintf(g_case, sizeof(g_case), "wide view ncg=%d esize=%d", ncg, esize);
      auto L = directory(rng, ncg, 6, 0.16, 0.0);
      for (int cg = ncg - 10; cg < ncg; ++cg)
        for (int k = 0; k < 6; ++k) L[static_cast<size_t>(cg) * 6 + k] = 32u | (uint32_t(128 * 64) << 8);
      const uint32_t fixed = 6 * 128 * 6 * 8 + (2 * 8 * 16 * 8 + 64 * 8) + (64 * 8 + 64);
      ++nview;
      const bool ok = check_view_resident(L, ncg, 6, esize, 170, 248, fixed);
      nview_ok += ok ? 1 : 0;
      REQUIRE(ok || esize == 8);
    }
  REQUIRE(nview_ok > nview / 2);
  REQUIRE(nres_ok > nres / 4);  // (the small and the sparse ones fit)
  std::printf("view-resident plans: %d (%d fit the chip)\n", nview, nview_ok);
  std::printf("planners ok: %d pass plans, %d resident plans (%d fit the chip)\n", npass, nres, nres_ok);
  return 0;
}
