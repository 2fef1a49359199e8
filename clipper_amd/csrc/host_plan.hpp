// host_plan.hpp — the planners that run on the host between a build and its first pass, as pure
// functions of the slice directory (no HIP, no context): plan_pass (the work list of the streaming
// pass on the slices), plan_resident and plan_view_resident (units, pieces and wave map of the resident solver, on M
// and on a row view; deal_pieces is what the two share), and the plan image (PlanLayout, plan_pack): how either
// resident plan lies in the memory its kernel reads. Included by clipper_hip.hip and by tests/cpp/test_planners.cpp,
// which checks on the CPU that every plan covers every step of every slice exactly once, that the plans are what
// they were, and that an image reads back as it was packed.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace clipper_plan {

// what the streaming pass's workgroup does: layout of clipper_hip::SliceWork (k_slices.hip.h)
struct Work {
  int strip, slot, t0, t1;
  int q0, q1, pad0, pad1;
};

struct PassConsts {
  int nw;   // column groups (waves) per workgroup     SL_NW
  int so;   // steps between two recorded step offsets  SL_SO
  int occ = 6;        // workgroups per CU the pass kernel is compiled for  SL_OCC
  int per_strip = 12; // work items per strip a large matrix is cut into (12: M itself, 8: a row view)
};

struct PassPlan {
  std::vector<Work> work;  // most expensive first
  int nslots = 1;          // partial-sum slots per column the tail adds
  uint64_t entries = 0;    // stored entries of the matrix
};

// L[cg * nchunks + k] = maxq | entries << 8 of slice (cg, k). target <= 0: the default number of
// workgroups — four per CU; for small matrices a quarter of the slices (fewer partial-sum slots for
// the tail to add) and exactly one per CU when that is close (a second short workgroup on a few CUs
// doubles those CUs' time): profiles/r02e_window_sweep.txt. LARGE matrices (round 3,
// profiles/r03_wgs_sweep.txt) get whole ROUNDS of the workgroups the chip holds at once (occ per CU):
// about per_strip items per strip — 1024 workgroups left a third of the 1536 places empty and every
// CU's last item uneven; with 3 - 8 rounds the dispatcher evens the items out: m = 100k 1.83 -> 1.57 ms
// per pass on M, 300k 16.8 -> 13.8 ms, at 8 - 16 partial-sum slots per strip for the tail.
inline void plan_pass(const uint32_t* L, int ncg, int nchunks, const PassConsts& K, int cus, double target,
                      double C0 /* cost of a chunk besides its steps, in steps */, PassPlan& out) {
  const int nstrips = (ncg + K.nw - 1) / K.nw;
  if (target <= 0.0) {
    const double quarter = static_cast<double>(ncg) * nchunks / 4.0;
    target = quarter < 1.5 * cus ? cus : std::min<double>(quarter, 4.0 * cus);
    const double places = static_cast<double>(K.occ) * cus;  // workgroups the chip holds at once
    const double want = static_cast<double>(K.per_strip) * nstrips;
    if (want >= 0.8 * places && quarter >= places)
      target = places * std::min(8.0, std::max(1.0, std::floor(want / places + 0.5)));
  }
  // (this runs between the fill and the first pass of every build: buffers are kept, the order is a
  // counting sort)
  // What a chunk of a strip costs: the longest of its waves' chains of lock-step steps. (Blending in the entries
  // the slices hold — the bytes view — was measured worse at every weight: profiles/r03_plan_cost_model.txt.)
  constexpr double entry_weight = 0.0;
  static thread_local std::vector<int> cost;
  static thread_local std::vector<double> bcost;
  static thread_local std::vector<Work> items;
  static thread_local std::vector<double> key;
  static thread_local std::vector<int> nslot_of;
  cost.resize(static_cast<size_t>(nstrips) * nchunks);
  bcost.assign(static_cast<size_t>(nstrips) * nchunks, 0.0);
  double total = 0.0;
  uint64_t entries = 0;
  for (int st = 0; st < nstrips; ++st) {
    int* crow = cost.data() + static_cast<size_t>(st) * nchunks;
    const int w1 = std::min(K.nw, ncg - st * K.nw);
    for (int k = 0; k < nchunks; ++k) crow[k] = 0;
    for (int w = 0; w < w1; ++w) {
      const uint32_t* lrow = L + static_cast<size_t>(st * K.nw + w) * nchunks;
      for (int k = 0; k < nchunks; ++k) {
        const uint32_t v = lrow[k];
        crow[k] = std::max(crow[k], static_cast<int>(v & 255u));
        entries += v >> 8;
        bcost[static_cast<size_t>(st) * nchunks + k] += static_cast<double>(v >> 8);
      }
    }
    for (int k = 0; k < nchunks; ++k) {
      double& b = bcost[static_cast<size_t>(st) * nchunks + k];
      b = (1.0 - entry_weight) * crow[k] + entry_weight * (b / (256.0 * w1) * 2.0);  // the chunk's blended cost
      total += b + C0;
    }
  }
  out.entries = entries;
  const double T = std::max(8.0, total / target);
  auto push = [&](double c, const Work& w) {
    items.push_back(w);
    key.push_back(c);
  };
  items.clear();
  key.clear();
  nslot_of.assign(static_cast<size_t>(nstrips), 0);
  int nslots = 1;
  for (int st = 0; st < nstrips; ++st) {
    int slot = 0, start = 0;
    double acc = 0.0;
    auto flush = [&](int end) {
      if (end > start) push(acc, Work{st, slot++, start, end, 0, 1 << 30, 0, 0});
      start = end;
      acc = 0.0;
    };
    const int* crow = cost.data() + static_cast<size_t>(st) * nchunks;
    const double* brow = bcost.data() + static_cast<size_t>(st) * nchunks;
    for (int k = 0; k < nchunks; ++k) {
      const int mq = crow[k];
      const double c = brow[k] + C0;
      if (c > 1.5 * T && mq >= 2 * K.so) {
        // a dense block's chunk: a chain of steps several times the average — cut by step range
        flush(k);
        const int parts = std::min(static_cast<int>(std::ceil(c / T)), (mq + K.so - 1) / K.so);
        const int per = ((mq + parts - 1) / parts + K.so - 1) / K.so * K.so;
        for (int q0 = 0; q0 < mq; q0 += per)
          push(std::min(per, mq - q0) + C0, Work{st, slot++, k, k + 1, q0, std::min(q0 + per, mq), 0, 0});
        start = k + 1;
      } else {
        acc += c;
        if (acc >= T) flush(k + 1);
      }
    }
    flush(nchunks);
    nslot_of[static_cast<size_t>(st)] = slot;
    nslots = std::max(nslots, slot);
  }
  for (int st = 0; st < nstrips; ++st)  // every (strip, slot) is written by some workgroup
    for (int slot = nslot_of[static_cast<size_t>(st)]; slot < nslots; ++slot)
      push(0.0, Work{st, slot, 0, 0, 0, 0, 0, 0});
  out.nslots = nslots;
  // most expensive first, stable: counting sort by the cost relative to the most expensive item
  constexpr int KEYS = 1024;
  const size_t nw = items.size();
  out.work.resize(nw);
  double cmax = 1e-9;
  for (size_t i = 0; i < nw; ++i) cmax = std::max(cmax, key[i]);
  const double scale = (KEYS - 1) / cmax;
  int count[KEYS + 1] = {0};
  for (size_t i = 0; i < nw; ++i) ++count[KEYS - 1 - static_cast<int>(key[i] * scale)];
  int run = 0;
  for (int b = 0; b < KEYS; ++b) {
    const int c = count[b];
    count[b] = run;
    run += c;
  }
  for (size_t i = 0; i < nw; ++i) out.work[static_cast<size_t>(count[KEYS - 1 - static_cast<int>(key[i] * scale)]++)] = items[i];
}

// ---- the resident solver (k_resident.hip.h) -----------------------------------------------------

struct Unit {  // layout of clipper_hip::ResidentUnit
  int cg0, ncgs;  // column groups [cg0, cg0 + ncgs)
  int k0, k1;     // chunks [k0, k1)
  int slot;       // which of the partial-sum slots of its columns this unit fills
  int pad0, pad1, pad2;
};

struct ResidentConsts {
  int nt;              // threads per workgroup                         RS_NT
  int nwv;             // waves per workgroup                           RS_NWV
  int tmax;            // slices a unit holds at most                   RS_TMAX
  int pmax;            // pieces a wave works on at most                RS_PMAX
  int maxe;            // elements per thread at most                   RS_MAXE
  uint32_t lds_max;    // dynamic LDS of a workgroup                    RS_LDS_MAX
  uint32_t red_bytes, tab_bytes, slice_pad;  //                         RS_RED_BYTES, RS_TAB_BYTES, RS_SLICE_PAD
  int so;              //                                               SL_SO
};

constexpr uint32_t so_bytes(int maxq, int so) { return static_cast<uint32_t>(((maxq + so - 1) / so * 4 + 15) & ~15); }
inline uint32_t xt_bytes(int V, int64_t mp, int nwv) {
  const uint32_t xt = static_cast<uint32_t>(mp) * V * 8u, sc = static_cast<uint32_t>(nwv) * (V + 1) * 64u * 8u;
  return xt > sc ? xt : sc;
}
// upper bound of the bytes of a slice from its directory word (maxq | entries << 8)
inline uint32_t slice_bound(uint32_t lq, uint32_t quad_bytes, int so) {
  const uint32_t maxq = lq & 255u, entries = lq >> 8;
  if (maxq == 0) return 16 + 64 + so_bytes(0, so);
  const uint32_t nquads = std::min<uint32_t>((entries + 3u * 64u) / 4u, 64u * maxq);
  return 16 + 64 + so_bytes(static_cast<int>(maxq), so) + nquads * (quad_bytes + 4u) + maxq * 12u;
}

// The pieces of unit `ui`, which holds `nsl` slices of each of its `ncgs` column groups, slice s of group cgl being
// a chain of steps_of(cgl, s) lock-step steps: waves to column groups in proportion to their steps (every group at
// least one), then the steps of a group's slices dealt out to its waves in equal shares (the dense slices of an
// inlier block are chains ten times as long as the others: cut, they end together). Writes the unit's part of
// wave_cg, npieces and pieces = slice | q0 << 8 | q1 << 16; T and nw are scratch. False: the last wave of a group
// would need more than K.pmax pieces — the plan does not fit the piece lists.
template <class StepsOf>
inline bool deal_pieces(size_t ui, int ncgs, int nsl, const ResidentConsts& K, StepsOf steps_of, std::vector<int>& T,
                        std::vector<int>& nw, std::vector<uint8_t>& npieces, std::vector<uint8_t>& wave_cg,
                        std::vector<uint32_t>& pieces) {
  const size_t NWV = static_cast<size_t>(K.nwv), PM = static_cast<size_t>(K.pmax);
  T.assign(NWV, 0);
  nw.assign(NWV, 0);
  for (int cgl = 0; cgl < ncgs; ++cgl) {
    for (int s = 0; s < nsl; ++s) T[cgl] += steps_of(cgl, s);
    nw[cgl] = 1;
  }
  for (int spare = K.nwv - ncgs; spare > 0; --spare) {
    int best = 0;
    for (int cgl = 1; cgl < ncgs; ++cgl)
      if (static_cast<int64_t>(T[cgl]) * nw[best] > static_cast<int64_t>(T[best]) * nw[cgl]) best = cgl;
    ++nw[best];
  }
  int wave = 0;
  for (int cgl = 0; cgl < ncgs; ++cgl) {
    const int nwc = nw[cgl];
    const int target = std::max(1, (T[cgl] + nwc - 1) / nwc);
    int scur = 0, qcur = 0;
    for (int sub = 0; sub < nwc; ++sub, ++wave) {
      const size_t wv = ui * NWV + static_cast<size_t>(wave);
      wave_cg[wv] = static_cast<uint8_t>(cgl);
      int rem = (sub == nwc - 1) ? (1 << 30) : target, n = 0;
      while (rem > 0 && scur < nsl) {
        const int mq = steps_of(cgl, scur);
        if (qcur >= mq) {
          ++scur;
          qcur = 0;
          continue;
        }
        if (n == K.pmax) {
          if (sub == nwc - 1) return false;
          break;
        }
        const int take = std::min(rem, mq - qcur);
        pieces[wv * PM + static_cast<size_t>(n++)] = static_cast<uint32_t>(scur) | (static_cast<uint32_t>(qcur) << 8) |
                                                     (static_cast<uint32_t>(qcur + take) << 16);
        qcur += take;
        rem -= take;
      }
      npieces[wv] = static_cast<uint8_t>(n);
    }
  }
  return true;
}

struct ResidentPlan {
  bool ok = false;
  int V = 0, E = 0, maxslots = 1;
  uint32_t lds_slices = 0;
  uint64_t total_bound = 0;
  std::vector<Unit> units;
  std::vector<uint8_t> nsl;       // [ncg] slots to add for a column of the group
  std::vector<uint8_t> npieces;   // [unit * nwv + wave]
  std::vector<uint8_t> wave_cg;   // [unit * nwv + wave] column group of the unit the wave works for (255: none)
  std::vector<uint32_t> pieces;   // [(unit * nwv + wave) * pmax + j] = chunk - k0 | q0 << 8 | q1 << 16
};

// Decides whether the slices fit the resident solver and lays out its units: a column group x a range
// of chunks sized by slice_bound() so that a unit fits the LDS beside the x table; one unit when
// everything fits one workgroup. Then the pieces of every unit (deal_pieces).
inline void plan_resident(const uint32_t* L, int ncg, int nchunks, int64_t m, int64_t mp, int esize,
                          int max_units, int v_forced, const ResidentConsts& K, ResidentPlan& out) {
  out = ResidentPlan{};
  if (m > static_cast<int64_t>(K.maxe) * K.nt || mp > static_cast<int64_t>(K.maxe) * K.nt) return;  // above: the streaming launches win
  const int E = (mp <= K.nt) ? 1 : (mp <= 2 * K.nt ? 2 : 4);
  const uint32_t QBY = 4u * static_cast<uint32_t>(esize);
  std::vector<uint32_t> ub(static_cast<size_t>(ncg) * nchunks);
  uint64_t total = 0;
  for (size_t i = 0; i < ub.size(); ++i) {
    ub[i] = slice_bound(L[i], QBY, K.so);
    total += ub[i];
  }
  out.total_bound = total;
  int vmax = 1;  // at these sizes the line search rarely rejects: a window only adds arithmetic
  if (v_forced) vmax = v_forced;
  std::vector<Unit>& units = out.units;
  out.nsl.assign(static_cast<size_t>(ncg), 0);
  int V = 0;
  for (int v = vmax; v >= 1; v = (v_forced ? 0 : v / 2)) {
    units.clear();
    const uint32_t fixed = xt_bytes(v, mp, K.nwv) + K.red_bytes + K.tab_bytes;
    // everything in ONE workgroup: no exchange at all
    if (ncg <= K.nwv) {
      const uint32_t fixed1 = fixed + static_cast<uint32_t>(mp) * (v + 1) * 8u;
      if (fixed1 + K.slice_pad < K.lds_max && total <= K.lds_max - fixed1 - K.slice_pad && ncg * nchunks <= K.tmax) {
        units.push_back(Unit{0, ncg, 0, nchunks, 0, 0, 0, 0});
        std::fill(out.nsl.begin(), out.nsl.end(), static_cast<uint8_t>(1));
        V = v;
        out.lds_slices = K.lds_max - fixed1;
        break;
      }
    }
    if (fixed + K.slice_pad + 4096 >= K.lds_max) continue;
    const uint32_t cap = K.lds_max - fixed - K.slice_pad;
    bool ok = true;
    for (int cg = 0; cg < ncg && ok; ++cg) {
      int slot = 0, k0 = 0;
      uint32_t acc = 0;
      for (int k = 0; k < nchunks; ++k) {
        const uint32_t b = ub[static_cast<size_t>(cg) * nchunks + k];
        if (b > cap) {
          ok = false;
          break;
        }
        if (acc + b > cap || k - k0 >= K.tmax) {
          units.push_back(Unit{cg, 1, k0, k, slot++, 0, 0, 0});
          k0 = k;
          acc = 0;
        }
        acc += b;
      }
      units.push_back(Unit{cg, 1, k0, nchunks, slot++, 0, 0, 0});
      out.nsl[static_cast<size_t>(cg)] = static_cast<uint8_t>(slot);
    }
    if (ok && static_cast<int>(units.size()) <= max_units) {
      V = v;
      out.lds_slices = K.lds_max - fixed;
      break;
    }
  }
  if (V == 0) return;
  out.V = V;
  out.E = E;
  out.maxslots = 1;
  for (uint8_t x : out.nsl) out.maxslots = std::max<int>(out.maxslots, x);

  const size_t NWV = static_cast<size_t>(K.nwv), PM = static_cast<size_t>(K.pmax);
  out.pieces.assign(units.size() * NWV * PM, 0u);
  out.npieces.assign(units.size() * NWV, 0);
  out.wave_cg.assign(units.size() * NWV, 255);
  std::vector<int> T, nw;
  for (size_t ui = 0; ui < units.size(); ++ui) {
    const Unit& U = units[ui];
    // (a unit's slices are the chunks [k0, k1) of its column groups)
    auto steps_of = [&](int cgl, int s) {
      return static_cast<int>(L[static_cast<size_t>(U.cg0 + cgl) * nchunks + U.k0 + s] & 255u);
    };
    if (!deal_pieces(ui, U.ncgs, U.k1 - U.k0, K, steps_of, T, nw, out.npieces, out.wave_cg, out.pieces))
      return;  // does not fit the piece lists: streaming launches (ok stays false)
  }
  out.ok = true;
}

// ---- the resident solver on a row view (k_rv_resident.hip.h) -------------------------------------------

struct ViewUnit {  // layout of clipper_hip::RvrUnit
  int cg0, ncgs;   // column groups [cg0, cg0 + ncgs) x every chunk of the view
  int l0, l1;      // lanes [l0, l1) of each
  int pack;        // 0, or G = 64 / (l1 - l0) >= 2: a unit of ONE group whose slices are packed G chunks side by
                   // side — lane group g of packed slice s holds the unit's columns of chunk s * G + g — so that a
                   // step keeps all 64 lanes busy and the chains of steps are G times shorter
  int pad1, pad2, pad3;
};

struct ViewResidentPlan {
  bool ok = false;
  uint32_t lds_slices = 0;        // bytes of LDS the slices of a unit may take
  uint64_t entries = 0;           // stored entries of the view
  std::vector<ViewUnit> units;
  std::vector<uint8_t> npieces;   // [unit * nwv + wave]
  std::vector<uint8_t> wave_cg;   // [unit * nwv + wave] column group of the unit the wave works for (255: none)
  std::vector<uint32_t> pieces;   // [(unit * nwv + wave) * pmax + j] = chunk | q0 << 8 | q1 << 16
  // scratch of the planner, kept from call to call (a view is planned between two iterations of a solve)
  std::vector<uint64_t> ent, byt;
  std::vector<int> stp, sorted_stp, T, nw;
};

// Units of COMPLETE columns: a unit holds every chunk of its column groups (so that a column's sums never
// leave the workgroup), as many groups as balance the ENTRIES (the LDS gathers of a pass go with them) up
// to `target_units` workgroups; a group whose slices exceed a unit's LDS or its share of the entries (the
// dense inlier block) is split by LANES into equal parts. Then the pieces of every unit (deal_pieces).
// xt_fixed: bytes of LDS a unit needs besides its slices.
inline void plan_view_resident(const uint32_t* L, int ncg, int nchunks, int esize, int target_units, int max_units,
                               uint32_t fixed_bytes, const ResidentConsts& K, ViewResidentPlan& out) {
  out.ok = false;
  out.units.clear();
  out.entries = 0;
  if (ncg < 1 || nchunks < 1 || nchunks > K.tmax || fixed_bytes + K.slice_pad + 8192 >= K.lds_max) return;
  const uint32_t cap = K.lds_max - fixed_bytes - K.slice_pad;
  out.lds_slices = K.lds_max - fixed_bytes;
  const uint32_t QBY = 4u * static_cast<uint32_t>(esize);
  std::vector<uint64_t>&ent = out.ent, &byt = out.byt;
  ent.assign(static_cast<size_t>(ncg), 0);
  byt.assign(static_cast<size_t>(ncg), 0);
  uint64_t total = 0;
  for (int cg = 0; cg < ncg; ++cg) {
    uint64_t e = 0, b = 0;
    for (int k = 0; k < nchunks; ++k) {
      const uint32_t lq = L[static_cast<size_t>(cg) * nchunks + k];
      e += lq >> 8;
      b += slice_bound(lq, QBY, K.so);
    }
    ent[static_cast<size_t>(cg)] = e;
    byt[static_cast<size_t>(cg)] = b;
    total += e;
  }
  out.entries = total;
  target_units = std::max(1, std::min(target_units, max_units));
  const double Te0 = std::max(256.0, static_cast<double>(total) / target_units);
  const int max_cgs = std::min(K.nwv, K.tmax / nchunks);  // one wave per group in the tail; slices per unit
  if (max_cgs < 1) return;
  // A pass's time in a unit goes with its lock-step STEPS (the CU's LDS pipe issues per wave-step, however few
  // lanes are busy: measured 0.45 us per step and wave on top of 4 us), and the steps of a sparse group are those
  // of its longest column: 30 .. 125 per group at the headline view for 3 400 .. 4 600 entries. A group far above
  // the median is cut into two packed halves (its long column weighs on one of them only, and each half walks
  // two chunks per step) — while the units still fit the chip.
  std::vector<int>&stp = out.stp, &sorted_stp = out.sorted_stp;
  stp.assign(static_cast<size_t>(ncg), 0);
  for (int c = 0; c < ncg; ++c) {
    int t = 0;
    for (int k = 0; k < nchunks; ++k) t += static_cast<int>(L[static_cast<size_t>(c) * nchunks + k] & 255u);
    stp[static_cast<size_t>(c)] = t;
  }
  sorted_stp = stp;
  std::nth_element(sorted_stp.begin(), sorted_stp.begin() + ncg / 2, sorted_stp.end());
  const double Tmed = std::max(1, sorted_stp[static_cast<size_t>(ncg / 2)]);
  std::vector<ViewUnit>& units = out.units;
  // Attempts: with the heavy groups split, without, then with more entries per unit — a view of 600 rows over
  // 12 000 columns has more column groups than the chip has places for units of one group each (round 4: such views
  // stayed with the streaming launches for no better reason)
  const double scales[] = {1.0, 1.0, 1.35, 1.8, 2.4, 3.2};
  for (int attempt = (nchunks >= 2 ? 0 : 1); attempt < 6; ++attempt) {
  const int heavy_split = attempt == 0 ? 1 : 0;
  const double Te = Te0 * scales[attempt];
  units.clear();
  int cg = 0;
  while (cg < ncg) {
    const uint64_t e = ent[static_cast<size_t>(cg)], b = byt[static_cast<size_t>(cg)];
    // (a lane subset keeps every step's padding and the header: its bytes fall a little slower than its lanes)
    int nsplit = std::max(static_cast<int>((b + cap - 1) / cap), static_cast<int>(std::floor(static_cast<double>(e) / (1.5 * Te) + 0.5)));
    nsplit = std::max(1, nsplit);
    if (nsplit == 1 && heavy_split && static_cast<double>(stp[static_cast<size_t>(cg)]) > 1.35 * Tmed) {
      units.push_back(ViewUnit{cg, 1, 0, 32, 2, 0, 0, 0});
      units.push_back(ViewUnit{cg, 1, 32, 64, 2, 0, 0, 0});
      ++cg;
      continue;
    }
    if (nsplit > 1) {
      // (lane parts of 32, 16 or 8 lanes: as many chunks side by side in a packed slice)
      int parts = 2;
      while (parts < nsplit) parts *= 2;
      while (parts < 8 && parts < nchunks) parts *= 2;  // (as few packed slices as the lanes allow: the chains of steps end sooner)
      while (parts < 8 && (b / parts) + static_cast<uint64_t>(nchunks) * (16 + 64 + 64 * 16) > cap) parts *= 2;
      if (parts > 8 || (b / parts) + static_cast<uint64_t>(nchunks) * (16 + 64 + 64 * 16) > cap) return;
      for (int p = 0; p < parts; ++p)
        units.push_back(ViewUnit{cg, 1, 64 * p / parts, 64 * (p + 1) / parts, parts, 0, 0, 0});
      ++cg;
      continue;
    }
    int n = 0;
    uint64_t eacc = 0, bacc = 0;
    while (cg + n < ncg && n < max_cgs) {
      const uint64_t e2 = ent[static_cast<size_t>(cg + n)], b2 = byt[static_cast<size_t>(cg + n)];
      if (n > 0 && (bacc + b2 > cap || static_cast<double>(eacc + e2) > 1.15 * Te || static_cast<double>(e2) > 1.5 * Te ||
                    (heavy_split && static_cast<double>(stp[static_cast<size_t>(cg + n)]) > 1.35 * Tmed)))
        break;
      eacc += e2;
      bacc += b2;
      ++n;
    }
    units.push_back(ViewUnit{cg, n, 0, 64, 0, 0, 0, 0});
    cg += n;
  }
  if (static_cast<int>(units.size()) <= max_units) break;
  }
  if (static_cast<int>(units.size()) > max_units) return;

  const size_t NWV = static_cast<size_t>(K.nwv), PM = static_cast<size_t>(K.pmax);
  out.pieces.assign(units.size() * NWV * PM, 0u);
  out.npieces.assign(units.size() * NWV, 0);
  out.wave_cg.assign(units.size() * NWV, 255);
  for (size_t ui = 0; ui < units.size(); ++ui) {
    const ViewUnit& U = units[ui];
    // (a packed unit: its slices are the packed ones, as long as the longest of the chunks in each)
    const int G = U.pack > 1 ? U.pack : 1;
    const int nsl = (nchunks + G - 1) / G;
    auto steps_of = [&](int cgl, int sidx) {
      const uint32_t* lrow = L + static_cast<size_t>(U.cg0 + cgl) * nchunks;
      int mq = 0;
      for (int g = 0; g < G && sidx * G + g < nchunks; ++g) mq = std::max(mq, static_cast<int>(lrow[sidx * G + g] & 255u));
      return mq;
    };
    if (!deal_pieces(ui, U.ncgs, nsl, K, steps_of, out.T, out.nw, out.npieces, out.wave_cg, out.pieces))
      return;  // does not fit the piece lists: the streaming launches keep the view
  }
  out.ok = true;
}

// ---- the plan image: a resident plan as its kernel reads it ----------------------------------------------------
// What either resident solver puts into mapped pinned memory: the unit records (UNIT_BYTES each), an optional block of
// bytes (the resident solver's slots per column group), the piece counts, the wave map and the pieces, every array
// at a multiple of 16 bytes, 64 bytes of tail behind the last piece. Of the pieces only those in use are written
// (a few per wave of the pmax places: a tenth of the table, into pinned memory); the kernels read a wave's pieces
// below its count only (rs_wave_pass), so what lies behind it is never used.
constexpr size_t UNIT_BYTES = 32;
static_assert(sizeof(Unit) == UNIT_BYTES && sizeof(ViewUnit) == UNIT_BYTES, "both units are records of UNIT_BYTES");

struct PlanLayout {
  size_t nunits = 0, nslots = 0, nwaves = 0, pmax = 0;  // records, bytes of the optional block, waves, pieces per wave
  size_t off_slots = 0, off_np = 0, off_wc = 0, off_pc = 0, bytes = 0;  // bytes: of the whole image, tail included
  // the five arrays of an image at `base` (the host's pointer or its device alias)
  template <class U>
  const U* units(const uint8_t* base) const { return reinterpret_cast<const U*>(base); }
  const uint8_t* slots(const uint8_t* base) const { return base + off_slots; }
  const uint8_t* npieces(const uint8_t* base) const { return base + off_np; }
  const uint8_t* wave_cg(const uint8_t* base) const { return base + off_wc; }
  const uint32_t* pieces(const uint8_t* base) const { return reinterpret_cast<const uint32_t*>(base + off_pc); }
};

inline PlanLayout plan_layout(size_t nunits, size_t nslots, size_t nwaves, size_t pmax) {
  auto up16 = [](size_t x) { return (x + 15) & ~static_cast<size_t>(15); };
  PlanLayout A{nunits, nslots, nwaves, pmax};
  A.off_slots = nunits * UNIT_BYTES;
  A.off_np = A.off_slots + up16(nslots);
  A.off_wc = A.off_np + up16(nwaves);
  A.off_pc = A.off_wc + up16(nwaves);
  A.bytes = A.off_pc + nwaves * pmax * sizeof(uint32_t) + 64;
  return A;
}

// writes a plan into the A.bytes at `base` (slots: A.nslots bytes, may be null when there are none)
inline void plan_pack(const PlanLayout& A, uint8_t* base, const void* units, const uint8_t* slots, const uint8_t* npieces,
                      const uint8_t* wave_cg, const uint32_t* pieces) {
  std::memcpy(base, units, A.nunits * UNIT_BYTES);
  if (A.nslots) std::memcpy(base + A.off_slots, slots, A.nslots);
  std::memcpy(base + A.off_np, npieces, A.nwaves);
  std::memcpy(base + A.off_wc, wave_cg, A.nwaves);
  uint32_t* dst = reinterpret_cast<uint32_t*>(base + A.off_pc);
  for (size_t wv = 0; wv < A.nwaves; ++wv)
    for (size_t j = 0; j < npieces[wv]; ++j) dst[wv * A.pmax + j] = pieces[wv * A.pmax + j];
}

}  // namespace clipper_plan
