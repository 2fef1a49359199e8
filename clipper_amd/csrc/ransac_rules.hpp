// ransac_rules.hpp — the rules of RANSAC over putative associations ("RANSAC over putative
// associations"), stated once for the kernels (k_ransac.hip.h), the driver (host_ransac.hpp) and the host: the sample
// of a hypothesis (an integer-only, counter-based draw), the edge-length check, the fit, the score (an inlier COUNT,
// ties to the smaller hypothesis number), the rounds and the stop rule, the polish (ICP's point-to-point sums, fold and
// step over the inliers) and what the call returns. Plain sequential functions of one hypothesis, one correspondence or
// one visit of the polish: which work item holds what belongs to the kernels. Every expression rounds as written (the
// build runs with -ffp-contract=off), no floating-point atomics anywhere, and the score is an integer, so that
// everything the call returns is a function of the inputs alone. No HIP: builds with g++ as well
// (tests/cpp/test_ransac_rules.cpp runs whole calls over this header); tests/ransac_model.py restates the same contract
// in numpy. The last section (ransac_needed, ransac_stop, ransac_host_call) is host only.
#pragma once

#include <math.h>
#include <stdint.h>

#include "icp_rules.hpp"

namespace clipper_hip {

constexpr int RANSAC_RUNNING = -1;
constexpr int RANSAC_CONVERGED = 0, RANSAC_MAX_HYPOTHESES = 1, RANSAC_NO_MODEL = 2;  // clipper_ransac_info_t.status
constexpr int RANSAC_MIN_SAMPLE = 3, RANSAC_MAX_SAMPLE = 8;
constexpr int RANSAC_ATTEMPTS = 64;    // draws a hypothesis may spend on its sample
constexpr int RANSAC_MIN_COUNT = 3;    // a best count below this is no model
constexpr int RANSAC_ROUND_UNIT = 256, RANSAC_MAX_ROUND = 65536;  // hypotheses_per_round: a multiple of the first
constexpr int RANSAC_MAX_REFINE = 10;

// ---- the draw ---------------------------------------------------------------------------------------------------------
// the finalizer of splitmix64
ICP_HD uint64_t ransac_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// attempt t of hypothesis h: an index in [0, m), a function of (seed, h, t) alone (the high half of x times m, no modulo)
ICP_HD int32_t ransac_draw(uint64_t seed, uint64_t h, int t, int32_t m) {
  const uint64_t x = ransac_mix(seed + 0x9E3779B97F4A7C15ull * (h * 64 + static_cast<uint64_t>(t) + 1));
  return static_cast<int32_t>(((x >> 32) * static_cast<uint64_t>(m)) >> 32);
}

// the sample of hypothesis h: the slots fill in order, an index already in the sample is skipped; false (the
// hypothesis is invalid; the open slots hold -1) when RANSAC_ATTEMPTS draws do not fill them
template <int N>
ICP_HD bool ransac_sample(uint64_t seed, uint64_t h, int32_t m, int32_t (&s)[N]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int a = 0; a < N; ++a) s[a] = -1;
  int filled = 0;
  for (int t = 0; t < RANSAC_ATTEMPTS && filled < N; ++t) {
    const int32_t idx = ransac_draw(seed, h, t, m);
    bool seen = false;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int a = 0; a < N; ++a) seen = seen || s[a] == idx;
    if (seen) continue;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int a = 0; a < N; ++a)
      if (a == filled) s[a] = idx;
    ++filled;
  }
  return filled == N;
}

// ---- the edge-length check --------------------------------------------------------------------------------------------
ICP_HD double ransac_sqlen(const double (&a)[3], const double (&b)[3]) {
  const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// every pair i < j of the sample: both lengths positive (no point of either cloud twice) and within the ratio;
// s2 = edge_similarity * edge_similarity, evaluated once by the caller
template <int N>
ICP_HD bool ransac_edges(const double (&P)[N][3], const double (&B)[N][3], double s2) {
  bool ok = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < N; ++i)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = i + 1; j < N; ++j) {
      const double l1 = ransac_sqlen(P[i], P[j]), l2 = ransac_sqlen(B[i], B[j]);
      ok = ok && (l1 > 0.0 && l2 > 0.0 && l1 >= s2 * l2 && l2 >= s2 * l1);
    }
  return ok;
}

// ---- the fit (the order of clipper_hip_estimate_rigid_transform) ------------------------------------------------------
// centroids: sums in sample order from +0.0, divided by N; H = sum (b - cb)(p - cp)^T in sample order from +0.0; R its
// rotation; t_r = ((cb_r - R_r0 cp_0) - R_r1 cp_1) - R_r2 cp_2. T: column-major 4 x 4. false: R is no rotation.
template <int N>
ICP_HD bool ransac_fit(const double (&P)[N][3], const double (&B)[N][3], double* T) {
  double cp[3] = {0.0, 0.0, 0.0}, cb[3] = {0.0, 0.0, 0.0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < N; ++i)
    for (int c = 0; c < 3; ++c) {
      cp[c] += P[i][c];
      cb[c] += B[i][c];
    }
  for (int c = 0; c < 3; ++c) {
    cp[c] /= static_cast<double>(N);
    cb[c] /= static_cast<double>(N);
  }
  double H[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, R[9];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < N; ++i)
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) H[r * 3 + c] += (B[i][r] - cb[r]) * (P[i][c] - cp[c]);
  rotation_from_cross_covariance(H, R);
  for (int r = 0; r < 3; ++r) {
    double t = cb[r];
    for (int c = 0; c < 3; ++c) {
      T[c * 4 + r] = R[r * 3 + c];
      t -= R[r * 3 + c] * cp[c];
    }
    T[3 * 4 + r] = t;
    T[r * 4 + 3] = 0.0;
  }
  T[15] = 1.0;
  return fabs(icp_det3(R) - 1.0) <= ICP_DET_TOL;
}

// Hypothesis h whole: the sample, both checks, the fit. get(k, p, b): correspondence k's pair. false: no score (T is
// then not to be read; s holds what the sample got to).
template <int N, class Get>
ICP_HD bool ransac_hypothesis(uint64_t seed, uint64_t h, int32_t m, double s2, Get get, int32_t (&s)[N], double* T) {
  if (!ransac_sample<N>(seed, h, m, s)) return false;
  double P[N][3], B[N][3];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < N; ++i) get(s[i], P[i], B[i]);
  if (!ransac_edges<N>(P, B, s2)) return false;
  return ransac_fit<N>(P, B, T);
}

// ---- the score --------------------------------------------------------------------------------------------------------
// sqd of correspondence (p, b) under T; an inlier iff sqd <= d2, d2 = max_distance * max_distance evaluated once
ICP_HD double ransac_sqd(const double* T, const double (&p)[3], const double (&b)[3], double (&q)[3]) {
  icp_transform_point(T, p, q);
  const double d0 = q[0] - b[0], d1 = q[1] - b[1], d2 = q[2] - b[2];
  return (d0 * d0 + d1 * d1) + d2 * d2;
}
ICP_HD bool ransac_inlier(double sqd, double d2) { return sqd <= d2; }

// (count, -h) as one key: the larger key is the better hypothesis, among equal counts the smaller h. count < 2^31,
// h < 2^32. -1: no hypothesis had a score.
ICP_HD int64_t ransac_key(int64_t count, uint64_t h) { return (count << 32) | static_cast<int64_t>(0xFFFFFFFFull - h); }
ICP_HD int64_t ransac_key_count(int64_t key) { return key < 0 ? 0 : key >> 32; }
ICP_HD int64_t ransac_key_h(int64_t key) { return key < 0 ? -1 : static_cast<int64_t>(0xFFFFFFFFull - (static_cast<uint64_t>(key) & 0xFFFFFFFFull)); }

// the record k_ransac_best leaves (64 bytes); the host reads it once per round
struct alignas(64) RansacRecord {
  int64_t best_key;    // of all rounds so far
  int64_t checked;     // hypotheses that passed both checks, all rounds
  int64_t evaluated;   // hypotheses formed, all rounds
  int32_t survivors;   // of the last round
  int32_t round;       // the last round's number, -1 before the first
  int64_t pad[4];
};
static_assert(sizeof(RansacRecord) == 64, "the round record is 64 bytes");

// the winner so far, beside the record
struct RansacBest {
  double T[16];
  int32_t sample[RANSAC_MAX_SAMPLE];
};

// ---- the polish -------------------------------------------------------------------------------------------------------
// the terms correspondence k adds to ICP's 17 point-to-point sums under T (+0.0 each from a non-inlier); true: an inlier
ICP_HD bool ransac_terms(const double* T, const double (&p)[3], const double (&b)[3], double d2, const double (&o)[3],
                         double (&t)[ICP_POINT_TERMS]) {
  double q[3];
  const double sqd = ransac_sqd(T, p, b, q);
  const bool in = ransac_inlier(sqd, d2);
  if (in) {
    icp_point_terms(q, b, sqd, o, t);
  } else {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int a = 0; a < ICP_POINT_TERMS; ++a) t[a] = 0.0;
  }
  return in;
}

// T: the accepted transform and S its sums; cand: the transform whose sums the next visit brings
struct RansacPolish {
  double T[16], cand[16], S[ICP_POINT_TERMS];
  int32_t refined, done;
};

// Visit i = 0 .. refine_iterations with Sc, the sums under cand. Visit 0 takes cand (the best hypothesis, or the
// identity) as it is; a later visit accepts cand iff its count is >= the current one, and the first rejection ends the
// loop. After an acceptance, unless the iterations are used up or the count is below RANSAC_MIN_COUNT, the next
// candidate is ICP's point-to-point step from S: cand = dT T; a degenerate step (or a value that is not finite) ends
// the loop.
ICP_HD void ransac_polish_visit(RansacPolish& r, int i, int refine, const double* Sc, const double (&o)[3]) {
  if (r.done) return;
  if (i > 0 && !(Sc[0] >= r.S[0])) {
    r.done = 1;
    return;
  }
  for (int a = 0; a < 16; ++a) r.T[a] = r.cand[a];
  for (int a = 0; a < ICP_POINT_TERMS; ++a) r.S[a] = Sc[a];
  if (i > 0) ++r.refined;
  if (i >= refine || r.S[0] < static_cast<double>(RANSAC_MIN_COUNT)) {
    r.done = 1;
    return;
  }
  double dT[16], N[16];
  const bool ok = icp_step_point(r.S, o, dT);
  for (int a = 0; a < 16; ++a) N[a] = r.T[a];
  icp_compose(dT, N);
  bool finite = true;
  for (int a = 0; a < 16; ++a) finite = finite && fabs(N[a]) <= 1.7976931348623157e308;
  if (ok && finite)
    for (int a = 0; a < 16; ++a) r.cand[a] = N[a];
  else
    r.done = 1;
}

// what the sums under the final T say
ICP_HD double ransac_rmse(const double* S) { return S[0] > 0.0 ? sqrt(S[ICP_POINT_TERMS - 1] / S[0]) : 0.0; }

}  // namespace clipper_hip

// ---- host only: the stop rule and a whole call, sequential or on a few threads ----------------------------------------
#include <cmath>
#include <thread>
#include <vector>

namespace clipper_hip {

struct RansacCall {
  double max_distance, edge_similarity, confidence;
  int64_t max_hypotheses;
  int32_t hypotheses_per_round, n_sample, refine_iterations;
  uint64_t seed;
};

struct RansacOutcome {
  int32_t status = RANSAC_NO_MODEL, refined = 0;
  int64_t evaluated = 0, checked = 0, best_hypothesis = -1, best_count = 0, count = 0;
  double fitness = 0.0, inlier_rmse = 0.0;
  int32_t sample[RANSAC_MAX_SAMPLE] = {-1, -1, -1, -1, -1, -1, -1, -1};
  double T[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};

// hypotheses needed to have drawn an all-inlier sample with probability `confidence` when a fraction w = count / m of
// the correspondences are inliers: ceil(log(1 - confidence) / log(1 - w^n)); 1 when w^n >= 1; INT64_MAX when 1 - w^n
// rounds to 1 (or the quotient is beyond int64)
inline int64_t ransac_needed(int64_t count, int64_t m, int32_t n_sample, double confidence) {
  const double w = static_cast<double>(count) / static_cast<double>(m);
  const double wn = std::pow(w, static_cast<double>(n_sample));
  if (wn >= 1.0) return 1;
  const double den = std::log(1.0 - wn);
  if (!(den < 0.0)) return INT64_MAX;
  const double k = std::ceil(std::log(1.0 - confidence) / den);
  if (!(k < 9.0e18)) return INT64_MAX;
  return k < 1.0 ? 1 : static_cast<int64_t>(k);
}

// after a round: RANSAC_RUNNING, or why the rounds end
inline int ransac_stop(int64_t best_count, int64_t evaluated, int64_t m, const RansacCall& c) {
  if (best_count >= RANSAC_MIN_COUNT && evaluated >= ransac_needed(best_count, m, c.n_sample, c.confidence)) return RANSAC_CONVERGED;
  if (evaluated >= c.max_hypotheses) return best_count >= RANSAC_MIN_COUNT ? RANSAC_MAX_HYPOTHESES : RANSAC_NO_MODEL;
  return RANSAC_RUNNING;
}

// the 17 sums over all m correspondences under T by ICP's order of addition (ICP_BLOCK per partial, the halving tree,
// partials t, t + 256, ... per item, the tree again); mask (may be null): the inlier flags
inline void ransac_host_sums(const double* T, const double* P, const double* B, int64_t m, double d2, const double (&o)[3],
                             double* S, uint8_t* mask) {
  constexpr int TT = ICP_POINT_TERMS;
  const int64_t nb = (m + ICP_BLOCK - 1) / ICP_BLOCK;
  std::vector<double> part(static_cast<size_t>(nb) * TT), v(static_cast<size_t>(ICP_BLOCK) * TT);
  for (int64_t blk = 0; blk < nb; ++blk) {
    for (int i = 0; i < ICP_BLOCK; ++i) {
      const int64_t k = blk * ICP_BLOCK + i;
      double t[TT];
      for (int a = 0; a < TT; ++a) t[a] = 0.0;
      if (k < m) {
        const double p[3] = {P[k * 3], P[k * 3 + 1], P[k * 3 + 2]}, b[3] = {B[k * 3], B[k * 3 + 1], B[k * 3 + 2]};
        const bool in = ransac_terms(T, p, b, d2, o, t);
        if (mask) mask[k] = in ? 1 : 0;
      }
      for (int a = 0; a < TT; ++a) v[static_cast<size_t>(i) * TT + a] = t[a];
    }
    for (int a = 0; a < TT; ++a) {
      icp_tree(v.data() + a, TT);
      part[static_cast<size_t>(blk) * TT + a] = v[a];
    }
  }
  for (auto& x : v) x = 0.0;
  for (int t = 0; t < ICP_BLOCK; ++t)
    for (int64_t b = t; b < nb; b += ICP_BLOCK)
      for (int a = 0; a < TT; ++a) v[static_cast<size_t>(t) * TT + a] = v[static_cast<size_t>(t) * TT + a] + part[static_cast<size_t>(b) * TT + a];
  for (int a = 0; a < TT; ++a) {
    icp_tree(v.data() + a, TT);
    S[a] = v[a];
  }
}

// hypothesis h against all m gathered pairs: false without a score
template <int N>
bool ransac_host_score(const RansacCall& c, uint64_t h, const double* P, const double* B, int32_t m, double s2, double d2,
                       int32_t (&s)[N], double* T, int64_t& count) {
  auto get = [&](int32_t k, double (&p)[3], double (&b)[3]) {
    for (int a = 0; a < 3; ++a) {
      p[a] = P[static_cast<int64_t>(k) * 3 + a];
      b[a] = B[static_cast<int64_t>(k) * 3 + a];
    }
  };
  count = 0;
  if (!ransac_hypothesis<N>(c.seed, h, m, s2, get, s, T)) return false;
  for (int32_t k = 0; k < m; ++k) {
    double p[3], b[3], q[3];
    get(k, p, b);
    count += ransac_inlier(ransac_sqd(T, p, b, q), d2) ? 1 : 0;
  }
  return true;
}

// A whole call on the host over the gathered pairs P, B (3 x m each), `threads` host threads sharing the hypotheses
// of a round (the result does not depend on their number). mask: m flags or null.
template <int N>
void ransac_host_call_n(const RansacCall& c, const double* P, const double* B, int32_t m, int threads, RansacOutcome& out,
                        uint8_t* mask) {
  const double s2 = c.edge_similarity * c.edge_similarity, d2 = c.max_distance * c.max_distance;
  int64_t best = -1;
  out = RansacOutcome{};
  const int nt = threads < 1 ? 1 : threads;
  for (;;) {
    const uint64_t h0 = static_cast<uint64_t>(out.evaluated);
    std::vector<int64_t> key(static_cast<size_t>(nt), -1), passed(static_cast<size_t>(nt), 0);
    auto work = [&](int w) {
      for (int64_t i = w; i < c.hypotheses_per_round; i += nt) {
        int32_t s[N];
        double T[16];
        int64_t cnt;
        if (!ransac_host_score<N>(c, h0 + static_cast<uint64_t>(i), P, B, m, s2, d2, s, T, cnt)) continue;
        ++passed[static_cast<size_t>(w)];
        const int64_t k = ransac_key(cnt, h0 + static_cast<uint64_t>(i));
        if (k > key[static_cast<size_t>(w)]) key[static_cast<size_t>(w)] = k;
      }
    };
    if (nt == 1) {
      work(0);
    } else {
      std::vector<std::thread> pool;
      for (int w = 0; w < nt; ++w) pool.emplace_back(work, w);
      for (auto& t : pool) t.join();
    }
    for (int w = 0; w < nt; ++w) {
      out.checked += passed[static_cast<size_t>(w)];
      if (key[static_cast<size_t>(w)] > best) best = key[static_cast<size_t>(w)];
    }
    out.evaluated += c.hypotheses_per_round;
    out.status = ransac_stop(ransac_key_count(best), out.evaluated, m, c);
    if (out.status != RANSAC_RUNNING) break;
  }
  RansacPolish pol{};
  for (int a = 0; a < 16; ++a) pol.cand[a] = out.T[a];  // the identity
  if (out.status != RANSAC_NO_MODEL) {
    out.best_hypothesis = ransac_key_h(best);
    out.best_count = ransac_key_count(best);
    int32_t s[N];
    int64_t cnt;
    ransac_host_score<N>(c, static_cast<uint64_t>(out.best_hypothesis), P, B, m, s2, d2, s, pol.cand, cnt);
    for (int a = 0; a < N; ++a) out.sample[a] = s[a];
  }
  // the origin of the sums: the centre of the exact box of the gathered targets
  double lo[3] = {B[0], B[1], B[2]}, hi[3] = {B[0], B[1], B[2]}, o[3];
  for (int32_t k = 1; k < m; ++k)
    for (int a = 0; a < 3; ++a) {
      const double x = B[static_cast<int64_t>(k) * 3 + a];
      lo[a] = x < lo[a] ? x : lo[a];
      hi[a] = x > hi[a] ? x : hi[a];
    }
  icp_origin(lo, hi, o);
  const int refine = out.status == RANSAC_NO_MODEL ? 0 : c.refine_iterations;
  for (int i = 0; i <= refine && !pol.done; ++i) {
    double Sc[ICP_POINT_TERMS];
    ransac_host_sums(pol.cand, P, B, m, d2, o, Sc, nullptr);
    ransac_polish_visit(pol, i, refine, Sc, o);
  }
  for (int a = 0; a < 16; ++a) out.T[a] = pol.T[a];
  out.refined = pol.refined;
  out.count = static_cast<int64_t>(pol.S[0]);
  out.fitness = pol.S[0] / static_cast<double>(m);
  out.inlier_rmse = ransac_rmse(pol.S);
  if (mask) {
    double Sc[ICP_POINT_TERMS];
    ransac_host_sums(out.T, P, B, m, d2, o, Sc, mask);
  }
}

inline void ransac_host_call(const RansacCall& c, const double* P, const double* B, int32_t m, int threads, RansacOutcome& out,
                             uint8_t* mask) {
  switch (c.n_sample) {
    case 3: return ransac_host_call_n<3>(c, P, B, m, threads, out, mask);
    case 4: return ransac_host_call_n<4>(c, P, B, m, threads, out, mask);
    case 5: return ransac_host_call_n<5>(c, P, B, m, threads, out, mask);
    case 6: return ransac_host_call_n<6>(c, P, B, m, threads, out, mask);
    case 7: return ransac_host_call_n<7>(c, P, B, m, threads, out, mask);
    default: return ransac_host_call_n<8>(c, P, B, m, threads, out, mask);
  }
}

}  // namespace clipper_hip
