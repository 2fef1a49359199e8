// The scalar rules of the semidefinite relaxation's iteration (clipper_amd/csrc/sdp_rules.hpp), host only: the simplex
// rule against its sort-and-cumulate definition and where no support is valid, the residual balancing and its schedule
// (a reversal doubles the interval, a one-way run keeps it), the gap test and the tolerances at their
// boundaries, the Jacobi rotation, and the constants (printed for tests/test_sdp_wide_cpu.py, which holds them to
// tests/sdp_model.py). The checks the rules are held to are exact; two side checks (the weights sum to 1,
// c^2 + s^2 = 1) allow a few roundings. Built with g++ by tests/test_sdp_wide_cpu.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "sdp_rules.hpp"

using namespace clipper_hip;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// ---- the simplex rule -----------------------------------------------------------------------------------------------
// tests/sdp_model.py::project_simplex, restated: v sorted descending, K the largest k with v_(k) > (cs_k - 1) / k
static void simplex_by_sorting(std::vector<double> v, int& K, double& tau) {
  std::sort(v.begin(), v.end(), std::greater<double>());
  K = 0;
  tau = 0.0;
  double cs = 0.0;
  for (size_t k = 1; k <= v.size(); ++k) {
    cs += v[k - 1];
    if (v[k - 1] > (cs - 1.0) / static_cast<double>(k)) {
      K = static_cast<int>(k);
      tau = (cs - 1.0) / static_cast<double>(k);
    }
  }
}

// the kernels' use of the rule (sdp_project_simplex): every index asks for its own support, the largest valid one wins
static void simplex_by_rule(const std::vector<double>& v, int& K, double& tau) {
  const int n = static_cast<int>(v.size());
  K = 0;
  tau = 0.0;
  for (int i = 0; i < n; ++i) {
    int cnt;
    double sum;
    if (sdp_support(v.data(), n, v[static_cast<size_t>(i)], cnt, sum) && cnt > K) {
      K = cnt;
      tau = sdp_support_tau(sum, cnt);
    }
  }
}

static int g_simplex_cases = 0;

// entries: integers times 2^-10 in [-4, 4], so every sum is exact in any order
static void check_simplex(const std::vector<int>& units) {
  std::vector<double> v;
  for (int u : units) {
    CHECK(-4096 <= u && u <= 4096);
    v.push_back(u / 1024.0);
  }
  int K0, K1;
  double t0, t1;
  simplex_by_sorting(v, K0, t0);
  simplex_by_rule(v, K1, t1);
  CHECK(K0 >= 1);  // (the largest entry alone is always a valid support)
  CHECK(K1 == K0);
  CHECK(t1 == t0);
  int pos = 0;
  double total = 0.0;
  for (double x : v) {
    const double w = sdp_simplex_weight(x, t1);
    CHECK(w >= 0.0);
    pos += w > 0.0;
    total += w;
  }
  CHECK(pos == K0);
  CHECK(std::fabs(total - 1.0) <= 1e-12);
  ++g_simplex_cases;
}

static void check_simplex_rule() {
  check_simplex({0});                          // n = 1
  check_simplex({4096});
  check_simplex({-4096});
  check_simplex({512, 512, 512, 512});         // all entries equal
  check_simplex({0, 0, 0, 0, 0, 0, 0});
  check_simplex({1024, 512, 512, -1024});      // a tie at the support's edge, inside the support
  check_simplex({1024, 0, 0});                 // a tie at the support's edge, outside it (0 > 0 fails)
  check_simplex({2048, 1024, 1024, 1024});     // the tied entries equal tau exactly: 1 > (2 + 3 - 1) / 4 fails
  check_simplex({1536, 1024, 1024});           // ... and just inside: 1 > (1.5 + 2 - 1) / 3
  check_simplex({-1024, -2048, -3072});        // all entries negative
  check_simplex({-4096, -4096, -4095});
  uint64_t state = 0x9e3779b97f4a7c15ull;  // (a fixed sequence: splitmix64)
  auto next = [&]() {
    uint64_t z = (state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  };
  for (int rep = 0; rep < 200; ++rep) {
    const int n = 1 + static_cast<int>(next() % 40);
    // every fourth vector on a coarse grid (many ties), the others on the full one
    const int step = rep % 4 == 0 ? 512 : 1;
    std::vector<int> units;
    for (int i = 0; i < n; ++i) units.push_back((static_cast<int>(next() % (8192 / step + 1)) - 4096 / step) * step);
    check_simplex(units);
  }
}

// ---- residual balancing ---------------------------------------------------------------------------------------------
static void check_balancing() {
  const double inf = INFINITY;
  const double above10 = std::nextafter(10.0, inf);
  const int dones[] = {9, 10, 11, 20};
  for (int done : dones) {
    SdpCtl k;
    sdp_init_ctl(k, 3);
    CHECK(k.adapt_next == 10 && k.adapt_every == 10 && k.adapt_dir == 0);
    // the record of a run whose moves kept one direction up to `done`: its checks fall on the multiples of 10, as the
    // schedule without memory had them (check_schedule walks such a run through the rules themselves)
    for (int it = 1; it < done; ++it)
      sdp_close_iteration(k, 20.0, 1.0, 0.0, false, sdp_balance_factor(k, it, false, 20.0, 1.0), 0);
    CHECK(k.iters == done - 1 && k.adapt_every == 10 && k.adapt_next == (done + 9) / 10 * 10);
    const bool due = done % 10 == 0;
    CHECK(sdp_balance_factor(k, done, false, 10.0, 1.0) == 1.0);             // r_p / r_d = 10 exactly: no change
    CHECK(sdp_balance_factor(k, done, false, above10, 1.0) == (due ? 2.0 : 1.0));
    CHECK(sdp_balance_factor(k, done, false, 1.0, 10.0) == 1.0);             // 1 / 10 exactly: no change
    CHECK(sdp_balance_factor(k, done, false, 1.0, above10) == (due ? 0.5 : 1.0));
    CHECK(sdp_balance_factor(k, done, false, 3.0, 3.0) == 1.0);
    CHECK(sdp_balance_factor(k, done, true, above10, 1.0) == 1.0);           // converged: no change
    CHECK(sdp_balance_factor(k, done, true, 1.0, above10) == 1.0);
  }
  CHECK(sdp_rescale_of(1.0) == SDP_RESCALE_NONE && sdp_rescale_of(2.0) == SDP_RESCALE_DIVIDE &&
        sdp_rescale_of(0.5) == SDP_RESCALE_MULTIPLY);
  CHECK(sdp_rescale_u(3.0, SDP_RESCALE_DIVIDE) == 1.5 && sdp_rescale_u(3.0, SDP_RESCALE_MULTIPLY) == 6.0);
  // rho U (the dual variable Y) does not move with a rescaling
  CHECK((1.0 * 2.0) * sdp_rescale_u(3.0, sdp_rescale_of(2.0)) == 3.0);
  CHECK((1.0 * 0.5) * sdp_rescale_u(3.0, sdp_rescale_of(0.5)) == 3.0);
  SdpCtl c, c0;
  sdp_init_ctl(c, 3);
  sdp_init_ctl(c0, 0);
  CHECK(c.rho == SDP_RHO0 && c.iters == 0 && c.converged == 0 && c.infeasible == 0 && c.sweeps == 0);
  CHECK(c0.infeasible == 1 && sdp_init_weight(0) == 0.0 && sdp_init_weight(4) == 0.25);
  c.iters = 9;
  c.sweeps = 5;
  sdp_close_iteration(c, 20.0, 1.0, -7.0, false, sdp_balance_factor(c, 10, false, 20.0, 1.0), 3);
  CHECK(c.iters == 10 && c.rho == 2.0 && c.r_prim == 20.0 && c.r_dual == 1.0 && c.pval == -7.0 && c.converged == 0 &&
        c.sweeps == 8);
  CHECK(c.adapt_next == 20 && c.adapt_every == 10 && c.adapt_dir == 1);
  sdp_close_iteration(c, 1.0, 1.0, -7.5, true, sdp_balance_factor(c, 11, true, 1.0, 1.0), 2);
  CHECK(c.iters == 11 && c.rho == 2.0 && c.converged == 1 && c.sweeps == 10 && c.pval == -7.5);
  CHECK(c.adapt_next == 20 && c.adapt_every == 10 && c.adapt_dir == 1);
}

// ---- the schedule of the residual balancing -------------------------------------------------------------------------
// One iteration with the residuals r_p, r_d through the rules, as k_sdpw_decide closes it; returns the factor
static double run_iteration(SdpCtl& c, double r_p, double r_d) {
  const double f = sdp_balance_factor(c, c.iters + 1, false, r_p, r_d);
  sdp_close_iteration(c, r_p, r_d, 0.0, false, f, 0);
  return f;
}

static void check_schedule() {
  const double UP[2] = {20.0, 1.0}, DOWN[2] = {1.0, 20.0}, NONE[2] = {3.0, 3.0};
  // a one-way run keeps the schedule: a move at every multiple of 10 and nowhere else, the interval stays 10
  for (const double* way : {UP, DOWN}) {
    SdpCtl c;
    sdp_init_ctl(c, 3);
    double rho = 1.0;
    for (int it = 1; it <= 100; ++it) {
      const double f = run_iteration(c, way[0], way[1]);
      CHECK(f == (it % 10 == 0 ? (way == UP ? 2.0 : 0.5) : 1.0));
      rho *= f;
      CHECK(c.rho == rho && c.adapt_every == 10 && c.adapt_next == (it / 10 + 1) * 10);
      CHECK(c.adapt_dir == (it < 10 ? 0 : (way == UP ? 1 : -1)));
    }
    CHECK(c.rho == (way == UP ? 1024.0 : 1.0 / 1024.0));
  }
  // a reversal doubles the interval; a check that moves nothing changes neither the interval nor the direction
  SdpCtl c;
  sdp_init_ctl(c, 3);
  struct Step { int at; const double* r; double f; int every, next, dir; };
  const Step steps[] = {
      {10, UP, 2.0, 10, 20, 1},      // the first move: nothing to reverse
      {20, NONE, 1.0, 10, 30, 1},    // no move: the interval and the direction stay
      {30, DOWN, 0.5, 20, 50, -1},   // down after up: 10 -> 20
      {50, DOWN, 0.5, 20, 70, -1},   // the same way again: stays 20
      {70, NONE, 1.0, 20, 90, -1},
      {90, UP, 2.0, 40, 130, 1},     // up after down (the check without a move in between does not hide it): 20 -> 40
      {130, DOWN, 0.5, 80, 210, -1},
  };
  int it = 0;
  for (const Step& s : steps) {
    for (++it; it < s.at; ++it) CHECK(run_iteration(c, UP[0], UP[1]) == 1.0);  // between checks nothing moves
    CHECK(run_iteration(c, s.r[0], s.r[1]) == s.f);
    CHECK(c.iters == s.at && c.adapt_every == s.every && c.adapt_next == s.next && c.adapt_dir == s.dir);
  }
  // a cycle like the star's (up at one check, down at the next, for ever): the moves thin out geometrically, so
  // 100 000 iterations hold at most log2(100 000 / 10) + 2 of them
  sdp_init_ctl(c, 3);
  int moves = 0;
  for (int k = 1; k <= 100000; ++k) {
    const bool up = c.adapt_dir <= 0;
    moves += run_iteration(c, up ? UP[0] : DOWN[0], up ? UP[1] : DOWN[1]) != 1.0;
  }
  CHECK(moves <= 15 && c.rho <= 2.0 && c.rho >= 0.5);
  // the interval stops doubling at SDP_ADAPT_MAX_EVERY and the next check never passes INT32_MAX
  sdp_init_ctl(c, 3);
  c.adapt_every = SDP_ADAPT_MAX_EVERY;
  c.adapt_dir = 1;
  c.adapt_next = INT32_MAX - 5;
  c.iters = INT32_MAX - 6;
  CHECK(run_iteration(c, DOWN[0], DOWN[1]) == 0.5);
  CHECK(c.adapt_every == SDP_ADAPT_MAX_EVERY && c.adapt_next == INT32_MAX && c.adapt_dir == -1);
}

// ---- no valid support -----------------------------------------------------------------------------------------------
static void check_fallback() {
  // (2^53 itself still passes: 2^53 - 1 is a double. From 2^54 on l - 1 rounds back to l for every power of two.)
  const double two53 = 9007199254740992.0, two54 = 2.0 * two53;
  int cnt;
  double sum;
  // every eigenvalue above 2^53: l - 1 rounds to l, and no index has a valid support
  const std::vector<std::vector<double>> none = {
      {two54},
      {two54, two54 * 2, two54 * 4},
      {two54 * 8, two54 * 8, two54},                      // the largest twice: the first of them
      {1e30, 1e300, 1e300, 1e299},
      {NAN},                                              // a NaN: every comparison with it fails
      {NAN, two54, two54 * 2, NAN, two54 * 2},            // ... and it is never chosen over a number
      {NAN, NAN},
  };
  const int want[] = {0, 2, 0, 1, 0, 2, 0};
  for (size_t k = 0; k < none.size(); ++k) {
    const std::vector<double>& v = none[k];
    const int n = static_cast<int>(v.size());
    for (int i = 0; i < n; ++i) CHECK(!sdp_support(v.data(), n, v[static_cast<size_t>(i)], cnt, sum));
    const int top = sdp_fallback_index(v.data(), n);
    CHECK(top == want[k]);
    double total = 0.0;
    for (int i = 0; i < n; ++i) {
      const double w = sdp_fallback_weight(i, top);
      CHECK(w == (i == top ? 1.0 : 0.0));
      total += w;
    }
    CHECK(total == 1.0);
  }
  // a NaN among eigenvalues the rule can handle lies outside every support and takes weight 0: the rule applies
  const double mixed[] = {1.0, NAN, 0.5};
  CHECK(sdp_support(mixed, 3, 1.0, cnt, sum) && cnt == 1 && sum == 1.0);
  CHECK(sdp_simplex_weight(mixed[1], sdp_support_tau(sum, cnt)) == 0.0);
  // just below: at 2^53 l - 1 is exact, the eigenvalue is its own valid support and the rule, not the fallback, applies
  CHECK(sdp_support(&two53, 1, two53, cnt, sum) && cnt == 1);
  // where the rule applies and the largest eigenvalue stands alone by more than 1, both give the same weights
  const double lone[] = {0.25, 3.0, -1.0};
  CHECK(sdp_support(lone, 3, 3.0, cnt, sum) && cnt == 1 && sdp_fallback_index(lone, 3) == 1);
  for (int i = 0; i < 3; ++i) CHECK(sdp_simplex_weight(lone[i], sdp_support_tau(sum, cnt)) == sdp_fallback_weight(i, 1));
}

// ---- the gap test and the tolerances, by hand -----------------------------------------------------------------------
static void check_stopping_rule() {
  // |2 - 1| = 1 against 0.5 + 0.25 * max(2, 1) = 1: equality passes
  CHECK(sdp_gap_closed(2.0, 1.0, 0.5, 0.25));
  CHECK(sdp_gap_closed(1.0, 2.0, 0.5, 0.25));
  CHECK(!sdp_gap_closed(2.0, 1.0, 0.25, 0.25));                        // 1 against 0.75
  // just past equality: |d - mx| = 1 + 2^-51 against 0.5 + 0.25 * (2 + 2^-51) = 1 + 2^-53, which rounds to 1
  CHECK(!sdp_gap_closed(std::nextafter(2.0, INFINITY), 1.0, 0.5, 0.25));
  CHECK(sdp_gap_closed(-4.0, -2.0, 0.0, 0.5));                         // 2 against 0.5 * max(4, 2) = 2
  CHECK(!sdp_gap_closed(-4.0, -2.0, 0.0, 0.25));
  CHECK(sdp_gap_closed(3.0, 3.0, 0.0, 0.0));
  // sums 9, 4, 16, 25, 36 and rho = 2, n = 2: r_p = 3, r_d = 2 * 2 = 4, the norms 4, 5 and 6
  SdpSums s{9.0, 4.0, 16.0, 25.0, 36.0, -1.0};
  double r_p = 0.0, r_d = 0.0;
  // e_pri = 2 * 0.5 + 0.5 * 5 = 3.5, e_dual = 2 * 0.5 + 0.5 * 2 * 6 = 7
  CHECK(sdp_residuals(s, 2.0, 2, 0.5, 0.5, r_p, r_d) && r_p == 3.0 && r_d == 4.0);
  // e_pri = 2 * 0.25 + 0.5 * 5 = 3 = r_p: equality passes; e_dual = 0.5 + 6 = 6.5
  CHECK(sdp_residuals(s, 2.0, 2, 0.25, 0.5, r_p, r_d));
  // e_dual = 2 * 0.5 + 0.25 * 2 * 6 = 4 = r_d: equality passes; e_pri = 1 + 1.25 = 2.25 < 3: the primal one fails
  CHECK(!sdp_residuals(s, 2.0, 2, 0.5, 0.25, r_p, r_d));
  s.rp2 = 4.0;  // r_p = 2 <= 2.25: both pass, the dual one at equality
  CHECK(sdp_residuals(s, 2.0, 2, 0.5, 0.25, r_p, r_d) && r_p == 2.0);
  s.rd2 = 6.25;  // r_d = 2 * 2.5 = 5 > 4: the dual one fails alone
  CHECK(!sdp_residuals(s, 2.0, 2, 0.5, 0.25, r_p, r_d) && r_d == 5.0);
  s = SdpSums{16.0, 4.0, 16.0, 25.0, 36.0, -1.0};  // r_p = 4 > 3: the primal one fails alone
  CHECK(!sdp_residuals(s, 2.0, 2, 0.25, 0.5, r_p, r_d) && r_p == 4.0);
  // the update of one entry and its six terms: x = 1.5, u = -2, z_old = 0.25, m = 3
  double zn, un;
  SdpSums t;
  sdp_update_entry(1.5, -2.0, 0.25, true, 3.0, zn, un, t);  // v = -0.5: clipped
  CHECK(zn == 0.0 && un == -0.5 && t.rp2 == 2.25 && t.rd2 == 0.0625 && t.xx == 2.25 && t.zz == 0.0 && t.uu == 0.25 &&
        t.mx == 4.5);
  sdp_update_entry(1.5, 2.0, 0.25, true, 3.0, zn, un, t);  // v = 3.5: kept
  CHECK(zn == 3.5 && un == 0.0 && t.rp2 == 4.0 && t.rd2 == 10.5625 && t.zz == 12.25 && t.uu == 0.0);
  sdp_update_entry(1.5, 2.0, 0.25, false, 3.0, zn, un, t);  // outside the mask: Z+ = 0
  CHECK(zn == 0.0 && un == 3.5 && t.rp2 == 2.25 && t.uu == 12.25);
  CHECK(sdp_z_plus(-0.5, true) == 0.0 && sdp_z_plus(3.5, true) == 3.5 && sdp_z_plus(3.5, false) == 0.0);
  CHECK(sdp_form_primal(3.0, 1.0, 4.0, 2.0) == 4.0 && sdp_form_dual(4.0, 1.5, 2.0) == 1.0);
  CHECK(sdp_init_entry(true, 0.25) == 0.25 && sdp_init_entry(false, 0.25) == 0.0);
  CHECK(sdp_init_q(2, 2) == 1.0 && sdp_init_q(2, 3) == 0.0);
  CHECK(sdp_sweep_again(1.0, 1.0) && !sdp_sweep_again(0.0, 1.0) && !sdp_sweep_again(0.0, 0.0));
  CHECK(!sdp_sweep_again(SDP_JACOBI_TOL * SDP_JACOBI_TOL, 1.0));  // equality: no further sweep
}

// ---- the rotation ---------------------------------------------------------------------------------------------------
static void check_rotation() {
  double c, s, tn;
  sdp_rotation(0.0, 3.0, -2.0, c, s, tn);
  CHECK(c == 1.0 && s == 0.0 && tn == 0.0);
  // |theta| above 1e150, up to infinity, in both signs
  const double far[][3] = {{0.5, 0.0, 1e200}, {0.5, 1e200, 0.0}, {1e-10, 0.0, 1e300}, {-1e-10, 0.0, 1e300},
                           {1e-300, -1e300, 1e300}, {4e-151, 0.0, 1.0}};
  for (const auto& f : far) {
    CHECK(std::fabs((f[2] - f[1]) / (2.0 * f[0])) > 1e150);
    sdp_rotation(f[0], f[1], f[2], c, s, tn);
    CHECK(std::isfinite(c) && std::isfinite(s) && std::isfinite(tn));
    CHECK(c == 1.0 && std::fabs(s) <= 1e-150);
  }
  // 2 x 2 matrices of small integers: the rotated off-diagonal entry c s (a_pp - a_qq) + (c^2 - s^2) a_pq is at most
  // 4 ulp of the largest entry. (theta, the root, tn, c and s round once each: five roundings, each of relative
  // size 2^-53, and the entry's derivative with respect to each of them is at most the largest entry times a
  // constant below 2; the expression itself is evaluated in long double.)
  double worst = 0.0;
  for (int app = -6; app <= 6; ++app)
    for (int aqq = -6; aqq <= 6; ++aqq)
      for (int apq = -6; apq <= 6; ++apq) {
        sdp_rotation(apq, app, aqq, c, s, tn);
        CHECK(std::fabs(c * c + s * s - 1.0) <= 4 * 2.3e-16);
        const long double lc = c, ls = s;
        const long double off = lc * ls * (static_cast<long double>(app) - aqq) + (lc * lc - ls * ls) * apq;
        const double big = std::max({std::abs(app), std::abs(aqq), std::abs(apq)});
        const double ulp = std::nextafter(big, INFINITY) - big;
        CHECK(std::fabs(static_cast<double>(off)) <= 4.0 * ulp);
        if (big > 0) worst = std::max(worst, std::fabs(static_cast<double>(off)) / ulp);
        // the diagonal block's rule: the trace is kept, a_pq goes to zero exactly
        const double B[4] = {static_cast<double>(app), static_cast<double>(apq), static_cast<double>(apq),
                             static_cast<double>(aqq)};
        double D[4] = {-1.0, -1.0, -1.0, -1.0};
        sdp_rotate_diag(B, D, 2, 0, 1, tn);
        CHECK(D[1] == 0.0 && D[2] == 0.0 && D[0] == app - tn * apq && D[3] == aqq + tn * apq);
      }
  std::printf("rotation: worst off-diagonal residue %.3f ulp of the largest entry\n", worst);
  // the block rule with identity rotations leaves the block; a quarter turn on the rows swaps them with a sign
  double npr, nps, nqr, nqs;
  sdp_rotate_block(1.0, 2.0, 3.0, 4.0, 1.0, 0.0, 1.0, 0.0, npr, nps, nqr, nqs);
  CHECK(npr == 1.0 && nps == 2.0 && nqr == 3.0 && nqs == 4.0);
  sdp_rotate_block(1.0, 2.0, 3.0, 4.0, 0.0, 1.0, 1.0, 0.0, npr, nps, nqr, nqs);
  CHECK(npr == -3.0 && nps == -4.0 && nqr == 1.0 && nqs == 2.0);
  double A[16] = {0};
  sdp_store_block(A, 4, 0, 1, 2, 3, 5.0, 6.0, 7.0, 8.0);
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) CHECK(A[i * 4 + j] == A[j * 4 + i]);
  CHECK(A[0 * 4 + 2] == 5.0 && A[0 * 4 + 3] == 6.0 && A[1 * 4 + 2] == 7.0 && A[1 * 4 + 3] == 8.0);
  double nqp, nqq2;
  sdp_rotate_q(1.0, 2.0, 0.0, 1.0, nqp, nqq2);
  CHECK(nqp == -2.0 && nqq2 == 1.0);
}

int main() {
  check_simplex_rule();
  check_balancing();
  check_schedule();
  check_fallback();
  check_stopping_rule();
  check_rotation();
  std::printf("simplex cases: %d\n", g_simplex_cases);
  std::printf("constants: RHO0 %.17g ADAPT_EVERY %d ADAPT_MU %.17g ADAPT_TAU %.17g JACOBI_TOL %.17g MAX_SWEEPS %d\n",
              SDP_RHO0, SDP_ADAPT_EVERY, SDP_ADAPT_MU, SDP_ADAPT_TAU, SDP_JACOBI_TOL, SDP_MAX_SWEEPS);
  std::printf("sdp rules ok\n");
  return 0;
}
