// test_icp_robust_rules.cpp — whole robust and trimmed ICPs on the host over clipper_amd/csrc/icp_rules.hpp (g++ only,
// -ffp-contract=off): the plain terms, the weight of a pair, the weighted terms, the trimming threshold by the header's
// radix select (a host loop over icp_select_step, the function the pick kernel's threads share), the addition tree as the
// kernels run it, icp_iterate_over. Prints T, the history, tau and the sum of the weights as hexadecimal bit patterns;
// tests/test_icp_robust_rules.py compares them with tests/icp_robust_model.py bit for bit.
//   usage: test_icp_robust_rules <case file>   (binary: int32 method, max_iterations, n_src, n_tgt, loss, 0; double
//          max_distance, rel_fitness, rel_rmse, scale, trim; T_init 16 column-major; src n_src x 3; tgt n_tgt x 3; normals
//          n_tgt x 3 iff method 1; covariances n_src x 6 and n_tgt x 6 iff method 2)
//          test_icp_robust_rules select <key file>   (binary: int64 n, rank; n uint64 keys): the rank-th smallest key
// Without an argument: the checks of host_icp_check.hpp's check_robust.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_icp_check.hpp"
#include "knn_grid_rules.hpp"

using namespace clipper_hip;

static int failures = 0;
#define EXPECT(c)                                              \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                              \
    }                                                          \
  } while (0)

static uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, 8);
  return b;
}

// the rank-th smallest (1-based) of the keys: ICP_SELECT_PASSES passes of histogram and icp_select_step
static uint64_t select_key(const std::vector<uint64_t>& keys, int64_t rank) {
  uint64_t prefix = 0;
  for (int pass = 0; pass < ICP_SELECT_PASSES; ++pass) {
    uint32_t hist[ICP_SELECT_RADIX] = {0};
    for (uint64_t k : keys)
      if (icp_select_candidate(k, prefix, pass)) ++hist[icp_select_digit(k, pass)];
    int digit;
    int64_t next;
    icp_select_step(hist, rank, digit, next);
    prefix = (prefix << ICP_SELECT_BITS) | static_cast<uint64_t>(digit);
    rank = next;
  }
  return prefix;
}

template <int TERMS>
static void fold(const std::vector<double>& terms, int n, double* S) {
  constexpr int T = TERMS;
  const int nb = (n + ICP_BLOCK - 1) / ICP_BLOCK;
  std::vector<double> part(static_cast<size_t>(nb) * T), v(static_cast<size_t>(ICP_BLOCK) * T);
  for (int b = 0; b < nb; ++b) {
    for (int i = 0; i < ICP_BLOCK; ++i)
      for (int a = 0; a < T; ++a) {
        const int p = b * ICP_BLOCK + i;
        v[static_cast<size_t>(i) * T + a] = p < n ? terms[static_cast<size_t>(p) * T + a] : 0.0;
      }
    for (int a = 0; a < T; ++a) {
      icp_tree(v.data() + a, T);
      part[static_cast<size_t>(b) * T + a] = v[a];
    }
  }
  for (int i = 0; i < ICP_BLOCK; ++i)
    for (int a = 0; a < T; ++a) {
      double acc = 0.0;
      for (int b = i; b < nb; b += ICP_BLOCK) acc = acc + part[static_cast<size_t>(b) * T + a];
      v[static_cast<size_t>(i) * T + a] = acc;
    }
  for (int a = 0; a < T; ++a) {
    icp_tree(v.data() + a, T);
    S[a] = v[a];
  }
}

struct Clouds {
  std::vector<double> src, tgt, nrm, cs, ct;
  int ns, nt;
};

template <int METHOD>
static void run(const Clouds& c, const clipper_icp::Params& prm, const clipper_icp::Robust& rb, double* T) {
  constexpr int TERMS = icp_robust_terms(METHOD);
  const int ns = c.ns, nt = c.nt;
  double lo[3], hi[3], o[3];
  for (int a = 0; a < 3; ++a) lo[a] = hi[a] = c.tgt[a];
  for (int j = 0; j < nt; ++j)
    for (int a = 0; a < 3; ++a) {
      lo[a] = c.tgt[j * 3 + a] < lo[a] ? c.tgt[j * 3 + a] : lo[a];
      hi[a] = c.tgt[j * 3 + a] > hi[a] ? c.tgt[j * 3 + a] : hi[a];
    }
  icp_origin(lo, hi, o);
  const double d2 = prm.max_distance * prm.max_distance, k2 = rb.scale * rb.scale;
  const IcpStop stop{prm.max_iterations, ns, prm.rel_fitness, prm.rel_rmse};
  std::vector<double> hist(static_cast<size_t>(prm.max_iterations + 1) * 3, 0.0), terms(static_cast<size_t>(ns) * TERMS);
  std::vector<double> q(static_cast<size_t>(ns) * 3), od(ns);
  std::vector<int32_t> oi(ns);
  IcpRecord rec{};
  rec.status = ICP_RUNNING;
  IcpSelect sel{};
  double S[TERMS];
  for (int k = 0; rec.status == ICP_RUNNING; ++k) {
    for (int i = 0; i < ns; ++i) {  // the transform and the search
      const double p[3] = {c.src[i * 3], c.src[i * 3 + 1], c.src[i * 3 + 2]};
      double qq[3], bd[1];
      int32_t bi[1];
      icp_transform_point(T, p, qq);
      knn_grid_clear(bd, bi);
      for (int j = 0; j < nt; ++j) {
        const double b[3] = {c.tgt[j * 3], c.tgt[j * 3 + 1], c.tgt[j * 3 + 2]};
        knn_grid_insert<1>(bd, bi, knn_grid_sqdist(qq, b), j);
      }
      for (int a = 0; a < 3; ++a) q[i * 3 + a] = qq[a];
      oi[i] = bi[0];
      od[i] = bd[0];
    }
    sel = IcpSelect{};  // the selection: the control block as the driver and the pick kernel leave it
    sel.tau = d2;
    sel.any = 1;
    if (rb.trim < 1.0) {
      std::vector<uint64_t> keys;
      for (int i = 0; i < ns; ++i)
        if (icp_inlier(oi[i], od[i], d2)) keys.push_back(bits(od[i]));
      sel.within = static_cast<int64_t>(keys.size());
      sel.keep = icp_trim_keep(rb.trim, sel.within);
      sel.any = sel.keep > 0;
      sel.tau = 0.0;
      if (sel.any) {
        const uint64_t key = select_key(keys, sel.keep);
        std::memcpy(&sel.tau, &key, 8);
      }
    }
    for (int i = 0; i < ns; ++i) {  // the weighted terms
      double t[TERMS];
      for (int a = 0; a < TERMS; ++a) t[a] = 0.0;
      if (icp_kept(oi[i], od[i], d2, sel.tau, sel.any)) {
        const int j = oi[i];
        const double qq[3] = {q[i * 3], q[i * 3 + 1], q[i * 3 + 2]};
        const double b[3] = {c.tgt[j * 3], c.tgt[j * 3 + 1], c.tgt[j * 3 + 2]};
        if constexpr (METHOD == ICP_POINT_TO_POINT) {
          double p[ICP_POINT_TERMS];
          icp_point_terms(qq, b, od[i], o, p);
          icp_point_terms_weighted(p, icp_weight(rb.loss, od[i], rb.scale, k2), t);
        } else {
          if constexpr (METHOD == ICP_POINT_TO_PLANE) {
            const double n[3] = {c.nrm[j * 3], c.nrm[j * 3 + 1], c.nrm[j * 3 + 2]};
            icp_plane_terms(qq, b, n, od[i], o, t);
          } else {
            double ca[6], cb[6];
            for (int a = 0; a < 6; ++a) {
              ca[a] = c.cs[static_cast<size_t>(i) * 6 + a];
              cb[a] = c.ct[static_cast<size_t>(j) * 6 + a];
            }
            icp_generalized_terms(qq, b, ca, cb, T, od[i], o, t);
          }
          icp_plane_terms_weighted(icp_weight(rb.loss, t[28], rb.scale, k2), t);
        }
      }
      for (int a = 0; a < TERMS; ++a) terms[static_cast<size_t>(i) * TERMS + a] = t[a];
    }
    fold<TERMS>(terms, ns, S);
    icp_iterate_over<METHOD, true>(stop, k, S, o, T, rec, hist.data() + static_cast<size_t>(k) * 3);
  }
  const int64_t within = rb.trim < 1.0 ? sel.within : rec.count;
  const double wsum = METHOD == ICP_POINT_TO_POINT ? S[ICP_POINT_WEIGHT_SUM] : 0.0;
  std::printf("status %d iterations %d count %" PRId64 " within %" PRId64 "\nT", rec.status, rec.iterations, rec.count, within);
  for (int i = 0; i < 16; ++i) std::printf(" %016" PRIx64, bits(T[i]));
  std::printf("\nhistory");
  for (double h : hist) std::printf(" %016" PRIx64, bits(h));
  std::printf("\nrobust %016" PRIx64 " %016" PRIx64 "\n", bits(sel.tau), bits(wsum));
}

static int checks() {
  namespace ci = clipper_icp;
  ci::Robust r{0, 0, 0.0, 1.0};
  EXPECT(ci::check_robust(&r).empty());  // without a loss the scale is not read
  EXPECT(ci::check_robust(nullptr) == "null robust");
  r.scale = -1.0;
  EXPECT(ci::check_robust(&r).empty());
  r.loss = 5;
  EXPECT(ci::check_robust(&r) == "unknown loss 5 (the losses are 0..4)");
  r.loss = -1;
  EXPECT(ci::check_robust(&r) == "unknown loss -1 (the losses are 0..4)");
  r = ci::Robust{ICP_LOSS_HUBER, 7, 0.01, 1.0};
  EXPECT(ci::check_robust(&r) == "robust: reserved must be 0 (reserved = 7)");
  r.reserved = 0;
  EXPECT(ci::check_robust(&r).empty());
  r.scale = 0.0;
  EXPECT(ci::check_robust(&r) == "scale must be positive and finite with a loss (scale = 0)");
  r.scale = -0.5;
  EXPECT(ci::check_robust(&r) == "scale must be positive and finite with a loss (scale = -0.5)");
  r.scale = INFINITY;
  EXPECT(ci::check_robust(&r) == "scale must be positive and finite with a loss (scale = inf)");
  r.scale = NAN;
  EXPECT(ci::check_robust(&r).find("(scale = ") != std::string::npos);
  r.scale = 0.01;
  r.trim = 0.0;
  EXPECT(ci::check_robust(&r) == "trim must be in (0, 1] (trim = 0)");
  r.trim = 1.25;
  EXPECT(ci::check_robust(&r) == "trim must be in (0, 1] (trim = 1.25)");
  r.trim = -0.5;
  EXPECT(ci::check_robust(&r) == "trim must be in (0, 1] (trim = -0.5)");
  r.trim = NAN;
  EXPECT(ci::check_robust(&r).find("trim must be in (0, 1] (trim = ") == 0);
  r.trim = 1e-300;
  EXPECT(ci::check_robust(&r).empty());
  // the pieces of the select
  EXPECT(icp_select_digit(0x0123456789abcdefULL, 0) == 0x01 && icp_select_digit(0x0123456789abcdefULL, 7) == 0xef);
  EXPECT(icp_select_candidate(0x0123456789abcdefULL, 0, 0) && icp_select_candidate(0x0123456789abcdefULL, 0x0123, 2));
  EXPECT(!icp_select_candidate(0x0123456789abcdefULL, 0x0124, 2));
  EXPECT(icp_trim_keep(0.5, 9) == 4 && icp_trim_keep(0.001, 300) == 0 && icp_trim_keep(0.9999, 300) == 299);
  EXPECT(icp_select_hit(0, 3, 1) && icp_select_hit(0, 3, 3) && !icp_select_hit(0, 3, 4) && !icp_select_hit(3, 0, 3));
  // the weights at the scale
  const double s = 0.03, k2 = s * s;
  EXPECT(icp_weight(ICP_LOSS_NONE, 5.0, s, k2) == 1.0 && icp_weight(ICP_LOSS_HUBER, k2, s, k2) == 1.0);
  EXPECT(icp_weight(ICP_LOSS_CAUCHY, k2, s, k2) == 0.5 && icp_weight(ICP_LOSS_TUKEY, k2, s, k2) == 0.0);
  EXPECT(icp_weight(ICP_LOSS_GEMAN_MCCLURE, k2, s, k2) == 0.25 && icp_weight(ICP_LOSS_TUKEY, 0.0, s, k2) == 1.0);
  std::puts(failures ? "icp robust checks FAILED" : "icp robust checks ok");
  return failures ? 1 : 0;
}

static int select_main(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  int64_t h[2];
  if (std::fread(h, 8, 2, f) != 2) return 3;
  std::vector<uint64_t> keys(static_cast<size_t>(h[0]));
  if (std::fread(keys.data(), 8, keys.size(), f) != keys.size()) return 4;
  std::fclose(f);
  std::printf("key %016" PRIx64 "\n", select_key(keys, h[1]));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return checks();
  if (argc == 3 && std::strcmp(argv[1], "select") == 0) return select_main(argv[2]);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[6];
  double d[5], T[16];
  if (std::fread(h, 4, 6, f) != 6 || std::fread(d, 8, 5, f) != 5 || std::fread(T, 8, 16, f) != 16) return 3;
  const int method = h[0];
  Clouds c;
  c.ns = h[2];
  c.nt = h[3];
  c.src.resize(static_cast<size_t>(c.ns) * 3);
  c.tgt.resize(static_cast<size_t>(c.nt) * 3);
  c.nrm.resize(method == 1 ? c.tgt.size() : 0);
  c.cs.resize(method == 2 ? static_cast<size_t>(c.ns) * 6 : 0);
  c.ct.resize(method == 2 ? static_cast<size_t>(c.nt) * 6 : 0);
  for (std::vector<double>* v : {&c.src, &c.tgt, &c.nrm, &c.cs, &c.ct})
    if (std::fread(v->data(), 8, v->size(), f) != v->size()) return 4;
  std::fclose(f);
  const clipper_icp::Params prm{method, h[1], d[0], d[1], d[2]};
  const clipper_icp::Robust rb{h[4], h[5], d[3], d[4]};
  if (!clipper_icp::check_robust(&rb).empty()) return 5;
  if (method == 2)
    run<ICP_GENERALIZED>(c, prm, rb, T);
  else if (method == 1)
    run<ICP_POINT_TO_PLANE>(c, prm, rb, T);
  else
    run<ICP_POINT_TO_POINT>(c, prm, rb, T);
  return 0;
}
