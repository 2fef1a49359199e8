// batch.cpp — clipper::CLIPPERBatch (include/clipper/batch.h) over the C ABI's clipper_hip_batch_*.
#include "clipper/batch.h"

#include <algorithm>
#include <iostream>
#include <stdexcept>
#include <string>
#include <typeinfo>

#include "clipper/utils.h"
#include "clipper_hip.h"

namespace clipper {

namespace sdp {
namespace detail {  // clipper.cpp
clipper_sdp_params_t abi_params(const Params& p);
void fill_solution(Solution& s, const clipper_sdp_info_t& info);
}  // namespace detail
}  // namespace sdp

CLIPPERBatch::CLIPPERBatch(const invariants::PairwiseInvariantPtr& invariant, const Params& params)
    : params_(params), invariant_(invariant) {
  // the built-ins only (a subclass that overrides operator() is a user-defined invariant)
  if (invariant_ && typeid(*invariant_) == typeid(invariants::EuclideanDistance)) kind_ = 1;
  else if (invariant_ && typeid(*invariant_) == typeid(invariants::PointNormalDistance)) kind_ = 2;
  else throw std::invalid_argument("clipper: CLIPPERBatch takes EuclideanDistance or PointNormalDistance only");
}

std::unique_ptr<CLIPPERBatch> CLIPPERBatch::withDeviceInvariant(const invariants::DeviceInvariantPtr& invariant,
                                                                const Params& params) {
  if (!invariant) throw std::invalid_argument("clipper: CLIPPERBatch::withDeviceInvariant needs an invariant");
  std::unique_ptr<CLIPPERBatch> b(new CLIPPERBatch(params));
  b->invariant_ = invariant;
  b->kind_ = 3;
  return b;
}

CLIPPERBatch::~CLIPPERBatch() {
  if (b_) clipper_hip_batch_destroy(b_);
}

void CLIPPERBatch::setDevice(int device) {
  if (b_) throw std::logic_error("clipper: setDevice after the first solve");
  device_ = device;
}

void CLIPPERBatch::setStorage(CLIPPER::Storage storage) {
  if (b_) throw std::logic_error("clipper: setStorage after the first solve");
  storage_ = storage;
}

void CLIPPERBatch::check(int rc, const char* what) const {
  if (rc < 0)
    throw std::runtime_error(std::string("clipper: ") + what + " failed (" + std::to_string(rc) +
                             "): " + clipper_hip_last_error());
}

std::vector<Solution> CLIPPERBatch::solve(const std::vector<BatchProblem>& problems) {
  if (!b_) {
    if (clipper_hip_batch_create(device_, static_cast<int>(storage_), &b_) < 0 || !b_) throw std::runtime_error(std::string("clipper: cannot create the batch: ") + clipper_hip_last_error());
  }
  const size_t n = problems.size();
  std::vector<clipper_batch_problem_t> p(n);
  std::vector<VectorXd> u0(n);
  int d = kind_ == 2 ? 6 : (n ? static_cast<int>(problems[0].D1.rows()) : 3);
  for (size_t i = 0; i < n; ++i) {
    const BatchProblem& q = problems[i];
    if (q.D1.rows() != q.D2.rows() || q.D1.rows() != d)
      throw std::invalid_argument("clipper: problem " + std::to_string(i) + ": D1 and D2 must have " +
                                  std::to_string(d) + " rows");
    const int64_t m = q.A.rows() > 0 ? static_cast<int64_t>(q.A.rows())
                                     : static_cast<int64_t>(q.D1.cols()) * static_cast<int64_t>(q.D2.cols());
    u0[i] = q.u0.size() == 0 ? utils::randvec(static_cast<size_t>(m)) : q.u0;
    if (static_cast<int64_t>(u0[i].size()) != m)
      throw std::invalid_argument("clipper: problem " + std::to_string(i) + ": u0 has the wrong length");
    p[i].D1 = q.D1.data();
    p[i].n1 = q.D1.cols();
    p[i].D2 = q.D2.data();
    p[i].n2 = q.D2.cols();
    p[i].A = q.A.rows() > 0 ? q.A.data() : nullptr;
    p[i].m = q.A.rows();
    p[i].u0 = u0[i].data();
  }
  clipper_params_t prm;
  clipper_params_default(&prm);
  prm.tol_u = params_.tol_u;
  prm.tol_F = params_.tol_F;
  prm.tol_Fop = params_.tol_Fop;
  prm.maxiniters = params_.maxiniters;
  prm.maxoliters = params_.maxoliters;
  prm.beta = params_.beta;
  prm.maxlsiters = params_.maxlsiters;
  prm.eps = params_.eps;
  prm.affinityeps = params_.affinityeps;
  prm.rescale_u0 = params_.rescale_u0 ? 1 : 0;
  prm.rounding = static_cast<int>(params_.rounding);
  const int32_t nn = static_cast<int32_t>(n);
  if (kind_ == 1) {
    const auto& e = std::static_pointer_cast<invariants::EuclideanDistance>(invariant_)->params();
    check(clipper_hip_batch_solve_euclidean(b_, p.data(), nn, d, e.sigma, e.epsilon, e.mindist, &prm), "batch solve");
  } else if (kind_ == 2) {
    const auto& e = std::static_pointer_cast<invariants::PointNormalDistance>(invariant_)->params();
    check(clipper_hip_batch_solve_pointnormal(b_, p.data(), nn, e.sigp, e.epsp, e.sign, e.epsn, &prm), "batch solve");
  } else {
    const auto inv = std::static_pointer_cast<invariants::DeviceInvariant>(invariant_);
    const std::vector<double>& f = inv->params();
    check(clipper_hip_batch_solve_custom(b_, inv->handle(d), p.data(), nn, f.data(), static_cast<int>(f.size()), &prm),
          "batch solve");
  }
  n_ = n;
  sdp_.clear();
  std::vector<Solution> out(n);
  for (size_t i = 0; i < n; ++i) {
    clipper_solve_info_t info;
    const int m = clipper_hip_batch_get_solution(b_, static_cast<int32_t>(i), nullptr, &info);
    check(m, "batch solve (solution)");
    Solution& s = out[i];
    s.u = VectorXd(m);
    check(clipper_hip_batch_get_solution(b_, static_cast<int32_t>(i), s.u.data(), &info), "batch solve (solution)");
    s.nodes.resize(static_cast<size_t>(info.num_nodes));
    if (info.num_nodes > 0)
      check(clipper_hip_batch_get_nodes(b_, static_cast<int32_t>(i), s.nodes.data(), info.num_nodes), "batch solve (nodes)");
    s.t = info.seconds;  // (the whole batch's wall time)
    s.ifinal = info.ifinal;
    s.u0 = u0[i];
    s.score = info.score;
  }
  return out;
}

// clipper_hip_batch_sdp on the problems of the last solve; per problem what CLIPPER::solveAsMSRCSDR leaves
std::vector<Solution> CLIPPERBatch::solveAsMSRCSDR(const sdp::Params& params) {
  if (!b_) throw std::logic_error("clipper: no batch has been solved");
  const clipper_sdp_params_t p = sdp::detail::abi_params(params);
  const int32_t count = static_cast<int32_t>(n_);
  std::vector<clipper_sdp_info_t> info(static_cast<size_t>(std::max<int32_t>(count, 1)));
  sdp_.clear();
  check(clipper_hip_batch_sdp(b_, &p, info.data()), "batch solveAsMSRCSDR");
  std::vector<Solution> out(static_cast<size_t>(count));
  sdp_.resize(static_cast<size_t>(count));
  for (int32_t i = 0; i < count; ++i) {
    const clipper_sdp_info_t& I = info[static_cast<size_t>(i)];
    sdp::Solution& s = sdp_[static_cast<size_t>(i)];
    const int m = clipper_hip_batch_get_sdp(b_, i, nullptr, nullptr, nullptr, nullptr);
    check(m, "batch solveAsMSRCSDR (sizes)");
    s.X = MatrixXd::Zero(m, m);
    s.lambdas = VectorXd::Zero(m);
    s.evec1 = VectorXd::Zero(m);
    check(clipper_hip_batch_get_sdp(b_, i, s.X.data(), nullptr, s.lambdas.data(), s.evec1.data()), "batch solveAsMSRCSDR (X)");
    s.nodes.resize(static_cast<size_t>(I.num_nodes));
    if (I.num_nodes > 0) check(clipper_hip_batch_get_nodes(b_, i, s.nodes.data(), I.num_nodes), "batch solveAsMSRCSDR (nodes)");
    sdp::detail::fill_solution(s, I);
    Solution& o = out[static_cast<size_t>(i)];  // clipper.cpp:108-112
    o.t = I.t_total;
    o.ifinal = 0;
    o.nodes = s.nodes;
    o.u = VectorXd::Zero(m);
    o.score = -1;
  }
  return out;
}

// clipper_hip_batch_max_clique on the problems of the last solve; per problem what CLIPPER::solveAsMaximumClique leaves
std::vector<Solution> CLIPPERBatch::solveAsMaximumClique(const maxclique::Params& params) {
  if (!b_) throw std::logic_error("clipper: no batch has been solved");
  const int method = params.method == maxclique::Method::EXACT ? CLIPPER_HIP_MC_EXACT
                     : params.method == maxclique::Method::HEU ? CLIPPER_HIP_MC_HEU
                                                               : CLIPPER_HIP_MC_KCORE;
  const int32_t count = static_cast<int32_t>(n_);
  std::vector<clipper_maxclique_info_t> info(static_cast<size_t>(std::max<int32_t>(count, 1)));
  std::vector<clipper_maxclique_seed_info_t> sinfo(info.size());
  if (params.warm_start)  // every problem from its own node list (DESIGN.md 9 "Seeded calls")
    check(clipper_hip_batch_max_clique_seeded(b_, method, static_cast<double>(params.time_limit), nullptr, nullptr,
                                              info.data(), sinfo.data()),
          "batch solveAsMaximumClique");
  else
    check(clipper_hip_batch_max_clique(b_, method, static_cast<double>(params.time_limit), info.data()),
          "batch solveAsMaximumClique");
  std::vector<Solution> out(static_cast<size_t>(count));
  for (int32_t i = 0; i < count; ++i) {
    const clipper_maxclique_info_t& I = info[static_cast<size_t>(i)];
    const int m = clipper_hip_batch_get_solution(b_, i, nullptr, nullptr);
    check(m, "batch solveAsMaximumClique (sizes)");
    Solution& o = out[static_cast<size_t>(i)];  // clipper.cpp:92-96
    o.nodes.resize(static_cast<size_t>(I.num_nodes));
    if (I.num_nodes > 0)
      check(clipper_hip_batch_get_nodes(b_, i, o.nodes.data(), I.num_nodes), "batch solveAsMaximumClique (nodes)");
    o.t = I.seconds;
    o.ifinal = 0;
    o.u = VectorXd::Zero(m);
    o.score = -1;
    if (params.verbose) {
      std::cout << "maxclique: problem " << i << ": m = " << m << ", edges = " << I.edges << ", max core = " << I.max_core
                << ", heuristic = " << I.heuristic_size << ", clique = " << I.num_nodes
                << (I.timed_out ? " (timed out)" : "") << ", bb nodes = " << I.bb_nodes;
      if (params.warm_start) {
        const clipper_maxclique_seed_info_t& S = sinfo[static_cast<size_t>(i)];
        std::cout << ", seed given / kept / clique = " << S.seed_given << " / " << S.seed_kept << " / " << S.seed_size;
      }
      std::cout << ", " << I.seconds << " s" << std::endl;
    }
  }
  return out;
}

Association CLIPPERBatch::getSelectedAssociations(int i) const {
  if (!b_) throw std::logic_error("clipper: no batch has been solved");
  clipper_solve_info_t info;
  check(clipper_hip_batch_get_solution(b_, i, nullptr, &info), "getSelectedAssociations");
  const int k = info.num_nodes;
  Association A(k, 2);
  if (k > 0) check(clipper_hip_batch_get_selected_associations(b_, i, A.data(), k), "getSelectedAssociations");
  return A;
}

bool CLIPPERBatch::solvedBatched(int i) const {
  if (!b_) throw std::logic_error("clipper: no batch has been solved");
  const int r = clipper_hip_batch_route(b_, i);
  check(r, "solvedBatched");
  return r == 1;
}

}  // namespace clipper
