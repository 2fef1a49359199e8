/**
 * clipper/batch.h — many independent CLIPPER problems solved together.
 *
 * An addition of this build (the reference has no batch): CLIPPERBatch scores and solves a list of problems with one
 * call into the C ABI's clipper_hip_batch_* — the problems the resident solver takes run side by side on the chip,
 * the others are solved one after the other as CLIPPER::solve would. Per problem the Solution is that of a lone
 * CLIPPER with the same invariant, params, storage, inputs and u0 (bit for bit on the same route), except Solution::t:
 * the wall time of the whole batch. The constructor takes the built-in invariants (EuclideanDistance,
 * PointNormalDistance); withDeviceInvariant makes a batch scored by a DeviceInvariant (invariants/device.h), one fill
 * launch for all its problems. No explicit matrices, one device.
 *
 * solveAsMSRCSDR runs the semidefinite relaxation of every problem of the last solve in one batched call
 * (clipper_hip_batch_sdp, DESIGN.md 11 "Batches"; every problem needs m <= 128). Its dual bound certifies the
 * dense-cluster answers: -sdpSolutions()[i].dobj is an upper bound on the optimum of the problem solve() attacks
 * locally. solveAsMaximumClique finds the maximum clique of every problem's consistency graph in one batched call
 * (clipper_hip_batch_max_clique, DESIGN.md 9 "Batches").
 */
#pragma once

#include <memory>
#include <vector>

#include "clipper/clipper.h"
#include "clipper/invariants/device.h"
#include "clipper/sdp.h"

struct clipper_hip_batch;

namespace clipper {

struct BatchProblem {
  invariants::Data D1, D2;
  Association A;  ///< empty: all-to-all
  VectorXd u0;    ///< empty: utils::randvec, as CLIPPER::solve
};

class CLIPPERBatch {
 public:
  /// throws std::invalid_argument for anything but an EuclideanDistance or a PointNormalDistance
  CLIPPERBatch(const invariants::PairwiseInvariantPtr& invariant, const Params& params);
  ~CLIPPERBatch();
  /// a batch scored by a user-defined invariant on the device: every problem's D1, D2 have the same number of rows,
  /// the dimension the invariant is compiled for (DeviceInvariant::handle) at solve time
  static std::unique_ptr<CLIPPERBatch> withDeviceInvariant(const invariants::DeviceInvariantPtr& invariant,
                                                           const Params& params);
  CLIPPERBatch(const CLIPPERBatch&) = delete;
  CLIPPERBatch& operator=(const CLIPPERBatch&) = delete;

  void setDevice(int device);                  ///< before the first solve
  void setStorage(CLIPPER::Storage storage);   ///< before the first solve; default F32_CSC

  std::vector<Solution> solve(const std::vector<BatchProblem>& problems);
  Association getSelectedAssociations(int i) const;  ///< of problem i of the last solve (clipper.cpp:124-127)
  bool solvedBatched(int i) const;                   ///< problem i ran in a batched resident launch

  /// CLIPPER::solveAsMSRCSDR (with setDeviceSdp) for every problem of the last solve(), in one batched call. Solution i
  /// is what clipper.cpp:108-112 makes of the relaxation (nodes, u = 0, score = -1, ifinal = 0; t: the whole call's);
  /// getSelectedAssociations(i) follows it. The solver state is untouched: a later solve() gives the same results.
  /// Throws std::logic_error before any solve, std::runtime_error when a problem has m > 128 (the message names it).
  std::vector<Solution> solveAsMSRCSDR(const sdp::Params& params = sdp::Params{});
  /// CLIPPER::solveAsMaximumClique for every problem of the last solve(), in one batched call
  /// (clipper_hip_batch_max_clique, DESIGN.md 9 "Batches"): problems up to m = 2048 side by side, larger ones one by
  /// one afterwards. Solution i is what clipper.cpp:92-96 leaves (nodes ascending, u = 0, score = -1, ifinal = 0; t:
  /// the whole call's), its nodes those of a lone CLIPPER::solveAsMaximumClique; getSelectedAssociations(i) follows it.
  /// params.time_limit bounds the whole call; params.threads is ignored; params.verbose prints one line per problem.
  /// params.warm_start starts every problem's search from its own node list (clipper_hip_batch_max_clique_seeded).
  /// The solver state is untouched. Throws std::logic_error before any solve.
  std::vector<Solution> solveAsMaximumClique(const maxclique::Params& params = maxclique::Params{});
  /// the relaxations of the last solveAsMSRCSDR (X, lambdas, evec1, thr, nodes, iters, pobj, dobj, times)
  const std::vector<sdp::Solution>& sdpSolutions() const { return sdp_; }

 private:
  Params params_;
  invariants::PairwiseInvariantPtr invariant_;
  int kind_ = 0;  ///< 1 = EuclideanDistance, 2 = PointNormalDistance, 3 = DeviceInvariant
  int device_ = 0;
  CLIPPER::Storage storage_ = CLIPPER::Storage::F32_CSC;
  clipper_hip_batch* b_ = nullptr;
  size_t n_ = 0;  ///< problems of the last solve
  std::vector<sdp::Solution> sdp_;
  void check(int rc, const char* what) const;
  explicit CLIPPERBatch(const Params& params) : params_(params) {}
};

}  // namespace clipper
