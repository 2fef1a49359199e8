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
 */
#pragma once

#include <memory>
#include <vector>

#include "clipper/clipper.h"
#include "clipper/invariants/device.h"

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

 private:
  Params params_;
  invariants::PairwiseInvariantPtr invariant_;
  int kind_ = 0;  ///< 1 = EuclideanDistance, 2 = PointNormalDistance, 3 = DeviceInvariant
  int device_ = 0;
  CLIPPER::Storage storage_ = CLIPPER::Storage::F32_CSC;
  clipper_hip_batch* b_ = nullptr;
  void check(int rc, const char* what) const;
  explicit CLIPPERBatch(const Params& params) : params_(params) {}
};

}  // namespace clipper
