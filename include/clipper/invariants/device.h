/**
 * @file device.h
 * @brief A user-defined invariant written as HIP device source, evaluated on the GPU.
 *
 * The source defines
 *
 *     __device__ double clipper_invariant(const double* ai, const double* aj,
 *                                         const double* bi, const double* bj,
 *                                         const double* params);
 *
 * where ai, aj, bi, bj point to CLIPPER_D doubles (the datum's dimension, defined by the library
 * before the source) and params to the object's parameters (at most 16). CLIPPER compiles it at
 * run time (hiprtc, gfx950) the first time it scores data of a dimension, and fills the affinity
 * matrix with it on the device: the matrix is the one the host loop (clipper.cpp:31-64) produces
 * for the same function. The parameters are passed at fill time; changing them compiles nothing.
 */
#pragma once

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "clipper/invariants/abstract.h"

struct clipper_hip_invariant;  // opaque handle of the C ABI (include/clipper_hip.h)

namespace clipper {
namespace invariants {

class DeviceInvariant : public PairwiseInvariant {
 public:
  explicit DeviceInvariant(std::string source, std::vector<double> params = {});
  ~DeviceInvariant() override;
  DeviceInvariant(const DeviceInvariant&) = delete;
  DeviceInvariant& operator=(const DeviceInvariant&) = delete;

  /// The function exists on the device only: calling it on the host throws std::logic_error.
  double operator()(const Datum& ai, const Datum& aj, const Datum& bi, const Datum& bj) override;

  const std::string& source() const { return source_; }
  const std::vector<double>& params() const { return params_; }

  /// The compiled program for datum dimension d, compiled on first use and kept (throws
  /// std::runtime_error with the compiler's log if the source does not compile).
  clipper_hip_invariant* handle(int d) const;

 private:
  std::string source_;
  std::vector<double> params_;
  mutable std::mutex mutex_;
  mutable std::map<int, clipper_hip_invariant*> compiled_;
};
using DeviceInvariantPtr = std::shared_ptr<DeviceInvariant>;

}  // namespace invariants
}  // namespace clipper
