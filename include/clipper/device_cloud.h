/**
 * @file device_cloud.h
 * @brief clipper::registration::DeviceCloud and DevicePairs: point clouds and association lists that LIVE ON THE
 *        DEVICE (clipper_hip_cloud_t, clipper_hip_pairs_t of include/clipper_hip.h), so that the front end — voxel
 *        down-sampling, normals, FPFH, covariances, the descriptor match, the staging of a solve, ICP — runs from raw
 *        scan to refined transform without crossing the bus between its stages. RAII, move-only; the methods mirror the
 *        free functions of registration.h and return their bits. A stage attaches what it computes to the cloud; a
 *        search against a cloud builds its grid once and keeps it. Not safe for concurrent mutation.
 *        CLIPPER::scorePairwiseConsistency(c1, c2, pairs) scores from them without host copies of the points.
 */
#pragma once

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "clipper/registration.h"

namespace clipper {
namespace registration {

namespace detail {
inline void cloud_check(int64_t rc) {
  if (rc >= 0) return;
  if (rc == CLIPPER_HIP_E_INVALID) throw std::invalid_argument(clipper_hip_last_error());
  throw std::runtime_error(clipper_hip_last_error());  // (a missing attachment, no device, the runtime)
}
}  // namespace detail

/// An association list on the device: m x 2, with one squared distance per row where it came from DeviceCloud::match
class DevicePairs {
 public:
  DevicePairs() = default;
  /// A: m x 2; sqd: one squared distance per row, or empty
  explicit DevicePairs(const Association& A, const std::vector<double>& sqd = {}, int device = 0) {
    if (!sqd.empty() && static_cast<int64_t>(sqd.size()) != A.rows())
      throw std::invalid_argument("sqd must hold one squared distance per row of A");
    detail::cloud_check(clipper_hip_pairs_create(device, A.data(), sqd.empty() ? nullptr : sqd.data(), A.rows(), &h_));
  }
  /// adopts a handle a call of the C ABI made
  explicit DevicePairs(clipper_hip_pairs_t* h) : h_(h) {}
  ~DevicePairs() { close(); }
  DevicePairs(const DevicePairs&) = delete;
  DevicePairs& operator=(const DevicePairs&) = delete;
  DevicePairs(DevicePairs&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  DevicePairs& operator=(DevicePairs&& o) noexcept {
    if (this != &o) {
      close();
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  void close() {
    clipper_hip_pairs_destroy(h_);
    h_ = nullptr;
  }
  clipper_hip_pairs_t* handle() const {
    if (!h_) throw std::logic_error("DevicePairs: closed or empty handle");
    return h_;
  }
  int64_t size() const {
    const int64_t m = clipper_hip_pairs_count(handle());
    detail::cloud_check(m);
    return m;
  }
  bool hasSqd() const {
    const int rc = clipper_hip_pairs_has_sqd(handle());
    detail::cloud_check(rc);
    return rc == 1;
  }
  /// the rows, m x 2; sqd (may be null): their squared distances (pairs that carry them: hasSqd())
  Association download(std::vector<double>* sqd = nullptr) const {
    const int64_t m = size();
    Association buf(m > 0 ? m : 1, 2);
    if (sqd) sqd->assign(static_cast<size_t>(m), 0.0);
    detail::cloud_check(clipper_hip_pairs_download(handle(), buf.data(), sqd && m > 0 ? sqd->data() : nullptr));
    Association A(m, 2);
    for (int64_t r = 0; r < m; ++r) {
      A(r, 0) = buf.data()[r];
      A(r, 1) = buf.data()[m + r];
    }
    return A;
  }

 private:
  clipper_hip_pairs_t* h_ = nullptr;
};

/// A point cloud on the device and what the stages have computed about it
class DeviceCloud {
 public:
  DeviceCloud() = default;
  /// P: 3 x n, one point per column; normals: 3 x n unit normals, or empty
  explicit DeviceCloud(const invariants::Data& P, const invariants::Data& normals = invariants::Data(), int device = 0) {
    if (P.cols() > 0 && P.rows() != 3) throw std::invalid_argument("points must be 3 x n");
    const bool has_normals = normals.cols() > 0;
    if (has_normals && (normals.rows() != 3 || normals.cols() != P.cols()))
      throw std::invalid_argument("normals must be 3 x n, one per point");
    detail::cloud_check(clipper_hip_cloud_create(device, P.cols() > 0 ? P.data() : nullptr, has_normals ? normals.data() : nullptr,
                                                 P.cols(), &h_));
  }
  explicit DeviceCloud(clipper_hip_cloud_t* h) : h_(h) {}
  ~DeviceCloud() { close(); }
  DeviceCloud(const DeviceCloud&) = delete;
  DeviceCloud& operator=(const DeviceCloud&) = delete;
  DeviceCloud(DeviceCloud&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  DeviceCloud& operator=(DeviceCloud&& o) noexcept {
    if (this != &o) {
      close();
      h_ = o.h_;
      o.h_ = nullptr;
    }
    return *this;
  }
  void close() {
    clipper_hip_cloud_destroy(h_);
    h_ = nullptr;
  }
  clipper_hip_cloud_t* handle() const {
    if (!h_) throw std::logic_error("DeviceCloud: closed or empty handle");
    return h_;
  }

  int64_t size() const {
    const int64_t n = clipper_hip_cloud_count(handle());
    detail::cloud_check(n);
    return n;
  }
  clipper_hip_cloud_info_t info() const {
    clipper_hip_cloud_info_t out{};
    detail::cloud_check(clipper_hip_cloud_info(handle(), &out));
    return out;
  }
  invariants::Data points() const { return matrix(CLIPPER_HIP_CLOUD_POINTS, 3); }
  invariants::Data normals() const { return matrix(CLIPPER_HIP_CLOUD_NORMALS, 3); }
  invariants::Data descriptors() const { return matrix(CLIPPER_HIP_CLOUD_DESCRIPTORS, info().descriptor_dim); }
  invariants::Data spfh() const { return matrix(CLIPPER_HIP_CLOUD_SPFH, 33); }
  invariants::Data covariances() const { return matrix(CLIPPER_HIP_CLOUD_COVARIANCES, 6); }
  /// an int32 attachment: CLIPPER_HIP_CLOUD_*_COUNTS or CLIPPER_HIP_CLOUD_VOXEL_TRACE
  std::vector<int32_t> counts(int what) const {
    const int64_t n = what == CLIPPER_HIP_CLOUD_VOXEL_TRACE ? info().trace_n : size();
    std::vector<int32_t> out(static_cast<size_t>(n > 0 ? n : 1));
    detail::cloud_check(clipper_hip_cloud_download(handle(), what, out.data()));
    out.resize(static_cast<size_t>(n));
    return out;
  }
  /// descriptors from elsewhere (d x n, d <= 64): they replace the cloud's
  DeviceCloud& setDescriptors(const invariants::Data& F) {
    if (F.cols() != size()) throw std::invalid_argument("descriptors must be d x n, one per point");
    detail::cloud_check(clipper_hip_cloud_set_descriptors(handle(), F.data(), static_cast<int>(F.rows())));
    return *this;
  }

  /// registration::voxel_down_sample: a NEW cloud of the centroids (and the normalised normal sums)
  DeviceCloud voxelDownSample(double voxel_size, bool with_trace = false, clipper_voxel_info_t* info = nullptr) {
    clipper_hip_cloud_t* out = nullptr;
    detail::cloud_check(clipper_hip_cloud_voxel_downsample(handle(), voxel_size, with_trace ? 1 : 0, &out, info));
    return DeviceCloud(out);
  }
  DeviceCloud& estimateNormals(const Neighborhood& nb = {}, const double* viewpoint = nullptr) {
    const clipper_neighborhood_t h{nb.knn, 0, nb.radius};
    detail::cloud_check(clipper_hip_cloud_estimate_normals(handle(), &h, viewpoint));
    return *this;
  }
  DeviceCloud& computeFpfh(const Neighborhood& nb = {32, 0.0}) {
    const clipper_neighborhood_t h{nb.knn, 0, nb.radius};
    detail::cloud_check(clipper_hip_cloud_compute_fpfh(handle(), &h));
    return *this;
  }
  DeviceCloud& computeFpfh(const Neighborhood& normal_nb, const double* viewpoint, const Neighborhood& feature_nb) {
    const clipper_neighborhood_t hn{normal_nb.knn, 0, normal_nb.radius}, hf{feature_nb.knn, 0, feature_nb.radius};
    detail::cloud_check(clipper_hip_cloud_fpfh_from_points(handle(), &hn, viewpoint, &hf));
    return *this;
  }
  DeviceCloud& estimateCovariances(const Neighborhood& nb = {20, 0.0}, double epsilon = 1e-3) {
    const clipper_neighborhood_t h{nb.knn, 0, nb.radius};
    detail::cloud_check(clipper_hip_cloud_estimate_covariances(handle(), &h, epsilon));
    return *this;
  }
  /// registration::match_descriptors against `other`'s descriptors, the filters run on the device
  DevicePairs match(const DeviceCloud& other, const MatchParams& params = {}) const {
    const clipper_match_params_t prm{params.knn, params.mutual ? 1 : 0, params.ratio, params.max_sqdist};
    clipper_hip_pairs_t* out = nullptr;
    detail::cloud_check(clipper_hip_cloud_match(handle(), other.handle(), &prm, &out, nullptr, nullptr));
    return DevicePairs(out);
  }
  /// the points idx names, 3 x k in the order of the list: what estimate_rigid_transform fits
  invariants::Data gatherPoints(const std::vector<int32_t>& idx) const {
    invariants::Data out(3, static_cast<int64_t>(idx.size()));
    detail::cloud_check(clipper_hip_cloud_gather_points(handle(), idx.data(), static_cast<int64_t>(idx.size()), out.data()));
    return out;
  }
  /// registration::icp / icp_generalized of this cloud onto `target`, whose search grid is built once and kept;
  /// params.method picks the metric (the target's normals, or both clouds' covariances, must be attached)
  IcpResult icp(DeviceCloud& target, const IcpParams& params, const double* T_init = nullptr) const {
    return icp_as<IcpResult>(target, params, nullptr, T_init);
  }
  /// registration::icp_robust / icp_generalized_robust on clouds: the same with a loss and / or trimming
  IcpRobustResult icp(DeviceCloud& target, const IcpParams& params, const IcpRobust& robust, const double* T_init = nullptr) const {
    return icp_as<IcpRobustResult>(target, params, &robust, T_init);
  }
  /// registration::evaluate_registration: {fitness, inlier_rmse} and the inlier count of the alignment T
  std::pair<double, double> evaluateRegistration(DeviceCloud& target, const double* T, double max_distance,
                                                 int64_t* count = nullptr) const {
    double fitness = 0.0, rmse = 0.0;
    detail::cloud_check(clipper_hip_cloud_evaluate_registration(handle(), target.handle(), T, max_distance, &fitness, &rmse,
                                                                count, nullptr));
    return {fitness, rmse};
  }

 private:
  template <typename Result>
  Result icp_as(DeviceCloud& target, const IcpParams& params, const IcpRobust* robust, const double* T_init) const {
    return detail::run_icp<Result>(params, robust, detail::cloud_check, [&](const detail::IcpCallArgs& a) {
      return clipper_hip_cloud_icp(handle(), target.handle(), T_init, a.prm, a.rb, a.T_out, a.info, a.ri, a.history);
    });
  }
  invariants::Data matrix(int what, int rows) const {
    const int64_t n = size();
    invariants::Data out(rows > 0 ? rows : 1, n > 0 ? n : 1);
    detail::cloud_check(clipper_hip_cloud_download(handle(), what, out.data()));
    if (n > 0 && rows > 0) return out;
    return invariants::Data(rows > 0 ? rows : 0, n);
  }
  clipper_hip_cloud_t* h_ = nullptr;
};

}  // namespace registration
}  // namespace clipper
