/**
 * @file registration.h
 * @brief The host-side neighbours of the CLIPPER hot path that the reference keeps in its
 *        benchmark utilities (benchmarks/bm_utils.h: namespace utils): PLY vertex reader, synthetic
 *        putative associations, precision / recall — plus the closed-form rigid transform that
 *        consumes the selected associations (examples/python/ex4_bunny.ipynb), the feature
 *        matcher that produces the putative ones, and the stage in front of it: raw cloud ->
 *        normals -> FPFH descriptors, and the step behind it: ICP over the whole clouds (icp,
 *        evaluate_registration), and the consensus estimator beside the solve (ransac_correspondences).
 *        Thin C++ wrappers over the C ABI (include/clipper_hip.h);
 *        match_descriptors, voxel_down_sample, estimate_normals, compute_fpfh, icp, estimate_covariances,
 *        icp_generalized, icp_robust, icp_generalized_robust, evaluate_registration and ransac_correspondences work
 *        on the device.
 */
#pragma once

#include <array>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../clipper_hip.h"
#include <cstdio>

#include "clipper/invariants/abstract.h"
#include "clipper/types.h"

namespace clipper {
namespace registration {

/// utils::read_ply (bm_utils.cpp:24-79). pts: 3 x n, one point per column. False on failure.
inline bool read_ply(const std::string& plyfile, invariants::Data& pts, bool silent = true) {
  const int64_t n = clipper_hip_read_ply_xyz(plyfile.c_str(), nullptr, 0);
  if (n < 0) {
    if (!silent) std::fprintf(stderr, "read_ply: %s\n", clipper_hip_last_error());
    return false;
  }
  pts = invariants::Data(3, n);
  return n == 0 || clipper_hip_read_ply_xyz(plyfile.c_str(), pts.data(), n) == n;
}

/// utils::generate_synthetic_correspondences (bm_utils.cpp:277-341); `seed` instead of the
/// reference's random_device. Returns {A, Agt}; two empty matrices when Agood is too small.
inline std::pair<Association, Association> generate_synthetic_correspondences(
    int64_t n0, int64_t n1, const Association& Agood, size_t m, double rho, uint64_t seed) {
  Association A(static_cast<int64_t>(m), 2), Agt(static_cast<int64_t>(m), 2);
  int64_t ni = 0;
  const int rc = clipper_hip_generate_synthetic_correspondences(
      n0, n1, Agood.data(), Agood.rows(), static_cast<int64_t>(m), rho, seed, A.data(), Agt.data(), &ni);
  if (rc == CLIPPER_HIP_E_STATE) return {};
  if (rc) throw std::invalid_argument(clipper_hip_last_error());
  Association G(ni, 2);
  for (int64_t i = 0; i < ni; ++i) {
    G(i, 0) = Agt.data()[i];
    G(i, 1) = Agt.data()[ni + i];
  }
  return {A, G};
}

/// utils::get_precision_recall (bm_utils.cpp:345-371)
inline std::pair<double, double> get_precision_recall(const Association& A, const Association& Agt) {
  double p = 0, r = 0;
  if (clipper_hip_precision_recall(A.data(), A.rows(), Agt.data(), Agt.rows(), &p, &r))
    throw std::invalid_argument(clipper_hip_last_error());
  return {p, r};
}

/// Least-squares rigid transform (column-major 4 x 4 in T[16]) over the associations A
inline void estimate_rigid_transform(const invariants::Data& D1, const invariants::Data& D2,
                                     const Association& A, double (&T)[16]) {
  if (D1.rows() != 3 || D2.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  if (clipper_hip_estimate_rigid_transform(D1.data(), D1.cols(), D2.data(), D2.cols(), A.data(), A.rows(), T))
    throw std::invalid_argument(clipper_hip_last_error());
}

/// The filters of match_descriptors (clipper_match_params_t)
struct MatchParams {
  int knn = 1;              ///< 1..8 nearest descriptors of F1 per point of F0
  bool mutual = true;       ///< keep (i, j) only if i is among the knn nearest descriptors of F0 to j
  double ratio = 0.0;       ///< 0 = off; else Lowe's test sqd_0 < ratio^2 sqd_1, in (0, 1), needs knn == 1
  double max_sqdist = 0.0;  ///< <= 0 = off; else the largest squared descriptor distance kept
};

/// Putative associations from feature descriptors, by brute-force nearest neighbours on the device
/// (clipper_hip_match_descriptors). F0: d x n0, F1: d x n1, one descriptor per column, d <= 64. Rows (i, j) with
/// i ascending, then by distance: what scorePairwiseConsistency takes.
inline Association match_descriptors(const invariants::Data& F0, const invariants::Data& F1,
                                     const MatchParams& params = {}, int device = 0) {
  if (F0.rows() != F1.rows()) throw std::invalid_argument("descriptors of different length");
  const clipper_match_params_t prm{params.knn, params.mutual ? 1 : 0, params.ratio, params.max_sqdist};
  const int64_t cap = static_cast<int64_t>(F0.cols()) * (params.knn > 0 ? params.knn : 0);
  Association buf(cap > 0 ? cap : 1, 2);
  const int64_t n = clipper_hip_match_descriptors(device, F0.data(), F0.cols(), F1.data(), F1.cols(),
                                                  static_cast<int>(F0.rows()), &prm, buf.data(), nullptr, cap,
                                                  nullptr, nullptr);
  if (n < 0) throw std::invalid_argument(clipper_hip_last_error());
  Association A(n, 2);
  for (int64_t r = 0; r < n; ++r) {
    A(r, 0) = buf.data()[r];
    A(r, 1) = buf.data()[n + r];
  }
  return A;
}

/// The route of the d = 3 nearest-neighbour search behind estimate_normals, compute_fpfh and the distance-based
/// correspondences (clipper_hip_knn_set_search): one process-wide setting. Brute, the default, evaluates every pair;
/// Grid bins the searched cloud into a uniform grid on the device; Auto takes the grid from
/// CLIPPER_HIP_KNN_AUTO_MIN_N searched points on. Every route returns the same lists, bit for bit.
enum class KnnSearch { Brute = 0, Grid = 1, Auto = 2 };
inline void setKnnSearch(KnnSearch search) {
  if (clipper_hip_knn_set_search(static_cast<int>(search)) < 0)
    throw std::invalid_argument(std::string("registration::setKnnSearch: ") + clipper_hip_last_error());
}
inline KnnSearch knnSearch() { return static_cast<KnnSearch>(clipper_hip_knn_search()); }

/// Which points form a point's neighbourhood (clipper_neighborhood_t): the first knn entries of its
/// nearest-neighbour list in its own cloud, itself included, with radius > 0 only those within it
struct Neighborhood {
  int knn = 16;         ///< 3..32
  double radius = 0.0;  ///< <= 0 = off
};

/// Unit surface normals of the cloud P (3 x n) on the device (clipper_hip_estimate_normals): 3 x n. The sign points
/// towards `viewpoint` (3 doubles), or with nullptr makes the largest component positive. Stacked under the points
/// (rows 0-2 the point, rows 3-5 the normal) they are the 6 x n data of invariants::PointNormalDistance.
inline invariants::Data estimate_normals(const invariants::Data& P, const Neighborhood& nb = {},
                                         const double* viewpoint = nullptr, int device = 0) {
  if (P.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  const clipper_neighborhood_t h{nb.knn, 0, nb.radius};
  invariants::Data N(3, P.cols());
  if (clipper_hip_estimate_normals(device, P.data(), P.cols(), &h, viewpoint, N.data(), nullptr))
    throw std::invalid_argument(clipper_hip_last_error());
  return N;
}

/// FPFH descriptors of the cloud P with unit normals N (both 3 x n) on the device (clipper_hip_compute_fpfh): 33 x n,
/// one descriptor per column: what match_descriptors takes.
inline invariants::Data compute_fpfh(const invariants::Data& P, const invariants::Data& N,
                                     const Neighborhood& nb = {32, 0.0}, int device = 0) {
  if (P.rows() != 3 || N.rows() != 3 || P.cols() != N.cols()) throw std::invalid_argument("points and normals must be 3 x n");
  const clipper_neighborhood_t h{nb.knn, 0, nb.radius};
  invariants::Data F(33, P.cols());
  if (clipper_hip_compute_fpfh(device, P.data(), N.data(), P.cols(), &h, F.data(), nullptr, nullptr))
    throw std::invalid_argument(clipper_hip_last_error());
  return F;
}

/// Both stages in one call (clipper_hip_fpfh_from_points): the descriptors of compute_fpfh(P, estimate_normals(P,
/// normal_nb, viewpoint), feature_nb), bit for bit, with one upload and one search.
inline invariants::Data compute_fpfh(const invariants::Data& P, const Neighborhood& normal_nb, const double* viewpoint,
                                     const Neighborhood& feature_nb, int device = 0) {
  if (P.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  const clipper_neighborhood_t hn{normal_nb.knn, 0, normal_nb.radius}, hf{feature_nb.knn, 0, feature_nb.radius};
  invariants::Data F(33, P.cols());
  if (clipper_hip_fpfh_from_points(device, P.data(), P.cols(), &hn, viewpoint, &hf, F.data(), nullptr))
    throw std::invalid_argument(clipper_hip_last_error());
  return F;
}

/// What voxel_down_sample returns: one column per occupied voxel, in ascending cell number (lexicographic in z, y, x)
struct VoxelDownSampled {
  invariants::Data points;      ///< 3 x n_out: the centroid of each voxel's points
  invariants::Data normals;     ///< 3 x n_out with normals given (3 x 0 otherwise): the voxel's normals summed and normalised
  std::vector<int32_t> counts;  ///< n_out: the points per voxel
  std::vector<int32_t> trace;   ///< n with with_trace (empty otherwise): for every input point its output column
  int dim[3];                   ///< voxels along x, y, z
  int passes;                   ///< 8-bit passes of the radix sort
  int max_count;                ///< the points of the fullest voxel
  double kernels_ms, sort_ms;   ///< device time of the kernels, and of the sort's passes among them
};

/// The cloud P (3 x n) cut to one point per occupied voxel of edge voxel_size, on the device
/// (clipper_hip_voxel_downsample): the step in front of estimate_normals. The grid's origin is the cloud's own minimum
/// corner. `normals` (3 x n, or empty) are summed per voxel and normalised, (0, 0, 1) where they cancel. The result is
/// a function of the inputs alone: the same bits from run to run.
inline VoxelDownSampled voxel_down_sample(const invariants::Data& P, double voxel_size,
                                          const invariants::Data& normals = invariants::Data(), bool with_trace = false,
                                          int device = 0) {
  if (P.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  const bool has_normals = normals.cols() > 0;
  if (has_normals && (normals.rows() != 3 || normals.cols() != P.cols()))
    throw std::invalid_argument("normals must be 3 x n, one per point");
  const size_t n = static_cast<size_t>(P.cols()), room = n > 0 ? n : 1;
  std::vector<double> po(3 * room), no(has_normals ? 3 * room : 0);
  VoxelDownSampled r{};
  r.counts.assign(room, 0);
  if (with_trace) r.trace.assign(room, 0);
  int64_t n_out = 0;
  clipper_voxel_info_t info{};
  if (clipper_hip_voxel_downsample(device, P.data(), has_normals ? normals.data() : nullptr, P.cols(), voxel_size, po.data(),
                                   has_normals ? no.data() : nullptr, r.counts.data(), with_trace ? r.trace.data() : nullptr,
                                   &n_out, &info))
    throw std::invalid_argument(clipper_hip_last_error());
  r.points = invariants::Data(3, n_out);
  r.normals = invariants::Data(3, has_normals ? n_out : 0);
  for (int64_t k = 0; k < 3 * n_out; ++k) r.points.data()[k] = po[static_cast<size_t>(k)];
  for (int64_t k = 0; has_normals && k < 3 * n_out; ++k) r.normals.data()[k] = no[static_cast<size_t>(k)];
  r.counts.resize(static_cast<size_t>(n_out));
  if (with_trace) r.trace.resize(n);
  for (int a = 0; a < 3; ++a) r.dim[a] = info.dim[a];
  r.passes = info.passes;
  r.max_count = info.max_count;
  r.kernels_ms = info.kernels_ms;
  r.sort_ms = info.sort_ms;
  return r;
}

/// The metrics of icp, and the one of icp_generalized
enum class IcpMethod { PointToPoint = 0, PointToPlane = 1, Generalized = 2 };
/// How an icp ended (clipper_icp_info_t.status)
enum class IcpStatus { Converged = 0, MaxIterations = 1, TooFew = 2, Degenerate = 3 };

/// clipper_icp_params_t with the defaults of the facades; max_distance has none
struct IcpParams {
  IcpMethod method = IcpMethod::PointToPoint;
  double max_distance = 0.0;  ///< positive and finite: a correspondence beyond it is no inlier
  int max_iterations = 30;    ///< 0..1000; 0 = evaluate only
  double rel_fitness = 1e-6;  ///< stop when fitness and rmse both change by less than these
  double rel_rmse = 1e-6;
};

/// What icp returns: the refined transform (column-major 4 x 4), how it ended, how good it is, and the rows
/// (count, fitness, rmse) of every evaluated T
struct IcpResult {
  double T[16];
  IcpStatus status;
  int iterations;
  int64_t count;
  double fitness, inlier_rmse;
  KnnSearch route;
  int64_t candidates;
  double device_ms;
  std::vector<std::array<double, 3>> history;
};

/// The losses of icp_robust and icp_generalized_robust (clipper_icp_robust_t.loss)
enum class IcpLoss { None = 0, Huber = 1, Cauchy = 2, Tukey = 3, GemanMcClure = 4 };

/// clipper_icp_robust_t: the defaults are the plain call
struct IcpRobust {
  IcpLoss loss = IcpLoss::None;
  double scale = 0.0;  ///< of the residual (a distance); positive and finite with a loss
  double trim = 1.0;   ///< in (0, 1]: the fraction kept, each iteration, of the points within max_distance
};

/// IcpResult and clipper_icp_robust_info_t (of the last history row)
struct IcpRobustResult : IcpResult {
  int64_t within = 0;       ///< points within max_distance, before trimming
  double weight_sum = 0.0;  ///< the sum of the weights (point-to-point; 0 otherwise)
  double trim_sqd = 0.0;    ///< the trimming threshold: max_distance^2 untrimmed, 0 when nothing was kept
};

namespace detail {
inline clipper_icp_params_t icp_params_c(const IcpParams& params) {
  return {static_cast<int32_t>(params.method), params.max_iterations, params.max_distance, params.rel_fitness, params.rel_rmse};
}
inline clipper_icp_robust_t icp_robust_c(const IcpRobust& r) { return {static_cast<int32_t>(r.loss), 0, r.scale, r.trim}; }

/// what an ICP call left in its info and history (rows of 3 doubles), into r (T is already there)
inline void fill_icp_result(const clipper_icp_info_t& info, const std::vector<double>& hist, IcpResult& r) {
  r.status = static_cast<IcpStatus>(info.status);
  r.iterations = info.iterations;
  r.count = info.count;
  r.fitness = info.fitness;
  r.inlier_rmse = info.inlier_rmse;
  r.route = static_cast<KnnSearch>(info.route);
  r.candidates = info.candidates;
  r.device_ms = info.device_ms;
  for (int k = 0; k <= info.iterations; ++k) r.history.push_back({hist[3 * k], hist[3 * k + 1], hist[3 * k + 2]});
}
inline void fill_icp_robust(const clipper_icp_robust_info_t&, IcpResult&) {}
inline void fill_icp_robust(const clipper_icp_robust_info_t& ri, IcpRobustResult& r) {
  r.within = ri.within;
  r.weight_sum = ri.weight_sum;
  r.trim_sqd = ri.trim_sqd;
}

/// a refusal of the library as the free functions throw it
inline void icp_check(int64_t rc) {
  if (rc < 0) throw std::invalid_argument(clipper_hip_last_error());
}

/// the arguments every ICP call of the C ABI takes besides its clouds; rb and ri are null without robust settings
struct IcpCallArgs {
  const clipper_icp_params_t* prm;
  const clipper_icp_robust_t* rb;
  double* T_out;
  clipper_icp_info_t* info;
  clipper_icp_robust_info_t* ri;
  double* history;
};

/// One ICP call into a Result (IcpResult; IcpRobustResult with robust given): owns the history buffer, runs `call`
/// (which makes the C call on an IcpCallArgs and returns its status), hands a negative status to `check` (which throws
/// with the library's message) and fills the result.
template <typename Result, typename Call>
Result run_icp(const IcpParams& params, const IcpRobust* robust, void (*check)(int64_t), Call&& call) {
  const clipper_icp_params_t prm = icp_params_c(params);
  const clipper_icp_robust_t rb = icp_robust_c(robust ? *robust : IcpRobust{});
  Result r{};
  clipper_icp_info_t info{};
  clipper_icp_robust_info_t ri{};
  std::vector<double> hist(3 * (static_cast<size_t>(params.max_iterations > 0 ? params.max_iterations : 0) + 1), 0.0);
  check(call(IcpCallArgs{&prm, robust ? &rb : nullptr, r.T, &info, robust ? &ri : nullptr, hist.data()}));
  fill_icp_result(info, hist, r);
  fill_icp_robust(ri, r);
  return r;
}

inline void check_icp_clouds(const invariants::Data& src, const invariants::Data& tgt, const invariants::Data& normals) {
  if (src.rows() != 3 || tgt.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  if (normals.cols() > 0 && (normals.rows() != 3 || normals.cols() != tgt.cols()))
    throw std::invalid_argument("normals must be 3 x n, one per target point");
}
inline void check_gicp_clouds(const invariants::Data& src, const invariants::Data& src_cov, const invariants::Data& tgt,
                              const invariants::Data& tgt_cov) {
  if (src.rows() != 3 || tgt.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  if (src_cov.rows() != 6 || src_cov.cols() != src.cols() || tgt_cov.rows() != 6 || tgt_cov.cols() != tgt.cols())
    throw std::invalid_argument("covariances must be 6 x n, one column per point");
}
}  // namespace detail

/// Local refinement of a registration on the device (clipper_hip_icp): ICP of the cloud src onto tgt (3 x n) from the
/// alignment T_init (column-major 4 x 4; nullptr = identity), e.g. estimate_rigid_transform's. PointToPlane needs the
/// target's unit normals (3 x n_tgt, e.g. estimate_normals(tgt)); pass an empty matrix otherwise. The result is the
/// same on every search route and from run to run.
inline IcpResult icp(const invariants::Data& src, const invariants::Data& tgt, const IcpParams& params,
                     const double* T_init = nullptr, const invariants::Data& normals = invariants::Data(), int device = 0) {
  detail::check_icp_clouds(src, tgt, normals);
  return detail::run_icp<IcpResult>(params, nullptr, detail::icp_check, [&](const detail::IcpCallArgs& a) {
    return clipper_hip_icp(device, src.data(), src.cols(), tgt.data(), normals.cols() > 0 ? normals.data() : nullptr, tgt.cols(),
                           T_init, a.prm, a.T_out, a.info, a.history);
  });
}

/// The per-point covariances of generalized ICP for the cloud P (3 x n) on the device
/// (clipper_hip_estimate_covariances): 6 x n, per column xx, xy, xz, yy, yz, zz of I - (1 - epsilon) nv nv^T, nv the
/// normal estimate_normals finds over the same neighbourhood; the identity where fewer than 3 neighbours are kept.
inline invariants::Data estimate_covariances(const invariants::Data& P, const Neighborhood& nb = {20, 0.0},
                                             double epsilon = 1e-3, int device = 0) {
  if (P.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  const clipper_neighborhood_t h{nb.knn, 0, nb.radius};
  invariants::Data C(6, P.cols());
  if (clipper_hip_estimate_covariances(device, P.data(), P.cols(), &h, epsilon, C.data(), nullptr))
    throw std::invalid_argument(clipper_hip_last_error());
  return C;
}

/// Generalized ICP on the device (clipper_hip_icp_generalized): icp's loop with the plane-to-plane metric over the
/// covariances of both clouds (6 x n each, e.g. estimate_covariances'). params.method is taken as given and must be
/// IcpMethod::Generalized. The result is the same on every search route and from run to run.
inline IcpResult icp_generalized(const invariants::Data& src, const invariants::Data& src_cov, const invariants::Data& tgt,
                                 const invariants::Data& tgt_cov, const IcpParams& params, const double* T_init = nullptr,
                                 int device = 0) {
  detail::check_gicp_clouds(src, src_cov, tgt, tgt_cov);
  return detail::run_icp<IcpResult>(params, nullptr, detail::icp_check, [&](const detail::IcpCallArgs& a) {
    return clipper_hip_icp_generalized(device, src.data(), src_cov.data(), src.cols(), tgt.data(), tgt_cov.data(), tgt.cols(),
                                       T_init, a.prm, a.T_out, a.info, a.history);
  });
}

/// icp with a robust loss and / or trimming (clipper_hip_icp_robust): every pair weighs by its residual against
/// robust.scale, and each iteration keeps the fraction robust.trim of the points within max_distance with the smallest
/// distances. count, fitness, inlier_rmse and the history are over the kept points. Tukey and GemanMcClure give pairs far
/// beyond the scale no weight: start them close to the answer. A bad setting throws with its value in the message.
inline IcpRobustResult icp_robust(const invariants::Data& src, const invariants::Data& tgt, const IcpParams& params,
                                  const IcpRobust& robust, const double* T_init = nullptr,
                                  const invariants::Data& normals = invariants::Data(), int device = 0) {
  detail::check_icp_clouds(src, tgt, normals);
  return detail::run_icp<IcpRobustResult>(params, &robust, detail::icp_check, [&](const detail::IcpCallArgs& a) {
    return clipper_hip_icp_robust(device, src.data(), src.cols(), tgt.data(), normals.cols() > 0 ? normals.data() : nullptr,
                                  tgt.cols(), T_init, a.prm, a.rb, a.T_out, a.info, a.ri, a.history);
  });
}

/// icp_generalized with icp_robust's loss and trimming (clipper_hip_icp_generalized_robust); the residual a loss weighs
/// is d^T M d of the pair.
inline IcpRobustResult icp_generalized_robust(const invariants::Data& src, const invariants::Data& src_cov,
                                              const invariants::Data& tgt, const invariants::Data& tgt_cov,
                                              const IcpParams& params, const IcpRobust& robust,
                                              const double* T_init = nullptr, int device = 0) {
  detail::check_gicp_clouds(src, src_cov, tgt, tgt_cov);
  return detail::run_icp<IcpRobustResult>(params, &robust, detail::icp_check, [&](const detail::IcpCallArgs& a) {
    return clipper_hip_icp_generalized_robust(device, src.data(), src_cov.data(), src.cols(), tgt.data(), tgt_cov.data(),
                                              tgt.cols(), T_init, a.prm, a.rb, a.T_out, a.info, a.ri, a.history);
  });
}

/// fitness, inlier rmse and inlier count of an alignment (clipper_hip_evaluate_registration)
struct RegistrationQuality {
  double fitness, inlier_rmse;
  int64_t count;
};

/// How good the alignment T (column-major 4 x 4; nullptr = identity) of src onto tgt (3 x n) is, over all source points.
/// correspondences (may be nullptr): per source point the index of its nearest target point, -1 beyond max_distance.
inline RegistrationQuality evaluate_registration(const invariants::Data& src, const invariants::Data& tgt, const double* T,
                                                 double max_distance, std::vector<int32_t>* correspondences = nullptr,
                                                 int device = 0) {
  if (src.rows() != 3 || tgt.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  RegistrationQuality q{};
  if (correspondences) correspondences->assign(static_cast<size_t>(src.cols() > 0 ? src.cols() : 1), -1);
  if (clipper_hip_evaluate_registration(device, src.data(), src.cols(), tgt.data(), tgt.cols(), T, max_distance, &q.fitness,
                                        &q.inlier_rmse, &q.count, correspondences ? correspondences->data() : nullptr))
    throw std::invalid_argument(clipper_hip_last_error());
  if (correspondences) correspondences->resize(static_cast<size_t>(src.cols()));
  return q;
}

/// The parameters of ransac_correspondences (clipper_ransac_params_t)
struct RansacParams {
  double max_distance = 0.0;        ///< an association is an inlier within this distance under T; must be set (> 0)
  int n_sample = 3;                 ///< 3..8 associations per hypothesis
  double edge_similarity = 0.9;     ///< [0, 1): the edges of a sample must agree within this ratio in both clouds; 0 = off
  int64_t max_hypotheses = 100000;  ///< 1..2^31 - 1
  double confidence = 0.999;        ///< (0, 1): stop once an all-inlier sample has been drawn with this probability
  uint64_t seed = 0;                ///< the same inputs and seed give the same bytes
  int refine_iterations = 1;        ///< 0..10 point-to-point steps over the winner's inliers
  int hypotheses_per_round = 4096;  ///< 256..65536, a multiple of 256
};

enum class RansacStatus { Converged = 0, MaxHypotheses = 1, NoModel = 2 };

/// What ransac_correspondences returns (clipper_ransac_info_t with T and the mask)
struct RansacInfo {
  double T[16];                  ///< column-major 4 x 4; the identity with NoModel
  std::vector<uint8_t> inliers;  ///< per association: within max_distance under T
  RansacStatus status;
  int refined;
  int64_t evaluated, checked, best_hypothesis, best_count, count;
  double fitness, inlier_rmse;
  std::array<int32_t, 8> sample;
  double device_ms;
};

/// RANSAC over the putative associations A (m x 2) between D1 and D2 (3 x n), on the device: the rigid transform most
/// associations agree on within max_distance, its inliers and how the search ended (clipper_hip_ransac_correspondences).
inline RansacInfo ransac_correspondences(const invariants::Data& D1, const invariants::Data& D2, const Association& A,
                                         const RansacParams& params, int device = 0) {
  if (D1.rows() != 3 || D2.rows() != 3) throw std::invalid_argument("points must be 3 x n");
  if (A.rows() > 0 && A.cols() != 2) throw std::invalid_argument("associations must be m x 2");
  clipper_ransac_params_t prm{params.max_distance, params.edge_similarity, params.confidence, params.max_hypotheses,
                              params.hypotheses_per_round, params.n_sample, params.refine_iterations, 0, params.seed};
  clipper_ransac_info_t info{};
  RansacInfo r{};
  r.inliers.assign(static_cast<size_t>(A.rows() > 0 ? A.rows() : 1), 0);
  if (clipper_hip_ransac_correspondences(device, D1.data(), D1.cols(), D2.data(), D2.cols(), A.data(), A.rows(), &prm, r.T,
                                         r.inliers.data(), &info))
    throw std::invalid_argument(clipper_hip_last_error());
  r.inliers.resize(static_cast<size_t>(A.rows()));
  r.status = static_cast<RansacStatus>(info.status);
  r.refined = info.refined;
  r.evaluated = info.evaluated;
  r.checked = info.checked;
  r.best_hypothesis = info.best_hypothesis;
  r.best_count = info.best_count;
  r.count = info.count;
  r.fitness = info.fitness;
  r.inlier_rmse = info.inlier_rmse;
  for (int a = 0; a < 8; ++a) r.sample[static_cast<size_t>(a)] = info.sample[a];
  r.device_ms = info.device_ms;
  return r;
}

}  // namespace registration
}  // namespace clipper
