/**
 * @file sdp.h
 * @brief clipper::sdp — the semidefinite relaxation of CLIPPER (MSRC-SDR), the reference's
 *        include/clipper/sdp.h:15-55 with the same names and fields, solved on the device
 *        (clipper_hip_sdp_solve: ADMM with a Jacobi eigensolver) instead of SCS.
 *
 *   maximize <M, X>  s.t.  tr X = 1, X psd, X_ij = 0 where C_ij = 0, X_ij >= 0 elsewhere
 *
 * Only the lower triangles of M and C (diagonal included) are read. n <= 128, or n <= 1024 after
 * setRoute(Route::Auto) (the wide route). pobj / dobj keep SCS's
 * sign (minimisation): pobj = -<M, X>, dobj = -lambda_max(M - Y), a certified bound on the optimum.
 * The t_scs_* fields keep their names: t_scs = t_scs_solve = t_scs_cone = the device iteration, the
 * others 0. sdp::Params lives in clipper.h (as the facade's solveAsMSRCSDR needs it).
 */
#pragma once

#include <vector>

#include "clipper/clipper.h"

namespace clipper {
namespace sdp {

struct Solution {
  MatrixXd X;
  VectorXd lambdas;  ///< the eigenvalues of X, ascending
  VectorXd evec1;    ///< the eigenvector of the largest; its largest-magnitude entry is positive

  double thr = 0;          ///< threshold for selecting nodes: max |evec1| / 2
  std::vector<int> nodes;  ///< indices of selected nodes: |evec1_i| > thr

  int iters = 0;   ///< number of iterations
  float pobj = 0;  ///< primal objective value
  float dobj = 0;  ///< dual objective value

  double t = 0;             ///< total time: parsing, solving, extraction
  double t_parse = 0;       ///< time spent setting up the problem data
  double t_scs = 0;         ///< total solver time
  double t_scs_setup = 0;   ///< solver setup time
  double t_scs_solve = 0;   ///< solver solve time
  double t_scs_linsys = 0;  ///< time in a linear system solver (none here)
  double t_scs_cone = 0;    ///< time in the cone projections
  double t_scs_accel = 0;   ///< time in the acceleration routine (none here)
  double t_extract = 0;     ///< time spent extracting which nodes to select
};

/// The route of the device solver (clipper_hip_sdp_set_route): Workgroup, the default, serves n <= 128 with one
/// workgroup per problem; Auto adds the wide route for n up to 1024 (one problem at a time over the whole chip);
/// Wide takes the wide route at every n <= 1024. Process-wide; solve (both overloads), CLIPPER::solveAsMSRCSDR with
/// setDeviceSdp(true) and CLIPPERBatch::solveAsMSRCSDR follow it.
enum class Route { Workgroup = 0, Auto = 1, Wide = 2 };
void setRoute(Route route);
Route route();

/// sdp.cpp:109-303 on HIP device 0; throws std::runtime_error when the device solver refuses (n above the route's
/// limit: 128 by default; no device).
Solution solve(const MatrixXd& M, const MatrixXd& C, const Params& params = Params{});

/// Many problems in one call (clipper_hip_sdp_solve_batch, DESIGN.md section 11 "Batches"): one workgroup per problem,
/// all side by side on the device. Solution i is solve(M[i], C[i], params), bit for bit; only the times differ: they
/// are the whole call's. time_limit_secs bounds the whole call. Throws std::invalid_argument when the lists' sizes
/// differ, std::runtime_error when the device solver refuses (the message names the problem).
std::vector<Solution> solve(const std::vector<MatrixXd>& M, const std::vector<MatrixXd>& C, const Params& params = Params{});

}  // namespace sdp
}  // namespace clipper
