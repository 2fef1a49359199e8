// clipper_hip.hip — the C ABI declared in include/clipper_hip.h. One translation unit: host_buf.hpp (the owners of
// device memory, pinned memory and events: the only callers of the runtime's allocation functions), host_state.hpp
// (context, shards, RCCL binding), host_call.hpp (the frame of a stand-alone call: device, temporaries, copies), host_solver.hpp (planning,
// dispatch, one iteration), host_matrix.hpp (compressed copy, affinity driver), host_solve.hpp (the solve of one context),
// host_maxclique.hpp (the maximum cliques of a context or a batch), host_matrix_io.hpp (the fills, matrix set / get,
// mat-vecs; the last driver of a context: it holds its kernels' place in the code object), behind it the stand-alone
// searches: host_knn.hpp (nearest neighbours: both routes and their seam), host_match.hpp (putative associations from
// feature descriptors), host_features.hpp, host_icp.hpp, host_voxel.hpp; host_csc_input.hpp (the sparse input's
// host-only checks) and the other host_*.hpp, then the extern "C" entry points, which check their arguments and call
// the internal functions. All arithmetic runs in the kernels of kernels.hip.h; there is no CPU fallback anywhere: if
// HIP is unusable the entry points return an error.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <queue>
#include <string>
#include <type_traits>
#include <utility>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <exception>
#include <vector>

#include "../../include/clipper_hip.h"
#include "kernels.hip.h"
#include "k_custom_invariant_src.h"
#include "dsd_host.h"
#include "host_batch.hpp"
#include "host_plan.hpp"
#include "host_csc_input.hpp"

using namespace clipper_hip;

#include "host_buf.hpp"
using clipper_hip_buf::DevBuf;
using clipper_hip_buf::Event;
using clipper_hip_buf::PinnedBuf;

#include "host_state.hpp"
#include "host_call.hpp"
#include "host_solver.hpp"
#include "host_matrix.hpp"
#include "host_rowview.hpp"
#include "host_resident.hpp"
#include "host_rv_resident.hpp"
#include "host_subproblem.hpp"
#include "host_registration.hpp"
#include "host_sdpwide.hpp"
#include "host_sdp.hpp"
#include "host_sdpbatch.hpp"
#include "host_solve.hpp"
#include "host_custom_invariant.hpp"
#include "host_batchsolve.hpp"
#include "host_maxclique.hpp"
#include "host_matrix_io.hpp"
#include "host_knn.hpp"
#include "host_match.hpp"
#include "host_features.hpp"
#include "host_icp.hpp"
#include "host_ransac.hpp"
#include "host_voxel.hpp"
#include "host_cloud.hpp"

extern "C" {

const char* clipper_hip_last_error(void) try {
  return g_err.c_str();
} CLIPPER_HIP_GUARD_STR

int clipper_hip_device_count(void) try {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return n;
} CLIPPER_HIP_GUARD_INT

clipper_hip_t* clipper_hip_create(int device, int storage) try {
  return make_ctx(&device, 1, storage, 1, 0, false);
} CLIPPER_HIP_GUARD_PTR

clipper_hip_t* clipper_hip_create_group(const int* devices, int nshards, int storage) try {
  if (!devices || nshards < 1) {
    fail(CLIPPER_HIP_E_INVALID, "invalid shard list");
    return nullptr;
  }
  return make_ctx(devices, nshards, storage, nshards, 0, false);
} CLIPPER_HIP_GUARD_PTR

clipper_hip_t* clipper_hip_create_rank(int device, int storage, int rank, int world) try {
  if (world < 1 || rank < 0 || rank >= world) {
    fail(CLIPPER_HIP_E_INVALID, "rank %d / world %d invalid", rank, world);
    return nullptr;
  }
  // CLIPPER_HIP_FORCE_RCCL=1 routes even a 1-rank world through ncclAllGather, so that the
  // communicator plumbing can be exercised on a single-GPU box
  const char* force = std::getenv("CLIPPER_HIP_FORCE_RCCL");
  const bool multiproc = world > 1 || (force && force[0] == '1');
  return make_ctx(&device, 1, storage, world, rank, multiproc);
} CLIPPER_HIP_GUARD_PTR

int clipper_hip_comm_unique_id(void* id128) try {
  if (!id128) return fail(CLIPPER_HIP_E_INVALID, "null id buffer");
  int rc = load_rccl();
  if (rc) return rc;
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  ncclUniqueId id;
  ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) return fail(CLIPPER_HIP_E_COMM, "ncclGetUniqueId failed (%d)", (int)r);
  std::memcpy(id128, &id, sizeof(id));
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_comm_init(clipper_hip_t* h, const void* id128) try {
  if (!h || !id128) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (!h->multiproc) return 0;  // nothing to exchange
  int rc = load_rccl();
  if (rc) return rc;
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof(id));
  HIPCHK(hipSetDevice(h->sh[0].device));
  ncclResult_t r = g_rccl.CommInitRank(&h->comm, h->world, id, h->sh[0].slot);
  if (r != ncclSuccess)
    return fail(CLIPPER_HIP_E_COMM, "ncclCommInitRank: %s",
                g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "error");
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_comm_init_callback(clipper_hip_t* h, clipper_hip_allgather_fn fn, void* user) try {
  if (!h || !fn) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (!h->multiproc) return 0;  // nothing to exchange
  h->xchg_fn = fn;
  h->xchg_user = user;
  return 0;
} CLIPPER_HIP_GUARD_INT

void clipper_hip_destroy(clipper_hip_t* h) try {
  destroy_ctx(h);
} CLIPPER_HIP_GUARD_VOID

// ---- affinity --------------------------------------------------------------------------

int clipper_hip_stage_inputs(clipper_hip_t* h, const double* D1, int d, int64_t n1,
                             const double* D2, int64_t n2, const int32_t* A, int64_t m) try {
  return stage_inputs(h, D1, d, n1, D2, n2, A, m);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_affinity_euclidean_staged(clipper_hip_t* h, double sigma, double epsilon,
                                          double mindist, double affinityeps) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return fill_euclidean(h, EuclidParams{sigma, epsilon, mindist, affinityeps});
} CLIPPER_HIP_GUARD_INT

int clipper_hip_affinity_pointnormal_staged(clipper_hip_t* h, double sigp, double epsp,
                                            double sign, double epsn, double affinityeps) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return fill_pointnormal(h, PointNormalParams{sigp, epsp, sign, epsn, affinityeps});
} CLIPPER_HIP_GUARD_INT

int clipper_hip_affinity_euclidean(clipper_hip_t* h, const double* D1, int d, int64_t n1,
                                   const double* D2, int64_t n2, const int32_t* A, int64_t m,
                                   double sigma, double epsilon, double mindist,
                                   double affinityeps) try {
  return stage_and_fill(h, D1, d, n1, D2, n2, A, m, fill_euclidean, EuclidParams{sigma, epsilon, mindist, affinityeps});
} CLIPPER_HIP_GUARD_INT

int clipper_hip_affinity_pointnormal(clipper_hip_t* h, const double* D1, int d, int64_t n1,
                                     const double* D2, int64_t n2, const int32_t* A, int64_t m,
                                     double sigp, double epsp, double sign, double epsn,
                                     double affinityeps) try {
  if (d != 6) return fail(CLIPPER_HIP_E_INVALID, "PointNormalDistance needs d == 6");
  return stage_and_fill(h, D1, d, n1, D2, n2, A, m, fill_pointnormal, PointNormalParams{sigp, epsp, sign, epsn, affinityeps});
} CLIPPER_HIP_GUARD_INT

// ---- user-defined invariants -------------------------------------------------------------

int clipper_hip_invariant_create(const char* source, int d, clipper_hip_invariant_t** out) try {
  if (out) *out = nullptr;
  if (!source || !out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (d < 1 || d > CLIPPER_HIP_INVARIANT_MAX_D)
    return fail(CLIPPER_HIP_E_INVALID, "invariant dimension d = %d outside [1, %d]", d, CLIPPER_HIP_INVARIANT_MAX_D);
  auto* inv = new clipper_hip_invariant;
  inv->d = d;
  if (int rc = compile_custom(source, d, inv->code)) {
    delete inv;
    return rc;
  }
  *out = inv;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_invariant_destroy(clipper_hip_invariant_t* inv) try {
  if (inv) destroy_invariant(inv);
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_affinity_custom_staged(clipper_hip_t* h, const clipper_hip_invariant_t* inv, const double* params,
                                       int nparams, double affinityeps) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  CustomFill f;
  if (int rc = custom_fill_args(inv, params, nparams, affinityeps, f)) return rc;
  return fill_custom(h, f);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_affinity_custom(clipper_hip_t* h, const clipper_hip_invariant_t* inv, const double* D1, int d,
                                int64_t n1, const double* D2, int64_t n2, const int32_t* A, int64_t m,
                                const double* params, int nparams, double affinityeps) try {
  CustomFill f;
  if (int rc = custom_fill_args(inv, params, nparams, affinityeps, f)) return rc;
  if (d != inv->d)
    return fail(CLIPPER_HIP_E_INVALID, "the invariant is compiled for d = %d, the data have d = %d", inv->d, d);
  return stage_and_fill(h, D1, d, n1, D2, n2, A, m, fill_custom, f);
} CLIPPER_HIP_GUARD_INT

int64_t clipper_hip_num_associations(const clipper_hip_t* h) try {
  return h ? h->m : 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_get_associations(const clipper_hip_t* h, int32_t* A_out) try {
  if (!h || !A_out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (h->A.size() != static_cast<size_t>(2 * h->m))
    return fail(CLIPPER_HIP_E_STATE, "no association list is held");
  std::memcpy(A_out, h->A.data(), h->A.size() * sizeof(int32_t));
  return 0;
} CLIPPER_HIP_GUARD_INT

// ---- matrix set / get ------------------------------------------------------------------

int clipper_hip_set_matrix(clipper_hip_t* h, const double* M, const double* C, int64_t m) try {
  if (!h || !M || !C || m < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return set_dense(h, M, C, m);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_set_sparse(clipper_hip_t* h, int64_t m, const int64_t* Mcolptr,
                           const int32_t* Mrow, const double* Mval, const int64_t* Ccolptr,
                           const int32_t* Crow, const double* Cval) try {
  if (!h || !Mcolptr || !Ccolptr || m < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return set_sparse(h, m, Mcolptr, Mrow, Mval, Ccolptr, Crow, Cval);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_get_matrix(clipper_hip_t* h, double* M_out, double* C_out) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return get_dense(h, M_out, C_out);
} CLIPPER_HIP_GUARD_INT

// ---- solver ------------------------------------------------------------------------------

int clipper_hip_stage_u0(clipper_hip_t* h, const double* u0) try {
  if (!h || !u0) return fail(CLIPPER_HIP_E_INVALID, "u0 is required");
  return stage_u0(h, u0);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_solve(clipper_hip_t* h, const double* u0, const clipper_params_t* P,
                      double* u_out, clipper_solve_info_t* info) try {
  if (!h || !u0 || !P) return fail(CLIPPER_HIP_E_INVALID, "u0 and params are required");
  return solve(h, u0, P, u_out, info);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_solve_staged(clipper_hip_t* h, const clipper_params_t* P, double* u_out,
                             clipper_solve_info_t* info) try {
  if (!h || !P) return fail(CLIPPER_HIP_E_INVALID, "params are required");
  return solve_staged(h, P, u_out, info);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_get_nodes(const clipper_hip_t* h, int32_t* out, int32_t capacity) try {
  if (!h || !out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  const int32_t k = static_cast<int32_t>(h->nodes.size());
  if (capacity < k) return fail(CLIPPER_HIP_E_INVALID, "capacity %d < %d nodes", capacity, k);
  if (k) std::memcpy(out, h->nodes.data(), static_cast<size_t>(k) * sizeof(int32_t));
  return k;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_get_selected_associations(const clipper_hip_t* h, int32_t* A_out,
                                          int32_t capacity) try {
  if (!h || !A_out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  const int32_t k = static_cast<int32_t>(h->nodes.size());
  if (capacity < k) return fail(CLIPPER_HIP_E_INVALID, "capacity %d < %d nodes", capacity, k);
  if (k == 0) return 0;
  if (h->A.size() != static_cast<size_t>(2 * h->m))
    return fail(CLIPPER_HIP_E_STATE, "no association list is held");
  selected_associations(h, h->nodes, A_out);
  return k;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_densest_subgraph(clipper_hip_t* h, const int32_t* S, int32_t k, int32_t* nodes_out,
                                 int32_t capacity) try {
  if (!h || !nodes_out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (h->multiproc)
    return fail(CLIPPER_HIP_E_SCOPE, "not available on a multi-process shard");
  std::vector<int32_t> sub;
  if (S == nullptr || k <= 0) {  // dsd.cpp:279-284: the whole graph
    sub.resize(static_cast<size_t>(h->m));
    for (int64_t i = 0; i < h->m; ++i) sub[static_cast<size_t>(i)] = static_cast<int32_t>(i);
  } else {
    sub.assign(S, S + k);
    for (int32_t v : sub)
      if (v < 0 || v >= h->m) return fail(CLIPPER_HIP_E_INVALID, "node %d out of range", v);
  }
  std::vector<int32_t> nodes;
  int rc = densest_subgraph_of(h, sub, nodes);
  if (rc) return rc;
  const int32_t n = static_cast<int32_t>(nodes.size());
  if (capacity < n) return fail(CLIPPER_HIP_E_INVALID, "capacity %d < %d nodes", capacity, n);
  if (n) std::memcpy(nodes_out, nodes.data(), static_cast<size_t>(n) * sizeof(int32_t));
  return n;
} CLIPPER_HIP_GUARD_INT

// ---- maximum clique of the consistency graph (maxclique::solve, host_maxclique.hpp) ---------------------------

int clipper_hip_max_clique(clipper_hip_t* h, int method, double time_limit_s, clipper_maxclique_info_t* info) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return max_clique_impl(h, method, time_limit_s, info);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_max_clique_seeded(clipper_hip_t* h, int method, double time_limit_s, const int32_t* seed, int32_t nseed,
                                  clipper_maxclique_info_t* info, clipper_maxclique_seed_info_t* seed_info) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return max_clique_seeded_impl(h, method, time_limit_s, seed, nseed, info, seed_info);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_core_numbers(clipper_hip_t* h, int32_t* core_out) try {
  if (!h || !core_out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return core_numbers_impl(h, core_out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_mc_budgets(long long peel_budget, long long wave_budget) try {
  return debug_mc_budgets(peel_budget, wave_budget);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_mc_launches(const clipper_hip_t* h) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return h->mc_launches;
} CLIPPER_HIP_GUARD_INT

// ---- the semidefinite relaxation (sdp::solve, host_sdp.hpp) ------------------------------------------------------

int clipper_hip_sdp(clipper_hip_t* h, const clipper_sdp_params_t* params, double* X_out, double* Y_out,
                    double* lambdas_out, double* evec1_out, clipper_sdp_info_t* info) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return sdp_ctx_impl(h, params, X_out, Y_out, lambdas_out, evec1_out, info);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_sdp_solve(int device, const double* M, const double* C, int64_t n, const clipper_sdp_params_t* params,
                          double* X_out, double* Y_out, double* lambdas_out, double* evec1_out, int32_t* nodes_out,
                          clipper_sdp_info_t* info) try {
  return sdp_solve_impl(device, M, C, n, params, X_out, Y_out, lambdas_out, evec1_out, nodes_out, info);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_sdp_set_route(int route) try {
  if (route != CLIPPER_HIP_SDP_ROUTE_WORKGROUP && route != CLIPPER_HIP_SDP_ROUTE_AUTO && route != CLIPPER_HIP_SDP_ROUTE_WIDE)
    return fail(CLIPPER_HIP_E_INVALID, "sdp: unknown route %d", route);
  return g_sdp_route.exchange(route);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_sdp_route(void) try {
  return g_sdp_route.load();
} CLIPPER_HIP_GUARD_INT

int clipper_hip_sdp_solve_batch(int device, const clipper_sdp_problem_t* problems, int32_t count,
                                const clipper_sdp_params_t* params, clipper_sdp_info_t* infos) try {
  return sdp_solve_batch_impl(device, problems, count, params, infos);
} CLIPPER_HIP_GUARD_INT

// ---- putative associations (before the path): nearest neighbours -------------------------------

int clipper_hip_knn_set_search(int mode) try {
  if (mode != CLIPPER_HIP_KNN_BRUTE && mode != CLIPPER_HIP_KNN_GRID && mode != CLIPPER_HIP_KNN_AUTO)
    return fail(CLIPPER_HIP_E_INVALID, "knn: unknown search mode %d", mode);
  return g_knn_search.exchange(mode);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_knn_search(void) try {
  return g_knn_search.load();
} CLIPPER_HIP_GUARD_INT

int clipper_hip_knn_last_search(clipper_hip_knn_stats_t* out) try {
  if (!out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  knn_events_read();
  *out = g_knn_stats;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_knn(int device, const double* P0, int64_t n0, const double* P1, int64_t n1, int d,
                    int knn, int32_t* idx_out, double* sqd_out) try {
  return knn_search(device, P0, n0, P1, n1, d, knn, idx_out, sqd_out);
} CLIPPER_HIP_GUARD_INT

int64_t clipper_hip_distance_based_correspondences(int device, const double* P0, int64_t n0,
                                                   const double* P1, int64_t n1, int d, int knn,
                                                   double radius, int enforce_1to1, int32_t* A_out,
                                                   int64_t capacity) try {
  if (!A_out && capacity > 0) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return distance_based_correspondences(device, P0, n0, P1, n1, d, knn, radius, enforce_1to1, A_out, capacity);
} CLIPPER_HIP_GUARD_INT

// ---- putative associations from feature descriptors (host_match.hpp) ---------------------------

int64_t clipper_hip_match_descriptors(int device, const double* F0, int64_t n0, const double* F1, int64_t n1, int d,
                                      const clipper_match_params_t* params, int32_t* A_out, double* sqd_out,
                                      int64_t capacity, int32_t* nn_idx_out, double* nn_sqd_out) try {
  return match_descriptors(device, F0, n0, F1, n1, d, params, A_out, sqd_out, capacity, nn_idx_out, nn_sqd_out);
} CLIPPER_HIP_GUARD_INT

// ---- normals and FPFH descriptors of a point cloud (host_features.hpp) -------------------------

int clipper_hip_estimate_normals(int device, const double* P, int64_t n, const clipper_neighborhood_t* nb,
                                 const double* viewpoint, double* N_out, int32_t* count_out) try {
  return estimate_normals(device, P, n, nb, viewpoint, N_out, count_out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_compute_fpfh(int device, const double* P, const double* N, int64_t n, const clipper_neighborhood_t* nb,
                             double* F_out, double* spfh_out, int32_t* count_out) try {
  return compute_fpfh(device, P, N, n, nb, F_out, spfh_out, count_out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_fpfh_from_points(int device, const double* P, int64_t n, const clipper_neighborhood_t* normal_nb,
                                 const double* viewpoint, const clipper_neighborhood_t* feature_nb, double* F_out,
                                 double* N_out) try {
  return fpfh_from_points(device, P, n, normal_nb, viewpoint, feature_nb, F_out, N_out);
} CLIPPER_HIP_GUARD_INT

// ---- ICP over a kept search grid, and the evaluation of a registration (host_icp.hpp) ----------

int clipper_hip_icp(int device, const double* P_src, int64_t n_src, const double* P_tgt, const double* N_tgt,
                    int64_t n_tgt, const double* T_init, const clipper_icp_params_t* params, double* T_out,
                    clipper_icp_info_t* info, double* history) try {
  return icp_call("icp", clipper_icp::FAMILY_POINT_PLANE, clipper_icp::ROBUST_ABSENT, device,
                  {P_src, n_src, P_tgt, n_tgt, N_tgt, nullptr, nullptr}, T_init, params, nullptr, T_out, info, nullptr, history);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_icp_generalized(int device, const double* P_src, const double* C_src, int64_t n_src, const double* P_tgt,
                                const double* C_tgt, int64_t n_tgt, const double* T_init, const clipper_icp_params_t* params,
                                double* T_out, clipper_icp_info_t* info, double* history) try {
  return icp_call("icp_generalized", clipper_icp::FAMILY_GENERALIZED, clipper_icp::ROBUST_ABSENT, device,
                  {P_src, n_src, P_tgt, n_tgt, nullptr, C_src, C_tgt}, T_init, params, nullptr, T_out, info, nullptr, history);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_icp_robust(int device, const double* P_src, int64_t n_src, const double* P_tgt, const double* N_tgt,
                           int64_t n_tgt, const double* T_init, const clipper_icp_params_t* params,
                           const clipper_icp_robust_t* robust, double* T_out, clipper_icp_info_t* info,
                           clipper_icp_robust_info_t* robust_info, double* history) try {
  return icp_call("icp_robust", clipper_icp::FAMILY_POINT_PLANE, clipper_icp::ROBUST_REQUIRED, device,
                  {P_src, n_src, P_tgt, n_tgt, N_tgt, nullptr, nullptr}, T_init, params, robust, T_out, info, robust_info, history);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_icp_generalized_robust(int device, const double* P_src, const double* C_src, int64_t n_src,
                                       const double* P_tgt, const double* C_tgt, int64_t n_tgt, const double* T_init,
                                       const clipper_icp_params_t* params, const clipper_icp_robust_t* robust, double* T_out,
                                       clipper_icp_info_t* info, clipper_icp_robust_info_t* robust_info, double* history) try {
  return icp_call("icp_generalized_robust", clipper_icp::FAMILY_GENERALIZED, clipper_icp::ROBUST_REQUIRED, device,
                  {P_src, n_src, P_tgt, n_tgt, nullptr, C_src, C_tgt}, T_init, params, robust, T_out, info, robust_info, history);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_estimate_covariances(int device, const double* P, int64_t n, const clipper_neighborhood_t* nb, double epsilon,
                                     double* C_out, int32_t* count_out) try {
  return estimate_covariances(device, P, n, nb, epsilon, C_out, count_out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_evaluate_registration(int device, const double* P_src, int64_t n_src, const double* P_tgt, int64_t n_tgt,
                                      const double* T, double max_distance, double* fitness, double* inlier_rmse,
                                      int64_t* count, int32_t* corr_out) try {
  return evaluate_registration(device, P_src, n_src, P_tgt, n_tgt, T, max_distance, fitness, inlier_rmse, count, corr_out);
} CLIPPER_HIP_GUARD_INT

// ---- RANSAC over putative associations (host_ransac.hpp) ------------------------------------------

int clipper_hip_ransac_correspondences(int device, const double* D1, int64_t n1, const double* D2, int64_t n2,
                                       const int32_t* A, int64_t m, const clipper_ransac_params_t* params,
                                       double* T_out, uint8_t* inlier_out, clipper_ransac_info_t* info) try {
  return ransac_correspondences(device, D1, n1, D2, n2, A, m, params, T_out, inlier_out, info);
} CLIPPER_HIP_GUARD_INT

int64_t clipper_hip_ransac_needed(int64_t count, int64_t m, int32_t n_sample, double confidence) try {
  if (m < 1 || count < 0 || count > m || n_sample < RANSAC_MIN_SAMPLE || n_sample > RANSAC_MAX_SAMPLE ||
      !(confidence > 0.0 && confidence < 1.0))
    return fail(CLIPPER_HIP_E_INVALID, "ransac_needed: count in 0..m, m >= 1, n_sample in 3..8 and confidence in (0, 1) are needed");
  return ransac_needed(count, m, n_sample, confidence);
} CLIPPER_HIP_GUARD_INT

// ---- voxel down-sampling of a point cloud (host_voxel.hpp) --------------------------------------

int clipper_hip_voxel_downsample(int device, const double* P, const double* N, int64_t n, double voxel_size,
                                 double* P_out, double* N_out, int32_t* count_out, int32_t* trace_out, int64_t* n_out,
                                 clipper_voxel_info_t* info) try {
  return voxel_downsample(device, P, N, n, voxel_size, P_out, N_out, count_out, trace_out, n_out, info);
} CLIPPER_HIP_GUARD_INT

// ---- clouds and association lists that live on the device (host_cloud.hpp) ------------------------

int clipper_hip_cloud_create(int device, const double* P, const double* N, int64_t n, clipper_hip_cloud_t** out) try {
  return cloud_create(device, P, N, n, out);
} CLIPPER_HIP_GUARD_INT

void clipper_hip_cloud_destroy(clipper_hip_cloud_t* cloud) try {
  delete cloud;
} CLIPPER_HIP_GUARD_VOID

int64_t clipper_hip_cloud_count(const clipper_hip_cloud_t* cloud) try {
  if (!cloud) return fail(CLIPPER_HIP_E_INVALID, "cloud_count: null handle");
  return cloud->n;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_download(const clipper_hip_cloud_t* cloud, int what, void* out) try {
  return cloud_download(cloud, what, out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_info(const clipper_hip_cloud_t* cloud, clipper_hip_cloud_info_t* out) try {
  return cloud_info(cloud, out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_set_descriptors(clipper_hip_cloud_t* cloud, const double* F, int d) try {
  return cloud_set_descriptors(cloud, F, d);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_pairs_create(int device, const int32_t* A, const double* sqd, int64_t m, clipper_hip_pairs_t** out) try {
  return pairs_create(device, A, sqd, m, out);
} CLIPPER_HIP_GUARD_INT

void clipper_hip_pairs_destroy(clipper_hip_pairs_t* pairs) try {
  delete pairs;
} CLIPPER_HIP_GUARD_VOID

int64_t clipper_hip_pairs_count(const clipper_hip_pairs_t* pairs) try {
  if (!pairs) return fail(CLIPPER_HIP_E_INVALID, "pairs_count: null handle");
  return pairs->m;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_pairs_has_sqd(const clipper_hip_pairs_t* pairs) try {
  if (!pairs) return fail(CLIPPER_HIP_E_INVALID, "pairs_has_sqd: null handle");
  return pairs->sqd ? 1 : 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_pairs_download(const clipper_hip_pairs_t* pairs, int32_t* A_out, double* sqd_out) try {
  return pairs_download(pairs, A_out, sqd_out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_voxel_downsample(clipper_hip_cloud_t* in, double voxel_size, int want_trace,
                                       clipper_hip_cloud_t** out, clipper_voxel_info_t* info) try {
  return cloud_voxel_downsample(in, voxel_size, want_trace, out, info);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_estimate_normals(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* nb, const double* viewpoint) try {
  return cloud_features(cloud, "cloud_estimate_normals", nb, viewpoint, nullptr, true, false);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_compute_fpfh(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* nb) try {
  return cloud_features(cloud, "cloud_compute_fpfh", nullptr, nullptr, nb, false, true);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_fpfh_from_points(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* normal_nb,
                                       const double* viewpoint, const clipper_neighborhood_t* feature_nb) try {
  return cloud_features(cloud, "cloud_fpfh_from_points", normal_nb, viewpoint, feature_nb, true, true);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_estimate_covariances(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* nb, double epsilon) try {
  return cloud_estimate_covariances(cloud, nb, epsilon);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_match(const clipper_hip_cloud_t* c0, const clipper_hip_cloud_t* c1, const clipper_match_params_t* params,
                            clipper_hip_pairs_t** out, int32_t* nn_idx_out, double* nn_sqd_out) try {
  return cloud_match(c0, c1, params, out, nn_idx_out, nn_sqd_out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_stage_inputs_clouds(clipper_hip_t* h, const clipper_hip_cloud_t* c0, const clipper_hip_cloud_t* c1,
                                    const clipper_hip_pairs_t* pairs, int with_normals) try {
  return stage_inputs_clouds(h, c0, c1, pairs, with_normals);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_gather_points(const clipper_hip_cloud_t* cloud, const int32_t* idx, int64_t k, double* out) try {
  return cloud_gather_points(cloud, idx, k, out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_icp(const clipper_hip_cloud_t* src, clipper_hip_cloud_t* tgt, const double* T_init,
                          const clipper_icp_params_t* params, const clipper_icp_robust_t* robust, double* T_out,
                          clipper_icp_info_t* info, clipper_icp_robust_info_t* robust_info, double* history) try {
  return cloud_icp(src, tgt, T_init, params, robust, T_out, info, robust_info, history);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_cloud_evaluate_registration(const clipper_hip_cloud_t* src, clipper_hip_cloud_t* tgt, const double* T,
                                            double max_distance, double* fitness, double* inlier_rmse, int64_t* count,
                                            int32_t* corr_out) try {
  return cloud_evaluate_registration(src, tgt, T, max_distance, fitness, inlier_rmse, count, corr_out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_set_window(clipper_hip_t* h, int window) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (window != 0 && window != 1 && window != 4 && window != 6 && window != 8)
    return fail(CLIPPER_HIP_E_INVALID, "window must be 0 (automatic), 1, 4, 6 or 8");
  h->V_forced = window;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_window(const clipper_hip_t* h) try {
  return h ? h->V : 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_set_resident(clipper_hip_t* h, int mode) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (mode != 0 && mode != 1 && mode != 2)
    return fail(CLIPPER_HIP_E_INVALID, "mode must be 0 (automatic), 1 (never) or 2 (the sub-problem always as slices)");
  h->resident_mode = mode;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_last_solver(const clipper_hip_t* h) try {
  return h ? h->last_solver : -1;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_set_row_view(clipper_hip_t* h, int mode) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (mode != 0 && mode != 1 && mode != 2)
    return fail(CLIPPER_HIP_E_INVALID, "mode must be 0 (automatic), 1 (never) or 2 (views, but streamed: never the resident solver on one)");
  h->rv_mode = mode;
  if (mode == 1) rowview_drop(h);
  if (mode != 0) h->vres.ready = false;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_set_subproblem(clipper_hip_t* h, int mode) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (mode != 0 && mode != 1 && mode != 2)
    return fail(CLIPPER_HIP_E_INVALID, "mode must be 0 (automatic), 1 (never) or 2 (the sub-problem always as slices)");
  h->sub_mode = mode;
  if (mode == 1) h->sub.ready = false;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_get_view_stats(const clipper_hip_t* h, clipper_hip_view_stats_t* out) try {
  if (!h || !out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  *out = h->rv_stats;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_storage_in_use(const clipper_hip_t* h) try {
  if (!h) return -1;
  if (!h->csc_valid) return h->storage;
  return h->storage == CLIPPER_HIP_STORE_F64 ? CLIPPER_HIP_STORE_F64_CSC : CLIPPER_HIP_STORE_F32_CSC;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_matvec(clipper_hip_t* h, const double* x, double* yM, double* yC) try {
  if (!h || !x) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return matvec(h, x, yM, yC);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_view_matvec(clipper_hip_t* h, const int32_t* rows, int64_t nrows, const double* x,
                            double* yM, double* yC) try {
  if (!h || !rows || !x || nrows < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return view_matvec(h, rows, nrows, x, yM, yC);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_sub_select(clipper_hip_t* h, const int32_t* rows, int64_t nrows, double s, int64_t capacity,
                                 int32_t* cnt, uint8_t* flags, int32_t* colmap, int32_t* pos,
                                 clipper_hip_sub_selection_t* out) try {
  if (!h || !rows || nrows < 1 || !out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return sub_select_rows(h, rows, nrows, s, capacity, cnt, flags, colmap, pos, out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_sub_last(clipper_hip_t* h, int64_t capacity, int32_t* cnt, uint8_t* flags, int32_t* colmap,
                               int32_t* pos, int32_t* rows, clipper_hip_sub_selection_t* out) try {
  if (!h || !out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return sub_last_selection(h, capacity, cnt, flags, colmap, pos, rows, out);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_sub_min_m(long long min_m) try {
  return debug_sub_min_m(min_m);
} CLIPPER_HIP_GUARD_INT

// ---- measurement ---------------------------------------------------------------------------

int clipper_hip_set_profiling(clipper_hip_t* h, int on) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  h->profiling = (on != 0);
  h->profiling_level = on;  // 2: also an event pair around every launch of the resident solver on a view
  if (h->profiling && h->ev_pairs.empty()) {  // here, not inside the first profiled solve (~1 ms)
    HIPCHK(hipSetDevice(h->sh[0].device));
    h->ev_pairs.resize(2 * MAX_EVENT_PAIRS);
    h->ev_launch_index.assign(MAX_EVENT_PAIRS, 0);
    for (auto& e : h->ev_pairs) HIPCHK(e.create());
    h->ev_xchg.resize(2 * MAX_EVENT_PAIRS);
    h->ev_xchg_used.assign(MAX_EVENT_PAIRS, 0);
    for (auto& e : h->ev_xchg) HIPCHK(e.create());
  }
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_get_timings(const clipper_hip_t* h, clipper_hip_timings_t* out) try {
  if (!h || !out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  *out = h->tm;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_bench_matvec(clipper_hip_t* h, int reps, double* avg_us) try {
  if (!h || reps < 1 || !avg_us) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return bench_matvec(h, reps, avg_us);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_stamps(clipper_hip_t* h, int64_t* out, int capacity) try {
  if (!h || !out || capacity < 0) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (!h->stamps_dev) return fail(CLIPPER_HIP_E_STATE, "CLIPPER_HIP_STAMPS was not set when the context was created");
  const int n = std::min(capacity, h->stamps_rows * 4);
  HIPCHK(hipSetDevice(h->sh[0].device));
  HIPCHK(hipStreamSynchronize(h->sh[0].stream));
  HIPCHK(hipMemcpy(out, h->stamps_dev, static_cast<size_t>(n) * sizeof(long long), hipMemcpyDeviceToHost));
  return n;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_occupy(int device, int workgroups, int lds_bytes, double milliseconds) try {
  if (workgroups < 1 || lds_bytes < 0 || lds_bytes > static_cast<int>(RS_LDS_MAX) || !(milliseconds >= 0.0) || milliseconds > 2000.0)
    return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return debug_occupy(device, workgroups, lds_bytes, milliseconds);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_debug_live_resources(int64_t out[5]) try {
  if (!out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  const clipper_hip_buf::LiveCounts& c = clipper_hip_buf::live();
  out[0] = c.dev_bufs, out[1] = c.dev_bytes, out[2] = c.pinned_bufs, out[3] = c.events, out[4] = c.allocs;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_device_info(const clipper_hip_t* h, char* name64, int* cus, int64_t* hbm_bytes) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, h->sh[0].device));
  if (name64) {
    std::snprintf(name64, 64, "%s (%s)", prop.name, prop.gcnArchName);
  }
  if (cus) *cus = prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = static_cast<int64_t>(prop.totalGlobalMem);
  return 0;
} CLIPPER_HIP_GUARD_INT

// ---- batched solves (host_batchsolve.hpp) --------------------------------------------------------------------------

int clipper_hip_batch_create(int device, int storage, clipper_hip_batch_t** out) try {
  if (!out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  *out = nullptr;
  if (int rc = use_device(device)) return rc;
  if (storage != CLIPPER_HIP_STORE_F32 && storage != CLIPPER_HIP_STORE_F64 && storage != CLIPPER_HIP_STORE_F32_CSC &&
      storage != CLIPPER_HIP_STORE_F64_CSC)
    return fail(CLIPPER_HIP_E_INVALID, "storage must be CLIPPER_HIP_STORE_F32, _F64, _F32_CSC or _F64_CSC");
  clipper_hip_batch_t* b = new clipper_hip_batch_t();
  b->device = device;
  b->storage = storage;
  if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
    delete b;
    return fail(CLIPPER_HIP_E_HIP, "cannot create a stream on device %d", device);
  }
  *out = b;
  return 0;
} CLIPPER_HIP_GUARD_INT

void clipper_hip_batch_destroy(clipper_hip_batch_t* b) try {
  if (!b) return;
  hipSetDevice(b->device);
  if (b->stream) hipStreamSynchronize(b->stream);
  for (Ctx* c : b->kids) destroy_ctx(c);  // (they borrow the batch's stream: it goes last)
  const hipStream_t st = b->stream;
  delete b;  // its staging buffers and events
  if (st) hipStreamDestroy(st);
} CLIPPER_HIP_GUARD_VOID

int clipper_hip_batch_solve_euclidean(clipper_hip_batch_t* b, const clipper_batch_problem_t* p, int32_t n, int d,
                                      double sigma, double epsilon, double mindist, const clipper_params_t* prm) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  const double f[3] = {sigma, epsilon, mindist};
  return batch_solve(b, p, n, d, 1, f, prm);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_solve_pointnormal(clipper_hip_batch_t* b, const clipper_batch_problem_t* p, int32_t n,
                                        double sigp, double epsp, double sign, double epsn,
                                        const clipper_params_t* prm) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  const double f[4] = {sigp, epsp, sign, epsn};
  return batch_solve(b, p, n, 6, 2, f, prm);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_solve_custom(clipper_hip_batch_t* b, const clipper_hip_invariant_t* inv,
                                   const clipper_batch_problem_t* p, int32_t n, const double* params, int nparams,
                                   const clipper_params_t* prm) try {
  CustomFill f;  // (inv and nparams first, as clipper_hip_affinity_custom checks them)
  if (int rc = custom_fill_args(inv, params, nparams, prm ? prm->affinityeps : 0.0, f)) return rc;
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return batch_solve(b, p, n, inv->d, 3, nullptr, prm, &f);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_get_solution(const clipper_hip_batch_t* b, int32_t i, double* u_out,
                                   clipper_solve_info_t* info) try {
  if (!b || i < 0 || static_cast<size_t>(i) >= b->res.size())
    return fail(CLIPPER_HIP_E_INVALID, "no problem %d in the last batch", i);
  const auto& R = b->res[static_cast<size_t>(i)];
  if (u_out && !R.u.empty()) std::memcpy(u_out, R.u.data(), R.u.size() * sizeof(double));
  if (info) *info = R.info;
  return static_cast<int>(R.u.size());
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_get_nodes(const clipper_hip_batch_t* b, int32_t i, int32_t* nodes_out, int32_t capacity) try {
  if (!b || !nodes_out || i < 0 || static_cast<size_t>(i) >= b->res.size())
    return fail(CLIPPER_HIP_E_INVALID, "invalid argument (problem %d)", i);
  const auto& nodes = b->res[static_cast<size_t>(i)].nodes;
  const int32_t k = static_cast<int32_t>(nodes.size());
  if (capacity < k) return fail(CLIPPER_HIP_E_INVALID, "capacity %d < %d nodes", capacity, k);
  if (k) std::memcpy(nodes_out, nodes.data(), static_cast<size_t>(k) * sizeof(int32_t));
  return k;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_get_selected_associations(const clipper_hip_batch_t* b, int32_t i, int32_t* A_out,
                                                int32_t capacity) try {
  if (!b || !A_out || i < 0 || static_cast<size_t>(i) >= b->res.size())
    return fail(CLIPPER_HIP_E_INVALID, "invalid argument (problem %d)", i);
  const auto& sel = b->res[static_cast<size_t>(i)].sel;
  const int32_t k = static_cast<int32_t>(sel.size() / 2);
  if (capacity < k) return fail(CLIPPER_HIP_E_INVALID, "capacity %d < %d nodes", capacity, k);
  if (k) std::memcpy(A_out, sel.data(), sel.size() * sizeof(int32_t));
  return k;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_sdp(clipper_hip_batch_t* b, const clipper_sdp_params_t* params, clipper_sdp_info_t* infos) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return batch_sdp(b, params, infos);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_get_sdp(const clipper_hip_batch_t* b, int32_t i, double* X_out, double* Y_out,
                              double* lambdas_out, double* evec1_out) try {
  if (!b || !b->sdp) return fail(CLIPPER_HIP_E_STATE, "sdp: no relaxation of this batch is held");
  if (i < 0 || static_cast<size_t>(i) >= b->sdp->count())
    return fail(CLIPPER_HIP_E_INVALID, "no problem %d in the last relaxation of the batch", i);
  if (int rc = sdp_batch_outputs(*b->sdp, static_cast<size_t>(i), X_out, Y_out, lambdas_out, evec1_out)) return rc;
  return b->sdp->n[static_cast<size_t>(i)];
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_max_clique(clipper_hip_batch_t* b, int method, double time_limit_s,
                                 clipper_maxclique_info_t* infos) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return batch_max_clique(b, method, time_limit_s, infos);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_max_clique_seeded(clipper_hip_batch_t* b, int method, double time_limit_s, const int32_t* seeds,
                                        const int64_t* offsets, clipper_maxclique_info_t* infos,
                                        clipper_maxclique_seed_info_t* seed_infos) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return batch_max_clique(b, method, time_limit_s, infos, true, seeds, offsets, seed_infos);
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_max_clique_stats(const clipper_hip_batch_t* b, int32_t* launches, int32_t* n_batched,
                                       int32_t* n_alone) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (launches) *launches = b->mc_launches;
  if (n_batched) *n_batched = b->mc_batched;
  if (n_alone) *n_alone = b->mc_alone;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_route(const clipper_hip_batch_t* b, int32_t i) try {
  if (!b || i < 0 || static_cast<size_t>(i) >= b->res.size())
    return fail(CLIPPER_HIP_E_INVALID, "no problem %d in the last batch", i);
  return b->res[static_cast<size_t>(i)].route;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_get_stats(const clipper_hip_batch_t* b, int32_t* launches, int32_t* n_batched,
                                int32_t* n_alone) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (launches) *launches = b->launches;
  if (n_batched) *n_batched = b->n_batched;
  if (n_alone) *n_alone = b->n_alone;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_batch_get_split(const clipper_hip_batch_t* b, double* fill_ms, double* launch_ms, double* alone_ms,
                                double* round_ms) try {
  if (!b) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (fill_ms) *fill_ms = b->t_fill;
  if (launch_ms) *launch_ms = b->t_launch;
  if (alone_ms) *alone_ms = b->t_alone;
  if (round_ms) *round_ms = b->t_round;
  return 0;
} CLIPPER_HIP_GUARD_INT

}  // extern "C"
