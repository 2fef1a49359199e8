// clipper_hip.hip — the C ABI declared in include/clipper_hip.h. One translation unit: host_state.hpp (context, shards,
// RCCL binding), host_solver.hpp (planning, dispatch, one iteration), host_matrix.hpp (compressed copy, affinity fills),
// host_solve.hpp (the solve of one context) and the other host_*.hpp, then the extern "C" entry points, which check
// their arguments and call the internal functions. All arithmetic runs in the kernels of kernels.hip.h; there is no
// CPU fallback anywhere: if HIP is unusable the entry points return an error.
#include <hip/hip_runtime.h>
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
#include <mutex>
#include <new>
#include <exception>
#include <vector>

#include "../../include/clipper_hip.h"
#include "kernels.hip.h"
#include "dsd_host.h"
#include "host_batch.hpp"
#include "host_plan.hpp"

using namespace clipper_hip;

#include "host_state.hpp"
#include "host_solver.hpp"
#include "host_matrix.hpp"
#include "host_rowview.hpp"
#include "host_resident.hpp"
#include "host_rv_resident.hpp"
#include "host_subproblem.hpp"
#include "host_registration.hpp"
#include "host_maxclique.hpp"
#include "host_solve.hpp"
#include "host_batchsolve.hpp"

// ============================================================================================
// brute-force nearest neighbours: launch of the two kernels for one (K, D)
namespace {

template <int K, int D>
int knn_run(const double* dP0, int64_t n0, const double* dP1, int64_t n1, int S, int64_t chunk,
            double* pd, int32_t* pi, double* od, int32_t* oi, hipStream_t st) {
  dim3 g(static_cast<unsigned>(ceil_div(n0, 256)), static_cast<unsigned>(S));
  hipLaunchKernelGGL((k_knn_partial<K, D>), g, dim3(256), 0, st, dP0, n0, dP1, n1, chunk, pd, pi);
  hipLaunchKernelGGL((k_knn_merge<K>), dim3(static_cast<unsigned>(ceil_div(n0, 256))), dim3(256), 0,
                     st, pd, pi, n0, S, od, oi);
  return 0;
}


// The two fills (declared in host_matrix.hpp): defined here, behind the batch, the fill kernels keep their place in the
// code object.
// EuclideanDistance over the staged points: the matrix of this context
int fill_euclidean(Ctx* h, const EuclidParams& prm) {
  if (h->staged_d < 1) return fail(CLIPPER_HIP_E_STATE, "clipper_hip_stage_inputs not called");
  const int64_t mm = h->m, W = h->W, pstride = h->staged_pstride;
  const int d = h->staged_d;
  h->fill_kind = 1;  // what a row view of this matrix is filled with later (host_rowview.hpp)
  h->fill_e = prm;
  h->fill_n = PointNormalParams{};
  h->fill_E2 = guarded_threshold_sq(guarded_threshold(prm.epsilon, h->staged_maxabs, d));
  return run_affinity(h, use_sym_fill(h) && (d == 2 || d == 3), [&](Shard& s) {
    dim3 grid(static_cast<unsigned>(ceil_div(W, 1024)),
              static_cast<unsigned>(ceil_div(mm, AFF_ROWS_PER_BLK))),
        block(256);
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    const int32_t* A0 = s.Adev;
    const int32_t* A1 = s.Adev + mm;
#define LAUNCH_EUCLID(T, D)                                                                 \
  hipLaunchKernelGGL((k_affinity_euclid<T, D>), grid, block, 0, s.stream,                   \
                     static_cast<T*>(s.S), W, mm, c0, AFF_ROWS_PER_BLK, d, s.P1, s.P2, pstride, \
                     A0, A1, prm)
#define LAUNCH_EUCLID_COMPACT(T, D)                                                         \
  hipLaunchKernelGGL((k_affinity_euclid_compact<T, D>), grid, block, 0, s.stream,           \
                     static_cast<T*>(s.S), W, mm, c0, AFF_ROWS_PER_BLK, s.P1, s.P2, s.P1f,  \
                     s.P2f, pstride, A0, A1, prm, thr)
    const float thr = guarded_threshold(prm.epsilon, h->staged_maxabs, d);
    if (use_sym_fill(h) && (d == 2 || d == 3)) {
      const int nT = static_cast<int>(ceil_div(mm, AT));
      dim3 g(static_cast<unsigned>(static_cast<int64_t>(nT) * (nT + 1) / 2));
      const PointNormalParams none{};
      const float E2 = guarded_threshold_sq(thr);
      if (h->storage == CLIPPER_HIP_STORE_F64) {  // (slices with fp64 values: no dense store on this route)
        if (d == 3)
          launch_sym<double>(k_affinity_sym<3, false, double>, g, s.stream, static_cast<double*>(nullptr), W, mm, nT, s,
                             pstride, A0, A1, prm, none, E2, h->csc_out);
        else
          launch_sym<double>(k_affinity_sym<2, false, double>, g, s.stream, static_cast<double*>(nullptr), W, mm, nT, s,
                             pstride, A0, A1, prm, none, E2, h->csc_out);
      } else if (d == 3)
        launch_sym<float>(k_affinity_sym<3, false>, g, s.stream, static_cast<float*>(s.S), W, mm, nT, s,
                          pstride, A0, A1, prm, none, E2, h->csc_out);
      else
        launch_sym<float>(k_affinity_sym<2, false>, g, s.stream, static_cast<float*>(s.S), W, mm, nT, s,
                          pstride, A0, A1, prm, none, E2, h->csc_out);
      h->csc_emitted = (h->csc_out.Pre != nullptr);
      return;
    }
    const bool compact = !h->plain_affinity && (d == 2 || d == 3);
    if (h->storage == CLIPPER_HIP_STORE_F64) {
      if (compact && d == 3) LAUNCH_EUCLID_COMPACT(double, 3);
      else if (compact && d == 2) LAUNCH_EUCLID_COMPACT(double, 2);
      else if (d == 3) LAUNCH_EUCLID(double, 3);
      else if (d == 2) LAUNCH_EUCLID(double, 2);
      else LAUNCH_EUCLID(double, 0);
    } else {
      if (compact && d == 3) LAUNCH_EUCLID_COMPACT(float, 3);
      else if (compact && d == 2) LAUNCH_EUCLID_COMPACT(float, 2);
      else if (d == 3) LAUNCH_EUCLID(float, 3);
      else if (d == 2) LAUNCH_EUCLID(float, 2);
      else LAUNCH_EUCLID(float, 0);
    }
#undef LAUNCH_EUCLID_COMPACT
#undef LAUNCH_EUCLID
  });
}


// PointNormalDistance over the staged points: the matrix of this context
int fill_pointnormal(Ctx* h, const PointNormalParams& prm) {
  if (h->staged_d != 6)
    return fail(CLIPPER_HIP_E_STATE, "PointNormalDistance needs staged inputs with d == 6");
  const int64_t mm = h->m, W = h->W, pstride = h->staged_pstride;
  h->fill_kind = 2;
  h->fill_e = EuclidParams{};
  h->fill_n = prm;
  h->fill_E2 = guarded_threshold_sq(guarded_threshold(prm.epsp, h->staged_maxabs, 3));
  return run_affinity(h, use_sym_fill(h), [&](Shard& s) {
    dim3 grid(static_cast<unsigned>(ceil_div(W, 1024)),
              static_cast<unsigned>(ceil_div(mm, AFF_ROWS_PER_BLK))),
        block(256);
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    const float thr = guarded_threshold(prm.epsp, h->staged_maxabs, 3);
    if (use_sym_fill(h)) {
      const int nT = static_cast<int>(ceil_div(mm, AT));
      dim3 g(static_cast<unsigned>(static_cast<int64_t>(nT) * (nT + 1) / 2));
      const EuclidParams none{};
      if (h->storage == CLIPPER_HIP_STORE_F64)
        launch_sym<double>(k_affinity_sym<3, true, double>, g, s.stream, static_cast<double*>(nullptr), W, mm, nT, s,
                           pstride, s.Adev, s.Adev + mm, none, prm, guarded_threshold_sq(thr), h->csc_out);
      else
        launch_sym<float>(k_affinity_sym<3, true>, g, s.stream, static_cast<float*>(s.S), W, mm, nT, s,
                          pstride, s.Adev, s.Adev + mm, none, prm, guarded_threshold_sq(thr), h->csc_out);
      h->csc_emitted = (h->csc_out.Pre != nullptr);
      return;
    }
    if (h->plain_affinity) {
      if (h->storage == CLIPPER_HIP_STORE_F64)
        hipLaunchKernelGGL((k_affinity_pointnormal<double>), grid, block, 0, s.stream,
                           static_cast<double*>(s.S), W, mm, c0, AFF_ROWS_PER_BLK, s.P1, s.P2,
                           pstride, s.Adev, s.Adev + mm, prm);
      else
        hipLaunchKernelGGL((k_affinity_pointnormal<float>), grid, block, 0, s.stream,
                           static_cast<float*>(s.S), W, mm, c0, AFF_ROWS_PER_BLK, s.P1, s.P2,
                           pstride, s.Adev, s.Adev + mm, prm);
    } else {
      if (h->storage == CLIPPER_HIP_STORE_F64)
        hipLaunchKernelGGL((k_affinity_pointnormal_compact<double>), grid, block, 0, s.stream,
                           static_cast<double*>(s.S), W, mm, c0, AFF_ROWS_PER_BLK, s.P1, s.P2,
                           s.P1f, s.P2f, pstride, s.Adev, s.Adev + mm, prm, thr);
      else
        hipLaunchKernelGGL((k_affinity_pointnormal_compact<float>), grid, block, 0, s.stream,
                           static_cast<float*>(s.S), W, mm, c0, AFF_ROWS_PER_BLK, s.P1, s.P2,
                           s.P1f, s.P2f, pstride, s.Adev, s.Adev + mm, prm, thr);
    }
  });
}

}  // namespace

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
  if (h->A.size() != static_cast<size_t>(2 * m)) h->A.clear();
  h->nodes.clear();
  h->has_matrix = false;  // until the new matrix is complete
  h->csc_valid = false;
  h->fill_kind = 0;  // no points behind this matrix: no row view
  rowview_drop(h);
  int rc = ensure_problem(h, m);
  if (rc) return rc;
  h->has_matrix = false;
  h->csc_valid = false;
  if ((rc = ensure_dense(h, false))) return rc;
  const size_t bytes = static_cast<size_t>(m) * m * sizeof(double);
  const int64_t W = h->W;
  // device temporaries of this call, released on every path
  struct Temps {
    std::vector<std::pair<int, void*>> v;
    ~Temps() {
      for (auto& p : v) {
        hipSetDevice(p.first);
        hipFree(p.second);
      }
    }
    int alloc(int dev, void** p, size_t n) {
      HIPCHK(hipMalloc(p, n));
      v.emplace_back(dev, *p);
      return 0;
    }
  } tmp;
  // pass 1: fill S and detect whether C is anything other than pattern(M)
  std::vector<double*> dM(h->sh.size(), nullptr), dC(h->sh.size(), nullptr);
  std::vector<int*> dflag(h->sh.size(), nullptr);
  int mismatch = 0;
  const unsigned gy = static_cast<unsigned>(std::min<int64_t>(m, 65535));
  for (size_t k = 0; k < h->sh.size(); ++k) {
    Shard& s = h->sh[k];
    HIPCHK(hipSetDevice(s.device));
    if ((rc = tmp.alloc(s.device, reinterpret_cast<void**>(&dM[k]), bytes))) return rc;
    if ((rc = tmp.alloc(s.device, reinterpret_cast<void**>(&dC[k]), bytes))) return rc;
    if ((rc = tmp.alloc(s.device, reinterpret_cast<void**>(&dflag[k]), sizeof(int)))) return rc;
    HIPCHK(hipMemsetAsync(dflag[k], 0, sizeof(int), s.stream));
    HIPCHK(hipMemcpyAsync(dM[k], M, bytes, hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(dC[k], C, bytes, hipMemcpyHostToDevice, s.stream));
    if (s.Cs) {
      hipFree(s.Cs);
      s.Cs = nullptr;
    }
    dim3 grid(static_cast<unsigned>(ceil_div(W, 256)), gy), block(256);
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    if (h->storage == CLIPPER_HIP_STORE_F64)
      hipLaunchKernelGGL((k_from_dense_upper<double>), grid, block, 0, s.stream,
                         static_cast<double*>(s.S), W, m, c0, dM[k], dC[k],
                         static_cast<double*>(nullptr), dflag[k]);
    else
      hipLaunchKernelGGL((k_from_dense_upper<float>), grid, block, 0, s.stream,
                         static_cast<float*>(s.S), W, m, c0, dM[k], dC[k],
                         static_cast<float*>(nullptr), dflag[k]);
    int f = 0;
    HIPCHK(hipMemcpyAsync(&f, dflag[k], sizeof(int), hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipGetLastError());
    mismatch |= f;
  }
  // NOTE: in multi-process mode every rank sees the whole (M, C), so `mismatch` agrees.
  // The full upper triangle must be inspected, not only owned columns: do it on the host
  // cheaply when sharded (owned columns cover all (lo,hi) pairs with hi or lo owned only).
  if (h->world > 1 && !mismatch) {
    for (int64_t hi = 1; hi < m && !mismatch; ++hi)
      for (int64_t lo = 0; lo < hi; ++lo) {
        const double mv = M[lo + hi * m], cv = C[lo + hi * m];
        if (cv != ((mv != 0.0) ? 1.0 : 0.0)) {
          mismatch = 1;
          break;
        }
      }
  }
  h->explicitC = (mismatch != 0);
  plan_tiles(h);
  if (h->explicitC) {
    for (size_t k = 0; k < h->sh.size(); ++k) {
      Shard& s = h->sh[k];
      HIPCHK(hipSetDevice(s.device));
      HIPCHK(hipMalloc(&s.Cs, s.bytes_S));
      dim3 grid(static_cast<unsigned>(ceil_div(W, 256)), gy), block(256);
      const int64_t c0 = static_cast<int64_t>(s.slot) * W;
      if (h->storage == CLIPPER_HIP_STORE_F64)
        hipLaunchKernelGGL((k_from_dense_upper<double>), grid, block, 0, s.stream,
                           static_cast<double*>(s.S), W, m, c0, dM[k], dC[k],
                           static_cast<double*>(s.Cs), static_cast<int*>(nullptr));
      else
        hipLaunchKernelGGL((k_from_dense_upper<float>), grid, block, 0, s.stream,
                           static_cast<float*>(s.S), W, m, c0, dM[k], dC[k],
                           static_cast<float*>(s.Cs), static_cast<int*>(nullptr));
    }
  }
  if ((rc = sync_all(h))) return rc;
  if ((rc = csc_rebuild(h))) return rc;
  h->has_matrix = true;
  return 0;
} CLIPPER_HIP_GUARD_INT

// setSparseMatrixData (clipper.cpp:162-166). Every stored (i, j) with i < j stands for the symmetric
// pair, as selfadjointView<Upper> reads it; entries below the diagonal are not read (the reference
// never does); the diagonal is implicit. With compressed storage and C == pattern(M) the slices
// are packed straight from the lists (no dense intermediate: O(nnz) memory); otherwise through the
// dense store.
int clipper_hip_set_sparse(clipper_hip_t* h, int64_t m, const int64_t* Mcolptr,
                           const int32_t* Mrow, const double* Mval, const int64_t* Ccolptr,
                           const int32_t* Crow, const double* Cval) try {
  if (!h || !Mcolptr || !Ccolptr || m < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  // the caller's arrays are not trusted: structure first
  auto check_csc = [&](const char* what, const int64_t* cp, const int32_t* ri, const double* va) -> int {
    if (cp[0] != 0) return fail(CLIPPER_HIP_E_INVALID, "%s: colptr[0] must be 0", what);
    for (int64_t c = 0; c < m; ++c)
      if (cp[c + 1] < cp[c]) return fail(CLIPPER_HIP_E_INVALID, "%s: colptr decreases at column %lld", what, static_cast<long long>(c));
    const int64_t nnz = cp[m];
    if (nnz > 0 && (!ri || !va)) return fail(CLIPPER_HIP_E_INVALID, "%s: null CSC arrays", what);
    for (int64_t p = 0; p < nnz; ++p)
      if (ri[p] < 0 || ri[p] >= m)
        return fail(CLIPPER_HIP_E_INVALID, "%s: row index %d out of range at entry %lld", what, ri[p], static_cast<long long>(p));
    return 0;
  };
  int rc;
  if ((rc = check_csc("M", Mcolptr, Mrow, Mval))) return rc;
  if ((rc = check_csc("C", Ccolptr, Crow, Cval))) return rc;
  // The reference keeps what it is handed (clipper.cpp:162-166) and reads it through
  // selfadjointView<Eigen::Upper> (clipper.cpp:194-271): an entry BELOW the diagonal is never read — a
  // full symmetric SpAffinity counts through its upper half, a lower-triangular one is an empty matrix —
  // and a stored diagonal would count once on top of the implicit identity. Same here for the lower
  // triangle (dropped, whatever it holds); the diagonal is implicit in every storage of this library, so a
  // stored non-zero diagonal — outside the reference's own contract, clipper.h:137-138 — is refused
  // rather than silently dropped.
  struct Csc {
    std::vector<int64_t> cp;
    std::vector<int32_t> ri;
    std::vector<double> va;
  } Mn, Cn;
  int64_t dropped_below = 0;  // entries below the diagonal, which the reference never reads: dropped, and reported
  auto upper_only = [&](const char* what, const int64_t*& cp, const int32_t*& ri, const double*& va, Csc& out) -> int {
    bool strict = true;
    for (int64_t j = 0; j < m && strict; ++j)
      for (int64_t p = cp[j]; p < cp[j + 1]; ++p)
        if (ri[p] >= j) {
          strict = false;
          break;
        }
    if (strict) return 0;  // (what Eigen hands over from a strictly upper matrix: nothing to copy)
    out.cp.assign(static_cast<size_t>(m) + 1, 0);
    for (int64_t j = 0; j < m; ++j) {
      for (int64_t p = cp[j]; p < cp[j + 1]; ++p) {
        const int64_t i = ri[p];
        if (i > j) {
          ++dropped_below;
          continue;
        }
        if (i == j) {
          if (va[p] != 0.0)
            return fail(CLIPPER_HIP_E_INVALID, "%s: a stored diagonal entry (%lld,%lld) — the matrices must not have diagonal values set",
                        what, static_cast<long long>(i), static_cast<long long>(j));
          continue;
        }
        out.ri.push_back(static_cast<int32_t>(i));
        out.va.push_back(va[p]);
      }
      out.cp[static_cast<size_t>(j) + 1] = static_cast<int64_t>(out.ri.size());
    }
    cp = out.cp.data();
    ri = out.ri.data();
    va = out.va.data();
    return 0;
  };
  if ((rc = upper_only("M", Mcolptr, Mrow, Mval, Mn))) return rc;
  if ((rc = upper_only("C", Ccolptr, Crow, Cval, Cn))) return rc;
  // (a warning, not an error — the call goes on and returns 0 unless something else fails: clipper_hip_last_error()
  // tells a caller who handed over both triangles, or only the lower one, what became of them)
  if (dropped_below > 0)
    (void)fail(0, "warning: %lld stored entries below the diagonal were ignored (the matrices are read through their upper "
                  "triangle, as the reference's selfadjointView<Upper> does: clipper.cpp:194-271)", static_cast<long long>(dropped_below));
  const int64_t nnzM = Mcolptr[m], nnzC = Ccolptr[m];
  if (h->A.size() != static_cast<size_t>(2 * m)) h->A.clear();
  h->nodes.clear();
  h->has_matrix = false;
  h->csc_valid = false;
  h->total_slice_bytes = 0.0;
  h->fill_kind = 0;  // no points behind this matrix: its row views are filtered out of its own slices
  rowview_drop(h);
  if ((rc = ensure_problem(h, m))) return rc;
  h->has_matrix = false;
  h->csc_valid = false;
  // C == pattern(M)?  (same structure, every stored C equal to 1, every stored M non-zero)
  bool pattern = (nnzM == nnzC) && std::equal(Mcolptr, Mcolptr + m + 1, Ccolptr) &&
                 (nnzM == 0 || std::equal(Mrow, Mrow + nnzM, Crow));
  for (int64_t p = 0; pattern && p < nnzM; ++p) pattern = (Cval[p] == 1.0) && (Mval[p] != 0.0);
  h->explicitC = !pattern;
  plan_tiles(h);
  const int64_t W = h->W;
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    if (s.Cs) {
      hipFree(s.Cs);
      s.Cs = nullptr;
    }
  }
  struct Temps {
    std::vector<std::pair<int, void*>> v;
    ~Temps() {
      for (auto& p : v) {
        hipSetDevice(p.first);
        hipFree(p.second);
      }
    }
    int alloc(int dev, void** p, size_t n) {
      HIPCHK(hipMalloc(p, std::max<size_t>(n, 16)));
      v.emplace_back(dev, *p);
      return 0;
    }
  } tmp;

  if (csc_applies(h)) {
    // ---- lists -> slices. Host: the full symmetric lists (both triangles), rows ascending.
    drop_dense(h);
    std::vector<int64_t> cp(static_cast<size_t>(m) + 1, 0);
    for (int64_t j = 0; j < m; ++j)
      for (int64_t p = Mcolptr[j]; p < Mcolptr[j + 1]; ++p) {
        const int64_t i = Mrow[p];
        if (i == j) continue;
        ++cp[static_cast<size_t>(i) + 1];
        ++cp[static_cast<size_t>(j) + 1];
      }
    for (int64_t c = 0; c < m; ++c) cp[static_cast<size_t>(c) + 1] += cp[static_cast<size_t>(c)];
    const int64_t nnz2 = cp[static_cast<size_t>(m)];
    std::vector<int32_t> ri(static_cast<size_t>(nnz2));
    std::vector<double> va(static_cast<size_t>(nnz2));
    {
      std::vector<int64_t> cur(cp.begin(), cp.end() - 1);
      for (int64_t j = 0; j < m; ++j)
        for (int64_t p = Mcolptr[j]; p < Mcolptr[j + 1]; ++p) {
          const int64_t i = Mrow[p];
          if (i == j) continue;
          int64_t& a = cur[static_cast<size_t>(j)];
          ri[static_cast<size_t>(a)] = static_cast<int32_t>(i);
          va[static_cast<size_t>(a)] = Mval[p];
          ++a;
          int64_t& b = cur[static_cast<size_t>(i)];
          ri[static_cast<size_t>(b)] = static_cast<int32_t>(j);
          va[static_cast<size_t>(b)] = Mval[p];
          ++b;
        }
    }
    // strictly-upper input with ascending rows (what Eigen hands over) comes out sorted; anything
    // else is sorted here; an entry given twice (e.g. in both triangles) is an error
    std::vector<std::pair<int32_t, double>> buf;
    for (int64_t c = 0; c < m; ++c) {
      const int64_t a = cp[static_cast<size_t>(c)], b = cp[static_cast<size_t>(c) + 1];
      bool sorted = true;
      for (int64_t p = a + 1; p < b && sorted; ++p) sorted = ri[static_cast<size_t>(p - 1)] < ri[static_cast<size_t>(p)];
      if (sorted) continue;
      buf.clear();
      for (int64_t p = a; p < b; ++p) buf.emplace_back(ri[static_cast<size_t>(p)], va[static_cast<size_t>(p)]);
      std::sort(buf.begin(), buf.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
      for (size_t q = 1; q < buf.size(); ++q)
        if (buf[q - 1].first == buf[q].first)
          return fail(CLIPPER_HIP_E_INVALID, "entry (%d,%lld) is stored more than once", buf[q].first,
                      static_cast<long long>(c));
      for (int64_t p = a; p < b; ++p) {
        ri[static_cast<size_t>(p)] = buf[static_cast<size_t>(p - a)].first;
        va[static_cast<size_t>(p)] = buf[static_cast<size_t>(p - a)].second;
      }
    }
    for (auto& s : h->sh) {
      HIPCHK(hipSetDevice(s.device));
      int64_t* dcp = nullptr;
      int32_t* dri = nullptr;
      double* dva = nullptr;
      if ((rc = tmp.alloc(s.device, reinterpret_cast<void**>(&dcp), cp.size() * sizeof(int64_t)))) return rc;
      if ((rc = tmp.alloc(s.device, reinterpret_cast<void**>(&dri), ri.size() * sizeof(int32_t)))) return rc;
      if ((rc = tmp.alloc(s.device, reinterpret_cast<void**>(&dva), va.size() * sizeof(double)))) return rc;
      HIPCHK(hipMemcpyAsync(dcp, cp.data(), cp.size() * sizeof(int64_t), hipMemcpyHostToDevice, s.stream));
      if (nnz2 > 0) {
        HIPCHK(hipMemcpyAsync(dri, ri.data(), ri.size() * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
        HIPCHK(hipMemcpyAsync(dva, va.data(), va.size() * sizeof(double), hipMemcpyHostToDevice, s.stream));
      }
      const int64_t c0 = static_cast<int64_t>(s.slot) * W;
      dispatch_vt(h, [&](auto t) {
        using VT = decltype(t);
        bool again = true;
        for (int attempt = 0; again && !rc; ++attempt) {
          if (attempt >= 3) {
            rc = fail(CLIPPER_HIP_E_HIP, "compressed storage: the build keeps overflowing");
            break;
          }
          GroupOut<VT> unused;
          if ((rc = groups_prepare<VT>(h, s, unused))) break;  // sizes the per-slice arrays
          CscSource<VT> src{};
          src.colptr = dcp + std::min<int64_t>(c0, m);
          src.rowidx = dri;
          src.values = dva;
          src.ncols = std::max<int64_t>(0, std::min<int64_t>(W, m - c0));
          if ((rc = slices_enqueue<VT>(h, s, src, nullptr))) break;
          if (hipStreamSynchronize(s.stream) != hipSuccess) {
            rc = fail(CLIPPER_HIP_E_HIP, "set_sparse: %s", hipGetErrorString(hipGetLastError()));
            break;
          }
          rc = slices_check<VT>(h, s, false, again);
        }
      });
      if (rc) return rc;
    }
    if ((rc = sync_all(h))) return rc;
    h->csc_valid = true;
    if ((rc = gather_slice_bytes(h))) return rc;  // column shards: the row-view policy's cost model
    h->has_matrix = true;
    return 0;
  }

  // ---- through the dense store (dense storage modes, or an explicit C) ----------------------
  if ((rc = ensure_dense(h, false))) return rc;
  auto scatter = [&](Shard& s, void* dst, const int64_t* cp, const int32_t* ri, const double* va,
                     int64_t nnz) -> int {
    int64_t* dcp = nullptr;
    int32_t* dri = nullptr;
    double* dva = nullptr;
    int r;
    if ((r = tmp.alloc(s.device, reinterpret_cast<void**>(&dcp), static_cast<size_t>(m + 1) * sizeof(int64_t)))) return r;
    if ((r = tmp.alloc(s.device, reinterpret_cast<void**>(&dri), static_cast<size_t>(nnz) * sizeof(int32_t)))) return r;
    if ((r = tmp.alloc(s.device, reinterpret_cast<void**>(&dva), static_cast<size_t>(nnz) * sizeof(double)))) return r;
    HIPCHK(hipMemcpyAsync(dcp, cp, static_cast<size_t>(m + 1) * sizeof(int64_t),
                          hipMemcpyHostToDevice, s.stream));
    if (nnz > 0) {
      HIPCHK(hipMemcpyAsync(dri, ri, static_cast<size_t>(nnz) * sizeof(int32_t),
                            hipMemcpyHostToDevice, s.stream));
      HIPCHK(hipMemcpyAsync(dva, va, static_cast<size_t>(nnz) * sizeof(double),
                            hipMemcpyHostToDevice, s.stream));
    }
    HIPCHK(hipMemsetAsync(dst, 0, s.bytes_S, s.stream));
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    dim3 grid(static_cast<unsigned>(std::min<int64_t>(m, 1 << 20))), block(256);
    if (h->storage == CLIPPER_HIP_STORE_F64)
      hipLaunchKernelGGL((k_from_csc<double>), grid, block, 0, s.stream,
                         static_cast<double*>(dst), W, m, c0, W, dcp, dri, dva);
    else
      hipLaunchKernelGGL((k_from_csc<float>), grid, block, 0, s.stream, static_cast<float*>(dst),
                         W, m, c0, W, dcp, dri, dva);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s.stream));
    return 0;
  };
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    rc = scatter(s, s.S, Mcolptr, Mrow, Mval, nnzM);
    if (rc) return rc;
    if (h->explicitC) {
      HIPCHK(hipMalloc(&s.Cs, s.bytes_S));
      rc = scatter(s, s.Cs, Ccolptr, Crow, Cval, nnzC);
      if (rc) return rc;
    }
  }
  rc = csc_rebuild(h);
  if (rc) return rc;
  h->has_matrix = true;
  return 0;
} CLIPPER_HIP_GUARD_INT

int clipper_hip_get_matrix(clipper_hip_t* h, double* M_out, double* C_out) try {
  if (!h) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (h->multiproc)
    return fail(CLIPPER_HIP_E_STATE, "get_matrix is not available on a multi-process shard");
  const int64_t m = h->m, W = h->W;
  const bool f64 = (h->storage == CLIPPER_HIP_STORE_F64);
  if (int rc = ensure_dense(h, true)) return rc;
  std::vector<unsigned char> buf;
  auto fetch = [&](Shard& s, const void* src, double* out, bool as_pattern) -> int {
    buf.resize(s.bytes_S);
    HIPCHK(hipSetDevice(s.device));
    HIPCHK(hipMemcpy(buf.data(), src, s.bytes_S, hipMemcpyDeviceToHost));
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    for (int64_t c = 0; c < W; ++c) {
      const int64_t g = c0 + c;
      if (g >= m) break;
      for (int64_t j = 0; j < m; ++j) {
        const double v = f64 ? reinterpret_cast<const double*>(buf.data())[j * W + c]
                             : static_cast<double>(
                                   reinterpret_cast<const float*>(buf.data())[j * W + c]);
        double o = as_pattern ? ((v != 0.0) ? 1.0 : 0.0) : v;
        if (j == g) o += 1.0;  // clipper.cpp:133-134, 142-143: identity added
        out[j + g * m] = o;
      }
    }
    return 0;
  };
  for (auto& s : h->sh) {
    int rc;
    if (M_out && (rc = fetch(s, s.S, M_out, false))) return rc;
    if (C_out) {
      rc = h->explicitC ? fetch(s, s.Cs, C_out, false) : fetch(s, s.S, C_out, true);
      if (rc) return rc;
    }
  }
  if (h->csc_valid) drop_dense(h);  // the copy was materialised for this call only: M lives in the slices
  return 0;
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

// utils::selectInlierAssociations — utils.cpp:101-108
int clipper_hip_get_selected_associations(const clipper_hip_t* h, int32_t* A_out,
                                          int32_t capacity) try {
  if (!h || !A_out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  const int32_t k = static_cast<int32_t>(h->nodes.size());
  if (capacity < k) return fail(CLIPPER_HIP_E_INVALID, "capacity %d < %d nodes", capacity, k);
  if (k == 0) return 0;
  if (h->A.size() != static_cast<size_t>(2 * h->m))
    return fail(CLIPPER_HIP_E_STATE, "no association list is held");
  for (int32_t r = 0; r < k; ++r) {
    const size_t n = static_cast<size_t>(h->nodes[static_cast<size_t>(r)]);
    A_out[r] = h->A[n];
    A_out[k + r] = h->A[static_cast<size_t>(h->m) + n];
  }
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

int clipper_hip_core_numbers(clipper_hip_t* h, int32_t* core_out) try {
  if (!h || !core_out) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  return core_numbers_impl(h, core_out);
} CLIPPER_HIP_GUARD_INT

// ---- putative associations (before the path): brute-force nearest neighbours -------------------

int clipper_hip_knn(int device, const double* P0, int64_t n0, const double* P1, int64_t n1, int d,
                    int knn, int32_t* idx_out, double* sqd_out) try {
  if (!P0 || !P1 || !idx_out || n0 < 1 || n1 < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (d != 2 && d != 3) return fail(CLIPPER_HIP_E_INVALID, "points must have 2 or 3 coordinates");
  if (knn < 1 || knn > 16) return fail(CLIPPER_HIP_E_INVALID, "knn must be in 1..16");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CLIPPER_HIP_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CLIPPER_HIP_E_INVALID, "device %d out of range", device);
  HIPCHK(hipSetDevice(device));
  const int K = knn <= 1 ? 1 : (knn <= 2 ? 2 : (knn <= 4 ? 4 : (knn <= 8 ? 8 : 16)));
  // enough workgroups to fill the chip: split pcd1 into S chunks of whole tiles
  const int64_t qblocks = ceil_div(n0, 256);
  const int64_t tiles = ceil_div(n1, KNN_TILE);
  const int S = static_cast<int>(std::max<int64_t>(1, std::min<int64_t>(tiles, ceil_div(512, qblocks))));
  const int64_t chunk = ceil_div(tiles, S) * KNN_TILE;
  double *dP0 = nullptr, *dP1 = nullptr, *pd = nullptr, *od = nullptr;
  int32_t *pi = nullptr, *oi = nullptr;
  auto cleanup = [&]() {
    hipFree(dP0); hipFree(dP1); hipFree(pd); hipFree(od); hipFree(pi); hipFree(oi);
  };
  const size_t b0 = static_cast<size_t>(n0) * d * sizeof(double), b1 = static_cast<size_t>(n1) * d * sizeof(double);
  const size_t np = static_cast<size_t>(S) * n0 * K, no = static_cast<size_t>(n0) * K;
  if (hipMalloc(&dP0, b0) != hipSuccess || hipMalloc(&dP1, b1) != hipSuccess ||
      hipMalloc(&pd, np * sizeof(double)) != hipSuccess || hipMalloc(&pi, np * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&od, no * sizeof(double)) != hipSuccess || hipMalloc(&oi, no * sizeof(int32_t)) != hipSuccess) {
    cleanup();
    return fail(CLIPPER_HIP_E_NOMEM, "device allocation failed");
  }
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  bool ok = hipMemcpyAsync(dP0, P0, b0, hipMemcpyHostToDevice, st) == hipSuccess &&
            hipMemcpyAsync(dP1, P1, b1, hipMemcpyHostToDevice, st) == hipSuccess;
  if (ok) {
#define KNN_CASE(KK)                                                                        \
  case KK:                                                                                  \
    if (d == 3) knn_run<KK, 3>(dP0, n0, dP1, n1, S, chunk, pd, pi, od, oi, st);             \
    else knn_run<KK, 2>(dP0, n0, dP1, n1, S, chunk, pd, pi, od, oi, st);                    \
    break
    switch (K) {
      KNN_CASE(1);
      KNN_CASE(2);
      KNN_CASE(4);
      KNN_CASE(8);
      default:
        if (d == 3) knn_run<16, 3>(dP0, n0, dP1, n1, S, chunk, pd, pi, od, oi, st);
        else knn_run<16, 2>(dP0, n0, dP1, n1, S, chunk, pd, pi, od, oi, st);
        break;
    }
#undef KNN_CASE
    std::vector<double> hd(no);
    std::vector<int32_t> hi(no);
    ok = hipMemcpy(hd.data(), od, no * sizeof(double), hipMemcpyDeviceToHost) == hipSuccess &&
         hipMemcpy(hi.data(), oi, no * sizeof(int32_t), hipMemcpyDeviceToHost) == hipSuccess &&
         hipGetLastError() == hipSuccess;
    if (ok) {
      for (int64_t i = 0; i < n0; ++i)
        for (int k = 0; k < knn; ++k) {
          idx_out[i * knn + k] = hi[static_cast<size_t>(i) * K + k];
          if (sqd_out) sqd_out[i * knn + k] = hd[static_cast<size_t>(i) * K + k];
        }
    }
  }
  cleanup();
  if (!ok) return fail(CLIPPER_HIP_E_HIP, "nearest-neighbour search failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
} CLIPPER_HIP_GUARD_INT

int64_t clipper_hip_distance_based_correspondences(int device, const double* P0, int64_t n0,
                                                   const double* P1, int64_t n1, int d, int knn,
                                                   double radius, int enforce_1to1, int32_t* A_out,
                                                   int64_t capacity) try {
  if (!A_out && capacity > 0) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  std::vector<int32_t> idx(static_cast<size_t>(std::max<int64_t>(n0, 0)) * std::max(knn, 0));
  std::vector<double> sqd(idx.size());
  int rc = clipper_hip_knn(device, P0, n0, P1, n1, d, knn, idx.data(), sqd.data());
  if (rc) return rc;
  // bm_utils.cpp:187-229: rows (i, nn_j(i)) for i ascending, neighbours by distance, kept if within
  // the radius; one-to-one: per point of pcd1 (ascending) the FIRST closest of its claimants
  const double r2 = radius * radius;
  std::vector<std::pair<int32_t, int32_t>> rows;
  std::map<int32_t, std::vector<std::pair<int32_t, double>>> claim;
  for (int64_t i = 0; i < n0; ++i)
    for (int k = 0; k < knn; ++k) {
      const int32_t c1 = idx[static_cast<size_t>(i) * knn + k];
      const double sd = sqd[static_cast<size_t>(i) * knn + k];
      if (c1 < 0) continue;  // fewer than knn points in pcd1
      if (sd <= r2) {
        rows.emplace_back(static_cast<int32_t>(i), c1);
        if (enforce_1to1) claim[c1].emplace_back(static_cast<int32_t>(i), sd);
      }
    }
  if (enforce_1to1) {
    rows.clear();
    for (const auto& it : claim) {
      size_t best = 0;
      for (size_t q = 1; q < it.second.size(); ++q)
        if (it.second[q].second < it.second[best].second) best = q;  // std::min_element: first minimum
      rows.emplace_back(it.second[best].first, it.first);
    }
  }
  const int64_t n = static_cast<int64_t>(rows.size());
  if (n > capacity) return fail(CLIPPER_HIP_E_INVALID, "capacity %lld < %lld associations",
                                static_cast<long long>(capacity), static_cast<long long>(n));
  for (int64_t r = 0; r < n; ++r) {  // column-major n x 2, as clipper::Association
    A_out[r] = rows[static_cast<size_t>(r)].first;
    A_out[n + r] = rows[static_cast<size_t>(r)].second;
  }
  return n;
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
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  const int64_t m = h->m, W = h->W;
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    // x -> candidate 0 of table 0 (staged through the u0 buffer)
    HIPCHK(hipMemcpyAsync(s.u0, x, static_cast<size_t>(m) * sizeof(double),
                          hipMemcpyHostToDevice, s.stream));
    hipLaunchKernelGGL(k_spread, dim3(static_cast<unsigned>(ceil_div(m, 256))), dim3(256), 0,
                       s.stream, s.u0, m, s.X[0]);
  }
  h->u0_staged = false;
  int rc = h->csc_valid ? 0 : ensure_dense(h, true);
  if (rc) return rc;
  if ((rc = enqueue_gemv_plain(h))) return rc;
  if ((rc = enqueue_reduce_exchange(h))) return rc;
  if ((rc = sync_all(h))) return rc;
  std::vector<double> ab(static_cast<size_t>(h->world) * 2 * W);
  Shard& s0 = h->sh[0];
  HIPCHK(hipSetDevice(s0.device));
  HIPCHK(hipMemcpy(ab.data(), s0.ab, ab.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < m; ++i) {
    const int64_t p = i / W, off = i - p * W;
    if (yM) yM[i] = ab[static_cast<size_t>(p * 2 * W + off)];
    if (yC) yC[i] = ab[static_cast<size_t>(p * 2 * W + W + off)];
  }
  return 0;
} CLIPPER_HIP_GUARD_INT

// The products of clipper_hip_matvec through a ROW VIEW of the given rows: yM = M_off[:, rows] x[rows],
// yC likewise — what a pass of the solver computes when it streams the view instead of M. Builds the
// slices of M[rows, :] with the rectangular fill kernel from the staged points (the view of a later
// solve is built anew). For tests: equal to clipper_hip_matvec of x with every other entry zeroed, up
// to the order of the partial sums.
int clipper_hip_view_matvec(clipper_hip_t* h, const int32_t* rows, int64_t nrows, const double* x,
                            double* yM, double* yC) try {
  if (!h || !rows || !x || nrows < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid argument");
  if (!h->has_matrix || !h->csc_valid || !csc_single(h) || !rect_fill_possible(h))
    return fail(CLIPPER_HIP_E_STATE, "a row view needs slices of a matrix scored from staged points on one device");
  const int64_t m = h->m, W = h->W;
  for (int64_t r = 0; r < nrows; ++r)
    if (rows[r] < 0 || rows[r] >= m || (r > 0 && rows[r] <= rows[r - 1]))
      return fail(CLIPPER_HIP_E_INVALID, "rows must be ascending association indices");
  Shard& s = h->sh[0];
  RowView& v = s.rv;
  HIPCHK(hipSetDevice(s.device));
  HIPCHK(hipStreamSynchronize(s.stream));
  v.valid = false;
  int rc;
  {
    size_t r0 = v.cap_rows, r1 = v.cap_rows;
    if ((rc = rv_grow(v.rowmap[0], r0, static_cast<size_t>(h->mp)))) return rc;
    if ((rc = rv_grow(v.rowmap[1], r1, static_cast<size_t>(h->mp)))) return rc;
    v.cap_rows = static_cast<size_t>(h->mp);
  }
  HIPCHK(hipMemcpyAsync(v.rowmap[0], rows, static_cast<size_t>(nrows) * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
  for (int attempt = 0;; ++attempt) {
    SliceOut O{};
    if ((rc = emit_prepare(h, s, v.st, nrows, O))) return rc;
    if ((rc = launch_rect(h, s, v.rowmap[0], nrows, O))) return rc;
    if ((rc = emit_enqueue(h, s, v.st))) return rc;
    HIPCHK(hipStreamSynchronize(s.stream));
    HIPCHK(hipGetLastError());
    bool again = false;
    if ((rc = emit_check(h, s, v.st, false, again))) return rc;
    if (!again) break;
    if (attempt >= 2) return fail(CLIPPER_HIP_E_HIP, "row view: the build keeps overflowing");
  }
  HIPCHK(hipMemcpyAsync(s.u0, x, static_cast<size_t>(m) * sizeof(double), hipMemcpyHostToDevice, s.stream));
  hipLaunchKernelGGL(k_spread, dim3(static_cast<unsigned>(ceil_div(m, 256))), dim3(256), 0, s.stream, s.u0, m, s.X[0]);
  h->u0_staged = false;
  SliceView R{};
  R.data = v.st.sdata;
  R.Pre = v.st.sPre;
  R.work = v.st.swork;
  R.nchunks = v.st.s_nchunks;
  R.ncg = v.st.s_ncg;
  R.nwork = v.st.s_nwork;
  R.rowmap = v.rowmap[0];
  R.nrows = nrows;
  R.pad = 0;
  dim3 grid(static_cast<unsigned>(R.nwork)), block(SL_NW * 64);
  if (h->storage == CLIPPER_HIP_STORE_F64)
    hipLaunchKernelGGL((k_gemv_slices_plain<double, 1>), grid, block, 0, s.stream, R, W, m, s.X[0], s.part);
  else
    hipLaunchKernelGGL((k_gemv_slices_plain<float, 1>), grid, block, 0, s.stream, R, W, m, s.X[0], s.part);
  hipLaunchKernelGGL(k_reduce, dim3(static_cast<unsigned>(ceil_div(2 * W, 256))), dim3(256), 0, s.stream, s.part,
                     v.st.s_nslots, 2, W, s.ab);
  std::vector<double> ab(static_cast<size_t>(2 * W));
  HIPCHK(hipMemcpyAsync(ab.data(), s.ab, ab.size() * sizeof(double), hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  HIPCHK(hipGetLastError());
  for (int64_t i = 0; i < m; ++i) {
    if (yM) yM[i] = ab[static_cast<size_t>(i)];
    if (yC) yC[i] = ab[static_cast<size_t>(W + i)];
  }
  return 0;
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
    for (auto& e : h->ev_pairs) HIPCHK(hipEventCreate(&e));
    h->ev_xchg.resize(2 * MAX_EVENT_PAIRS);
    h->ev_xchg_used.assign(MAX_EVENT_PAIRS, 0);
    for (auto& e : h->ev_xchg) HIPCHK(hipEventCreate(&e));
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
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (!h->csc_valid)
    if (int rc = ensure_dense(h, true)) return rc;
  Shard& s = h->sh[0];
  HIPCHK(hipSetDevice(s.device));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0));
  HIPCHK(hipEventCreate(&e1));
  for (int w = 0; w < 3; ++w) launch_plain(h, s, s.X[0]);
  HIPCHK(hipEventRecord(e0, s.stream));
  for (int r = 0; r < reps; ++r) launch_plain(h, s, s.X[0]);
  HIPCHK(hipEventRecord(e1, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  *avg_us = static_cast<double>(ms) * 1e3 / reps;
  h->tm.gemv_bytes = algorithmic_gemv_bytes(h, /*dense=*/!h->csc_valid);
  return 0;
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
  HIPCHK(hipSetDevice(device));
  if (!raise_dynamic_lds(reinterpret_cast<const void*>(k_debug_occupy), device, static_cast<int>(RS_LDS_MAX)))
    return fail(CLIPPER_HIP_E_HIP, "the device refuses %u bytes of dynamic LDS", RS_LDS_MAX);
  hipStream_t st = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  hipLaunchKernelGGL(k_debug_occupy, dim3(static_cast<unsigned>(workgroups)), dim3(64), static_cast<size_t>(lds_bytes), st,
                     static_cast<long long>(milliseconds * 1e5));
  const hipError_t e = hipStreamSynchronize(st);
  hipStreamDestroy(st);
  HIPCHK(e);
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
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CLIPPER_HIP_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CLIPPER_HIP_E_INVALID, "device %d out of range (%d visible)", device, ndev);
  if (storage != CLIPPER_HIP_STORE_F32 && storage != CLIPPER_HIP_STORE_F64 && storage != CLIPPER_HIP_STORE_F32_CSC &&
      storage != CLIPPER_HIP_STORE_F64_CSC)
    return fail(CLIPPER_HIP_E_INVALID, "storage must be CLIPPER_HIP_STORE_F32, _F64, _F32_CSC or _F64_CSC");
  clipper_hip_batch_t* b = new clipper_hip_batch_t();
  b->device = device;
  b->storage = storage;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess) {
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
  if (b->hstage) hipHostFree(b->hstage);
  if (b->dstage) hipFree(b->dstage);
  if (b->stream) hipStreamDestroy(b->stream);
  delete b;
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
