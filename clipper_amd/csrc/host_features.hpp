// host_features.hpp — normals and FPFH descriptors of a point cloud (before the path, in front of the matcher): the
// driver of clipper_hip_estimate_normals, clipper_hip_compute_fpfh and clipper_hip_fpfh_from_points. One body serves
// the three: the cloud goes to the device once, the cloud is searched against itself once at the larger knn (nearest-K
// lists are nested: the shorter neighbourhood is a prefix of the longer list), the normals stage and the feature stage
// are queued on one stream with no host wait in between (the normals stay on the device), and what the caller asked
// for comes back behind the one wait of the call (the grid route of the search waits twice more inside it: host_knn_grid.hpp).
// Stand-alone: needs no context. The checks are
// host_features_check.hpp's. Part of clipper_hip.hip (one translation unit; included there after host_match.hpp).
#pragma once

#include "host_features_check.hpp"

namespace {

template <int SLOTS>
void feat_spfh_run(const double* dP, const double* dN, int64_t n, const int32_t* oi, const double* od, int stride, int knn,
                   int use_r, double r2, double* dS, int32_t* dcnt, hipStream_t st) {
  hipLaunchKernelGGL((k_feat_spfh<SLOTS>), dim3(static_cast<unsigned>(ceil_div(n, 256 / SLOTS))), dim3(256), 0, st, dP, dN,
                     n, oi, od, stride, knn, use_r, r2, dS, dcnt);
}

// nnb: the neighbourhood of the normals stage (null: the normals are N_in); fnb: the feature stage's (null: none).
// Every argument has been checked. Outputs may be null where the entry points allow it.
int features_run(int device, const double* P, const double* N_in, int64_t n, const clipper_features::Neighborhood* nnb,
                 const double* view, const clipper_features::Neighborhood* fnb, double* N_out, int32_t* ncnt_out,
                 double* F_out, double* spfh_out, int32_t* fcnt_out) {
  namespace cf = clipper_features;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CLIPPER_HIP_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail(CLIPPER_HIP_E_INVALID, "device %d out of range", device);
  HIPCHK(hipSetDevice(device));

  const int K = cf::list_k(std::max(nnb ? nnb->knn : 0, fnb ? fnb->knn : 0));
  const size_t n3 = static_cast<size_t>(n) * 3, nf = fnb ? static_cast<size_t>(n) * FEAT_DIM : 0;
  const size_t no = static_cast<size_t>(n) * K;
  double *dP = nullptr, *dN = nullptr, *dV = nullptr, *od = nullptr, *dS = nullptr, *dF = nullptr;
  int32_t *oi = nullptr, *dcn = nullptr, *dcf = nullptr;
  DevTemps tmp;
  if (tmp.alloc(device, dP, n3 * sizeof(double)) || tmp.alloc(device, dN, n3 * sizeof(double)) ||
      tmp.alloc(device, dV, 3 * sizeof(double)) || tmp.alloc(device, od, no * sizeof(double)) ||
      tmp.alloc(device, oi, no * sizeof(int32_t)) || tmp.alloc(device, dS, nf * sizeof(double)) ||
      tmp.alloc(device, dF, nf * sizeof(double)) || tmp.alloc(device, dcn, static_cast<size_t>(n) * sizeof(int32_t)) ||
      tmp.alloc(device, dcf, static_cast<size_t>(n) * sizeof(int32_t))) {
    tmp.release();
    return fail(CLIPPER_HIP_E_NOMEM, "device allocation failed");
  }
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  auto up = [&](double* dst, const double* src, size_t count) {
    return hipMemcpyAsync(dst, src, count * sizeof(double), hipMemcpyHostToDevice, st) == hipSuccess;
  };
  auto down = [&](void* dst, const void* src, size_t bytes) {
    return !dst || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess;
  };
  bool ok = up(dP, P, n3) && (nnb || up(dN, N_in, n3)) && (!(nnb && view) || up(dV, view, 3));
  if (ok) {
    // the cloud's nearest-neighbour lists in itself, K in {4, 8, 16, 32}, by the route of the process-wide mode
    if (int rc = knn_lists(device, K, 3, dP, n, dP, n, od, oi, st, tmp)) return rc;
    if (nnb) {
      const int use_r = nnb->radius > 0.0;
      hipLaunchKernelGGL(k_feat_normals<>, dim3(static_cast<unsigned>(ceil_div(n, 256))), dim3(256), 0, st, dP, n, oi, od, K,
                         nnb->knn, use_r, nnb->radius * nnb->radius, view ? dV : nullptr, dN, dcn);
      ok = down(N_out, dN, n3 * sizeof(double)) && down(ncnt_out, dcn, static_cast<size_t>(n) * sizeof(int32_t));
    }
    if (ok && fnb) {
      const int use_r = fnb->radius > 0.0;
      const double r2 = fnb->radius * fnb->radius;
      switch (cf::list_k(fnb->knn)) {
        case 4: feat_spfh_run<4>(dP, dN, n, oi, od, K, fnb->knn, use_r, r2, dS, dcf, st); break;
        case 8: feat_spfh_run<8>(dP, dN, n, oi, od, K, fnb->knn, use_r, r2, dS, dcf, st); break;
        case 16: feat_spfh_run<16>(dP, dN, n, oi, od, K, fnb->knn, use_r, r2, dS, dcf, st); break;
        default: feat_spfh_run<32>(dP, dN, n, oi, od, K, fnb->knn, use_r, r2, dS, dcf, st); break;
      }
      hipLaunchKernelGGL(k_feat_fpfh<>, dim3(static_cast<unsigned>(ceil_div(n, FEAT_FPFH_POINTS))), dim3(256), 0, st, dS, n,
                         oi, od, K, fnb->knn, use_r, r2, dF);
      ok = down(F_out, dF, nf * sizeof(double)) && down(spfh_out, dS, nf * sizeof(double)) &&
           down(fcnt_out, dcf, static_cast<size_t>(n) * sizeof(int32_t));
    }
    ok = hipStreamSynchronize(st) == hipSuccess && ok && hipGetLastError() == hipSuccess;  // the one wait of the call
  }
  tmp.release();
  if (!ok) return fail(CLIPPER_HIP_E_HIP, "point-cloud features failed: %s", hipGetErrorString(hipGetLastError()));
  return 0;
}

inline clipper_features::Neighborhood feat_nb(const clipper_neighborhood_t* nb) {
  return nb ? clipper_features::Neighborhood{nb->knn, nb->radius} : clipper_features::Neighborhood{0, 0.0};
}

int estimate_normals(int device, const double* P, int64_t n, const clipper_neighborhood_t* nb, const double* viewpoint,
                     double* N_out, int32_t* count_out) {
  namespace cf = clipper_features;
  const cf::Neighborhood h = feat_nb(nb);
  std::string why = !P ? "null point array" : (!N_out ? "null normal output array" : "");
  if (why.empty()) why = cf::check_neighborhood("neighbourhood", nb ? &h : nullptr);
  if (why.empty()) why = cf::check_count(n);
  if (why.empty()) why = cf::check_viewpoint(viewpoint);
  if (why.empty()) why = cf::check_points(P, n);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  return features_run(device, P, nullptr, n, &h, viewpoint, nullptr, N_out, count_out, nullptr, nullptr, nullptr);
}

int compute_fpfh(int device, const double* P, const double* N, int64_t n, const clipper_neighborhood_t* nb, double* F_out,
                 double* spfh_out, int32_t* count_out) {
  namespace cf = clipper_features;
  const cf::Neighborhood h = feat_nb(nb);
  std::string why = !P ? "null point array" : (!N ? "null normal array" : (!F_out ? "null descriptor output array" : ""));
  if (why.empty()) why = cf::check_neighborhood("neighbourhood", nb ? &h : nullptr);
  if (why.empty()) why = cf::check_count(n);
  if (why.empty()) why = cf::check_points(P, n);
  if (why.empty()) why = cf::check_normals(N, n);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  return features_run(device, P, N, n, nullptr, nullptr, &h, nullptr, nullptr, F_out, spfh_out, count_out);
}

int fpfh_from_points(int device, const double* P, int64_t n, const clipper_neighborhood_t* normal_nb, const double* viewpoint,
                     const clipper_neighborhood_t* feature_nb, double* F_out, double* N_out) {
  namespace cf = clipper_features;
  const cf::Neighborhood hn = feat_nb(normal_nb), hf = feat_nb(feature_nb);
  std::string why = !P ? "null point array" : (!F_out ? "null descriptor output array" : "");
  if (why.empty()) why = cf::check_neighborhood("normal neighbourhood", normal_nb ? &hn : nullptr);
  if (why.empty()) why = cf::check_neighborhood("feature neighbourhood", feature_nb ? &hf : nullptr);
  if (why.empty()) why = cf::check_count(n);
  if (why.empty()) why = cf::check_viewpoint(viewpoint);
  if (why.empty()) why = cf::check_points(P, n);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  return features_run(device, P, nullptr, n, &hn, viewpoint, &hf, N_out, nullptr, F_out, nullptr, nullptr);
}

}  // namespace
