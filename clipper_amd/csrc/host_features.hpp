// host_features.hpp — normals and FPFH descriptors of a point cloud (before the path, in front of the matcher): the
// driver of clipper_hip_estimate_normals, clipper_hip_compute_fpfh and clipper_hip_fpfh_from_points. One body serves
// the three: the cloud goes to the device once, the cloud is searched against itself once at the larger knn (nearest-K
// lists are nested: the shorter neighbourhood is a prefix of the longer list), the normals stage and the feature stage
// are queued on one stream with no host wait in between (the normals stay on the device), and what the caller asked
// for comes back behind the one wait of the call (the grid route of the search waits twice more inside it: host_knn_grid.hpp).
// Stand-alone: needs no context. The checks are host_features_check.hpp's, the frame host_call.hpp's. Part of
// clipper_hip.hip (one translation unit; included there after host_match.hpp).
#pragma once

#include "host_features_check.hpp"

namespace {

template <int SLOTS>
void feat_spfh_run(const double* dP, const double* dN, int64_t n, const int32_t* oi, const double* od, int stride, int knn,
                   int use_r, double r2, double* dS, int32_t* dcnt, hipStream_t st) {
  hipLaunchKernelGGL((k_feat_spfh<SLOTS>), dim3(static_cast<unsigned>(ceil_div(n, 256 / SLOTS))), dim3(256), 0, st, dP, dN,
                     n, oi, od, stride, knn, use_r, r2, dS, dcnt);
}

// THE BODY of the stages, on device pointers: dP the cloud (n x 3); nnb: the neighbourhood of the normals stage, which
// writes dN (n x 3) and dcn (n) and reads the viewpoint dV (null: none) — with nnb null dN holds the normals already;
// fnb: the feature stage's (null: none), which writes dS, dF (n x 33 each) and dcf (n). The lists of the search join
// tmp; everything is queued on st (the grid route of the search has waited inside it); target as knn_lists'. The
// host-buffer calls (below) and the calls on clouds (host_cloud.hpp) both run this.
int features_body(int device, const double* dP, int64_t n, const clipper_features::Neighborhood* nnb, const double* dV,
                  const clipper_features::Neighborhood* fnb, double* dN, int32_t* dcn, double* dS, double* dF,
                  int32_t* dcf, hipStream_t st, DevTemps& tmp, KnnTarget& target) {
  const int K = clipper_features::list_k(std::max(nnb ? nnb->knn : 0, fnb ? fnb->knn : 0));
  const size_t no = static_cast<size_t>(n) * K;
  double* od = nullptr;
  int32_t* oi = nullptr;
  if (int rc = tmp.alloc(device, od, no * sizeof(double), oi, no * sizeof(int32_t))) return rc;
  // the cloud's nearest-neighbour lists in itself, K in {4, 8, 16, 32}, by the route of the process-wide mode
  if (int rc = knn_lists(device, K, 3, dP, n, dP, n, od, oi, st, tmp, target)) return rc;
  if (nnb) {
    const int use_r = nnb->radius > 0.0;
    hipLaunchKernelGGL(k_feat_normals<>, dim3(static_cast<unsigned>(ceil_div(n, 256))), dim3(256), 0, st, dP, n, oi, od, K,
                       nnb->knn, use_r, nnb->radius * nnb->radius, dV, dN, dcn);
  }
  if (fnb) {
    const int use_r = fnb->radius > 0.0;
    const double r2 = fnb->radius * fnb->radius;
    const int slots = clipper_features::list_k(fnb->knn);
    if (!dispatch_k<4, 8, 16, 32>(slots, [&](auto k) {
          feat_spfh_run<decltype(k)::value>(dP, dN, n, oi, od, K, fnb->knn, use_r, r2, dS, dcf, st);
        }))
      return fail(CLIPPER_HIP_E_INTERNAL, "no SPFH kernel for %d slots", slots);
    hipLaunchKernelGGL(k_feat_fpfh<>, dim3(static_cast<unsigned>(ceil_div(n, FEAT_FPFH_POINTS))), dim3(256), 0, st, dS, n,
                       oi, od, K, fnb->knn, use_r, r2, dF);
  }
  return 0;
}

// nnb: the neighbourhood of the normals stage (null: the normals are N_in); fnb: the feature stage's (null: none).
// Every argument has been checked. Outputs may be null where the entry points allow it.
int features_run(int device, const double* P, const double* N_in, int64_t n, const clipper_features::Neighborhood* nnb,
                 const double* view, const clipper_features::Neighborhood* fnb, double* N_out, int32_t* ncnt_out,
                 double* F_out, double* spfh_out, int32_t* fcnt_out) {
  if (int rc = use_device(device)) return rc;

  const size_t n3 = static_cast<size_t>(n) * 3, nf = fnb ? static_cast<size_t>(n) * FEAT_DIM : 0;
  const size_t nn = static_cast<size_t>(n);
  double *dP = nullptr, *dN = nullptr, *dV = nullptr, *dS = nullptr, *dF = nullptr;
  int32_t *dcn = nullptr, *dcf = nullptr;
  DevTemps tmp;
  if (int rc = tmp.alloc(device, dP, n3 * sizeof(double), dN, n3 * sizeof(double), dV, 3 * sizeof(double),
                         dS, nf * sizeof(double), dF, nf * sizeof(double), dcn, nn * sizeof(int32_t), dcf, nn * sizeof(int32_t)))
    return rc;
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  if (int rc = copy_up(dP, P, n3, st)) return rc;
  if (!nnb)
    if (int rc = copy_up(dN, N_in, n3, st)) return rc;
  if (nnb && view)
    if (int rc = copy_up(dV, view, 3, st)) return rc;
  KnnTarget target;  // (of this call alone)
  if (int rc = features_body(device, dP, n, nnb, (nnb && view) ? dV : nullptr, fnb, dN, dcn, dS, dF, dcf, st, tmp, target))
    return rc;
  if (nnb) {
    if (int rc = copy_down(N_out, dN, n3, st)) return rc;
    if (int rc = copy_down(ncnt_out, dcn, nn, st)) return rc;
  }
  if (fnb) {
    if (int rc = copy_down(F_out, dF, nf, st)) return rc;
    if (int rc = copy_down(spfh_out, dS, nf, st)) return rc;
    if (int rc = copy_down(fcnt_out, dcf, nn, st)) return rc;
  }
  HIPCHK(hipStreamSynchronize(st));  // the one wait of the call
  HIPCHK(hipGetLastError());
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
