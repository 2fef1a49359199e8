// host_cloud.hpp — clouds and association lists that LIVE ON THE DEVICE ("Clouds on the device"):
// the two owning handles of the C ABI, clipper_hip_cloud_t and clipper_hip_pairs_t, and the stages of the front end on
// them. A cloud is n points on one device with what the stages have computed about it attached: normals, descriptors
// (and the zero-padded image the matcher's kernel reads, made once), SPFH, covariances, the neighbour counts of each
// stage, the members and the trace of the voxel stage that made it, and one KnnTarget (host_knn_grid.hpp): what a search
// against it needs, made on first use by knn_target_ensure and KEPT. That is the grid index (grid route: ICP, the
// evaluation and the self-search of the normals, FPFH and covariance stages all query the one index; it depends on the
// cloud alone, not on K) and the bounding box (brute-force route). An attachment is PRESENT EXACTLY WHEN ITS DevBuf IS
// OWNED: there is no flag beside a buffer (cloud_part is the one table of what each attachment is). The voxel stage also
// writes the corners of a stage-made input cloud on first use (lo, hi, has_corners), and copies its rows from the
// body's n-sized temporaries into exact-sized buffers of the new cloud (a second pass over the output, device to
// device). Every stage here runs the BODY its host-buffer call runs (match_lists, features_body, covariances_body,
// voxel_body, icp_body, stage_inputs), on the cloud's buffers instead of on copies made for the call: one statement of
// each stage, the same bits; the bodies read the search mode, the stages do not. A stage computes into local buffers
// and moves them into the cloud after its wait: a refused or failed stage leaves the cloud as it was. The filters of
// the matcher run on the device (k_match_select: match_rules.hpp, the host's own rules). What a stage attaches is valid
// by construction; what comes from the host is checked once, at create / set_descriptors, by the checks of the
// host-buffer calls. All work is on the default stream, and every call has waited for it when it returns. A cloud is
// not safe for concurrent mutation. Part of clipper_hip.hip (one translation unit; included there last, after
// host_voxel.hpp).
#pragma once

struct clipper_hip_cloud {
  int device = 0;
  int64_t n = 0;
  DevBuf<double> P;              // n x 3
  DevBuf<double> N;              // n x 3 unit normals
  DevBuf<double> F, Fpad;        // n x fd descriptors; n x 8 fG: the rows padded with zeros (k_match.hip.h)
  DevBuf<double> S;              // n x 33 SPFH (of compute_fpfh)
  DevBuf<double> C;              // n x 6 covariances
  DevBuf<int32_t> ncnt, fcnt, ccnt;  // n each: the neighbours kept by the normals, the FPFH and the covariance stage
  DevBuf<int32_t> vcnt, vtrace;  // n: the members of each voxel; trace_n: the row of each point of the voxel stage's input
  int fd = 0, fG = 0;            // coordinates per descriptor (0: none), groups of 8 of the padded image
  int64_t trace_n = 0;           // 0: no trace
  // the corners of the cloud as the voxel stage plans with them: the host's scan at create, else the device's fold
  bool has_corners = false;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  KnnTarget target{true};        // what a search AGAINST this cloud needs: it outlives the calls
};

struct clipper_hip_pairs {
  int device = 0;
  int64_t m = 0;
  DevBuf<int32_t> A;   // m x 2 column-major as clipper::Association
  DevBuf<double> sqd;  // m, or none
};

namespace {

typedef clipper_hip_cloud Cloud;
typedef clipper_hip_pairs Pairs;

// exactly `count` elements (one where count is 0: a buffer that exists)
template <typename T>
int cloud_alloc(DevBuf<T>& b, size_t count) {
  HIPCHK(b.alloc(std::max<size_t>(count, 1)));
  return 0;
}

// `count` elements from device to device, queued on st
template <typename T>
int copy_across(T* dst, const T* src, size_t count, hipStream_t st) {
  if (count) HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToDevice, st));
  return 0;
}

// the end of every call on a handle: nothing it queued is in flight when it returns
int cloud_wait(hipStream_t st) {
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipGetLastError());
  return 0;
}

// ---- the handles ------------------------------------------------------------------------------------------------------

int cloud_create(int device, const double* P, const double* N, int64_t n, Cloud** out) {
  if (out) *out = nullptr;
  if (!out) return fail(CLIPPER_HIP_E_INVALID, "cloud_create: null output handle");
  std::string why = clipper_voxel::check_count(n);
  if (why.empty() && n > 0 && !P) why = "null point array";
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (why.empty()) why = clipper_voxel::check_points_bounds(P, n, lo, hi);
  if (why.empty() && N) why = clipper_features::check_normals(N, n);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "cloud_create: %s", why.c_str());
  if (int rc = use_device(device)) return rc;
  std::unique_ptr<Cloud> c(new Cloud);
  c->device = device;
  c->n = n;
  const size_t n3 = static_cast<size_t>(n) * 3;
  hipStream_t st = nullptr;
  if (int rc = cloud_alloc(c->P, n3)) return rc;
  if (n3)
    if (int rc = copy_up(c->P.get(), P, n3, st)) return rc;
  if (N) {
    if (int rc = cloud_alloc(c->N, n3)) return rc;
    if (n3)
      if (int rc = copy_up(c->N.get(), N, n3, st)) return rc;
  }
  if (int rc = cloud_wait(st)) return rc;  // (the caller's arrays may go once this returns)
  for (int a = 0; a < 3; ++a) c->lo[a] = lo[a], c->hi[a] = hi[a];
  c->has_corners = n > 0;
  *out = c.release();
  return 0;
}

int pairs_create(int device, const int32_t* A, const double* sqd, int64_t m, Pairs** out) {
  if (out) *out = nullptr;
  if (!out) return fail(CLIPPER_HIP_E_INVALID, "pairs_create: null output handle");
  if (m < 0 || m > INT32_MAX) return fail(CLIPPER_HIP_E_INVALID, "pairs_create: m = %lld outside 0 .. 2^31 - 1", static_cast<long long>(m));
  if (m > 0 && !A) return fail(CLIPPER_HIP_E_INVALID, "pairs_create: null association array");
  for (int64_t r = 0; r < 2 * m; ++r)
    if (A[r] < 0)
      return fail(CLIPPER_HIP_E_INVALID, "pairs_create: negative index %d in row %lld", A[r], static_cast<long long>(r % m));
  for (int64_t r = 0; sqd && r < m; ++r)
    if (std::isnan(sqd[r])) return fail(CLIPPER_HIP_E_INVALID, "pairs_create: sqd of row %lld is not a number", static_cast<long long>(r));
  if (int rc = use_device(device)) return rc;
  std::unique_ptr<Pairs> p(new Pairs);
  p->device = device;
  p->m = m;
  const size_t mm = static_cast<size_t>(m);
  hipStream_t st = nullptr;
  if (int rc = cloud_alloc(p->A, 2 * mm)) return rc;
  if (mm)
    if (int rc = copy_up(p->A.get(), A, 2 * mm, st)) return rc;
  if (sqd) {
    if (int rc = cloud_alloc(p->sqd, mm)) return rc;
    if (mm)
      if (int rc = copy_up(p->sqd.get(), sqd, mm, st)) return rc;
  }
  if (int rc = cloud_wait(st)) return rc;
  *out = p.release();
  return 0;
}

int pairs_download(const Pairs* p, int32_t* A_out, double* sqd_out) {
  if (!p) return fail(CLIPPER_HIP_E_INVALID, "pairs_download: null handle");
  if (p->m > 0 && !A_out) return fail(CLIPPER_HIP_E_INVALID, "pairs_download: null association buffer");
  if (sqd_out && !p->sqd) return fail(CLIPPER_HIP_E_STATE, "pairs_download: these pairs carry no squared distances");
  if (p->m == 0) return 0;
  if (int rc = use_device(p->device)) return rc;
  hipStream_t st = nullptr;
  const size_t mm = static_cast<size_t>(p->m);
  if (int rc = copy_down(A_out, p->A.get(), 2 * mm, st)) return rc;
  if (int rc = copy_down(sqd_out, p->sqd.get(), mm, st)) return rc;
  return cloud_wait(st);
}

// THE TABLE of a cloud's attachments: where CLIPPER_HIP_CLOUD_<what> lies, its bytes, and whether it is there (its
// buffer is owned). Unknown `what`: {nullptr, 0, false} with known = false.
struct CloudPart {
  const void* p;
  size_t bytes;
  bool present, known;
};
CloudPart cloud_part(const Cloud* c, int what) {
  const size_t n = static_cast<size_t>(c->n);
  const auto part = [](const auto& buf, size_t count) {
    return CloudPart{buf.get(), count * sizeof(*buf.get()), buf.get() != nullptr, true};
  };
  switch (what) {
    case CLIPPER_HIP_CLOUD_POINTS: return part(c->P, n * 3);
    case CLIPPER_HIP_CLOUD_NORMALS: return part(c->N, n * 3);
    case CLIPPER_HIP_CLOUD_DESCRIPTORS: return part(c->F, n * c->fd);
    case CLIPPER_HIP_CLOUD_SPFH: return part(c->S, n * FEAT_DIM);
    case CLIPPER_HIP_CLOUD_COVARIANCES: return part(c->C, n * 6);
    case CLIPPER_HIP_CLOUD_NORMAL_COUNTS: return part(c->ncnt, n);
    case CLIPPER_HIP_CLOUD_FPFH_COUNTS: return part(c->fcnt, n);
    case CLIPPER_HIP_CLOUD_COVARIANCE_COUNTS: return part(c->ccnt, n);
    case CLIPPER_HIP_CLOUD_VOXEL_COUNTS: return part(c->vcnt, n);
    case CLIPPER_HIP_CLOUD_VOXEL_TRACE: return part(c->vtrace, static_cast<size_t>(c->trace_n));
    default: return CloudPart{nullptr, 0, false, false};
  }
}

int cloud_download(const Cloud* c, int what, void* out) {
  if (!c || !out) return fail(CLIPPER_HIP_E_INVALID, "cloud_download: null %s", !c ? "handle" : "output array");
  const CloudPart a = cloud_part(c, what);
  if (!a.known) return fail(CLIPPER_HIP_E_INVALID, "cloud_download: unknown attachment %d", what);
  if (!a.present) return fail(CLIPPER_HIP_E_STATE, "cloud_download: attachment %d was never computed for this cloud", what);
  if (a.bytes == 0) return 0;
  if (int rc = use_device(c->device)) return rc;
  HIPCHK(hipMemcpy(out, a.p, a.bytes, hipMemcpyDeviceToHost));
  return 0;
}

int cloud_info(const Cloud* c, clipper_hip_cloud_info_t* out) {
  if (!c || !out) return fail(CLIPPER_HIP_E_INVALID, "cloud_info: null %s", !c ? "handle" : "output");
  out->n = c->n;
  out->trace_n = c->trace_n;
  out->device = c->device;
  out->has_normals = cloud_part(c, CLIPPER_HIP_CLOUD_NORMALS).present;
  out->descriptor_dim = c->fd;
  out->has_spfh = cloud_part(c, CLIPPER_HIP_CLOUD_SPFH).present;
  out->has_covariances = cloud_part(c, CLIPPER_HIP_CLOUD_COVARIANCES).present;
  out->grid_builds = c->target.grid_builds;
  for (int a = 0; a < 3; ++a) out->grid_dim[a] = c->target.ix.S ? c->target.ix.g.dim[a] : 0;
  out->has_voxel_counts = cloud_part(c, CLIPPER_HIP_CLOUD_VOXEL_COUNTS).present;
  return 0;
}

// descriptors from elsewhere (a network's: FCGF, SpinNet, Predator): checked as clipper_hip_match_descriptors checks
// them, uploaded, and padded on the device
int cloud_pad_descriptors(Cloud* c, DevBuf<double>& F, int d, DevBuf<double>& Fpad, hipStream_t st) {
  const int G = match_groups(d), dp = G * MATCH_GROUP;
  const int64_t ne = c->n * dp;
  if (int rc = cloud_alloc(Fpad, static_cast<size_t>(ne))) return rc;
  hipLaunchKernelGGL(k_match_pad<>, dim3(static_cast<unsigned>(ceil_div(ne, 256))), dim3(256), 0, st, F.get(), c->n, d, dp,
                     Fpad.get());
  return 0;
}

int cloud_set_descriptors(Cloud* c, const double* F, int d) {
  namespace cm = clipper_match;
  if (!c || !F) return fail(CLIPPER_HIP_E_INVALID, "cloud_set_descriptors: null %s", !c ? "handle" : "descriptor array");
  if (d < 1 || d > cm::MAX_D)
    return fail(CLIPPER_HIP_E_INVALID, "cloud_set_descriptors: descriptors must have 1..%d coordinates (d = %d)", cm::MAX_D, d);
  if (c->n < 1) return fail(CLIPPER_HIP_E_INVALID, "cloud_set_descriptors: the cloud has no points");
  const std::string why = cm::check_finite("F", F, c->n, d);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "cloud_set_descriptors: %s", why.c_str());
  if (int rc = use_device(c->device)) return rc;
  hipStream_t st = nullptr;
  DevBuf<double> dF, dFp;
  const size_t nf = static_cast<size_t>(c->n) * d;
  if (int rc = cloud_alloc(dF, nf)) return rc;
  if (int rc = copy_up(dF.get(), F, nf, st)) return rc;
  if (int rc = cloud_pad_descriptors(c, dF, d, dFp, st)) return rc;
  if (int rc = cloud_wait(st)) return rc;
  c->F = std::move(dF), c->Fpad = std::move(dFp);
  c->fd = d, c->fG = match_groups(d);
  c->S.reset(), c->fcnt.reset();  // (they described the FPFH these replace)
  return 0;
}

// ---- the stages ---------------------------------------------------------------------------------------------------------

int cloud_voxel_downsample(Cloud* in, double voxel_size, int want_trace, Cloud** out, clipper_voxel_info_t* info) {
  if (out) *out = nullptr;
  if (!in || !out) return fail(CLIPPER_HIP_E_INVALID, "cloud_voxel_downsample: null %s", !in ? "handle" : "output handle");
  std::string why = clipper_voxel::check_voxel_size(voxel_size);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  if (int rc = use_device(in->device)) return rc;
  hipStream_t st = nullptr;
  const int64_t n = in->n;
  clipper_voxel::Plan plan{};
  DevTemps tmp;
  if (n == 0) {
    plan.g = VoxelGrid{{0.0, 0.0, 0.0}, 1.0 / voxel_size, {1, 1, 1}};
    plan.passes = 0;
  } else {
    if (!in->has_corners) {  // a cloud a stage made: min and max are exact on the device as on the host
      if (int rc = knn_grid_bounds(in->device, in->P.get(), static_cast<int32_t>(n), in->lo, in->hi, st, tmp)) return rc;
      in->has_corners = true;
    }
    why = clipper_voxel::plan(in->lo, in->hi, voxel_size, plan);
    if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  }
  voxel_info_begin(info, plan, n);
  std::unique_ptr<Cloud> c(new Cloud);
  c->device = in->device;
  if (n == 0) {  // an empty cloud has no voxels
    if (int rc = cloud_alloc(c->P, 0)) return rc;
    if (in->N)
      if (int rc = cloud_alloc(c->N, 0)) return rc;
    *out = c.release();
    return 0;
  }
  VoxelResult R;
  if (int rc = voxel_body(in->device, in->P.get(), in->N.get(), n, plan, want_trace != 0, R, st, tmp))
    return rc;
  const size_t nr = static_cast<size_t>(R.rows);
  c->n = R.rows;
  if (int rc = cloud_alloc(c->P, nr * 3)) return rc;
  if (int rc = copy_across(c->P.get(), R.dPo, nr * 3, st)) return rc;
  if (in->N) {
    if (int rc = cloud_alloc(c->N, nr * 3)) return rc;
    if (int rc = copy_across(c->N.get(), R.dNo, nr * 3, st)) return rc;
  }
  if (int rc = cloud_alloc(c->vcnt, nr)) return rc;
  if (int rc = copy_across(c->vcnt.get(), R.dcnt, nr, st)) return rc;
  if (want_trace) {
    if (int rc = cloud_alloc(c->vtrace, static_cast<size_t>(n))) return rc;
    if (int rc = copy_across(c->vtrace.get(), R.dtrace, static_cast<size_t>(n), st)) return rc;
    c->trace_n = n;
  }
  if (int rc = cloud_wait(st)) return rc;
  voxel_info_end(info, R);
  *out = c.release();
  return 0;
}

// the normals stage and / or the feature stage on c: nnb / fnb as features_body's. What they compute is attached to c.
int cloud_features(Cloud* c, const char* who, const clipper_neighborhood_t* normal_nb, const double* viewpoint,
                   const clipper_neighborhood_t* feature_nb, bool normals, bool features) {
  namespace cf = clipper_features;
  if (!c) return fail(CLIPPER_HIP_E_INVALID, "%s: null handle", who);
  const cf::Neighborhood hn = feat_nb(normal_nb), hf = feat_nb(feature_nb);
  std::string why;
  if (normals) why = cf::check_neighborhood(features ? "normal neighbourhood" : "neighbourhood", normal_nb ? &hn : nullptr);
  if (why.empty() && features)
    why = cf::check_neighborhood(normals ? "feature neighbourhood" : "neighbourhood", feature_nb ? &hf : nullptr);
  if (why.empty()) why = cf::check_count(c->n);
  if (why.empty() && normals) why = cf::check_viewpoint(viewpoint);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s: %s", who, why.c_str());
  if (!normals && !c->N) return fail(CLIPPER_HIP_E_STATE, "%s: the cloud has no normals (estimate them first)", who);
  if (int rc = use_device(c->device)) return rc;
  hipStream_t st = nullptr;
  const size_t nn = static_cast<size_t>(c->n);
  DevBuf<double> dN, dS, dF, dFp;
  DevBuf<int32_t> dcn, dcf;
  double* dV = nullptr;
  DevTemps tmp;
  if (normals) {
    if (int rc = cloud_alloc(dN, nn * 3)) return rc;
    if (int rc = cloud_alloc(dcn, nn)) return rc;
    if (viewpoint) {
      if (int rc = tmp.alloc(c->device, dV, 3 * sizeof(double))) return rc;
      if (int rc = copy_up(dV, viewpoint, 3, st)) return rc;
    }
  }
  if (features) {
    if (int rc = cloud_alloc(dS, nn * FEAT_DIM)) return rc;
    if (int rc = cloud_alloc(dF, nn * FEAT_DIM)) return rc;
    if (int rc = cloud_alloc(dcf, nn)) return rc;
  }
  if (int rc = features_body(c->device, c->P.get(), c->n, normals ? &hn : nullptr, dV, features ? &hf : nullptr,
                             normals ? dN.get() : c->N.get(), dcn.get(), dS.get(), dF.get(), dcf.get(), st, tmp, c->target))
    return rc;
  if (features)
    if (int rc = cloud_pad_descriptors(c, dF, FEAT_DIM, dFp, st)) return rc;
  if (int rc = cloud_wait(st)) return rc;
  if (normals) c->N = std::move(dN), c->ncnt = std::move(dcn);
  if (features) {
    c->F = std::move(dF), c->Fpad = std::move(dFp), c->S = std::move(dS), c->fcnt = std::move(dcf);
    c->fd = FEAT_DIM, c->fG = match_groups(FEAT_DIM);
  }
  return 0;
}

int cloud_estimate_covariances(Cloud* c, const clipper_neighborhood_t* nb, double epsilon) {
  namespace cf = clipper_features;
  if (!c) return fail(CLIPPER_HIP_E_INVALID, "cloud_estimate_covariances: null handle");
  const cf::Neighborhood h = feat_nb(nb);
  std::string why = cf::check_neighborhood("neighbourhood", nb ? &h : nullptr);
  if (why.empty()) why = clipper_icp::check_epsilon(epsilon);
  if (why.empty()) why = cf::check_count(c->n);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "cloud_estimate_covariances: %s", why.c_str());
  if (int rc = use_device(c->device)) return rc;
  hipStream_t st = nullptr;
  const size_t nn = static_cast<size_t>(c->n);
  DevBuf<double> dC;
  DevBuf<int32_t> dcn;
  DevTemps tmp;
  if (int rc = cloud_alloc(dC, nn * 6)) return rc;
  if (int rc = cloud_alloc(dcn, nn)) return rc;
  if (int rc = covariances_body(c->device, c->P.get(), c->n, h, epsilon, dC.get(), dcn.get(), st, tmp, c->target)) return rc;
  if (int rc = cloud_wait(st)) return rc;
  c->C = std::move(dC), c->ccnt = std::move(dcn);
  return 0;
}

// The matcher on two clouds' descriptor images: the searches of match_lists, then the filters ON THE DEVICE: the kept
// entries of every query counted, the counts scanned (k_row_scan), the rows written in the host's order. The one host
// read in the middle is the number of rows (it sizes the pairs). nn_idx_out / nn_sqd_out as clipper_hip_match_descriptors'.
int cloud_match(const Cloud* c0, const Cloud* c1, const clipper_match_params_t* params, Pairs** out, int32_t* nn_idx_out,
                double* nn_sqd_out) {
  namespace cm = clipper_match;
  if (out) *out = nullptr;
  if (!c0 || !c1 || !out) return fail(CLIPPER_HIP_E_INVALID, "cloud_match: null %s", !out ? "output handle" : "cloud handle");
  if (c0->device != c1->device)
    return fail(CLIPPER_HIP_E_INVALID, "cloud_match: the clouds live on devices %d and %d", c0->device, c1->device);
  const cm::Params prm = params ? cm::Params{params->knn, params->mutual, params->ratio, params->max_sqdist} : cm::Params{};
  if (!params) return fail(CLIPPER_HIP_E_INVALID, "cloud_match: null match parameters");
  if (c0->fd < 1 || c1->fd < 1)
    return fail(CLIPPER_HIP_E_STATE, "cloud_match: a cloud has no descriptors (compute_fpfh or set_descriptors first)");
  if (c0->fd != c1->fd)
    return fail(CLIPPER_HIP_E_INVALID, "cloud_match: descriptors of %d and %d coordinates", c0->fd, c1->fd);
  const int64_t n0 = c0->n, n1 = c1->n;
  const std::string why = cm::check_args(c0->F.get(), n0, c1->F.get(), n1, c0->fd, &prm);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "cloud_match: %s", why.c_str());
  if (n0 * prm.knn > INT32_MAX)
    return fail(CLIPPER_HIP_E_SCOPE, "cloud_match: %lld x %d candidate rows exceed 2^31 - 1", static_cast<long long>(n0), prm.knn);
  if (int rc = use_device(c0->device)) return rc;
  hipStream_t st = nullptr;
  std::vector<double> fd;  // (declared before tmp: its release waits for the device, so they outlive every copy)
  std::vector<int32_t> fi;
  DevTemps tmp;
  MatchLists L;
  if (int rc = match_lists(c0->device, prm, c0->fG, c0->Fpad.get(), n0, c1->Fpad.get(), n1, L, tmp, st)) return rc;
  int32_t *cnt = nullptr, *off = nullptr;
  const size_t nq = static_cast<size_t>(n0);
  if (int rc = tmp.alloc(c0->device, cnt, nq * sizeof(int32_t), off, (nq + 1) * sizeof(int32_t))) return rc;
  const dim3 qb(static_cast<unsigned>(ceil_div(n0, 256)));
  hipLaunchKernelGGL(k_match_select<0>, qb, dim3(256), 0, st, prm, L.oif, L.odf, n0, L.Kf, L.oib, L.Kb, cnt, nullptr,
                     static_cast<int64_t>(0), nullptr, nullptr);
  hipLaunchKernelGGL(k_row_scan<>, dim3(1), dim3(ROW_SCAN_THREADS), 0, st, cnt, static_cast<int32_t>(n0), off, nullptr, 1);
  int32_t rows = 0;
  HIPCHK(hipMemcpyAsync(&rows, off + nq, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // how many rows there are
  HIPCHK(hipGetLastError());
  if (rows < 0 || rows > n0 * prm.knn) return fail(CLIPPER_HIP_E_INTERNAL, "cloud_match: %d rows from %lld queries", rows, static_cast<long long>(n0));
  std::unique_ptr<Pairs> p(new Pairs);
  p->device = c0->device;
  p->m = rows;
  const size_t mm = static_cast<size_t>(rows);
  if (int rc = cloud_alloc(p->A, 2 * mm)) return rc;
  if (int rc = cloud_alloc(p->sqd, mm)) return rc;
  if (rows > 0)
    hipLaunchKernelGGL(k_match_select<1>, qb, dim3(256), 0, st, prm, L.oif, L.odf, n0, L.Kf, L.oib, L.Kb, nullptr, off,
                       static_cast<int64_t>(rows), p->A.get(), p->sqd.get());
  if (nn_idx_out || nn_sqd_out) {
    fd.resize(L.nof), fi.resize(L.nof);
    if (int rc = copy_down(fd.data(), L.odf, L.nof, st)) return rc;
    if (int rc = copy_down(fi.data(), L.oif, L.nof, st)) return rc;
  }
  if (int rc = cloud_wait(st)) return rc;
  for (int64_t i = 0; i < n0 && !fi.empty(); ++i)
    for (int k = 0; k < prm.knn; ++k) {
      if (nn_idx_out) nn_idx_out[i * prm.knn + k] = fi[static_cast<size_t>(i) * L.Kf + k];
      if (nn_sqd_out) nn_sqd_out[i * prm.knn + k] = fd[static_cast<size_t>(i) * L.Kf + k];
    }
  *out = p.release();
  return 0;
}

// max |x| over the `count` numbers at in, to *out on the device: partial results of up to CLOUD_MAXABS_BLOCKS workgroups
// at part (zeroed by the caller where no workgroup writes)
void cloud_maxabs_partials(const double* in, int64_t count, double* part, hipStream_t st) {
  const unsigned nb = static_cast<unsigned>(std::min<int64_t>(CLOUD_MAXABS_BLOCKS, ceil_div(count, 256)));
  hipLaunchKernelGGL(k_cloud_maxabs<>, dim3(nb), dim3(256), 0, st, in, count, part);
}

// clipper_hip_stage_inputs from device data: the point tables are gathered by the pairs with device-to-device traffic
// only (stage_inputs' StagedInputs route), max |coordinate| is folded on the device, and the pairs come down once, for
// the host copy of A the solver's rounding reads. d = 3, or 6 (point, then normal) with with_normals.
int stage_inputs_clouds(Ctx* h, const Cloud* c0, const Cloud* c1, const Pairs* pairs, int with_normals) {
  if (!h || !c0 || !c1 || !pairs) return fail(CLIPPER_HIP_E_INVALID, "stage_inputs_clouds: null handle");
  if (h->multiproc || h->world != 1 || h->sh.size() != 1)
    return fail(CLIPPER_HIP_E_SCOPE, "stage_inputs_clouds: one-shard contexts only (this one holds column shards)");
  const int device = h->sh[0].device;
  if (c0->device != device || c1->device != device || pairs->device != device)
    return fail(CLIPPER_HIP_E_INVALID, "stage_inputs_clouds: the context lives on device %d, the clouds on %d and %d, the pairs on %d",
                device, c0->device, c1->device, pairs->device);
  if (c0->n < 1 || c1->n < 1) return fail(CLIPPER_HIP_E_INVALID, "stage_inputs_clouds: a cloud has no points");
  if (pairs->m < 1)
    return fail(CLIPPER_HIP_E_INVALID, "stage_inputs_clouds: no associations (the all-to-all hypothesis is not built for clouds)");
  if (with_normals && (!c0->N || !c1->N))
    return fail(CLIPPER_HIP_E_STATE, "stage_inputs_clouds: with_normals needs the normals of both clouds");
  if (int rc = use_device(device)) return rc;
  hipStream_t st = nullptr;
  const int d = with_normals ? 6 : 3;
  const int64_t n0 = c0->n, n1 = c1->n;
  std::vector<int32_t> A(static_cast<size_t>(2 * pairs->m));
  DevTemps tmp;
  const double *D1 = c0->P.get(), *D2 = c1->P.get();
  if (with_normals) {
    double *t0 = nullptr, *t1 = nullptr;
    if (int rc = tmp.alloc(device, t0, static_cast<size_t>(n0) * 6 * sizeof(double), t1, static_cast<size_t>(n1) * 6 * sizeof(double)))
      return rc;
    hipLaunchKernelGGL(k_cloud_point_normal<>, dim3(static_cast<unsigned>(ceil_div(6 * n0, 256))), dim3(256), 0, st, c0->P.get(),
                       c0->N.get(), n0, t0);
    hipLaunchKernelGGL(k_cloud_point_normal<>, dim3(static_cast<unsigned>(ceil_div(6 * n1, 256))), dim3(256), 0, st, c1->P.get(),
                       c1->N.get(), n1, t1);
    D1 = t0, D2 = t1;
  }
  double* part = nullptr;
  const size_t nparts = 2 * CLOUD_MAXABS_BLOCKS;
  if (int rc = tmp.alloc(device, part, (nparts + 1) * sizeof(double))) return rc;
  HIPCHK(hipMemsetAsync(part, 0, (nparts + 1) * sizeof(double), st));
  cloud_maxabs_partials(D1, d * n0, part, st);
  cloud_maxabs_partials(D2, d * n1, part + CLOUD_MAXABS_BLOCKS, st);
  hipLaunchKernelGGL(k_cloud_maxabs<>, dim3(1), dim3(256), 0, st, part, static_cast<int64_t>(nparts), part + nparts);
  StagedInputs dev;
  dev.D1 = D1, dev.D2 = D2, dev.A = pairs->A.get();
  if (int rc = copy_down(&dev.maxabs, part + nparts, 1, st)) return rc;
  if (int rc = copy_down(A.data(), pairs->A.get(), A.size(), st)) return rc;  // the one download of the pairs
  if (int rc = cloud_wait(st)) return rc;
  if (!(dev.maxabs >= 0.0)) return fail(CLIPPER_HIP_E_INTERNAL, "stage_inputs_clouds: max |coordinate| = %g", dev.maxabs);
  if (int rc = stage_inputs(h, nullptr, d, n0, nullptr, n1, A.data(), pairs->m, &dev)) return rc;
  HIPCHK(hipStreamSynchronize(h->sh[0].stream));  // (the tables are gathered: the clouds and the pairs may go)
  return 0;
}

// the k points idx names, in the order of the list, to the host: 3 x k as `clipper::Data`
int cloud_gather_points(const Cloud* c, const int32_t* idx, int64_t k, double* out) {
  if (!c) return fail(CLIPPER_HIP_E_INVALID, "cloud_gather_points: null handle");
  if (k < 0 || k > INT32_MAX) return fail(CLIPPER_HIP_E_INVALID, "cloud_gather_points: k = %lld outside 0 .. 2^31 - 1", static_cast<long long>(k));
  if (k > 0 && (!idx || !out)) return fail(CLIPPER_HIP_E_INVALID, "cloud_gather_points: null %s", !idx ? "index array" : "output array");
  for (int64_t r = 0; r < k; ++r)
    if (idx[r] < 0 || idx[r] >= c->n)
      return fail(CLIPPER_HIP_E_INVALID, "cloud_gather_points: index %d at position %lld outside the cloud's %lld points", idx[r],
                  static_cast<long long>(r), static_cast<long long>(c->n));
  if (k == 0) return 0;
  if (int rc = use_device(c->device)) return rc;
  hipStream_t st = nullptr;
  int32_t* di = nullptr;
  double* dout = nullptr;
  DevTemps tmp;
  const size_t kk = static_cast<size_t>(k);
  if (int rc = tmp.alloc(c->device, di, kk * sizeof(int32_t), dout, kk * 3 * sizeof(double))) return rc;
  if (int rc = copy_up(di, idx, kk, st)) return rc;
  hipLaunchKernelGGL(k_cloud_gather<>, dim3(static_cast<unsigned>(ceil_div(3 * k, 256))), dim3(256), 0, st, c->P.get(), di, k, dout);
  if (int rc = copy_down(out, dout, kk * 3, st)) return rc;
  return cloud_wait(st);
}

// icp_body on two clouds: the method picks point-to-point, point-to-plane (the target's normals) or generalized (both
// clouds' covariances); robust may be null. The target's index or bounding box is its KnnTarget's, kept between calls.
// T_out null with corr_out: clipper_hip_cloud_evaluate_registration.
int cloud_icp_run(const char* who, const Cloud* src, Cloud* tgt, const double* T0, const clipper_icp::Params& prm,
                  const clipper_icp::Robust* rb, double* T_out, clipper_icp_info_t* info, clipper_icp_robust_info_t* rinfo,
                  double* history, int32_t* corr_out) {
  if (src->device != tgt->device)
    return fail(CLIPPER_HIP_E_INVALID, "%s: the clouds live on devices %d and %d", who, src->device, tgt->device);
  if (src->n < 1 || tgt->n < 1) return fail(CLIPPER_HIP_E_INVALID, "%s: a cloud needs at least one point", who);
  if (prm.method == ICP_POINT_TO_PLANE && !tgt->N)
    return fail(CLIPPER_HIP_E_STATE, "%s: point-to-plane needs the target's normals (estimate them first)", who);
  if (prm.method == ICP_GENERALIZED && (!src->C || !tgt->C))
    return fail(CLIPPER_HIP_E_STATE, "%s: the generalized metric needs the covariances of both clouds (estimate them first)", who);
  if (int rc = use_device(tgt->device)) return rc;
  IcpInputs in;
  in.Ps = src->P.get(), in.Pt = tgt->P.get(), in.target = &tgt->target;
  in.Nt = prm.method == ICP_POINT_TO_PLANE ? tgt->N.get() : nullptr;
  if (prm.method == ICP_GENERALIZED) in.Cs = src->C.get(), in.Ct = tgt->C.get();
  DevTemps tmp;
  return icp_body(tgt->device, in, src->n, tgt->n, T0 ? T0 : ICP_IDENTITY, prm, T_out, info, history, corr_out, rb, rinfo, tmp);
}

int cloud_icp(const Cloud* src, Cloud* tgt, const double* T_init, const clipper_icp_params_t* params,
              const clipper_icp_robust_t* robust, double* T_out, clipper_icp_info_t* info, clipper_icp_robust_info_t* robust_info,
              double* history) {
  namespace ci = clipper_icp;
  if (!src || !tgt) return fail(CLIPPER_HIP_E_INVALID, "cloud_icp: null cloud handle");
  const ci::Params h = icp_params_of(params);
  const ci::Robust rb = icp_robust_of(robust);
  const std::string why = ci::check_call(ci::FAMILY_BY_METHOD, ci::ROBUST_OPTIONAL, params ? &h : nullptr, robust ? &rb : nullptr,
                                         T_out != nullptr, T_init, nullptr);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "cloud_icp: %s", why.c_str());
  return cloud_icp_run("cloud_icp", src, tgt, T_init, h, robust ? &rb : nullptr, T_out, info, robust ? robust_info : nullptr,
                       history, nullptr);
}

int cloud_evaluate_registration(const Cloud* src, Cloud* tgt, const double* T, double max_distance, double* fitness,
                                double* inlier_rmse, int64_t* count, int32_t* corr_out) {
  namespace ci = clipper_icp;
  if (!src || !tgt) return fail(CLIPPER_HIP_E_INVALID, "cloud_evaluate_registration: null cloud handle");
  std::string why = ci::check_max_distance(max_distance);
  if (why.empty()) why = ci::check_transform("T", T);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "cloud_evaluate_registration: %s", why.c_str());
  const ci::Params h{ICP_POINT_TO_POINT, 0, max_distance, 0.0, 0.0};
  clipper_icp_info_t info{};
  if (int rc = cloud_icp_run("cloud_evaluate_registration", src, tgt, T, h, nullptr, nullptr, &info, nullptr, nullptr, corr_out))
    return rc;
  icp_evaluation_out(info, fitness, inlier_rmse, count);
  return 0;
}

}  // namespace
