// host_voxel.hpp — voxel down-sampling of a point cloud (the step in front of the normals): the driver of
// clipper_hip_voxel_downsample. The host's finiteness scan yields the cloud's corners, so the grid and the number of
// sort passes are planned before anything is queued; then keys, the passes of the radix sort (histogram, scan,
// scatter), the segments (heads, scan, rows) and the sums (partials of the long voxels, reduce) are queued on one
// stream with no host wait in between. The call waits once for the kernels (n_out decides how many rows come down)
// and once for the copies. Stand-alone: needs no context. The checks are host_voxel_check.hpp's, the frame
// host_call.hpp's. Part of clipper_hip.hip (one translation unit; included there after host_icp.hpp).
#pragma once

#include "host_voxel_check.hpp"

namespace {

// four events (around the kernels, and around the sort's passes among them), released on every path
struct VoxelEvents {
  Event a, b, sa, sb;
};

// what the body leaves on the device (tmp's arrays, sized for n rows) and what the host knows of it after its one wait
struct VoxelResult {
  double *dPo = nullptr, *dNo = nullptr;  // rows x 3: the centroids; the normalised normal sums (with normals)
  int32_t *dcnt = nullptr, *dtrace = nullptr;  // rows: the members per voxel; n: each input point's row (with want_trace)
  int32_t rows = 0, max_count = 0;
  float ms = 0.f, sort_ms = 0.f;
};

// THE BODY of the down-sampling, on device pointers: dP the cloud (n x 3), dN its normals or null; n >= 1. Everything is
// queued on st and waited for once (the number of rows decides what the caller copies). The host-buffer call (below)
// and the call on a cloud (host_cloud.hpp) both run this.
int voxel_body(int device, const double* dP, const double* dN, int64_t n_, const clipper_voxel::Plan& plan, bool want_trace,
               VoxelResult& R, hipStream_t st, DevTemps& tmp) {
  const int32_t n = static_cast<int32_t>(n_);
  const size_t nn = static_cast<size_t>(n), n3 = nn * 3;
  const int32_t ntiles = static_cast<int32_t>(ceil_div(n_, SORT_TILE));
  const int32_t ntable = ntiles * SORT_RADIX;  // (n < 2^31: at most 2^20 tiles of 2^8 digits)
  const size_t nslots = static_cast<size_t>(vx_partial_slots(n_));

  double* dpart = nullptr;
  unsigned long long* keys[2] = {nullptr, nullptr};
  int32_t* idx[2] = {nullptr, nullptr};
  int32_t *table = nullptr, *first = nullptr, *heads = nullptr, *tile_first = nullptr, *row = nullptr, *start = nullptr,
          *dmax = nullptr, *totals = nullptr;
  VoxelEvents ev;
  const bool sorts = plan.passes > 0;
  if (int rc = tmp.alloc(device, keys[0], nn * sizeof(unsigned long long), idx[0], nn * sizeof(int32_t),
                         keys[1], (sorts ? nn : 0) * sizeof(unsigned long long), idx[1], (sorts ? nn : 0) * sizeof(int32_t),
                         table, static_cast<size_t>(sorts ? ntable : 0) * sizeof(int32_t),
                         first, (static_cast<size_t>(sorts ? ntable : 0) + 1) * sizeof(int32_t),
                         heads, static_cast<size_t>(ntiles) * sizeof(int32_t),
                         tile_first, (static_cast<size_t>(ntiles) + 1) * sizeof(int32_t), row, nn * sizeof(int32_t),
                         start, (nn + 1) * sizeof(int32_t), dpart, nslots * 6 * sizeof(double), R.dPo, n3 * sizeof(double),
                         R.dNo, (dN ? n3 : 0) * sizeof(double), R.dcnt, nn * sizeof(int32_t),
                         R.dtrace, (want_trace ? nn : 0) * sizeof(int32_t), dmax, sizeof(int32_t),
                         totals, static_cast<size_t>(8 * SORT_RADIX) * sizeof(int32_t)))
    return rc;
  HIPCHK(ev.a.create());
  HIPCHK(ev.b.create());
  HIPCHK(ev.sa.create());
  HIPCHK(ev.sb.create());

  HIPCHK(hipMemsetAsync(dmax, 0, sizeof(int32_t), st));
  HIPCHK(hipMemsetAsync(totals, 0, static_cast<size_t>(8 * SORT_RADIX) * sizeof(int32_t), st));  // 256 per pass, <= 8 passes

  const dim3 per_point(static_cast<unsigned>(ceil_div(n_, 256))), per_tile(static_cast<unsigned>(ntiles));
  HIPCHK(hipEventRecord(ev.a, st));
  hipLaunchKernelGGL(k_vx_keys<>, per_point, dim3(256), 0, st, dP, n, plan.g, keys[0], idx[0]);
  HIPCHK(hipEventRecord(ev.sa, st));
  int cur = 0;
  for (int pass = 0; pass < plan.passes; ++pass, cur ^= 1) {
    int32_t* const tot = totals + pass * SORT_RADIX;
    hipLaunchKernelGGL(k_sort_hist<>, per_tile, dim3(SORT_THREADS), 0, st, keys[cur], n, pass, ntiles, table, tot);
    hipLaunchKernelGGL(k_row_scan<>, dim3(SORT_RADIX), dim3(ROW_SCAN_THREADS), 0, st, table, ntiles, first, nullptr, 0);
    hipLaunchKernelGGL(k_sort_scatter<>, per_tile, dim3(SORT_THREADS), 0, st, keys[cur], idx[cur], n, pass, ntiles, first, tot,
                       keys[cur ^ 1], idx[cur ^ 1]);
  }
  HIPCHK(hipEventRecord(ev.sb, st));
  const unsigned long long* sk = keys[cur];
  const int32_t* si = idx[cur];
  hipLaunchKernelGGL(k_vx_heads<>, per_tile, dim3(SORT_THREADS), 0, st, sk, n, heads);
  hipLaunchKernelGGL(k_row_scan<>, dim3(1), dim3(ROW_SCAN_THREADS), 0, st, heads, ntiles, tile_first, nullptr, 1);
  hipLaunchKernelGGL(k_vx_rows<>, per_tile, dim3(SORT_THREADS), 0, st, sk, si, n, tile_first, row, start,
                     want_trace ? R.dtrace : nullptr);
  hipLaunchKernelGGL(k_vx_partials<>, per_point, dim3(256), 0, st, dP, dN, n, plan.g, si, row, start, dpart);
  hipLaunchKernelGGL(k_vx_reduce<>, per_point, dim3(256), 0, st, dP, dN, n, plan.g, si, tile_first + ntiles, start,
                     dpart, R.dPo, R.dNo, R.dcnt, dmax);
  HIPCHK(hipEventRecord(ev.b, st));

  HIPCHK(hipMemcpyAsync(&R.rows, tile_first + ntiles, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&R.max_count, dmax, sizeof(int32_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // the kernels: how many rows there are
  HIPCHK(hipGetLastError());
  if (R.rows < 1 || R.rows > n) return fail(CLIPPER_HIP_E_INTERNAL, "voxel_downsample: %d rows from %d points", R.rows, n);
  HIPCHK(hipEventElapsedTime(&R.ms, ev.a, ev.b));
  if (sorts) HIPCHK(hipEventElapsedTime(&R.sort_ms, ev.sa, ev.sb));
  return 0;
}

// what the call reports of its plan before anything runs
void voxel_info_begin(clipper_voxel_info_t* info, const clipper_voxel::Plan& plan, int64_t n) {
  if (!info) return;
  for (int a = 0; a < 3; ++a) info->dim[a] = n > 0 ? plan.g.dim[a] : 0;
  info->passes = plan.passes;
  info->sort_tile = SORT_TILE;
  info->chunk = VOXEL_CHUNK;
  info->max_count = 0;
  info->reserved = 0;
  info->kernels_ms = 0.0;
  info->sort_ms = 0.0;
}

void voxel_info_end(clipper_voxel_info_t* info, const VoxelResult& R) {
  if (!info) return;
  info->max_count = R.max_count;
  info->kernels_ms = static_cast<double>(R.ms);
  info->sort_ms = static_cast<double>(R.sort_ms);
}

// The host-buffer frame around the body. Every argument has been checked; n >= 1.
int voxel_run(int device, const double* P, const double* N, int64_t n_, const clipper_voxel::Plan& plan, double* P_out,
              double* N_out, int32_t* count_out, int32_t* trace_out, int64_t* n_out, clipper_voxel_info_t* info) {
  const size_t nn = static_cast<size_t>(n_), n3 = nn * 3;
  double *dP = nullptr, *dN = nullptr;
  DevTemps tmp;
  if (int rc = tmp.alloc(device, dP, n3 * sizeof(double), dN, (N ? n3 : 0) * sizeof(double))) return rc;
  hipStream_t st = nullptr;  // the default stream: a stand-alone call
  if (int rc = copy_up(dP, P, n3, st)) return rc;
  if (N)
    if (int rc = copy_up(dN, N, n3, st)) return rc;
  VoxelResult R;
  if (int rc = voxel_body(device, dP, N ? dN : nullptr, n_, plan, trace_out != nullptr, R, st, tmp)) return rc;
  const size_t nr = static_cast<size_t>(R.rows);
  if (int rc = copy_down(P_out, R.dPo, nr * 3, st)) return rc;
  if (N)
    if (int rc = copy_down(N_out, R.dNo, nr * 3, st)) return rc;
  if (int rc = copy_down(count_out, R.dcnt, nr, st)) return rc;
  if (int rc = copy_down(trace_out, R.dtrace, nn, st)) return rc;
  HIPCHK(hipStreamSynchronize(st));  // the copies
  *n_out = R.rows;
  voxel_info_end(info, R);
  return 0;
}

int voxel_downsample(int device, const double* P, const double* N, int64_t n, double voxel_size, double* P_out, double* N_out,
                     int32_t* count_out, int32_t* trace_out, int64_t* n_out, clipper_voxel_info_t* info) {
  clipper_voxel::Plan plan{};
  const std::string why = clipper_voxel::check_all(P, N, n, voxel_size, n_out, N_out, plan);
  if (!why.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", why.c_str());
  if (int rc = use_device(device)) return rc;
  *n_out = 0;
  voxel_info_begin(info, plan, n);
  if (n == 0) return 0;  // an empty cloud has no voxels
  return voxel_run(device, P, N, n, plan, P_out, N_out, count_out, trace_out, n_out, info);
}

}  // namespace
