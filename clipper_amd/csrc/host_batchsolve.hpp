// host_batchsolve.hpp — batched solves: many independent small problems in one call.
// Part of clipper_hip.hip (one translation unit; included there, after the context's helpers).
//
// A batch owns one child context per problem slot, all on the batch's device and ONE stream (the children borrow it).
// A call
//   1. checks every problem (nothing reaches the device if one is invalid),
//   2. stages all inputs (D1, D2, the association lists, u0) in one pinned buffer and copies it with ONE H2D copy,
//   3. queues every child's fill back to back (run_affinity in its deferred mode) and waits ONCE; children whose
//      slice arenas overflowed (the first use of a size) fill again, in a second round of their own. A user-defined
//      invariant (kind 3, batch_fill_custom) fills every child's dense store in ONE launch instead, then queues the
//      children's slice builds back to back and waits once per round of builds,
//   4. plans each child exactly as a lone solve would (the fill's own slices_plan -> resident_plan): the unit split,
//      hence the order of every addition, is the lone solve's,
//   5. packs the resident plans into launches of k_solve_resident_batch (host_batchpack.hpp), queues them back to
//      back and waits once,
//   6. solves alone, on its child context's ordinary path, every problem with no resident plan or whose launch gave
//      up or was refused,
//   7. rounds each problem on the host with the lone solve's code.
// Per problem the results are bit for bit those of a lone context on the same route; only `seconds` differs (the
// wall time of the whole call).
// batch_sdp (at the end) runs the semidefinite relaxation of every problem of the last call in one batched call
// (host_sdpbatch.hpp) on the children's stores.
#pragma once

#include "host_batchpack.hpp"

struct clipper_hip_batch {
  int device = 0;
  int storage = CLIPPER_HIP_STORE_F32_CSC;
  hipStream_t stream = nullptr;
  std::vector<Ctx*> kids;  // one per problem slot, kept from call to call
  struct Result {
    std::vector<double> u;
    std::vector<int32_t> nodes;
    std::vector<int32_t> sel;  // selected associations, column-major k x 2
    clipper_solve_info_t info{};
    int route = 0;
  };
  std::vector<Result> res;  // of the last call
  int launches = 0, n_batched = 0, n_alone = 0;
  double t_fill = 0.0, t_launch = 0.0, t_alone = 0.0, t_round = 0.0;
  uint8_t* hstage = nullptr;  // pinned staging of the inputs, then of the launch tables
  size_t hstage_cap = 0;
  uint8_t* dstage = nullptr;  // its device copy
  size_t dstage_cap = 0;
  uint8_t* hfill = nullptr;  // pinned staging of a custom fill's problems and tiles (kind 3)
  size_t hfill_cap = 0;
  uint8_t* dfill = nullptr;  // its device copy
  size_t dfill_cap = 0;
  hipEvent_t ev_fill[2] = {nullptr, nullptr};  // around a custom fill's launch
  double t_fill_begin = 0.0, t_fill_launch = 0.0, t_fill_build = 0.0;  // kind 3: the parts of t_fill (ms)
  bool solved = false;                  // a solve call has succeeded: `res` and the children describe its problems
  std::unique_ptr<SdpBatchState> sdp;   // the last clipper_hip_batch_sdp (host_sdpbatch.hpp), until the next call
};

namespace {

using Batch = clipper_hip_batch;

// a pinned buffer and its device copy of at least `bytes` each (contents lost when they grow)
int stage_grow(uint8_t*& hbuf, size_t& hcap, uint8_t*& dbuf, size_t& dcap, size_t bytes) {
  if (bytes > hcap) {
    if (hbuf) HIPCHK(hipHostFree(hbuf));
    hbuf = nullptr;
    hcap = 0;
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&hbuf), bytes, hipHostMallocDefault));
    hcap = bytes;
  }
  if (bytes > dcap) {
    if (dbuf) HIPCHK(hipFree(dbuf));
    dbuf = nullptr;
    dcap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&dbuf), bytes));
    dcap = bytes;
  }
  return 0;
}

int batch_grow(Batch* b, size_t bytes) { return stage_grow(b->hstage, b->hstage_cap, b->dstage, b->dstage_cap, bytes); }

// Step 3 for a user-defined invariant (kind 3). Every child: its inputs staged, then fill_custom's and run_affinity's
// steps before a launch (custom_fill_begin, affinity_begin: the dense store allocated). Then ONE launch of the
// batched fill kernel over every child's tiles (the lone kernel's grid, problem after problem), whose descriptors and
// tile table reach the device in one copy of their own. Then csc_rebuild in its deferred form: every compressed child's
// build queued back to back, one wait, the checks; children that overflowed build again (three builds at most, as
// pack_until_fits allows). Dense storages keep their store. A child's affinity_kernel_ms is the batched launch's time
// (shared by every problem of the call), without the build.
int batch_fill_custom(Batch* b, const clipper_batch_problem_t* p, int32_t n, int d,
                      const std::vector<std::vector<int32_t>>& Afull, const std::vector<StagedInputs>& dev,
                      const std::vector<size_t>& off_u0, const CustomFill& cf) {
  const auto t0 = std::chrono::high_resolution_clock::now();
  hipFunction_t fn = nullptr;
  size_t ntiles = 0;
  for (int32_t i = 0; i < n; ++i) {
    Ctx* c = b->kids[static_cast<size_t>(i)];
    const clipper_batch_problem_t& q = p[i];
    const std::vector<int32_t>& A = Afull[static_cast<size_t>(i)];
    const int64_t m = static_cast<int64_t>(A.size() / 2);
    if (int rc = stage_inputs(c, q.D1, d, q.n1, q.D2, q.n2, A.data(), m, &dev[static_cast<size_t>(i)])) return rc;
    std::vector<hipFunction_t> f;
    if (int rc = custom_fill_begin(c, cf, true, f)) return rc;
    fn = f[0];
    bool emit = false, rect = false;
    if (int rc = affinity_begin(c, false, emit, rect)) return rc;
    if (emit || rect) return fail(CLIPPER_HIP_E_INTERNAL, "problem %d: a custom fill goes through the dense store", i);
    c->csc_emitted = false;  // (as run_affinity's launch loop leaves a fill that does not emit)
    c->csc_out = CscOut{};
    HIPCHK(hipMemcpyAsync(c->sh[0].u0, b->dstage + off_u0[static_cast<size_t>(i)], static_cast<size_t>(m) * 8,
                          hipMemcpyDeviceToDevice, b->stream));
    c->u0_staged = true;
    ntiles += static_cast<size_t>(ceil_div(c->W, 1024) * ceil_div(m, AFF_ROWS_PER_BLK));
  }
  if (ntiles > 0x7fffffffu) return fail(CLIPPER_HIP_E_SCOPE, "a batched fill of %zu workgroups", ntiles);

  // the problems and the tile table: one copy, one launch
  const size_t pbytes = static_cast<size_t>(round_up(static_cast<int64_t>(n) * sizeof(CustomFillProblem), 256));
  if (int rc = stage_grow(b->hfill, b->hfill_cap, b->dfill, b->dfill_cap, pbytes + ntiles * sizeof(CustomFillTile)))
    return rc;
  CustomFillProblem* probs = reinterpret_cast<CustomFillProblem*>(b->hfill);
  CustomFillTile* tiles = reinterpret_cast<CustomFillTile*>(b->hfill + pbytes);
  size_t t = 0;
  for (int32_t i = 0; i < n; ++i) {
    const Ctx* c = b->kids[static_cast<size_t>(i)];
    const Shard& s = c->sh[0];
    probs[i] = CustomFillProblem{s.S, c->W, c->m, s.P1, s.P2, c->staged_pstride, s.Adev, s.Adev + c->m};
    const int nc = static_cast<int>(ceil_div(c->W, 1024)), nr = static_cast<int>(ceil_div(c->m, AFF_ROWS_PER_BLK));
    for (int y = 0; y < nr; ++y)
      for (int x = 0; x < nc; ++x) tiles[t++] = CustomFillTile{i, x, y};
  }
  HIPCHK(hipMemcpyAsync(b->dfill, b->hfill, pbytes + ntiles * sizeof(CustomFillTile), hipMemcpyHostToDevice, b->stream));
  if (!b->ev_fill[0]) {
    HIPCHK(hipEventCreate(&b->ev_fill[0]));
    HIPCHK(hipEventCreate(&b->ev_fill[1]));
  }
  const auto t1 = std::chrono::high_resolution_clock::now();
  {
    const CustomFillProblem* dprobs = reinterpret_cast<const CustomFillProblem*>(b->dfill);
    const CustomFillTile* dtiles = reinterpret_cast<const CustomFillTile*>(b->dfill + pbytes);
    int rows = AFF_ROWS_PER_BLK;
    CustomParams prm = cf.prm;
    void* args[] = {&dprobs, &dtiles, &rows, &prm};
    HIPCHK(hipEventRecord(b->ev_fill[0], b->stream));
    const hipError_t e = hipModuleLaunchKernel(fn, static_cast<unsigned>(ntiles), 1, 1, 256, 1, 1, 0, b->stream, args,
                                               nullptr);
    if (e != hipSuccess)
      return fail(CLIPPER_HIP_E_HIP, "hipModuleLaunchKernel (user-defined invariant, batched): %s", hipGetErrorString(e));
    HIPCHK(hipEventRecord(b->ev_fill[1], b->stream));
  }

  // the slice builds: queued back to back, one wait per round
  std::vector<int32_t> todo;
  for (int32_t i = 0; i < n; ++i)
    if (csc_applies(b->kids[static_cast<size_t>(i)])) todo.push_back(i);
  float kms = 0.f;
  int rounds = 0;
  for (int round = 0;; ++round) {
    rounds = round + 1;
    for (int32_t i : todo)
      if (int rc = csc_build_enqueue(b->kids[static_cast<size_t>(i)])) return rc;
    if (hipStreamSynchronize(b->stream) != hipSuccess)
      return fail(CLIPPER_HIP_E_HIP, "batched custom fill: %s", hipGetErrorString(hipGetLastError()));
    if (round == 0) HIPCHK(hipEventElapsedTime(&kms, b->ev_fill[0], b->ev_fill[1]));
    std::vector<int32_t> again_list;
    for (int32_t i : todo) {
      bool again = false;
      if (int rc = csc_build_complete(b->kids[static_cast<size_t>(i)], again)) return rc;
      if (again) again_list.push_back(i);
    }
    if (again_list.empty()) break;
    if (round >= 2) return fail(CLIPPER_HIP_E_HIP, "compressed storage: the build keeps overflowing");
    todo.swap(again_list);
  }
  for (int32_t i = 0; i < n; ++i) fill_held(b->kids[static_cast<size_t>(i)], kms);
  const auto t2 = std::chrono::high_resolution_clock::now();
  b->t_fill_begin = std::chrono::duration<double, std::milli>(t1 - t0).count();
  b->t_fill_launch = kms;
  b->t_fill_build = std::chrono::duration<double, std::milli>(t2 - t1).count();
  if (std::getenv("CLIPPER_HIP_HOST_TIMING"))
    std::fprintf(stderr, "[batch-custom] n = %d: stage + begin (dense stores) %.3f ms, %zu tiles %.3f ms (events), "
                 "launch + builds %.3f ms, %d build round%s\n", n, b->t_fill_begin, ntiles, b->t_fill_launch,
                 b->t_fill_build, rounds, rounds == 1 ? "" : "s");
  return 0;
}

template <typename VT, int V, int E>
int batch_launch_t(Batch* b, unsigned grid, const ResidentLaunchEntry* table, const ResidentArgs* args) {
  auto kern = k_solve_resident_batch<VT, V, E>;
  static std::atomic<bool> attr_set[64] = {};  // per instantiation and device
  const int dv = (b->device >= 0 && b->device < 64) ? b->device : 0;
  if (!attr_set[dv]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                            static_cast<int>(RS_LDS_MAX)) != hipSuccess) {
      (void)hipGetLastError();
      return 1;  // no 159 KB of LDS for a workgroup on this device: the problems are solved alone
    }
    attr_set[dv] = true;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(RS_NT), RS_LDS_MAX, b->stream, table, args);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    if (rs_debug()) std::fprintf(stderr, "[batch] launch failed: %s\n", hipGetErrorString(e));
    return 1;
  }
  return 0;
}

// key = VT (0: float, 1: double) * 100 + V * 10 + E
int batch_launch(Batch* b, int key, unsigned grid, const ResidentLaunchEntry* table, const ResidentArgs* args) {
  const bool f64 = key >= 100;
  switch (key % 100) {
#define BATCH_CASE(V, E)                                                                            \
  case V * 10 + E:                                                                                  \
    return f64 ? batch_launch_t<double, V, E>(b, grid, table, args) : batch_launch_t<float, V, E>(b, grid, table, args);
    BATCH_CASE(1, 1)
    BATCH_CASE(1, 2)
    BATCH_CASE(1, 4)
    BATCH_CASE(2, 1)
    BATCH_CASE(2, 2)
    BATCH_CASE(2, 4)
#undef BATCH_CASE
    default: return 1;
  }
}

// kind 1: EuclideanDistance (f = {sigma, epsilon, mindist}), 2: PointNormalDistance (f = {sigp, epsp, sign, epsn}),
// 3: a user-defined invariant (cf; d = its dimension)
int batch_solve(Batch* b, const clipper_batch_problem_t* p, int32_t n, int d, int kind, const double* f,
                const clipper_params_t* P, const CustomFill* cf = nullptr) {
  const auto t0 = std::chrono::high_resolution_clock::now();
  b->res.clear();
  b->solved = false;
  b->sdp.reset();
  b->launches = b->n_batched = b->n_alone = 0;
  b->t_fill = b->t_launch = b->t_alone = b->t_round = 0.0;
  b->t_fill_begin = b->t_fill_launch = b->t_fill_build = 0.0;
  // ---- 1. every problem checked before any device work -------------------------------------------------------------
  SolverParams prm;
  if (int rc = solver_params(P, prm)) return rc;
  if (n < 0 || (n > 0 && !p)) return fail(CLIPPER_HIP_E_INVALID, "invalid problem list");
  if (kind == 2 && d != 6) return fail(CLIPPER_HIP_E_INVALID, "PointNormalDistance data are 6 x n");
  if (kind == 3 && (!cf || d != cf->inv->d)) return fail(CLIPPER_HIP_E_INVALID, "no invariant of dimension d = %d", d);
  if (d < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid dimension d = %d", d);
  std::vector<std::vector<int32_t>> Afull(static_cast<size_t>(n));  // the lists as stage_inputs holds them
  size_t bytes = 0;
  for (int32_t i = 0; i < n; ++i) {
    const clipper_batch_problem_t& q = p[i];
    if (!q.D1 || !q.D2 || q.n1 < 1 || q.n2 < 1) return fail(CLIPPER_HIP_E_INVALID, "problem %d: invalid point data", i);
    if (!q.u0) return fail(CLIPPER_HIP_E_INVALID, "problem %d: u0 is required", i);
    if (q.m < 0) return fail(CLIPPER_HIP_E_INVALID, "problem %d: m = %lld", i, static_cast<long long>(q.m));
    const int64_t m = (q.A == nullptr || q.m == 0) ? q.n1 * q.n2 : q.m;  // (all pairs: association_list)
    if (m > 0x7fffffff) return fail(CLIPPER_HIP_E_INVALID, "problem %d: %lld associations", i, static_cast<long long>(m));
    if (association_list(q.A, q.m, q.n1, q.n2, Afull[static_cast<size_t>(i)]))
      return fail(CLIPPER_HIP_E_INVALID, "problem %d: %s", i, std::string(g_err).c_str());
    bytes += static_cast<size_t>(round_up(static_cast<int64_t>(d) * (q.n1 + q.n2) * 8 + m * 16 + m * 8, 256));
  }
  b->res.resize(static_cast<size_t>(n));
  if (n == 0) {
    b->solved = true;
    return 0;
  }
  HIPCHK(hipSetDevice(b->device));
  while (b->kids.size() < static_cast<size_t>(n)) {
    Ctx* c = make_ctx(&b->device, 1, b->storage, 1, 0, false);
    if (!c) return CLIPPER_HIP_E_HIP;
    hipStreamDestroy(c->sh[0].stream);
    c->sh[0].stream = b->stream;
    c->borrowed_stream = true;
    b->kids.push_back(c);
  }

  // ---- 2. the inputs: one pinned buffer, one copy ------------------------------------------------------------------
  if (int rc = batch_grow(b, bytes)) return rc;
  std::vector<StagedInputs> dev(static_cast<size_t>(n));
  std::vector<size_t> off_u0(static_cast<size_t>(n));
  {
    size_t o = 0;
    for (int32_t i = 0; i < n; ++i) {
      const clipper_batch_problem_t& q = p[i];
      const int64_t m = static_cast<int64_t>(Afull[static_cast<size_t>(i)].size() / 2);
      const size_t b1 = static_cast<size_t>(d) * q.n1 * 8, b2 = static_cast<size_t>(d) * q.n2 * 8;
      const size_t o0 = o;
      std::memcpy(b->hstage + o, q.D1, b1);
      dev[static_cast<size_t>(i)].D1 = reinterpret_cast<const double*>(b->dstage + o);
      o += b1;
      std::memcpy(b->hstage + o, q.D2, b2);
      dev[static_cast<size_t>(i)].D2 = reinterpret_cast<const double*>(b->dstage + o);
      o += b2;
      std::memcpy(b->hstage + o, q.u0, static_cast<size_t>(m) * 8);
      off_u0[static_cast<size_t>(i)] = o;
      o += static_cast<size_t>(m) * 8;
      std::memcpy(b->hstage + o, Afull[static_cast<size_t>(i)].data(), static_cast<size_t>(m) * 8);
      dev[static_cast<size_t>(i)].A = reinterpret_cast<const int32_t*>(b->dstage + o);
      o = o0 + static_cast<size_t>(round_up(static_cast<int64_t>(d) * (q.n1 + q.n2) * 8 + m * 16 + m * 8, 256));
    }
    HIPCHK(hipMemcpyAsync(b->dstage, b->hstage, o, hipMemcpyHostToDevice, b->stream));
  }

  // ---- 3. the fills, queued back to back; one wait; the overflowed ones again ----------------------------------------
  if (kind == 3) {
    if (int rc = batch_fill_custom(b, p, n, d, Afull, dev, off_u0, *cf)) return rc;
  } else {
    auto fill = [&](Ctx* c) -> int {
      c->fill_deferred = true;
      const int rc = kind == 1 ? fill_euclidean(c, EuclidParams{f[0], f[1], f[2], P->affinityeps})
                               : fill_pointnormal(c, PointNormalParams{f[0], f[1], f[2], f[3], P->affinityeps});
      c->fill_deferred = false;
      return rc;
    };
    for (int32_t i = 0; i < n; ++i) {
      Ctx* c = b->kids[static_cast<size_t>(i)];
      const clipper_batch_problem_t& q = p[i];
      const int64_t m = static_cast<int64_t>(Afull[static_cast<size_t>(i)].size() / 2);
      const std::vector<int32_t>& A = Afull[static_cast<size_t>(i)];
      if (int rc = stage_inputs(c, q.D1, d, q.n1, q.D2, q.n2, A.data(), m, &dev[static_cast<size_t>(i)])) return rc;
      if (int rc = fill(c)) return rc;
      HIPCHK(hipMemcpyAsync(c->sh[0].u0, b->dstage + off_u0[static_cast<size_t>(i)], static_cast<size_t>(m) * 8,
                            hipMemcpyDeviceToDevice, b->stream));
      c->u0_staged = true;
    }
    std::vector<int32_t> todo;
    for (int32_t i = 0; i < n; ++i) todo.push_back(i);
    for (int round = 0; !todo.empty(); ++round) {
      HIPCHK(hipStreamSynchronize(b->stream));
      std::vector<int32_t> again_list;
      for (int32_t i : todo) {
        bool again = false;
        if (int rc = fill_complete(b->kids[static_cast<size_t>(i)], again)) return rc;
        if (again) again_list.push_back(i);
      }
      if (again_list.empty()) break;
      if (round >= 2) return fail(CLIPPER_HIP_E_HIP, "compressed storage: the build keeps overflowing");
      for (int32_t i : again_list)
        if (int rc = fill(b->kids[static_cast<size_t>(i)])) return rc;
      todo.swap(again_list);
    }
  }
  const auto t1 = std::chrono::high_resolution_clock::now();
  b->t_fill = std::chrono::duration<double, std::milli>(t1 - t0).count();

  // ---- 4./5. the resident plans, packed into launches ----------------------------------------------------------------
  long long timeout_override = 0;  // (the lone solve's test knob)
  if (const char* e = std::getenv("CLIPPER_HIP_RESIDENT_TIMEOUT_TICKS")) timeout_override = std::atoll(e);
  std::vector<int32_t> batched, alone;
  std::vector<ResidentArgs> args;
  std::vector<clipper_batch::PackItem> items;
  for (int32_t i = 0; i < n; ++i) {
    Ctx* c = b->kids[static_cast<size_t>(i)];
    if (!resident_applies(c)) {
      alone.push_back(i);
      continue;
    }
    if (int rc = ensure_u_pinned(c)) return rc;
    ResidentArgs a = resident_args(c, prm, P->rescale_u0 != 0);
    // the lone solve's placement-free wait: 5 ms for one pass's sums, ten times as long on a context's first launch
    a.timeout_ticks = timeout_override ? timeout_override : 500000ll * (c->res.epoch == 0 ? 10 : 1);
    std::memset(c->mirror, 0, sizeof(HostMirror));
    batched.push_back(i);
    args.push_back(a);
    items.push_back({(c->esize() == 8 ? 100 : 0) + c->res.V * 10 + c->res.E, c->res.nunits});
  }
  std::atomic_thread_fence(std::memory_order_seq_cst);
  const int cap = std::max(1, b->kids[0]->cus - 8);
  std::vector<int> rejected;
  const std::vector<clipper_batch::PackLaunch> L = clipper_batch::pack_launches(items, cap, &rejected);
  std::vector<char> launched(batched.size(), 0);
  for (int k : rejected) b->kids[static_cast<size_t>(batched[static_cast<size_t>(k)])]->res.failed = true;
  if (!L.empty()) {
    // launch tables behind the argument array, one copy for all launches
    const size_t args_bytes = static_cast<size_t>(round_up(static_cast<int64_t>(args.size() * sizeof(ResidentArgs)), 256));
    size_t nent = 0;
    for (const auto& l : L) nent += static_cast<size_t>(l.workgroups);
    const size_t tb = args_bytes + nent * sizeof(ResidentLaunchEntry);
    HIPCHK(hipStreamSynchronize(b->stream));  // (the staging buffers are reused: the inputs' copy is through)
    if (int rc = batch_grow(b, tb)) return rc;
    std::memcpy(b->hstage, args.data(), args.size() * sizeof(ResidentArgs));
    ResidentLaunchEntry* tab = reinterpret_cast<ResidentLaunchEntry*>(b->hstage + args_bytes);
    size_t e = 0;
    for (const auto& l : L)
      for (int k : l.items)
        for (int u = 0; u < items[static_cast<size_t>(k)].units; ++u) tab[e++] = ResidentLaunchEntry{k, u};
    HIPCHK(hipMemcpyAsync(b->dstage, b->hstage, tb, hipMemcpyHostToDevice, b->stream));
    const ResidentArgs* dargs = reinterpret_cast<const ResidentArgs*>(b->dstage);
    const ResidentLaunchEntry* dtab = reinterpret_cast<const ResidentLaunchEntry*>(b->dstage + args_bytes);
    size_t e0 = 0;
    for (const auto& l : L) {
      if (batch_launch(b, l.key, static_cast<unsigned>(l.workgroups), dtab + e0, dargs) == 0) {
        ++b->launches;
        for (int k : l.items) launched[static_cast<size_t>(k)] = 1;
      } else {
        for (int k : l.items) b->kids[static_cast<size_t>(batched[static_cast<size_t>(k)])]->res.failed = true;
      }
      e0 += static_cast<size_t>(l.workgroups);
    }
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  for (size_t k = 0; k < batched.size(); ++k) {
    const int32_t i = batched[k];
    Ctx* c = b->kids[static_cast<size_t>(i)];
    volatile HostMirror* hm = c->mirror;
    if (launched[k] && hm->done) {
      std::atomic_thread_fence(std::memory_order_acquire);
      Batch::Result& R = b->res[static_cast<size_t>(i)];
      R.route = 1;
      solve_info(R.info, mirror_result(hm));
      if (int rc = resident_finished(c, hm->iters)) return rc;  // (the epochs as the lone solve moves them)
      c->last_solver = 1;
      continue;
    }
    if (launched[k]) {  // gave up (a time-out, an LDS plan the device refused): as the lone solve does
      uint32_t err = 0;
      if (int rc = resident_gave_up(c, err)) return rc;
      c->res.failed = true;  // until the next build
      if (rs_debug()) std::fprintf(stderr, "[batch] problem %d gave up: error %u\n", i, err);
    }
    alone.push_back(i);
  }
  std::sort(alone.begin(), alone.end());
  const auto t2 = std::chrono::high_resolution_clock::now();
  b->t_launch = std::chrono::duration<double, std::milli>(t2 - t1).count();

  // ---- 6. the others alone, on their child's ordinary path ---------------------------------------------------------
  for (int32_t i : alone) {
    Ctx* c = b->kids[static_cast<size_t>(i)];
    Batch::Result& R = b->res[static_cast<size_t>(i)];
    if (int rc = solve_staged(c, P, nullptr, &R.info)) return rc;
    R.route = 0;
    R.u = c->u_host;
    R.nodes = c->nodes;
  }
  const auto t3 = std::chrono::high_resolution_clock::now();
  b->t_alone = std::chrono::duration<double, std::milli>(t3 - t2).count();

  // ---- 7. rounding of the batched ones, with the lone solve's code ----------------------------------------------------
  for (int32_t i = 0; i < n; ++i) {
    Batch::Result& R = b->res[static_cast<size_t>(i)];
    Ctx* c = b->kids[static_cast<size_t>(i)];
    if (R.route == 1) {
      c->u_host.assign(c->u_pinned, c->u_pinned + c->m);
      if (int rc = round_nodes(c, P->rounding, c->u_host, R.info.score, R.nodes)) return rc;
      c->nodes = R.nodes;
      R.u = c->u_host;
      R.info.num_nodes = static_cast<int32_t>(R.nodes.size());
    }
    const size_t k = R.nodes.size();  // utils::selectInlierAssociations
    R.sel.assign(2 * k, 0);
    for (size_t r = 0; r < k; ++r) {
      const size_t a = static_cast<size_t>(R.nodes[r]);
      R.sel[r] = c->A[a];
      R.sel[k + r] = c->A[static_cast<size_t>(c->m) + a];
    }
  }
  const auto t4 = std::chrono::high_resolution_clock::now();
  b->t_round = std::chrono::duration<double, std::milli>(t4 - t3).count();
  const double secs = std::chrono::duration<double>(t4 - t0).count();
  for (auto& R : b->res) R.info.seconds = secs;
  b->n_batched = static_cast<int>(std::count_if(b->res.begin(), b->res.end(), [](const Batch::Result& R) { return R.route == 1; }));
  b->n_alone = n - b->n_batched;
  b->solved = true;
  return 0;
}

// clipper_hip_batch_sdp: the relaxation of every problem of the last solve call, on each child's M and C with their
// identity diagonals (what sdp_ctx_impl gathers for a lone context), in the launches of one sdp_batch_run. A child's
// store is read where it lives: the dense store, or a dense copy of its slices made for this call only. Each
// problem's selection becomes its node list (the child's, and the batch's results); nothing the solver keeps is
// touched.
int batch_sdp(Batch* b, const clipper_sdp_params_t* P, clipper_sdp_info_t* infos) {
  const auto t0 = std::chrono::steady_clock::now();
  if (!b->solved) return fail(CLIPPER_HIP_E_STATE, "sdp: no batch has been solved");
  if (int rc = sdp_check_params(P, 1)) return rc;
  const size_t count = b->res.size();
  for (size_t i = 0; i < count; ++i) {
    const Ctx* c = b->kids[i];
    if (!c->has_matrix) return fail(CLIPPER_HIP_E_STATE, "problem %zu: no matrix has been built", i);
    if (c->m < 1) return fail(CLIPPER_HIP_E_INVALID, "problem %zu: sdp: empty problem", i);
    if (c->m > SDP_MAX_N)
      return fail(CLIPPER_HIP_E_SCOPE, "problem %zu: sdp: n = %lld is above the device solver's limit of %d", i,
                  (long long)c->m, SDP_MAX_N);
  }
  b->sdp.reset();
  if (count == 0) return 0;
  HIPCHK(hipSetDevice(b->device));
  std::unique_ptr<SdpBatchState> S(new SdpBatchState());
  S->device = b->device;
  S->n.resize(count);
  for (size_t i = 0; i < count; ++i) S->n[i] = static_cast<int32_t>(b->kids[i]->m);
  auto drop_copies = [&] {
    for (size_t i = 0; i < count; ++i)
      if (b->kids[i]->csc_valid) drop_dense(b->kids[i]);
  };
  auto source = [&](size_t i, SdpGatherSrc& g) -> int {
    Ctx* c = b->kids[i];
    if (int rc = ensure_dense(c, true)) return rc;  // (a copy of the slices for this call only)
    const Shard& s = c->sh[0];
    g.srcM = s.S;
    g.srcC = c->explicitC ? s.Cs : s.S;
    if (!g.srcM || !g.srcC) return fail(CLIPPER_HIP_E_STATE, "problem %zu: sdp: the store of M or C is not on the device", i);
    g.rs = c->W;
    g.cs = 1;
    g.ident = 1.0;
    g.f64 = c->storage == CLIPPER_HIP_STORE_F64;
    g.c_pattern_of_m = !c->explicitC;
    return 0;
  };
  bool dropped = false;
  const int rc = sdp_batch_run(*S, b->stream, P, false, source, [](uint8_t*) {}, [&] { drop_copies(); dropped = true; }, t0);
  if (!dropped) drop_copies();
  if (rc) return rc;
  for (size_t i = 0; i < count; ++i) {
    Ctx* c = b->kids[i];
    Batch::Result& R = b->res[i];
    const size_t k = static_cast<size_t>(S->round(i).count);
    R.nodes.assign(S->nodes(i), S->nodes(i) + k);
    c->nodes = R.nodes;
    R.info.num_nodes = static_cast<int32_t>(k);  // (what the getters size their buffers by)
    R.sel.assign(2 * k, 0);  // utils::selectInlierAssociations
    for (size_t r = 0; r < k; ++r) {
      const size_t a = static_cast<size_t>(R.nodes[r]);
      R.sel[r] = c->A[a];
      R.sel[k + r] = c->A[static_cast<size_t>(c->m) + a];
    }
    if (infos) infos[i] = S->info[i];
  }
  b->sdp = std::move(S);
  return 0;
}

}  // namespace
