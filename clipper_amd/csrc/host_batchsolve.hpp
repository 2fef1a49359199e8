// host_batchsolve.hpp — batched solves: many independent small problems in one call.
// Part of clipper_hip.hip (one translation unit; included there, after the context's helpers).
//
// A batch owns one child context per problem slot, all on the batch's device and ONE stream (the children borrow it).
// A call
//   1. checks every problem (nothing reaches the device if one is invalid),
//   2. stages all inputs (D1, D2, the association lists, u0) in one pinned buffer and copies it with ONE H2D copy,
//   3. queues every child's fill back to back (fill_builtin with `queued`: run_affinity's) and waits ONCE; children whose
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
  PinnedBuf<uint8_t> hstage;  // staging of the inputs, then of the launch tables
  DevBuf<uint8_t> dstage;     // its device copy
  PinnedBuf<uint8_t> hfill;   // staging of a custom fill's problems and tiles (kind 3)
  DevBuf<uint8_t> dfill;      // its device copy
  Event ev_fill[2];           // around a custom fill's launch
  double t_fill_begin = 0.0, t_fill_launch = 0.0, t_fill_build = 0.0;  // kind 3: the parts of t_fill (ms)
  bool solved = false;                  // a solve call has succeeded: `res` and the children describe its problems
  std::unique_ptr<SdpBatchState> sdp;   // the last clipper_hip_batch_sdp (host_sdpbatch.hpp), until the next call
  int mc_launches = 0, mc_batched = 0, mc_alone = 0;  // the last clipper_hip_batch_max_clique (host_maxclique.hpp)
  PinnedBuf<uint8_t> hmc;  // its staging buffer, kept from call to call
};

namespace {

using Batch = clipper_hip_batch;

// a pinned buffer and its device copy of at least `bytes` each (contents lost when they grow)
int stage_grow(PinnedBuf<uint8_t>& hbuf, DevBuf<uint8_t>& dbuf, size_t bytes) {
  HIPCHK(hbuf.grow(bytes));
  HIPCHK(dbuf.grow(bytes));
  return 0;
}

int batch_grow(Batch* b, size_t bytes) { return stage_grow(b->hstage, b->dstage, bytes); }

// what lives for one batch_solve call: its arguments, and
struct BatchCall {
  const clipper_batch_problem_t* p;
  int32_t n;
  int d, kind;
  const double* f;
  const clipper_params_t* P;
  const CustomFill* cf;
  SolverParams prm;
  std::vector<std::vector<int32_t>> Afull;  // the association lists as stage_inputs holds them
  std::vector<size_t> off;                  // where each problem's inputs start in the staging buffer ...
  size_t bytes = 0;                         // ... and where they end
  std::vector<StagedInputs> dev;            // where each problem's inputs lie on the device ...
  std::vector<size_t> off_u0;               // ... and its u0
  std::vector<int32_t> batched, alone;      // problems with a resident plan (in launch-table order); the others
  std::vector<char> launched;               // per batched problem: its launch went out
};

// problem i's staged inputs handed to its child (step 3, before its fill) ...
int batch_stage_child(Batch* b, const BatchCall& K, size_t i) {
  const clipper_batch_problem_t& q = K.p[i];
  return stage_inputs(b->kids[i], q.D1, K.d, q.n1, q.D2, q.n2, K.Afull[i].data(),
                      static_cast<int64_t>(K.Afull[i].size() / 2), &K.dev[i]);
}

// ... and its u0 (behind the fill)
int batch_stage_u0(Batch* b, const BatchCall& K, size_t i) {
  Ctx* c = b->kids[i];
  HIPCHK(hipMemcpyAsync(c->sh[0].u0, b->dstage + K.off_u0[i], static_cast<size_t>(c->m) * 8, hipMemcpyDeviceToDevice,
                        b->stream));
  c->u0_staged = true;
  return 0;
}

// Step 3 for a user-defined invariant (kind 3). Every child: its inputs staged, then fill_custom's and run_affinity's
// steps before a launch (custom_fill_begin, affinity_begin: the dense store allocated). Then ONE launch of the
// batched fill kernel over every child's tiles (the lone kernel's grid, problem after problem), whose descriptors and
// tile table reach the device in one copy of their own. Then csc_rebuild's pair over the children: every compressed
// child's build queued back to back (csc_shard_enqueue), one wait, the checks (csc_shard_complete); children that
// overflowed build again (until_fits, as many builds as csc_rebuild allows). Dense storages keep their store. A child's
// affinity_kernel_ms is the batched launch's time (shared by every problem of the call), without the build.
int batch_fill_custom(Batch* b, const BatchCall& K) {
  const int32_t n = K.n;
  const CustomFill& cf = *K.cf;
  const auto t0 = std::chrono::high_resolution_clock::now();
  hipFunction_t fn = nullptr;
  size_t ntiles = 0;
  for (int32_t i = 0; i < n; ++i) {
    Ctx* c = b->kids[static_cast<size_t>(i)];
    if (int rc = batch_stage_child(b, K, static_cast<size_t>(i))) return rc;
    std::vector<hipFunction_t> f;
    if (int rc = custom_fill_begin(c, cf, true, f)) return rc;
    fn = f[0];
    bool emit = false, rect = false;
    if (int rc = affinity_begin(c, false, emit, rect)) return rc;
    if (emit || rect) return fail(CLIPPER_HIP_E_INTERNAL, "problem %d: a custom fill goes through the dense store", i);
    c->csc_emitted = false;  // (as fill_enqueue leaves a fill that does not emit)
    c->csc_out = CscOut{};
    if (int rc = batch_stage_u0(b, K, static_cast<size_t>(i))) return rc;
    ntiles += static_cast<size_t>(ceil_div(c->W, 1024) * ceil_div(c->m, AFF_ROWS_PER_BLK));
  }
  if (ntiles > 0x7fffffffu) return fail(CLIPPER_HIP_E_SCOPE, "a batched fill of %zu workgroups", ntiles);

  // the problems and the tile table: one copy, one launch
  const size_t pbytes = static_cast<size_t>(round_up(static_cast<int64_t>(n) * sizeof(CustomFillProblem), 256));
  if (int rc = stage_grow(b->hfill, b->dfill, pbytes + ntiles * sizeof(CustomFillTile)))
    return rc;
  CustomFillProblem* probs = reinterpret_cast<CustomFillProblem*>(b->hfill.p);
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
    HIPCHK(b->ev_fill[0].create());
    HIPCHK(b->ev_fill[1].create());
  }
  const auto t1 = std::chrono::high_resolution_clock::now();
  {
    const CustomFillProblem* dprobs = b->dfill.as<const CustomFillProblem>();
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
  std::vector<Ctx*> todo;
  for (int32_t i = 0; i < n; ++i)
    if (csc_applies(b->kids[static_cast<size_t>(i)])) todo.push_back(b->kids[static_cast<size_t>(i)]);
  float kms = 0.f;
  int rounds = 0;
  auto wait = [&]() -> int {
    if (hipStreamSynchronize(b->stream) != hipSuccess)
      return fail(CLIPPER_HIP_E_HIP, "batched custom fill: %s", hipGetErrorString(hipGetLastError()));
    if (rounds++ == 0) HIPCHK(hipEventElapsedTime(&kms, b->ev_fill[0], b->ev_fill[1]));
    return 0;
  };
  // (no compressed child: nothing to build, but the fill's events are read only once it is through)
  const int rc = todo.empty() ? wait() : clipper_fits::until_fits(
      todo.size(), clipper_fits::MAX_BUILDS, [&](size_t k) { return csc_shard_enqueue(todo[k], todo[k]->sh[0]); }, wait,
      [&](size_t k, bool& again) {
        if (int rcc = csc_shard_complete(todo[k], todo[k]->sh[0], again)) return rcc;
        return again ? 0 : csc_rebuilt(todo[k]);
      },
      [] { return build_overflows(); });
  if (rc) return rc;
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

// Where the batch kernels stand in the code object: kernels stand there in the order they are first named (and the
// order matters to this project: host_matrix_io.hpp), which for these was V = 1 first and double beside float — not
// the order of with_resident_instance's cases, which is the lone kernels'. This is their first naming. Nothing reads it,
// and it is not dead: without it the batch kernels move and the code object's .text changes (the section hashes of
// NOTEBOOK.md, "The resident solvers' host side", are the check to repeat before touching it).
[[maybe_unused]] void (*const batch_kernel_order[])(const ResidentLaunchEntry*, const ResidentArgs*) = {
    k_solve_resident_batch<double, 1, 1>, k_solve_resident_batch<float, 1, 1>, k_solve_resident_batch<double, 1, 2>,
    k_solve_resident_batch<float, 1, 2>,  k_solve_resident_batch<double, 1, 4>, k_solve_resident_batch<float, 1, 4>,
    k_solve_resident_batch<double, 2, 1>, k_solve_resident_batch<float, 2, 1>, k_solve_resident_batch<double, 2, 2>,
    k_solve_resident_batch<float, 2, 2>,  k_solve_resident_batch<double, 2, 4>, k_solve_resident_batch<float, 2, 4>};

// key = VT (0: float, 1: double) * 100 + V * 10 + E. 1: the launch did not go out (no such instance, no 159 KB of
// LDS for a workgroup on this device): the problems are solved alone
int batch_launch(Batch* b, int key, unsigned grid, const ResidentLaunchEntry* table, const ResidentArgs* args) {
  return with_resident_instance(key >= 100, key % 100 / 10, key % 10, [&](auto vt, auto v, auto e) {
    return resident_launch(k_solve_resident_batch<decltype(vt), decltype(v)::value, decltype(e)::value>, "batch", b->device,
                           grid, b->stream, table, args);
  });
}

// ---- 1. every problem checked before any device work; the children made ----------------------------------------------
int batch_check(Batch* b, BatchCall& K) {
  const int32_t n = K.n;
  const int d = K.d;
  if (int rc = solver_params(K.P, K.prm)) return rc;
  if (n < 0 || (n > 0 && !K.p)) return fail(CLIPPER_HIP_E_INVALID, "invalid problem list");
  if (K.kind == 2 && d != 6) return fail(CLIPPER_HIP_E_INVALID, "PointNormalDistance data are 6 x n");
  if (K.kind == 3 && (!K.cf || d != K.cf->inv->d)) return fail(CLIPPER_HIP_E_INVALID, "no invariant of dimension d = %d", d);
  if (d < 1) return fail(CLIPPER_HIP_E_INVALID, "invalid dimension d = %d", d);
  K.Afull.resize(static_cast<size_t>(n));
  for (int32_t i = 0; i < n; ++i) {
    const clipper_batch_problem_t& q = K.p[i];
    if (!q.D1 || !q.D2 || q.n1 < 1 || q.n2 < 1) return fail(CLIPPER_HIP_E_INVALID, "problem %d: invalid point data", i);
    if (!q.u0) return fail(CLIPPER_HIP_E_INVALID, "problem %d: u0 is required", i);
    if (q.m < 0) return fail(CLIPPER_HIP_E_INVALID, "problem %d: m = %lld", i, static_cast<long long>(q.m));
    const int64_t m = (q.A == nullptr || q.m == 0) ? q.n1 * q.n2 : q.m;  // (all pairs: association_list)
    if (m > 0x7fffffff) return fail(CLIPPER_HIP_E_INVALID, "problem %d: %lld associations", i, static_cast<long long>(m));
    if (association_list(q.A, q.m, q.n1, q.n2, K.Afull[static_cast<size_t>(i)]))
      return fail(CLIPPER_HIP_E_INVALID, "problem %d: %s", i, std::string(g_err).c_str());
    K.off.push_back(K.bytes);
    K.bytes += static_cast<size_t>(round_up(static_cast<int64_t>(d) * (q.n1 + q.n2) * 8 + m * 16 + m * 8, 256));
  }
  b->res.resize(static_cast<size_t>(n));
  if (n == 0) return 0;
  HIPCHK(hipSetDevice(b->device));
  while (b->kids.size() < static_cast<size_t>(n)) {
    Ctx* c = make_ctx(&b->device, 1, b->storage, 1, 0, false);
    if (!c) return CLIPPER_HIP_E_HIP;
    hipStreamDestroy(c->sh[0].stream);
    c->sh[0].stream = b->stream;
    c->borrowed_stream = true;
    b->kids.push_back(c);
  }
  return 0;
}

// ---- 2. the inputs: one pinned buffer, one copy ----------------------------------------------------------------------
int batch_stage(Batch* b, BatchCall& K) {
  if (int rc = batch_grow(b, K.bytes)) return rc;
  const size_t n = static_cast<size_t>(K.n);
  K.dev.resize(n);
  K.off_u0.resize(n);
  for (size_t i = 0; i < n; ++i) {
    const clipper_batch_problem_t& q = K.p[i];
    const size_t bm = K.Afull[i].size() * 4;  // u0 (m doubles) and the list (2 m indices) alike
    size_t o = K.off[i];
    auto put = [&](const void* src, size_t bytes) {  // -> where it lies on the device
      std::memcpy(b->hstage + o, src, bytes);
      o += bytes;
      return b->dstage + o - bytes;
    };
    K.dev[i].D1 = reinterpret_cast<const double*>(put(q.D1, static_cast<size_t>(K.d) * q.n1 * 8));
    K.dev[i].D2 = reinterpret_cast<const double*>(put(q.D2, static_cast<size_t>(K.d) * q.n2 * 8));
    K.off_u0[i] = static_cast<size_t>(put(q.u0, bm) - b->dstage);
    K.dev[i].A = reinterpret_cast<const int32_t*>(put(K.Afull[i].data(), bm));
  }
  HIPCHK(hipMemcpyAsync(b->dstage, b->hstage, K.bytes, hipMemcpyHostToDevice, b->stream));
  return 0;
}

// ---- 3. the fills, queued back to back; one wait; the overflowed ones again (the built-in invariants) -----------------
// A child whose route cannot be queued (d not 2 or 3, dense storage, the rectangular route) has run its fill to the
// end inside its turn: it is not `queued`, and nothing is left to complete.
int batch_fill(Batch* b, const BatchCall& K) {
  const FillInvariant inv = FillInvariant::from_list(K.kind, K.f, K.P->affinityeps);
  std::vector<char> queued(static_cast<size_t>(K.n), 0);
  bool first = true;  // round 0 hands every child its inputs as well
  return clipper_fits::until_fits(
      queued.size(), clipper_fits::MAX_BUILDS,
      [&](size_t i) -> int {
        if (first)
          if (int rc = batch_stage_child(b, K, i)) return rc;
        bool q = false;
        if (int rc = fill_builtin(b->kids[i], inv, &q)) return rc;
        queued[i] = q;
        return first ? batch_stage_u0(b, K, i) : 0;
      },
      [&]() -> int {
        first = false;
        HIPCHK(hipStreamSynchronize(b->stream));
        return 0;
      },
      [&](size_t i, bool& again) { return queued[i] ? fill_complete(b->kids[i], again) : 0; },
      [] { return build_overflows(); });
}

// ---- 4./5. the resident plans, packed into launches; one wait --------------------------------------------------------
int batch_launch_resident(Batch* b, BatchCall& K) {
  std::vector<ResidentArgs> args;
  std::vector<clipper_batch::PackItem> items;
  for (int32_t i = 0; i < K.n; ++i) {
    Ctx* c = b->kids[static_cast<size_t>(i)];
    if (!resident_applies(c)) {
      K.alone.push_back(i);
      continue;
    }
    if (int rc = ensure_u_pinned(c)) return rc;
    ResidentArgs a = resident_args(c, K.prm, K.P->rescale_u0 != 0);
    // (the lone solve's placement-free wait, and its test knob)
    a.timeout_ticks = resident_timeout_ticks(c, Places::free);
    std::memset(c->mirror, 0, sizeof(HostMirror));
    K.batched.push_back(i);
    args.push_back(a);
    items.push_back({(c->esize() == 8 ? 100 : 0) + c->res.V * 10 + c->res.E, c->res.nunits});
  }
  std::atomic_thread_fence(std::memory_order_seq_cst);
  const int cap = std::max(1, b->kids[0]->cus - 8);
  std::vector<int> rejected;
  const std::vector<clipper_batch::PackLaunch> L = clipper_batch::pack_launches(items, cap, &rejected);
  K.launched.assign(K.batched.size(), 0);
  for (int k : rejected) b->kids[static_cast<size_t>(K.batched[static_cast<size_t>(k)])]->res.failed = true;
  if (L.empty()) return 0;
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
  const ResidentArgs* dargs = b->dstage.as<const ResidentArgs>();
  const ResidentLaunchEntry* dtab = reinterpret_cast<const ResidentLaunchEntry*>(b->dstage + args_bytes);
  size_t e0 = 0;
  for (const auto& l : L) {
    if (batch_launch(b, l.key, static_cast<unsigned>(l.workgroups), dtab + e0, dargs) == 0) {
      ++b->launches;
      for (int k : l.items) K.launched[static_cast<size_t>(k)] = 1;
    } else {
      for (int k : l.items) b->kids[static_cast<size_t>(K.batched[static_cast<size_t>(k)])]->res.failed = true;
    }
    e0 += static_cast<size_t>(l.workgroups);
  }
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

// ---- 5. (its end) the progress records read back; a problem that gave up or never went out joins `alone` -------------
int batch_read_back(Batch* b, BatchCall& K) {
  for (size_t k = 0; k < K.batched.size(); ++k) {
    const int32_t i = K.batched[k];
    Ctx* c = b->kids[static_cast<size_t>(i)];
    volatile HostMirror* hm = c->mirror;
    if (K.launched[k] && hm->done) {
      std::atomic_thread_fence(std::memory_order_acquire);
      Batch::Result& R = b->res[static_cast<size_t>(i)];
      R.route = 1;
      solve_info(R.info, mirror_result(hm));
      if (int rc = c->res.x.finished(hm->iters, c->sh[0].stream)) return rc;  // (the epochs as the lone solve moves them)
      c->last_solver = 1;
      continue;
    }
    if (K.launched[k]) {  // gave up (a time-out, an LDS plan the device refused): as the lone solve does
      uint32_t err = 0;
      if (int rc = resident_gave_up(c, err)) return rc;
      c->res.failed = true;  // until the next build
      if (rs_debug()) std::fprintf(stderr, "[batch] problem %d gave up: error %u\n", i, err);
    }
    K.alone.push_back(i);
  }
  std::sort(K.alone.begin(), K.alone.end());
  return 0;
}

// ---- 6. the others alone, on their child's ordinary path -------------------------------------------------------------
int batch_solve_alone(Batch* b, const BatchCall& K) {
  for (int32_t i : K.alone) {
    Ctx* c = b->kids[static_cast<size_t>(i)];
    Batch::Result& R = b->res[static_cast<size_t>(i)];
    if (int rc = solve_staged(c, K.P, nullptr, &R.info)) return rc;
    R.route = 0;
    R.u = c->u_host;
    R.nodes = c->nodes;
  }
  return 0;
}

// ---- 7. rounding of the batched ones, with the lone solve's code; every problem's selected associations --------------
int batch_round(Batch* b, const BatchCall& K) {
  for (int32_t i = 0; i < K.n; ++i) {
    Batch::Result& R = b->res[static_cast<size_t>(i)];
    Ctx* c = b->kids[static_cast<size_t>(i)];
    if (R.route == 1) {
      c->u_host.assign(c->u_pinned.p, c->u_pinned.p + c->m);
      if (int rc = round_nodes(c, K.P->rounding, c->u_host, R.info.score, R.nodes)) return rc;
      c->nodes = R.nodes;
      R.u = c->u_host;
      R.info.num_nodes = static_cast<int32_t>(R.nodes.size());
    }
    R.sel.assign(2 * R.nodes.size(), 0);
    selected_associations(c, R.nodes, R.sel.data());
  }
  return 0;
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
  BatchCall K{p, n, d, kind, f, P, cf};
  int rc = batch_check(b, K);
  if (rc || n == 0) {
    b->solved = !rc;
    return rc;
  }
  if ((rc = batch_stage(b, K)) || (rc = kind == 3 ? batch_fill_custom(b, K) : batch_fill(b, K))) return rc;
  const auto t1 = std::chrono::high_resolution_clock::now();
  b->t_fill = std::chrono::duration<double, std::milli>(t1 - t0).count();
  if ((rc = batch_launch_resident(b, K)) || (rc = batch_read_back(b, K))) return rc;
  const auto t2 = std::chrono::high_resolution_clock::now();
  b->t_launch = std::chrono::duration<double, std::milli>(t2 - t1).count();
  if ((rc = batch_solve_alone(b, K))) return rc;
  const auto t3 = std::chrono::high_resolution_clock::now();
  b->t_alone = std::chrono::duration<double, std::milli>(t3 - t2).count();
  if ((rc = batch_round(b, K))) return rc;
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
  const int route = g_sdp_route.load();
  if (int rc = sdp_check_params(P, 1, route)) return rc;
  const size_t count = b->res.size();
  for (size_t i = 0; i < count; ++i) {
    const Ctx* c = b->kids[i];
    if (!c->has_matrix) return fail(CLIPPER_HIP_E_STATE, "problem %zu: no matrix has been built", i);
    if (c->m < 1) return fail(CLIPPER_HIP_E_INVALID, "problem %zu: sdp: empty problem", i);
    if (c->m > clipper_sdpw_plan::route_limit(route))
      return fail(CLIPPER_HIP_E_SCOPE, "problem %zu: sdp: n = %lld is above the device solver's limit of %d", i,
                  (long long)c->m, clipper_sdpw_plan::route_limit(route));
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
  const int rc = sdp_batch_run(*S, b->stream, P, route, false, source, [](uint8_t*) {}, [&] { drop_copies(); dropped = true; }, t0);
  if (!dropped) drop_copies();
  if (rc) return rc;
  for (size_t i = 0; i < count; ++i) {
    Ctx* c = b->kids[i];
    Batch::Result& R = b->res[i];
    const size_t k = static_cast<size_t>(S->round(i).count);
    R.nodes.assign(S->nodes(i), S->nodes(i) + k);
    c->nodes = R.nodes;
    R.info.num_nodes = static_cast<int32_t>(k);  // (what the getters size their buffers by)
    R.sel.assign(2 * k, 0);
    selected_associations(c, R.nodes, R.sel.data());
    if (infos) infos[i] = S->info[i];
  }
  b->sdp = std::move(S);
  return 0;
}

}  // namespace
