// host_resident.hpp — planning and launch of the resident solver (k_resident.hip.h)
// Part of clipper_hip.hip (one translation unit; included there, in order).
#pragma once

namespace {

constexpr uint32_t RS_LDS_MAX = 159u * 1024u;  // dynamic LDS of a workgroup: the 160 KB of a gfx950 CU less the kernel's few static words
constexpr int RS_MAX_UNITS = 64;  // beyond (dense problems of m ~ 2000: > 5 MB of slices) the streaming
                                  // launches with their window of 4 win (profiles/r02c_bm_table*.md)

bool rs_debug() {
  static const bool on = std::getenv("CLIPPER_HIP_RESIDENT_DEBUG") != nullptr;
  return on;
}

// A plan of either planner into a context's image (slots: the optional block, null with nslots = 0): the buffer grown
// where the plan does not fit, the plan packed, and all of it written before a launch can read it.
template <class Plan>
int plan_image_store(PlanImage& im, const Plan& P, const uint8_t* slots, size_t nslots, int pmax) {
  im.at = clipper_plan::plan_layout(P.units.size(), nslots, P.npieces.size(), static_cast<size_t>(pmax));
  if (im.at.bytes > im.buf.cap) HIPCHK(im.buf.alloc(im.at.bytes + 4096, hipHostMallocMapped | hipHostMallocCoherent));
  clipper_plan::plan_pack(im.at, im.buf, P.units.data(), slots, P.npieces.data(), P.wave_cg.data(), P.pieces.data());
  std::atomic_thread_fence(std::memory_order_seq_cst);
  return 0;
}

// Decide whether the current slices fit the resident solver and lay out its units (host_plan.hpp).
// Called when a build's directory (csc_hLq) is on the host. Leaves r.ready = false when the problem
// does not fit.
int resident_plan(Ctx* h, Shard& s) {
  Resident& r = h->res;
  r.ready = false;
  r.failed = false;
  if (h->resident_mode == 1 || h->V_forced != 0 || h->world != 1 || h->multiproc || h->explicitC) return 0;
  static_assert(sizeof(clipper_plan::Unit) == sizeof(ResidentUnit), "the planner's unit is the kernel's");
  static_assert(clipper_plan::so_bytes(17, SL_SO) == sl_so_bytes(17) && clipper_plan::so_bytes(32, SL_SO) == sl_so_bytes(32) &&
                    clipper_plan::so_bytes(0, SL_SO) == sl_so_bytes(0),
                "the planner sizes the step-offset table as the format does");
  const clipper_plan::ResidentConsts K{RS_NT, RS_NWV, RS_TMAX, RS_PMAX, RS_MAXE, RS_LDS_MAX,
                                       RS_RED_BYTES, RS_TAB_BYTES, RS_SLICE_PAD, SL_SO};
  static thread_local clipper_plan::ResidentPlan plan;
  const int ncg = s.s_ncg, nchunks = s.s_nchunks;
  clipper_plan::plan_resident(h->csc_hLq, ncg, nchunks, h->m, h->mp, static_cast<int>(h->esize()),
                              std::min(RS_MAX_UNITS, h->cus - 8), r.V_forced, K, plan);
  if (rs_debug())
    std::fprintf(stderr, "[resident] plan m=%lld ncg=%d nchunks=%d total_ub=%llu -> V=%d E=%d units=%zu ok=%d\n",
                 static_cast<long long>(h->m), ncg, nchunks, static_cast<unsigned long long>(plan.total_bound),
                 plan.V, plan.E, plan.units.size(), plan.ok ? 1 : 0);
  if (!plan.ok) return 0;
  HIPCHK(hipSetDevice(s.device));
  if (int rc = plan_image_store(r.plan, plan, plan.nsl.data(), plan.nsl.size(), RS_PMAX)) return rc;
  if (int rc = r.x.ensure(2ull * plan.maxslots * (plan.V + 1) * static_cast<size_t>(h->mp) * 2, s.stream)) return rc;
  if (!r.ctl) {  // the error word and the two counters of the one-XCD mode
    HIPCHK(r.ctl.alloc(4));
    HIPCHK(hipMemsetAsync(r.ctl, 0, 4 * sizeof(unsigned long long), s.stream));
  }
  r.V = plan.V;
  r.E = plan.E;
  r.nunits = static_cast<int>(plan.units.size());
  r.maxslots = plan.maxslots;
  r.lds_slices = plan.lds_slices;
  r.ready = true;
  return 0;
}

// One launch of a kernel of the resident family (k_solve_resident, k_solve_resident_batch, k_solve_view_resident): a
// workgroup of RS_NT threads with the whole dynamic LDS of a CU. 1: this device does not give a workgroup 159 KB of
// LDS, or refuses the launch — not an error: the caller goes on without the resident solver.
template <typename... P, typename... A>
int resident_launch(void (*kern)(P...), const char* who, int device, unsigned grid, hipStream_t stream, const A&... args) {
  static_assert(RVR_NT == RS_NT, "the view kernel's workgroup is the resident kernel's");
  const void* fn = reinterpret_cast<const void*>(kern);
  if (!raise_dynamic_lds(fn, device, static_cast<int>(RS_LDS_MAX))) {
    if (rs_debug()) {  // (asked once more, for the runtime's reason: raise_dynamic_lds keeps none)
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(RS_LDS_MAX));
      (void)hipGetLastError();
      hipFuncAttributes fa{};
      (void)hipFuncGetAttributes(&fa, fn);
      int optin = 0, perblk = 0;
      (void)hipDeviceGetAttribute(&perblk, hipDeviceAttributeMaxSharedMemoryPerBlock, device);
      (void)hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, device);
      std::fprintf(stderr, "[%s] hipFuncSetAttribute: %s (static LDS %zu, max dynamic %d, device per block %d, optin %d)\n",
                   who, hipGetErrorString(e), fa.sharedSizeBytes, fa.maxDynamicSharedSizeBytes, perblk, optin);
    }
    return 1;
  }
  hipLaunchKernelGGL(kern, dim3(grid), dim3(RS_NT), RS_LDS_MAX, stream, args...);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {  // refused: the streaming launches take over
    if (rs_debug()) std::fprintf(stderr, "[%s] launch failed: %s\n", who, hipGetErrorString(e));
    return 1;
  }
  return 0;
}

// (value type, V, E) -> f(value type tag, V, E as integral constants), which names its kernel's instance; 1: there is
// none. The lone launch (k_solve_resident) and the batched one (k_solve_resident_batch) both come through here.
template <typename F>
int with_resident_instance(bool f64, int V, int E, F&& f) {
  auto of = [&](auto vt) {
    using std::integral_constant;
    switch (V * 10 + E) {
      case 21: return f(vt, integral_constant<int, 2>{}, integral_constant<int, 1>{});
      case 22: return f(vt, integral_constant<int, 2>{}, integral_constant<int, 2>{});
      case 24: return f(vt, integral_constant<int, 2>{}, integral_constant<int, 4>{});
      case 11: return f(vt, integral_constant<int, 1>{}, integral_constant<int, 1>{});
      case 12: return f(vt, integral_constant<int, 1>{}, integral_constant<int, 2>{});
      case 14: return f(vt, integral_constant<int, 1>{}, integral_constant<int, 4>{});
      default: return 1;
    }
  };
  return f64 ? of(double{}) : of(float{});
}

// The longest a unit waits for the other units' sums of ONE pass (one exchange), in ticks of the 100 MHz wall clock.
// Placement-free: 5 ms — five hundred passes' worth (a pass is 3-11 us). Where the units share their places with whatever
// else runs there — the one-XCD mode, whose units compete for one XCD's CUs; a view, whose launch sits inside a solve
// (an iteration is 14 us, the first exchange comes 25 us into the launch) — 2 ms: rather launch again. A unit that is not
// resident by then is behind another tenant's work: the streaming launches, which need no co-residency, take over.
// (Round 4 waited 0.5 s — a thousand solves' worth — before a 0.3 ms solve went on; on a view 0.2 s before a 1.2 ms one.)
constexpr long long RS_TIMEOUT_TICKS = 500000, RS_TIMEOUT_TICKS_SHARED = 200000;
// (ten times as long for a context's first launch — a cold code object, a clock that ramps up or a profiler
// that serialises kernels must not look like another tenant)
constexpr long long RS_TIMEOUT_FIRST_LAUNCH = 10;
enum class Places { free, shared };
constexpr long long exchange_timeout_ticks(Places places, bool first_launch) {
  return (places == Places::shared ? RS_TIMEOUT_TICKS_SHARED : RS_TIMEOUT_TICKS) * (first_launch ? RS_TIMEOUT_FIRST_LAUNCH : 1);
}
// The time-out of a launch of k_solve_resident or k_solve_resident_batch of context h. The test knob, read at every
// call (tests set and unset it between solves of one process), overrides when it parses to a NON-ZERO value;
// `overridden` then tells the lone solve not to repeat a one-XCD launch that timed out. (The view solver's knob
// overrides whenever it is set, zero included: rvr_timeout_ticks, host_rv_resident.hpp. Tests rely on both.)
long long resident_timeout_ticks(const Ctx* h, Places places, bool* overridden = nullptr) {
  const char* e = std::getenv("CLIPPER_HIP_RESIDENT_TIMEOUT_TICKS");
  const long long knob = e ? std::atoll(e) : 0;
  if (overridden) *overridden = knob != 0;
  return knob ? knob : exchange_timeout_ticks(places, h->res.x.epoch == 0);
}

// the context's values are doubles (dispatch_vt's criterion, for the instance tables below and of the view solver)
bool stores_f64(const Ctx* h) { return h->storage == CLIPPER_HIP_STORE_F64; }

// the current slices have a resident plan the next solve may launch
bool resident_applies(const Ctx* h) {
  const Resident& r = h->res;
  return r.ready && !r.failed && h->csc_valid && h->resident_mode != 1 && h->V_forced == 0;
}

// The arguments of a resident launch of the current plan (placement-free; the caller sets the mode, the
// home XCD and the time-out). The lone solve (below) and the batched one (host_batchsolve.hpp) both start here.
ResidentArgs resident_args(Ctx* h, const SolverParams& prm, bool rescale) {
  Resident& r = h->res;
  Shard& s = h->sh[0];
  ResidentArgs a;
  a.M = slice_view(h, s);
  a.units = r.plan.at.units<ResidentUnit>(r.plan.buf.dev);
  a.nunits = r.nunits;
  a.nslots_of_cg = r.plan.at.slots(r.plan.buf.dev);
  a.npieces = r.plan.at.npieces(r.plan.buf.dev);
  a.wave_cg = r.plan.at.wave_cg(r.plan.buf.dev);
  a.pieces = r.plan.at.pieces(r.plan.buf.dev);
  a.maxslots = r.maxslots;
  a.m = h->m;
  a.mp = h->mp;
  a.prm = prm;
  a.rescale = rescale ? 1 : 0;
  a.u0 = s.u0;
  a.xb = r.x.xb;
  a.epoch0 = r.x.epoch;
  a.err = r.ctl.as<uint32_t>();
  a.lds_slices = r.lds_slices;
  a.u_dev = s.pt;  // point slot (0, 0), array u
  a.host_u = h->u_pinned.dev;
  a.host = h->mirror.dev;
  a.shared = s.shared;
  a.stamps = h->stamps_dev;
  a.ctrs = r.ctl + 1;
  a.xcd_mode = 0;
  a.home = 0;
  a.timeout_ticks = 0;
  return a;
}

// a launch that gave up (the stream has drained): its error word; the word, the counters and the granules cleared.
// Whether the context tries again (r.failed) is the caller's.
int resident_gave_up(Ctx* h, uint32_t& err) {
  Resident& r = h->res;
  err = 0;
  HIPCHK(hipMemcpy(&err, r.ctl, sizeof(err), hipMemcpyDeviceToHost));
  HIPCHK(hipMemsetAsync(r.ctl, 0, 4 * sizeof(unsigned long long), h->sh[0].stream));
  if (int rc = r.x.gave_up(h->sh[0].stream)) return rc;
  r.last_error = static_cast<int>(err);
  return 0;
}

// Runs the whole solve as one launch. ran = false: the resident solver did not apply or gave up
// (nothing of the solver state was touched: the caller runs the streaming solver).
int resident_solve(Ctx* h, const SolverParams& prm, bool rescale, SolveShared& fin, bool& ran) {
  ran = false;
  Resident& r = h->res;
  if (rs_debug())
    std::fprintf(stderr, "[resident] solve: ready=%d failed=%d csc_valid=%d mode=%d Vf=%d\n", r.ready, r.failed,
                 h->csc_valid, h->resident_mode, h->V_forced);
  if (!resident_applies(h)) return 0;
  Shard& s = h->sh[0];
  HIPCHK(hipSetDevice(s.device));
  ResidentArgs a = resident_args(h, prm, rescale);
  // contexts take their home XCD in turn, so that concurrent solves of several contexts do not
  // queue for the 32 CUs of one XCD
  static std::atomic<int> next_home{0};
  if (r.home < 0) r.home = next_home.fetch_add(1) & 7;
  a.home = r.home;
  // test knobs: a home XCD that does not exist (the one-XCD launch must be refused and repeated in
  // the placement-free mode), a time-out of a few ticks (the streaming launches must take over)
  if (const char* e = std::getenv("CLIPPER_HIP_RESIDENT_HOME")) a.home = std::atoi(e);
  bool timeout_overridden = false;
  // One-XCD mode: with at most 28 units (an XCD has 32 CUs) the launch is 8 x units workgroups and the
  // ones on XCD 0 do the work, exchanging through their common L2 (per pass ~2.5 us less). Refused
  // once (the hardware did not put enough workgroups there), it is not tried again.
  const char* xe = std::getenv("CLIPPER_HIP_RESIDENT_XCD");
  const bool xcd_env_off = xe && std::atoi(xe) == 0;
  volatile HostMirror* hm = h->mirror;
  for (int attempt = 0;; ++attempt) {
    a.xcd_mode = (!r.xcd_off && !xcd_env_off && r.nunits >= 2 && r.nunits <= 28) ? 1 : 0;
    // (a launch that times out: the streaming launches take over, and this matrix is not tried again — r.failed)
    a.timeout_ticks = resident_timeout_ticks(h, a.xcd_mode ? Places::shared : Places::free, &timeout_overridden);
    a.epoch0 = r.x.epoch;
    std::memset(h->mirror, 0, sizeof(HostMirror));
    std::atomic_thread_fence(std::memory_order_seq_cst);
    const unsigned grid = static_cast<unsigned>(a.xcd_mode ? 8 * a.nunits : a.nunits);
    const int lr = with_resident_instance(stores_f64(h), r.V, r.E, [&](auto vt, auto v, auto e) {
      return resident_launch(k_solve_resident<decltype(vt), decltype(v)::value, decltype(e)::value>, "resident", s.device, grid, s.stream, a);
    });
    if (lr != 0) {
      if (rs_debug()) std::fprintf(stderr, "[resident] launch refused (V=%d E=%d)\n", r.V, r.E);
      r.failed = true;
      return 0;
    }
    uint64_t spins = 0;
    bool finished = true;
    while (!hm->done) {
      if ((++spins & 0x3fff) == 0) {
        hipError_t q = hipStreamQuery(s.stream);
        if (q != hipSuccess && q != hipErrorNotReady)
          return fail(CLIPPER_HIP_E_HIP, "resident solver failed: %s", hipGetErrorString(q));
        if (q == hipSuccess && !hm->done) {  // the launch is over and did not finish the solve
          finished = false;
          break;
        }
      }
    }
    if (finished) break;
    uint32_t err = 0;
    if (int rc = resident_gave_up(h, err)) return rc;
    if (rs_debug()) std::fprintf(stderr, "[resident] gave up: error %u (one-XCD mode %d)\n", err, a.xcd_mode);
    if ((err == RS_ERR_PLAN || err == RS_ERR_TIMEOUT) && a.xcd_mode && attempt == 0 && !timeout_overridden) {
      r.xcd_off = true;  // placement-free mode from now on
      continue;
    }
    r.failed = true;  // until the next build
    return 0;
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  fin = mirror_result(hm);
  if (int rc = r.x.finished(hm->iters, s.stream)) return rc;
  if (rs_debug()) std::fprintf(stderr, "[resident] solved: units=%d one-XCD mode=%d passes=%lld\n", r.nunits, a.xcd_mode,
                               static_cast<long long>(fin.n_passes));
  ran = true;
  return 0;
}

}  // namespace
