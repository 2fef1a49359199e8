// host_custom_invariant.hpp — user-defined invariants: the hiprtc binding (loaded at run time, as RCCL
// is), the compile of one invariant's program (k_custom_invariant_src.h around the user's source) and the handle that
// keeps its code object and the modules loaded from it, one per device. The fill itself is fill_custom
// (host_matrix_io.hpp), a batch's fill batch_fill_custom (host_batchsolve.hpp). Part of clipper_hip.hip (one
// translation unit; included there, in order).
#pragma once

namespace {

// ---- hiprtc, bound at run time: a library without it fails the user-defined invariants only ----------------------
struct Hiprtc {
  void* lib = nullptr;
  hiprtcResult (*CreateProgram)(hiprtcProgram*, const char*, const char*, int, const char* const*,
                                const char* const*) = nullptr;
  hiprtcResult (*CompileProgram)(hiprtcProgram, int, const char* const*) = nullptr;
  hiprtcResult (*GetProgramLogSize)(hiprtcProgram, size_t*) = nullptr;
  hiprtcResult (*GetProgramLog)(hiprtcProgram, char*) = nullptr;
  hiprtcResult (*GetCodeSize)(hiprtcProgram, size_t*) = nullptr;
  hiprtcResult (*GetCode)(hiprtcProgram, char*) = nullptr;
  hiprtcResult (*DestroyProgram)(hiprtcProgram*) = nullptr;
  const char* (*GetErrorString)(hiprtcResult) = nullptr;
};
Hiprtc g_hiprtc;
std::mutex g_hiprtc_mutex;

int load_hiprtc() {
  std::lock_guard<std::mutex> lock(g_hiprtc_mutex);
  if (g_hiprtc.lib) return 0;
  const char* names[] = {"libhiprtc.so.7", "libhiprtc.so", "/opt/rocm/lib/libhiprtc.so"};
  void* lib = nullptr;
  for (const char* n : names) {
    lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (lib) break;
  }
  if (!lib) return fail(CLIPPER_HIP_E_SCOPE, "cannot load libhiprtc (user-defined invariants): %s", dlerror());
  Hiprtc r;
  auto sym = [&](auto& f, const char* s) { f = reinterpret_cast<std::remove_reference_t<decltype(f)>>(dlsym(lib, s)); };
  sym(r.CreateProgram, "hiprtcCreateProgram");
  sym(r.CompileProgram, "hiprtcCompileProgram");
  sym(r.GetProgramLogSize, "hiprtcGetProgramLogSize");
  sym(r.GetProgramLog, "hiprtcGetProgramLog");
  sym(r.GetCodeSize, "hiprtcGetCodeSize");
  sym(r.GetCode, "hiprtcGetCode");
  sym(r.DestroyProgram, "hiprtcDestroyProgram");
  sym(r.GetErrorString, "hiprtcGetErrorString");
  if (!r.CreateProgram || !r.CompileProgram || !r.GetProgramLogSize || !r.GetProgramLog || !r.GetCodeSize ||
      !r.GetCode || !r.DestroyProgram || !r.GetErrorString)
    return fail(CLIPPER_HIP_E_SCOPE, "libhiprtc is missing required symbols");
  r.lib = lib;
  g_hiprtc = r;
  return 0;
}

}  // namespace

// one compiled invariant: its code object, and the module loaded from it on each device that filled with it
struct clipper_hip_invariant {
  int d = 0;
  std::vector<char> code;
  struct Loaded {
    hipModule_t module = nullptr;
    hipFunction_t fill[2] = {nullptr, nullptr};   // fp32, fp64 dense store
    hipFunction_t batch[2] = {nullptr, nullptr};  // the same, a batch's fill (one launch for every problem)
  };
  mutable std::mutex mutex;
  mutable std::map<int, Loaded> loaded;  // by device
};

namespace {

using Invariant = clipper_hip_invariant;

// what one fill with a user-defined invariant is given (fill_custom, host_matrix_io.hpp)
struct CustomFill {
  const Invariant* inv;
  CustomParams prm;
};

// the program text of an invariant: prelude, the user's source, epilogue (k_custom_invariant_src.h)
std::string custom_program(const char* source, int d) {
  std::string pre = kCustomPrelude;
  pre.replace(pre.find("%d"), 2, std::to_string(d));
  return pre + source + kCustomEpilogue;
}

// hiprtc with the library's own HIP_FLAGS semantics (clipper_amd/build.py): fp64 rounds as written, an fma only where
// the source spells it; never xnack+.
int compile_custom(const char* source, int d, std::vector<char>& code) {
  if (int rc = load_hiprtc()) return rc;
  const std::string text = custom_program(source, d);
  // hiprtc brings the HIP device runtime with it: the user's #include <hip/hip_runtime.h> resolves to a stub
  const char* hdr_text[] = {"#pragma once\n"};
  const char* hdr_name[] = {"hip/hip_runtime.h"};
  hiprtcProgram prog = nullptr;
  hiprtcResult r = g_hiprtc.CreateProgram(&prog, text.c_str(), "clipper_invariant.hip", 1, hdr_text, hdr_name);
  if (r != HIPRTC_SUCCESS) return fail(CLIPPER_HIP_E_INTERNAL, "hiprtcCreateProgram: %s", g_hiprtc.GetErrorString(r));
  std::vector<const char*> opts = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"};
  r = g_hiprtc.CompileProgram(prog, static_cast<int>(opts.size()), opts.data());
  size_t nlog = 0;
  std::string log;
  if (g_hiprtc.GetProgramLogSize(prog, &nlog) == HIPRTC_SUCCESS && nlog > 1) {
    log.resize(nlog);
    if (g_hiprtc.GetProgramLog(prog, &log[0]) != HIPRTC_SUCCESS) log.clear();
    while (!log.empty() && (log.back() == '\0' || log.back() == '\n')) log.pop_back();
  }
  int rc = 0;
  if (r != HIPRTC_SUCCESS) {
    // (fail() cuts at 512 bytes: a compiler log goes whole)
    g_err = std::string("invariant does not compile (") + g_hiprtc.GetErrorString(r) + "):\n" + log;
    rc = CLIPPER_HIP_E_INVALID;
  } else {
    size_t n = 0;
    if (g_hiprtc.GetCodeSize(prog, &n) != HIPRTC_SUCCESS || n == 0) {
      rc = fail(CLIPPER_HIP_E_INTERNAL, "hiprtc returned no code object");
    } else {
      code.resize(n);
      if (g_hiprtc.GetCode(prog, code.data()) != HIPRTC_SUCCESS) rc = fail(CLIPPER_HIP_E_INTERNAL, "hiprtcGetCode failed");
    }
  }
  g_hiprtc.DestroyProgram(&prog);
  return rc;
}

// the fill kernel of `inv` for this device and value type, lone or a batch's, its module loaded on first use (the
// caller has set the device)
int custom_function(const Invariant* inv, int device, bool f64, hipFunction_t& fn, bool batched = false) {
  std::lock_guard<std::mutex> lock(inv->mutex);
  auto it = inv->loaded.find(device);
  if (it == inv->loaded.end()) {
    Invariant::Loaded l;
    HIPCHK(hipModuleLoadData(&l.module, inv->code.data()));
    if (hipModuleGetFunction(&l.fill[0], l.module, "clipper_custom_fill_f32") != hipSuccess ||
        hipModuleGetFunction(&l.fill[1], l.module, "clipper_custom_fill_f64") != hipSuccess ||
        hipModuleGetFunction(&l.batch[0], l.module, "clipper_custom_fill_batch_f32") != hipSuccess ||
        hipModuleGetFunction(&l.batch[1], l.module, "clipper_custom_fill_batch_f64") != hipSuccess) {
      (void)hipModuleUnload(l.module);
      return fail(CLIPPER_HIP_E_HIP, "the invariant's code object lacks its fill kernels");
    }
    it = inv->loaded.emplace(device, l).first;
  }
  fn = batched ? it->second.batch[f64 ? 1 : 0] : it->second.fill[f64 ? 1 : 0];
  return 0;
}

// the arguments of a fill with a user-defined invariant, checked before any device work
int custom_fill_args(const Invariant* inv, const double* params, int nparams, double affinityeps,
                     CustomFill& f) {
  if (!inv) return fail(CLIPPER_HIP_E_INVALID, "invalid argument: no invariant");
  if (nparams < 0 || nparams > CLIPPER_HIP_INVARIANT_MAX_PARAMS || (nparams > 0 && !params))
    return fail(CLIPPER_HIP_E_INVALID, "nparams = %d: 0 to %d parameters", nparams, CLIPPER_HIP_INVARIANT_MAX_PARAMS);
  f.inv = inv;
  f.prm = CustomParams{};
  for (int k = 0; k < nparams; ++k) f.prm.p[k] = params[k];
  f.prm.affinityeps = affinityeps;
  return 0;
}

// A fill's steps with a user-defined invariant before run_affinity (fill_custom, host_matrix_io.hpp; a batch's fill,
// host_batchsolve.hpp): the staged dimension checked, every shard's fill kernel (lone or batched) loaded before the
// build starts — a failed load leaves the matrix held untouched — then the fill's kind set.
int custom_fill_begin(Ctx* h, const CustomFill& f, bool batched, std::vector<hipFunction_t>& fn) {
  if (h->staged_d < 1) return fail(CLIPPER_HIP_E_STATE, "clipper_hip_stage_inputs not called");
  if (h->staged_d != f.inv->d)
    return fail(CLIPPER_HIP_E_INVALID, "the invariant is compiled for d = %d, the staged inputs have d = %d", f.inv->d,
                h->staged_d);
  const bool f64 = h->storage == CLIPPER_HIP_STORE_F64;  // the dense store's value type (dispatch_vt)
  fn.assign(h->sh.size(), nullptr);
  for (size_t k = 0; k < h->sh.size(); ++k) {
    HIPCHK(hipSetDevice(h->sh[k].device));
    if (int rc = custom_function(f.inv, h->sh[k].device, f64, fn[k], batched)) return rc;
  }
  h->fill = FillInvariant{};
  h->fill.kind = 3;
  return 0;
}

void destroy_invariant(Invariant* inv) {
  for (auto& kv : inv->loaded) {
    hipSetDevice(kv.first);
    hipModuleUnload(kv.second.module);
  }
  delete inv;
}

}  // namespace
