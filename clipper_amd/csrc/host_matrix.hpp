// host_matrix.hpp — the compressed copy of M (build, plan, expand), the affinity driver, gathers
// Part of clipper_hip.hip (one translation unit; included there, in order).
#pragma once

#include "host_fits.hpp"

namespace {

// ---- the compressed storage (CLIPPER_HIP_STORE_F32_CSC / _F64_CSC): groups -> slices ----------
bool csc_applies(const Ctx* h) { return csc_possible(h) && !h->explicitC; }
constexpr int SL_H = 1;  // sub-blocks per chunk (R = SL_SUB * SL_H = 128 rows): see k_slices.hip.h / DESIGN.md

// the descriptor of the slices in `st` for `nrows` rows through `rowmap` (null: the rows of M)
SliceView store_view(const SliceStore& st, const int32_t* rowmap, int64_t nrows) {
  SliceView v{};
  v.data = st.sdata;
  v.Pre = st.sPre;
  v.work = st.swork;
  v.nchunks = st.s_nchunks;
  v.ncg = st.s_ncg;
  v.nwork = st.s_nwork;
  v.rowmap = rowmap;
  v.nrows = nrows;
  return v;
}

SliceView slice_view(const Ctx* h, const Shard& s) { return store_view(s, nullptr, h->m); }

// the row view of this shard's columns (data == null: none in use)
SliceView row_view(const Ctx* h, const Shard& s) {
  if (!s.rv.valid || !h->csc_valid) return SliceView{};
  return store_view(s.rv.st, s.rv.rowmap[s.rv.cur], s.rv.nrows);
}

// the replica of the view over ALL columns (column shards; data == null: none). No work list: nothing streams it.
SliceView row_view_full(const Ctx* h, const Shard& s) {
  if (!s.rv.valid || !s.rv.full_valid || !h->csc_valid) return SliceView{};
  SliceView R = store_view(s.rv.full, s.rv.rowmap[s.rv.cur], s.rv.nrows);
  R.work = nullptr;
  R.nwork = 0;
  return R;
}

// The dense store of every local shard, allocated if it is not; with `from_csc` its content is
// materialised from the slices when they are all there is.
int ensure_dense(Ctx* h, bool from_csc) {
  for (auto& s : h->sh) {
    if (s.S) continue;
    HIPCHK(hipSetDevice(s.device));
    if (s.S.alloc(s.bytes_S) != hipSuccess) {
      (void)hipGetLastError();
      return fail(CLIPPER_HIP_E_NOMEM, "dense store of %zu bytes (this call needs one) does not fit",
                  s.bytes_S);
    }
    if (from_csc && h->csc_valid) {
      const int64_t nsl = static_cast<int64_t>(s.s_ncg) * s.s_nchunks;
      dim3 grid(static_cast<unsigned>(ceil_div(nsl, 4))), block(256);
      dispatch_vt(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_slice_expand<T, SL_H, T>), grid, block, 0, s.stream, slice_view(h, s),
                           s.S.as<T>(), h->W, h->m);
      });
      HIPCHK(hipStreamSynchronize(s.stream));
    }
  }
  return 0;
}

// the explicit constraint store of every local shard (C != pattern(M)) released
void drop_explicit_c(Ctx* h) {
  for (auto& s : h->sh) {
    hipSetDevice(s.device);
    s.Cs.reset();
  }
}

void drop_dense(Ctx* h) {
  for (auto& s : h->sh) {
    hipSetDevice(s.device);
    s.S.reset();
  }
}

// A small copy between pinned host memory and the device: a k_copy_words launch of `grid` workgroups through the
// mapped pointer of `pinned` (a launch beats a DMA copy at these sizes), hipMemcpyAsync when the copy is larger than
// `max_bytes` or the pointer is not mapped. `bytes` is a multiple of 16.
int copy_small(hipStream_t st, void* pinned, void* dev, size_t bytes, bool to_dev, unsigned grid, size_t max_bytes) {
  void* mapped = nullptr;
  if (bytes <= max_bytes && hipHostGetDevicePointer(&mapped, pinned, 0) == hipSuccess && mapped) {
    hipLaunchKernelGGL(k_copy_words, dim3(grid), dim3(256), 0, st, static_cast<const uint4*>(to_dev ? mapped : dev),
                       static_cast<uint4*>(to_dev ? dev : mapped), static_cast<int64_t>(bytes / 16));
  } else {
    (void)hipGetLastError();
    HIPCHK(hipMemcpyAsync(to_dev ? dev : pinned, to_dev ? pinned : dev, bytes,
                          to_dev ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, st));
  }
  return 0;
}
// the grid of a copy_small of `bytes`: a 256-lane workgroup per 4 KB, at most 64
unsigned copy_grid(size_t bytes) { return static_cast<unsigned>(std::min<size_t>(ceil_div(bytes / 16, 256), 64)); }

// the per-slice arrays (directory, sizes, costs) of the store `st` (this shard's columns x `nrows`
// rows) and the pinned staging of this build
// (wcols: the store's columns, a multiple of 64 — the shard's pitch W unless the store is a REPLICA of a row view
// over all columns, host_rowview.hpp)
int slices_arrays(Ctx* h, Shard& sh, SliceStore& s, int64_t nrows, int64_t wcols = -1) {
  HIPCHK(hipSetDevice(sh.device));
  if (!sh.cctl) HIPCHK(sh.cctl.alloc(CSC_ARENAS));
  s.s_ncg = static_cast<int>((wcols > 0 ? wcols : h->W) / SL_W);
  s.s_nchunks = static_cast<int>(ceil_div(nrows, SL_SUB * SL_H));
  const size_t nsl = static_cast<size_t>(s.s_ncg) * s.s_nchunks;
  // (room behind the directory words for the arena counters of a direct emission: one read-back)
  const size_t dir_bytes = round_up(nsl, 32) * sizeof(uint32_t) + CSC_ARENAS * sizeof(CscBuildCtl);
  if (nsl > s.sSizes.cap || !s.sBlk) {  // the four go together, then come together (sBlk last: without it the group is not whole)
    s.sSizes.reset(), s.sLq.reset(), s.sPre.reset(), s.sBlk.reset();
    HIPCHK(s.sSizes.alloc(nsl));
    HIPCHK(s.sLq.alloc_bytes(dir_bytes));
    HIPCHK(s.sPre.alloc(nsl));
    HIPCHK(s.sBlk.alloc(ceil_div(nsl, SCAN_BLK) + 4));
  }
  if (nsl > h->csc_hLq_slices || !h->csc_hLq) {
    h->csc_hLq_slices = 0;
    HIPCHK(h->csc_hLq.alloc_bytes(dir_bytes));
    h->csc_hLq_slices = nsl;
  }
  if (!h->csc_hctl) HIPCHK(h->csc_hctl.alloc(2 * CSC_ARENAS));
  if (!h->csc_htotal) HIPCHK(h->csc_htotal.alloc(2));
  return 0;
}
int slices_arrays(Ctx* h, Shard& s) { return slices_arrays(h, s, s, h->m); }

// the arenas' start values, `units` split evenly, in the second half of the pinned counters (what the device starts from)
CscBuildCtl* arena_init(Ctx* h, size_t units) {
  CscBuildCtl* init = h->csc_hctl + CSC_ARENAS;
  for (int k = 0; k < CSC_ARENAS; ++k) {
    init[k].cursor = 0;
    init[k].capacity = units / CSC_ARENAS;
    init[k].origin = static_cast<unsigned long long>(k) * (units / CSC_ARENAS);
    init[k].overflow = 0;
  }
  return init;
}

// Before a fill that writes the slices itself (k_affinity_sym): the arenas of the slice store
// reset. out.Pre == null: compressed storage not in use.
int emit_prepare(Ctx* h, Shard& sh, SliceStore& s, int64_t nrows, SliceOut& out, int64_t wcols = -1) {
  out = SliceOut{};
  if (!csc_applies(h)) return 0;
  if (int rc = slices_arrays(h, sh, s, nrows, wcols)) return rc;
  const size_t units = s.sdata.cap >= SL_TAILPAD ? (s.sdata.cap - SL_TAILPAD) / 16 : 0;
  CscBuildCtl* init = arena_init(h, units);
  // the counters live right behind this build's directory words: both come back in ONE copy
  CscBuildCtl* ectl = reinterpret_cast<CscBuildCtl*>(
      s.sLq + round_up(static_cast<int64_t>(s.s_ncg) * s.s_nchunks, 32));
  // (the arenas' start values, 8 KB: one workgroup, whatever the size)
  if (int rc = copy_small(sh.stream, init, ectl, CSC_ARENAS * sizeof(CscBuildCtl), true, 1, SIZE_MAX)) return rc;
  out.Pre = s.sPre;
  out.Lq = s.sLq;
  out.data = s.sdata;
  out.ctl = ectl;
  out.nchunks = s.s_nchunks;
  out.ncg = s.s_ncg;
  out.stamps = h->stamps_dev ? h->stamps_dev + 8192 : nullptr;
  return 0;
}
int emit_prepare(Ctx* h, Shard& s, SliceOut& out) {
  h->csc_valid = false;
  h->csc_emitted = false;
  return emit_prepare(h, s, s, h->m, out);
}

// After such a fill: the counters to pinned host memory; emit_check() reads them once the stream
// was synchronised, grows the arena if a slice did not fit (`again`), else plans the passes.
int emit_enqueue(Ctx* h, Shard& sh, SliceStore& s) {
  HIPCHK(hipSetDevice(sh.device));
  const size_t nsl8 = static_cast<size_t>(round_up(static_cast<int64_t>(s.s_ncg) * s.s_nchunks, 32));
  const size_t bytes = nsl8 * sizeof(uint32_t) + CSC_ARENAS * sizeof(CscBuildCtl);
  return copy_small(sh.stream, h->csc_hLq, s.sLq, bytes, false, copy_grid(bytes), 1u << 20);
}
int emit_enqueue(Ctx* h, Shard& s) { return emit_enqueue(h, s, s); }

int slices_plan(Ctx* h, Shard& sh, SliceStore& s, bool whole);
int slices_plan(Ctx* h, Shard& s) { return slices_plan(h, s, s, true); }
int resident_plan(Ctx* h, Shard& s);

int emit_check(Ctx* h, Shard& sh, SliceStore& s, bool whole, bool& again, bool plan = true) {
  again = false;
  HIPCHK(hipSetDevice(sh.device));
  bool over = false;
  size_t worst = 0;
  uint64_t sum = 0;
  const CscBuildCtl* rb = reinterpret_cast<const CscBuildCtl*>(
      h->csc_hLq + round_up(static_cast<int64_t>(s.s_ncg) * s.s_nchunks, 32));
  for (int k = 0; k < CSC_ARENAS; ++k) {
    over = over || rb[k].overflow != 0;
    worst = std::max(worst, static_cast<size_t>(rb[k].cursor));
    sum += rb[k].cursor;
  }
  if (over) {
    const size_t need = worst * CSC_ARENAS;  // every arena as large as the fullest one
    const size_t units = (need + need / 8 + 256 * CSC_ARENAS) / CSC_ARENAS * CSC_ARENAS;
    HIPCHK(s.sdata.alloc(units * 16 + SL_TAILPAD));
    HIPCHK(hipMemsetAsync(s.sdata + units * 16, 0, SL_TAILPAD, sh.stream));
    again = true;
    return 0;
  }
  s.s_bytes = sum * 16;
  if (!plan) {  // (a row view the resident solver takes: its work list is planned behind that launch, host_rowview.hpp)
    s.s_nwork = 0;
    return 0;
  }
  return slices_plan(h, sh, s, whole);
}
int emit_check(Ctx* h, Shard& s, bool& again) { return emit_check(h, s, s, true, again); }

// Before a build through groups: the group directory, the arenas' cursors reset, the per-slice arrays. Returns
// what a kernel that emits groups needs; out.Goff == null: compressed storage not in use.
template <typename VT>
int groups_prepare(Ctx* h, Shard& s, GroupOut<VT>& out) {
  out = GroupOut<VT>{};
  h->csc_valid = false;
  h->csc_emitted = false;
  if (!csc_applies(h)) return 0;
  HIPCHK(hipSetDevice(s.device));
  h->csc_nblocks = static_cast<int>(ceil_div(h->m, GR_RB));
  h->csc_nstrips = static_cast<int>(ceil_div(h->W, GR_CW));
  const size_t G = static_cast<size_t>(h->csc_nstrips) * static_cast<size_t>(h->csc_nblocks);
  if (G > s.gPre.cap) {
    s.gOff.reset(), s.gPre.reset();
    HIPCHK(s.gOff.alloc(G * GR_OFFS));
    HIPCHK(s.gPre.alloc(G));
  }
  if (int rc = slices_arrays(h, s)) return rc;
  HIPCHK(hipMemcpyAsync(s.cctl, arena_init(h, s.gcap_units()), CSC_ARENAS * sizeof(CscBuildCtl), hipMemcpyHostToDevice,
                        s.stream));
  out.Goff = s.gOff;
  out.Gpre = s.gPre;
  out.vals = s.gvals.as<VT>();
  out.rows = s.grows;
  out.ctl = s.cctl;
  out.nblocks = h->csc_nblocks;
  return 0;
}

// count -> scan -> pack (the pack returns at once if the groups overflowed or the slice arena is
// too small) -> copies of the counters to pinned host memory; slices_check() reads them once
// the stream was synchronised.
template <typename VT, typename Source>
int slices_enqueue(Ctx* h, Shard& s, const Source& src, const CscBuildCtl* ctl) {
  HIPCHK(hipSetDevice(s.device));
  const int64_t nsl = static_cast<int64_t>(s.s_ncg) * s.s_nchunks;
  const int64_t nblk = ceil_div(nsl, SCAN_BLK);
  dim3 g4(static_cast<unsigned>(ceil_div(nsl, 4))), b256(256);
  hipLaunchKernelGGL((k_slice_count<VT, SL_H, Source>), g4, b256, 0, s.stream, src, s.s_ncg,
                     s.s_nchunks, s.sSizes, s.sLq, ctl, s.sBlk + nblk + 1);
  if (nsl <= 32768) {
    hipLaunchKernelGGL(k_slice_scan_small, dim3(1), dim3(1024), 0, s.stream, s.sSizes, nsl, s.sPre,
                       s.sBlk + nblk);
  } else {
    hipLaunchKernelGGL(k_slice_scan_local, dim3(static_cast<unsigned>(nblk)), b256, 0, s.stream,
                       s.sSizes, nsl, s.sPre, s.sBlk);
    hipLaunchKernelGGL(k_slice_scan_blocks, dim3(1), b256, 0, s.stream, s.sBlk, nblk);
    hipLaunchKernelGGL(k_slice_scan_add, dim3(static_cast<unsigned>(nblk)), b256, 0, s.stream, s.sPre,
                       nsl, s.sBlk);
  }
  const uint64_t cap_units = s.sdata.cap >= SL_TAILPAD ? (s.sdata.cap - SL_TAILPAD) / 16 : 0;
  int heavy_only = 0;
  if constexpr (std::is_same<Source, GroupSource<VT>>::value && SL_H == 1) {
    // the common case through LDS (coalesced), only the slices of dense blocks by per-lane gathers
    hipLaunchKernelGGL((k_slice_pack_staged<VT>), g4, b256, 0, s.stream, src, s.s_ncg, s.s_nchunks,
                       s.sPre, s.sdata, s.sBlk + nblk, cap_units);
    heavy_only = 1;
  }
  hipLaunchKernelGGL((k_slice_pack<VT, SL_H, Source>),
                     dim3(static_cast<unsigned>(std::min<int64_t>(nsl, 1 << 20))),
                     dim3(SL_PACKW * 64), 0, s.stream, src, s.s_ncg, s.s_nchunks, s.sPre, s.sdata,
                     s.sBlk + nblk, cap_units, s.sLq, heavy_only);
  if (ctl)
    HIPCHK(hipMemcpyAsync(h->csc_hctl, s.cctl, CSC_ARENAS * sizeof(CscBuildCtl),
                          hipMemcpyDeviceToHost, s.stream));
  HIPCHK(hipMemcpyAsync(h->csc_htotal, s.sBlk + nblk, sizeof(uint64_t), hipMemcpyDeviceToHost,
                        s.stream));
  HIPCHK(hipMemcpyAsync(h->csc_hLq, s.sLq, static_cast<size_t>(nsl) * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, s.stream));
  return 0;
}

template <typename VT>
GroupSource<VT> group_source(const Ctx* h, const Shard& s) {
  GroupSource<VT> g{};
  g.Goff = s.gOff;
  g.Gpre = s.gPre;
  g.vals = s.gvals.as<const VT>();
  g.rows = s.grows;
  g.nblocks = h->csc_nblocks;
  g.ncols = static_cast<int64_t>(h->csc_nstrips) * GR_CW;
  return g;
}

// What a pass's workgroups do (SliceWork), planned per matrix from the slices' costs: per strip
// of SL_NW column groups, runs of chunks of about equal cost (cost of a chunk: its slowest
// slice — the waves of a workgroup meet at every chunk — plus a constant for the staging); a
// chunk that alone exceeds the target is split by step range. Most expensive first.
int slices_plan(Ctx* h, Shard& sh, SliceStore& s, bool whole) {
  static const double target_env = std::getenv("CLIPPER_HIP_CSC_WGS") ? std::max(1.0, std::atof(std::getenv("CLIPPER_HIP_CSC_WGS"))) : 0.0;
  static_assert(sizeof(clipper_plan::Work) == sizeof(SliceWork), "the planner's work item is the kernel's");
  static thread_local clipper_plan::PassPlan plan;  // (buffers kept from build to build)
  clipper_plan::plan_pass(h->csc_hLq, s.s_ncg, s.s_nchunks, clipper_plan::PassConsts{SL_NW, SL_SO, SL_OCC, whole ? 12 : 8},
                          h->cus, target_env, 2.0, plan);
  s.s_entries = plan.entries;
  const int nslots = plan.nslots;
  const size_t nw = plan.work.size();
  if (nw > h->csc_hwork.cap) HIPCHK(h->csc_hwork.alloc(nw + 1024));
  std::memcpy(h->csc_hwork, plan.work.data(), nw * sizeof(SliceWork));
  HIPCHK(hipSetDevice(sh.device));
  HIPCHK(s.swork.grow(std::max<size_t>(nw, 1)));
  int rc;
  const size_t bytes = nw * sizeof(SliceWork);  // 32 bytes each
  if ((rc = copy_small(sh.stream, h->csc_hwork, s.swork, bytes, true, copy_grid(bytes), 1u << 20))) return rc;
  // the pinned staging is shared by every store and shard of the context: the copy has to be
  // through before the next plan overwrites it (one shard's own builds are ordered by its stream
  // and by the wait that precedes every plan)
  if (h->sh.size() > 1) HIPCHK(hipStreamSynchronize(sh.stream));
  const size_t NSLOT = static_cast<size_t>(nslot(h->V));
  if (static_cast<size_t>(nslots) > sh.part_tiles) {
    HIPCHK(hipStreamSynchronize(sh.stream));
    sh.part_tiles = 0;
    HIPCHK(sh.part.alloc((static_cast<size_t>(nslots) + 8) * NSLOT * static_cast<size_t>(h->W)));
    sh.part_tiles = static_cast<size_t>(nslots) + 8;
  }
  s.s_nwork = static_cast<int>(nw);
  s.s_nslots = nslots;
  return whole ? resident_plan(h, sh) : 0;  // small problems: the whole solve as one launch
}

// After the stream was synchronised: did everything fit? If not (always the case for the first
// matrix of a size) the buffers are grown and `again` is set — the caller repeats the step that
// produces the groups; otherwise the work list is planned and the slices are valid.
template <typename VT>
int slices_check(Ctx* h, Shard& s, bool with_groups, bool& again) {
  again = false;
  if (!csc_applies(h)) return 0;
  HIPCHK(hipSetDevice(s.device));
  if (with_groups) {
    bool over = false;
    size_t worst = 0;
    for (int k = 0; k < CSC_ARENAS; ++k) {
      over = over || h->csc_hctl[k].overflow != 0;
      worst = std::max(worst, static_cast<size_t>(h->csc_hctl[k].cursor));
    }
    if (over) {
      const size_t need = worst * CSC_ARENAS;  // every arena as large as the fullest one
      s.gvals.reset(), s.grows.reset();
      const size_t units = (need + need / 8 + 64 * CSC_ARENAS) / CSC_ARENAS * CSC_ARENAS;
      HIPCHK(s.gvals.alloc(units * 4 * sizeof(VT)));
      HIPCHK(s.grows.alloc(units * 4));
      again = true;
    }
  }
  const uint64_t bytes = h->csc_htotal[0] * 16;
  if (bytes + SL_TAILPAD > s.sdata.cap) {
    const size_t cap = static_cast<size_t>(bytes) + static_cast<size_t>(bytes) / 16 + SL_TAILPAD + 4096;
    HIPCHK(s.sdata.alloc(cap));
    HIPCHK(hipMemsetAsync(s.sdata + bytes, 0, cap - bytes, s.stream));
    again = true;
  }
  if (again) return 0;
  s.s_bytes = bytes;
  return slices_plan(h, s);  // the caller declares the slices valid once every shard has them
}

int gather_slice_bytes(Ctx* h);

int build_overflows(const char* what = "compressed storage") {
  return fail(CLIPPER_HIP_E_HIP, "%s: the build keeps overflowing", what);
}

// the wait of a lone build on shard s (`what` heads the message if it fails)
int build_wait(Shard& s, const char* what) {
  if (hipStreamSynchronize(s.stream) != hipSuccess)
    return fail(CLIPPER_HIP_E_HIP, "%s: %s", what, hipGetErrorString(hipGetLastError()));
  return 0;
}

// groups from shard s's dense store, then the slices from the groups, queued on its stream (O: groups_prepare's)
template <typename VT>
int groups_enqueue(Ctx* h, Shard& s, const GroupOut<VT>& O) {
  dim3 grid(h->csc_nstrips, static_cast<unsigned>(ceil_div(h->csc_nblocks, 2))), block(256);
  hipLaunchKernelGGL((k_groups_from_dense<VT>), grid, block, 0, s.stream, s.S.as<const VT>(), h->W, h->m, O);
  return slices_enqueue<VT>(h, s, group_source<VT>(h, s), s.cctl);
}

// the end of a build from the dense store(s), once every shard's slices fit: M lives in the slices from here on
// (getters materialise a dense copy on demand)
int csc_rebuilt(Ctx* h) {
  h->csc_valid = true;
  drop_dense(h);
  if (int rc = sync_all(h)) return rc;
  return gather_slice_bytes(h);  // column shards: the row-view policy's cost model is about THIS matrix
}

// One build of shard s's slices from its dense store: queued; checked once the stream has drained (again = true: the
// buffers were grown, enqueue again). csc_rebuild runs the pair shard by shard, a batch over its children.
int csc_shard_enqueue(Ctx* h, Shard& s) {
  int rc = 0;
  dispatch_vt(h, [&](auto t) {
    using VT = decltype(t);
    GroupOut<VT> O;
    if ((rc = groups_prepare<VT>(h, s, O))) return;
    rc = groups_enqueue<VT>(h, s, O);
  });
  return rc;
}

int csc_shard_complete(Ctx* h, Shard& s, bool& again) {
  int rc = 0;
  dispatch_vt(h, [&](auto t) { rc = slices_check<decltype(t)>(h, s, true, again); });
  return rc;
}

// groups from the dense store(s) + pack + wait + plan: the setMatrixData paths, and every fill
// that went through a dense store. Shard by shard (the pinned staging is shared).
int csc_rebuild(Ctx* h) {
  h->csc_valid = false;
  h->total_slice_bytes = 0.0;
  if (!csc_applies(h)) return 0;
  for (auto& s : h->sh) {
    const int rc = clipper_fits::until_fits(
        1, clipper_fits::MAX_BUILDS, [&](size_t) { return csc_shard_enqueue(h, s); },
        [&] { return build_wait(s, "compressed storage: build failed"); },
        [&](size_t, bool& again) { return csc_shard_complete(h, s, again); }, [] { return build_overflows(); });
    if (rc) return rc;
  }
  return csc_rebuilt(h);
}

bool rect_fill_possible(const Ctx* h);
int launch_rect(Ctx* h, Shard& s, const int32_t* rowmap, int64_t nrows, const SliceOut& O, int64_t col0 = -1, int64_t wcols = -1);

// The slices of M[rows, columns] into `st` by the rectangular fill, repeated (the arenas grown) until they fit, `rounds`
// fills at most. (col0, wcols) = (-1, -1): this shard's columns. `plan`: the streamed pass's work list as well.
int emit_rect(Ctx* h, Shard& s, SliceStore& st, const int32_t* rowmap, int64_t nrows, int64_t col0, int64_t wcols,
              bool plan, int rounds, const char* what) {
  return clipper_fits::until_fits(
      1, rounds,
      [&](size_t) {
        SliceOut O{};
        int rc;
        if ((rc = emit_prepare(h, s, st, nrows, O, wcols))) return rc;
        if ((rc = launch_rect(h, s, rowmap, nrows, O, col0, wcols))) return rc;
        return emit_enqueue(h, s, st);
      },
      [&] {
        HIPCHK(hipStreamSynchronize(s.stream));
        HIPCHK(hipGetLastError());
        return 0;
      },
      [&](size_t, bool& again) { return emit_check(h, s, st, false, again, plan); }, [&] { return build_overflows(what); });
}

// Every compressed build the symmetric kernel cannot serve (fp64 values, column shards): the
// rectangular tile kernel writes each shard's slices straight from its LDS images — no dense store, no
// groups, no packers, whatever the size. The shards fill concurrently; their directories come back one
// after the other (the pinned staging is the context's).
int run_affinity_rect(Ctx* h, double& kernel_ms) {
  drop_dense(h);
  Shard& s0 = h->sh[0];
  HIPCHK(hipSetDevice(s0.device));
  if (!h->ev_aff[0]) {
    HIPCHK(h->ev_aff[0].create());
    HIPCHK(h->ev_aff[1].create());
  }
  std::vector<char> pending(h->sh.size(), 1);
  kernel_ms = 0.0;
  for (int attempt = 0;; ++attempt) {
    if (attempt >= clipper_fits::MAX_BUILDS)
      return fail(CLIPPER_HIP_E_HIP, "compressed storage: the build keeps overflowing");
    HIPCHK(hipSetDevice(s0.device));
    HIPCHK(hipEventRecord(h->ev_aff[0], s0.stream));
    std::vector<SliceOut> outs(h->sh.size());
    for (size_t k = 0; k < h->sh.size(); ++k) {
      if (!pending[k]) continue;
      Shard& s = h->sh[k];
      HIPCHK(hipSetDevice(s.device));
      int rc = emit_prepare(h, s, s, h->m, outs[k]);
      if (rc) return rc;
      // (emit_prepare stages the arenas' start values in pinned memory shared by all shards)
      if (h->sh.size() > 1) HIPCHK(hipStreamSynchronize(s.stream));
      if ((rc = launch_rect(h, s, nullptr, h->m, outs[k]))) return rc;
    }
    HIPCHK(hipSetDevice(s0.device));
    HIPCHK(hipEventRecord(h->ev_aff[1], s0.stream));
    bool any = false;
    for (size_t k = 0; k < h->sh.size(); ++k) {
      if (!pending[k]) continue;
      Shard& s = h->sh[k];
      int rc = emit_enqueue(h, s, s);
      if (rc) return rc;
      HIPCHK(hipStreamSynchronize(s.stream));
      HIPCHK(hipGetLastError());
      bool again = false;
      if ((rc = emit_check(h, s, s, csc_single(h), again))) return rc;
      pending[k] = again ? 1 : 0;
      any = any || again;
    }
    float ms = 0.f;
    HIPCHK(hipSetDevice(s0.device));
    HIPCHK(hipEventElapsedTime(&ms, h->ev_aff[0], h->ev_aff[1]));
    kernel_ms = ms;  // the last round of fills (the first of a problem size only sizes the arenas)
    if (!any) break;
  }
  return sync_all(h);
}

// `emits`: the fill kernel `launch` starts writes the slices itself when asked to
// (k_affinity_sym, fp32) — then neither a dense store nor groups are needed
int fill_done(Ctx* h, double build_ms);

// What a fill through run_affinity does before it launches anything: the matrix held is given up, the tiles planned,
// the route chosen (emit: the fill kernel writes the slices; rect: the rectangular fill builds them, no dense store) and,
// on the dense-store route, the store allocated. A batch's custom fill (host_batchsolve.hpp) starts with it too.
int affinity_begin(Ctx* h, bool emits, bool& emit, bool& rect) {
  h->has_matrix = false;  // until the build has succeeded (a failed rebuild leaves no matrix)
  h->csc_valid = false;
  h->total_slice_bytes = 0.0;  // (column shards: gathered again once this build's slices exist)
  for (auto& s : h->sh) s.rv.valid = false;  // a row view of the previous matrix
  h->nodes.clear();
  drop_explicit_c(h);  // not needed on this path: C == pattern(M)
  h->explicitC = false;
  plan_tiles(h);
  emit = csc_applies(h) && csc_single(h) && emits;  // (fp32 values, or fp64 values: k_affinity_sym<.., VT>)
  rect = !emit && csc_applies(h) && rect_fill_possible(h) && !h->plain_affinity && !h->strip_affinity;
  if (rect) return 0;
  if (emit) drop_dense(h);  // a materialised copy would be stale
  else if (int rc = ensure_dense(h, false)) return rc;
  return 0;
}

int fill_complete(Ctx* h, bool& again);

// One run of a fill's kernel, queued between the two events. emit: the arenas prepared before it, the directory's way
// back queued behind it; fill_complete() finishes such a build once the stream has drained.
template <typename Launch>
int fill_enqueue(Ctx* h, bool emit, Launch& launch) {
  Shard& s0 = h->sh[0];
  CscOut O{};
  if (emit) {
    if (int rc = emit_prepare(h, s0, O)) return rc;
  } else {
    h->csc_valid = false;
    h->csc_emitted = false;
  }
  h->csc_out = O;
  HIPCHK(hipSetDevice(s0.device));
  HIPCHK(hipEventRecord(h->ev_aff[0], s0.stream));
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    launch(s);  // k_affinity_sym writes the slices itself and sets csc_emitted
  }
  if (emit)
    if (int rc = emit_enqueue(h, s0)) return rc;
  HIPCHK(hipSetDevice(s0.device));
  HIPCHK(hipEventRecord(h->ev_aff[1], s0.stream));
  return 0;
}

// `queued` null: the fill runs to its end. Otherwise (a batch's fill) a fill that emits is only queued — the batch waits
// once for all its problems, then fill_complete() — and *queued says so; every other route runs to its end all the same.
template <typename Launch>
int run_affinity(Ctx* h, bool emits, Launch launch, bool* queued = nullptr) {
  if (queued) *queued = false;
  bool emit = false, rect = false;
  int rc = affinity_begin(h, emits, emit, rect);
  if (rc) return rc;
  if (rect) {
    double kms = 0.0;
    if ((rc = run_affinity_rect(h, kms))) return rc;
    h->csc_valid = true;
    h->csc_emitted = true;
    if ((rc = gather_slice_bytes(h))) return rc;
    h->tm.affinity_kernel_ms = kms;
    h->tm.affinity_bytes = static_cast<double>(h->sh[0].s_bytes);
    h->has_matrix = true;
    return 0;
  }
  Shard& s0 = h->sh[0];
  HIPCHK(hipSetDevice(s0.device));
  if (!h->ev_aff[0]) {
    HIPCHK(h->ev_aff[0].create());
    HIPCHK(h->ev_aff[1].create());
  }
  if (emit && queued) {
    *queued = true;
    return fill_enqueue(h, true, launch);
  }
  if (emit) {
    std::chrono::high_resolution_clock::time_point th0, th1;
    return clipper_fits::until_fits(
        1, clipper_fits::MAX_BUILDS, [&](size_t) { return fill_enqueue(h, true, launch); },
        [&] {
          th0 = std::chrono::high_resolution_clock::now();
          const int rcw = sync_all(h);
          th1 = std::chrono::high_resolution_clock::now();
          return rcw;
        },
        [&](size_t, bool& again) {
          const int rcc = fill_complete(h, again);
          if (!rcc && std::getenv("CLIPPER_HIP_HOST_TIMING")) {
            const auto th2 = std::chrono::high_resolution_clock::now();
            float kms = 0.f;
            (void)hipEventElapsedTime(&kms, h->ev_aff[0], h->ev_aff[1]);
            std::fprintf(stderr, "[affinity] enqueue->synced %.1f us (events %.1f us), check+plan %.1f us\n",
                         std::chrono::duration<double, std::micro>(th1 - th0).count(), kms * 1e3,
                         std::chrono::duration<double, std::micro>(th2 - th1).count());
          }
          return rcc;
        },
        [] { return build_overflows(); });
  }
  // dense slices (column shards, the other fill kernels, fp64 storage): the store filled, slices from it
  if ((rc = fill_enqueue(h, false, launch))) return rc;
  if ((rc = sync_all(h))) return rc;
  const auto t0 = std::chrono::high_resolution_clock::now();
  if ((rc = csc_rebuild(h))) return rc;
  return fill_done(h, std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count());
}

// the matrix is held: its fill's timings recorded (kernel_ms: the fill kernel's time, and the build's if any)
void fill_held(Ctx* h, double kernel_ms) {
  h->tm.affinity_kernel_ms = kernel_ms;
  h->tm.affinity_bytes = h->csc_valid ? static_cast<double>(h->sh[0].s_bytes)
                                      : static_cast<double>(h->sh[0].bytes_S);
  h->has_matrix = true;
}

// the end of a fill through run_affinity: timings, the matrix is held
int fill_done(Ctx* h, double build_ms) {
  float ms = 0.f;
  HIPCHK(hipSetDevice(h->sh[0].device));
  HIPCHK(hipEventElapsedTime(&ms, h->ev_aff[0], h->ev_aff[1]));
  fill_held(h, ms + (h->csc_valid ? build_ms : 0.0));
  return 0;
}

// The second half of fill_enqueue, once the stream has drained: the directory's check, the plans, the timings.
// again = true: an arena overflowed (they have been grown) — the caller repeats the fill.
int fill_complete(Ctx* h, bool& again) {
  if (int rc = emit_check(h, h->sh[0], again)) return rc;
  if (again) return 0;
  h->csc_valid = true;
  return fill_done(h, 0.0);
}

constexpr int AFF_ROWS_PER_BLK = 32;

// ALGORITHMIC bytes one mat-vec launch of shard 0 must move: s * m * (valid owned columns)
// (= s*m^2 on one GPU; the zero padding up to the 64-column pitch is not counted), doubled
// when an explicit constraint matrix is read as well.
double algorithmic_gemv_bytes(const Ctx* h, bool dense = false) {
  if (h->csc_valid && !dense)  // the slices (headers, lengths, step offsets, quads) + their directory
    return static_cast<double>(h->sh[0].s_bytes) +
           static_cast<double>(h->sh[0].s_ncg) * h->sh[0].s_nchunks * 8.0;
  const int64_t c0 = static_cast<int64_t>(h->sh[0].slot) * h->W;
  const int64_t valid = std::max<int64_t>(0, std::min<int64_t>(h->W, h->m - c0));
  return static_cast<double>(h->esize()) * static_cast<double>(h->m) *
         static_cast<double>(valid) * (h->explicitC ? 2.0 : 1.0);
}

// dsd::solve(M_, S) (dsd.cpp:274-320): gathers the sub-matrix induced by S from the device and runs
// Goldberg's algorithm on the host (dsd_host.h). Nodes come back ascending. With M in slices the gather
// walks the slices themselves (k_slice_gather_sub: one read of M, no dense copy — at m = 300 000 there
// could not be one); a dense store is gathered by index (k_gather_sub).
int densest_subgraph_of(Ctx* h, const std::vector<int32_t>& S, std::vector<int32_t>& nodes) {
  nodes.clear();
  const int k = static_cast<int>(S.size());
  if (k < 2) return 0;
  // k x k doubles on the host (twice while the shards' parts are added, once more inside the flow) and
  // on the device: a list of 100 000 nodes would ask for 80 GB each — refused, not thrown
  std::vector<double> Wsub, tmp;
  std::vector<int32_t> pos;
  try {
    Wsub.assign(static_cast<size_t>(k) * k, 0.0);
    tmp.resize(static_cast<size_t>(k) * k);
    pos.assign(static_cast<size_t>(h->m), -1);  // position of every node in the list
  } catch (const std::bad_alloc&) {
    return fail(CLIPPER_HIP_E_NOMEM, "densest subgraph of %d nodes: %.1f GB of host memory per copy of the sub-matrix", k,
                static_cast<double>(k) * k * 8e-9);
  }
  // a list that names a node twice is gathered by index
  bool listed_once = true;
  for (int a = 0; a < k; ++a) {
    int32_t& p = pos[static_cast<size_t>(S[static_cast<size_t>(a)])];
    listed_once = listed_once && p < 0;
    p = a;
  }
  const bool from_slices = h->csc_valid && listed_once;
  const auto t0 = std::chrono::high_resolution_clock::now();
  if (!from_slices)
    if (int rc = ensure_dense(h, true)) return rc;
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    DevBuf<int32_t> didx;
    DevBuf<double> dout;
    const size_t nidx = from_slices ? pos.size() : static_cast<size_t>(k);
    HIPCHK(didx.alloc(nidx));
    HIPCHK(dout.alloc(tmp.size()));
    HIPCHK(hipMemcpyAsync(didx, from_slices ? pos.data() : S.data(), nidx * sizeof(int32_t),
                          hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemsetAsync(dout, 0, tmp.size() * sizeof(double), s.stream));
    const int64_t c0 = static_cast<int64_t>(s.slot) * h->W;
    if (from_slices) {
      const int64_t nsl = static_cast<int64_t>(s.s_ncg) * s.s_nchunks;
      dim3 grid(static_cast<unsigned>(ceil_div(nsl, 4))), block(256);
      dispatch_vt(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_slice_gather_sub<T, SL_H>), grid, block, 0, s.stream, slice_view(h, s), didx,
                           c0, h->m, k, dout);
      });
    } else {
      dim3 grid(static_cast<unsigned>(ceil_div(static_cast<int64_t>(k) * k, 256))), block(256);
      dispatch_vt(h, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((k_gather_sub<T>), grid, block, 0, s.stream, s.S.as<const T>(), h->W, c0, h->W, didx,
                           k, dout);
      });
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(tmp.data(), dout, tmp.size() * sizeof(double), hipMemcpyDeviceToHost,
                          s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    didx.reset();
    dout.reset();
    for (size_t e = 0; e < tmp.size(); ++e) Wsub[e] += tmp[e];  // disjoint column sets
  }
  if (h->csc_valid) drop_dense(h);  // a copy materialised for this gather only: M lives in the slices
  const auto t1 = std::chrono::high_resolution_clock::now();
  int flows = 0;
  tmp = std::vector<double>();  // (the flow's residual matrix takes its place)
  try {
    for (int32_t a : dsd::densest_subgraph(Wsub, k, h->m, &flows)) nodes.push_back(S[static_cast<size_t>(a)]);
  } catch (const std::bad_alloc&) {
    return fail(CLIPPER_HIP_E_NOMEM, "densest subgraph of %d nodes: the flow network does not fit the host's memory", k);
  }
  if (std::getenv("CLIPPER_HIP_HOST_TIMING"))
    std::fprintf(stderr, "[dsd] k = %d: gather (%s) %.2f ms, host %.2f ms, %d maximum flows%s, %zu nodes\n", k,
                 from_slices ? "slices" : "dense store", std::chrono::duration<double, std::milli>(t1 - t0).count(),
                 std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t1).count(),
                 flows < 0 ? -flows : flows, flows < 0 ? " (plain bisection)" : "", nodes.size());
  return 0;
}

int fill_euclidean(Ctx* h, const EuclidParams& prm);  // the matrix from the staged points (clipper_hip.hip)
int fill_pointnormal(Ctx* h, const PointNormalParams& prm);
// the body behind both, for callers that hold the invariant as a record (the live sub-problem's child, a batch's
// children: `queued` as run_affinity's)
int fill_builtin(Ctx* h, const FillInvariant& inv, bool* queued);

// stage_inputs, then the fill: affinity_total_ms counts both
template <typename Params>
int stage_and_fill(Ctx* h, const double* D1, int d, int64_t n1, const double* D2, int64_t n2, const int32_t* A,
                   int64_t m, int (*fill)(Ctx*, const Params&), const Params& prm) {
  const auto t0 = std::chrono::high_resolution_clock::now();
  int rc = stage_inputs(h, D1, d, n1, D2, n2, A, m);
  if (rc || (rc = fill(h, prm))) return rc;
  h->tm.affinity_total_ms = std::chrono::duration<double, std::milli>(std::chrono::high_resolution_clock::now() - t0).count();
  return 0;
}

}  // namespace
