// host_matrix_io.hpp — the matrix in and out of a context: the affinity fill, the dense and sparse setters, the
// getter and the mat-vecs of the test API. Part of clipper_hip.hip (one translation unit; included there behind every
// other driver of a context and in front of the stand-alone searches: host_knn.hpp and what follows it). The order of
// the bodies here is the order in which the code object holds their kernels (the fill's: with_builtin_invariant's
// order of invariants).
#pragma once

namespace {

// The fill with a built-in invariant (declared in host_matrix.hpp): defined here, behind the batch, so that the fill
// kernels keep their place in the code object. One body for every invariant, reached with `queued` null (the fill runs
// to its end) or not (a batch's: see run_affinity's `queued`). `inv`: the kind and its parameters; the matrix of this
// context is then the one scored with it over the staged points, and a row view of it is filled from them later.
int fill_builtin(Ctx* h, const FillInvariant& inv, bool* queued) {
  // refused before anything changes: the matrix held stays, and the record of what it was scored with
  if (!with_builtin_invariant(inv, h->staged_d, [](auto, const auto&) {}))
    return fail(inv.kind == 1 || inv.kind == 2 ? CLIPPER_HIP_E_STATE : CLIPPER_HIP_E_INVALID,
                inv.kind == 1   ? "clipper_hip_stage_inputs not called"
                : inv.kind == 2 ? "PointNormalDistance needs staged inputs with d == 6"
                                : "not a built-in invariant");
  h->fill = inv;
  int rc = 0;
  with_builtin_invariant(h, [&](auto tag, const auto& prm) {
    using Inv = decltype(tag);
    const int64_t mm = h->m, W = h->W, pstride = h->staged_pstride;
    const int d = h->staged_d;
    h->fill.E = guarded_threshold(Inv::threshold(prm), h->staged_maxabs, Inv::prefilter_dim(d));
    h->fill.E2 = guarded_threshold_sq(h->fill.E);
    const float thr = h->fill.E, E2 = h->fill.E2;
    // the route: the symmetric tiles, else the compacting strips, else the plain kernel (the only one without a
    // prefilter: run-time dimensions, CLIPPER_HIP_AFFINITY=plain)
    const bool sym = Inv::PD > 0 && use_sym_fill(h);
    const bool compact = Inv::PD > 0 && !h->plain_affinity;
    rc = run_affinity(h, sym, [&](Shard& s) {
      const int64_t c0 = static_cast<int64_t>(s.slot) * W;
      const int32_t* A0 = s.Adev;
      const int32_t* A1 = s.Adev + mm;
      dispatch_vt(h, [&](auto t) {
        using T = decltype(t);
        if constexpr (Inv::PD > 0) {
          if (sym) {
            const int nT = static_cast<int>(ceil_div(mm, AT));
            const dim3 g(static_cast<unsigned>(static_cast<int64_t>(nT) * (nT + 1) / 2));
            T* S = static_cast<T*>(sizeof(T) == 8 ? nullptr : s.S);  // (slices with fp64 values: no dense store on this route)
            launch_sym<T>(k_affinity_sym<Inv, T>, g, s.stream, S, W, mm, nT, s, pstride, A0, A1, prm, E2, h->csc_out);
            return;
          }
        }
        const dim3 grid(static_cast<unsigned>(ceil_div(W, 1024)), static_cast<unsigned>(ceil_div(mm, AFF_ROWS_PER_BLK)));
        if constexpr (Inv::PD > 0) {
          if (compact) {
            hipLaunchKernelGGL((k_affinity_compact<T, Inv>), grid, dim3(256), 0, s.stream, s.S.as<T>(), W, mm, c0,
                               AFF_ROWS_PER_BLK, s.P1, s.P2, s.P1f, s.P2f, pstride, A0, A1, prm, thr);
            return;
          }
        }
        hipLaunchKernelGGL((k_affinity_plain<T, Inv>), grid, dim3(256), 0, s.stream, s.S.as<T>(), W, mm, c0,
                           AFF_ROWS_PER_BLK, d, s.P1, s.P2, pstride, A0, A1, prm);
      });
      if (sym) h->csc_emitted = (h->csc_out.Pre != nullptr);
    }, queued);
  });
  return rc;
}
int fill_euclidean(Ctx* h, const EuclidParams& prm) { return fill_builtin(h, FillInvariant::euclid(prm), nullptr); }
int fill_pointnormal(Ctx* h, const PointNormalParams& prm) { return fill_builtin(h, FillInvariant::pointnormal(prm), nullptr); }

// A user-defined invariant over the staged points (host_custom_invariant.hpp): every shard's dense store from the
// invariant's own fill kernel, then the slices from it as for any dense store. No rectangular fill exists for it
// (rect_fill_possible is false for kind 3): row views are built by filter, the live sub-problem stays off.
int fill_custom(Ctx* h, const CustomFill& f) {
  std::vector<hipFunction_t> fn;
  if (int rc = custom_fill_begin(h, f, false, fn)) return rc;
  const int64_t mm = h->m, W = h->W, pstride = h->staged_pstride;
  int launch_rc = 0;
  int rc = run_affinity(h, false, [&](Shard& s) {
    dim3 grid(static_cast<unsigned>(ceil_div(W, 1024)), static_cast<unsigned>(ceil_div(mm, AFF_ROWS_PER_BLK)));
    long long ld = W, m = mm, c0 = static_cast<int64_t>(s.slot) * W, ps = pstride;
    int rows = AFF_ROWS_PER_BLK;
    void* S = s.S;
    const double *P1 = s.P1, *P2 = s.P2;
    const int32_t *A0 = s.Adev, *A1 = s.Adev + mm;
    CustomParams prm = f.prm;
    void* args[] = {&S, &ld, &m, &c0, &rows, &P1, &P2, &ps, &A0, &A1, &prm};
    const hipFunction_t k = fn[static_cast<size_t>(&s - h->sh.data())];
    const hipError_t e = hipModuleLaunchKernel(k, grid.x, grid.y, 1, 256, 1, 1, 0, s.stream, args, nullptr);
    if (e != hipSuccess && !launch_rc)
      launch_rc = fail(CLIPPER_HIP_E_HIP, "hipModuleLaunchKernel (user-defined invariant): %s", hipGetErrorString(e));
  });
  if (launch_rc) {  // (run_affinity went on with a store the kernel never wrote)
    h->has_matrix = false;
    h->csc_valid = false;
    return launch_rc;
  }
  return rc;
}

// A matrix the caller hands over replaces the one held: no nodes, no row view, no points behind it, no explicit C
// store; the problem sized for m. has_matrix stays false until the new matrix is complete.
int begin_matrix(Ctx* h, int64_t m) {
  if (h->A.size() != static_cast<size_t>(2 * m)) h->A.clear();
  h->nodes.clear();
  h->has_matrix = false;
  h->csc_valid = false;
  h->total_slice_bytes = 0.0;
  h->fill.kind = 0;
  rowview_drop(h);
  drop_explicit_c(h);
  return ensure_problem(h, m);
}

// a CSC matrix of m columns to the device of shard s, its arrays held by `tmp`: `d` points at them
int upload_csc(DevTemps& tmp, Shard& s, int64_t m, const clipper_csc::CscRef& a, clipper_csc::CscRef& d) {
  const int64_t nnz = a.cp[m];
  int64_t* dcp = nullptr;
  int32_t* dri = nullptr;
  double* dva = nullptr;
  int rc;
  if ((rc = tmp.alloc(s.device, dcp, static_cast<size_t>(m + 1) * sizeof(int64_t)))) return rc;
  if ((rc = tmp.alloc(s.device, dri, static_cast<size_t>(nnz) * sizeof(int32_t)))) return rc;
  if ((rc = tmp.alloc(s.device, dva, static_cast<size_t>(nnz) * sizeof(double)))) return rc;
  HIPCHK(hipMemcpyAsync(dcp, a.cp, static_cast<size_t>(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s.stream));
  if (nnz > 0) {
    HIPCHK(hipMemcpyAsync(dri, a.ri, static_cast<size_t>(nnz) * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(dva, a.va, static_cast<size_t>(nnz) * sizeof(double), hipMemcpyHostToDevice, s.stream));
  }
  d = clipper_csc::CscRef{dcp, dri, dva};
  return 0;
}

// setMatrixData with dense (M, C), column-major m x m: pass 1 fills the store and finds out whether C is anything
// other than pattern(M); only then does an explicit C get a store of its own (pass 2).
int set_dense(Ctx* h, const double* M, const double* C, int64_t m) {
  int rc;
  {  // refused before anything changes: the matrix held stays (host_csc_input.hpp; C is 0 / 1: no range to leave)
    std::string err = clipper_csc::check_values_dense_upper("M", m, M, h->storage != CLIPPER_HIP_STORE_F64);
    if (err.empty()) err = clipper_csc::check_values_dense_upper("C", m, C, false);
    if (!err.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", err.c_str());
  }
  if ((rc = begin_matrix(h, m))) return rc;
  if ((rc = ensure_dense(h, false))) return rc;
  const size_t bytes = static_cast<size_t>(m) * m * sizeof(double);
  const int64_t W = h->W;
  DevTemps tmp;
  std::vector<double*> dM(h->sh.size(), nullptr), dC(h->sh.size(), nullptr);
  std::vector<int*> dflag(h->sh.size(), nullptr);
  const unsigned gy = static_cast<unsigned>(std::min<int64_t>(m, 65535));
  auto from_dense = [&](size_t k, void* Cs, int* flag) {
    Shard& s = h->sh[k];
    dim3 grid(static_cast<unsigned>(ceil_div(W, 256)), gy), block(256);
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    dispatch_vt(h, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_from_dense_upper<T>), grid, block, 0, s.stream, s.S.as<T>(), W, m, c0, dM[k],
                         dC[k], static_cast<T*>(Cs), flag);
    });
  };
  int mismatch = 0;
  for (size_t k = 0; k < h->sh.size(); ++k) {
    Shard& s = h->sh[k];
    HIPCHK(hipSetDevice(s.device));
    if ((rc = tmp.alloc(s.device, dM[k], bytes))) return rc;
    if ((rc = tmp.alloc(s.device, dC[k], bytes))) return rc;
    if ((rc = tmp.alloc(s.device, dflag[k], sizeof(int)))) return rc;
    HIPCHK(hipMemsetAsync(dflag[k], 0, sizeof(int), s.stream));
    HIPCHK(hipMemcpyAsync(dM[k], M, bytes, hipMemcpyHostToDevice, s.stream));
    HIPCHK(hipMemcpyAsync(dC[k], C, bytes, hipMemcpyHostToDevice, s.stream));
    from_dense(k, nullptr, dflag[k]);
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
      HIPCHK(s.Cs.alloc(s.bytes_S));
      from_dense(k, s.Cs, nullptr);
    }
  }
  if ((rc = sync_all(h))) return rc;
  if ((rc = csc_rebuild(h))) return rc;
  h->has_matrix = true;
  return 0;
}

// set_sparse with compressed storage and C == pattern(M): the slices packed straight from the symmetric lists (no
// dense intermediate: O(nnz) memory)
int sparse_to_slices(Ctx* h, const clipper_csc::CscRef& M) {
  const int64_t m = h->m, W = h->W;
  drop_dense(h);
  clipper_csc::CscLists L;
  const std::string err = clipper_csc::symmetric_lists(m, M, L);
  if (!err.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", err.c_str());
  DevTemps tmp;
  int rc = 0;
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    clipper_csc::CscRef d{};
    if ((rc = upload_csc(tmp, s, m, clipper_csc::CscRef{L.cp.data(), L.ri.data(), L.va.data()}, d))) return rc;
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    dispatch_vt(h, [&](auto t) {
      using VT = decltype(t);
      rc = clipper_fits::until_fits(
          1, clipper_fits::MAX_BUILDS,
          [&](size_t) {
            GroupOut<VT> O;  // (the groups go unused: groups_prepare sizes the slices' arrays as well)
            if (int r = groups_prepare<VT>(h, s, O)) return r;
            CscSource<VT> src{};
            src.colptr = d.cp + std::min<int64_t>(c0, m);
            src.rowidx = d.ri;
            src.values = d.va;
            src.ncols = std::max<int64_t>(0, std::min<int64_t>(W, m - c0));
            return slices_enqueue<VT>(h, s, src, nullptr);
          },
          [&] { return build_wait(s, "set_sparse"); },
          [&](size_t, bool& again) { return slices_check<VT>(h, s, false, again); }, [] { return build_overflows(); });
    });
    if (rc) return rc;
  }
  if ((rc = sync_all(h))) return rc;
  h->csc_valid = true;
  if ((rc = gather_slice_bytes(h))) return rc;  // column shards: the row-view policy's cost model
  h->has_matrix = true;
  return 0;
}

// set_sparse through the dense store (dense storage modes, or an explicit C): the lists scattered into it
int sparse_to_dense(Ctx* h, const clipper_csc::CscRef& M, const clipper_csc::CscRef& C) {
  int rc;
  if ((rc = ensure_dense(h, false))) return rc;
  const int64_t m = h->m, W = h->W;
  DevTemps tmp;
  auto scatter = [&](Shard& s, void* dst, const clipper_csc::CscRef& a) -> int {
    clipper_csc::CscRef d{};
    if (int r = upload_csc(tmp, s, m, a, d)) return r;
    HIPCHK(hipMemsetAsync(dst, 0, s.bytes_S, s.stream));
    const int64_t c0 = static_cast<int64_t>(s.slot) * W;
    dim3 grid(static_cast<unsigned>(std::min<int64_t>(m, 1 << 20))), block(256);
    dispatch_vt(h, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_from_csc<T>), grid, block, 0, s.stream, static_cast<T*>(dst), W, m, c0, W, d.cp, d.ri, d.va);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s.stream));
    return 0;
  };
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    if ((rc = scatter(s, s.S, M))) return rc;
    if (h->explicitC) {
      HIPCHK(s.Cs.alloc(s.bytes_S));
      if ((rc = scatter(s, s.Cs, C))) return rc;
    }
  }
  if ((rc = csc_rebuild(h))) return rc;
  h->has_matrix = true;
  return 0;
}

// setSparseMatrixData (clipper.cpp:162-166). Every stored (i, j) with i < j stands for the symmetric pair, as
// selfadjointView<Upper> reads it; entries below the diagonal are not read (the reference never does); the diagonal is
// implicit (host_csc_input.hpp). With compressed storage and C == pattern(M) the slices are packed straight from the
// lists; otherwise through the dense store. A call refused before begin_matrix leaves the matrix held as it was.
int set_sparse(Ctx* h, int64_t m, const int64_t* Mcolptr, const int32_t* Mrow, const double* Mval,
               const int64_t* Ccolptr, const int32_t* Crow, const double* Cval) {
  clipper_csc::CscRef M{Mcolptr, Mrow, Mval}, C{Ccolptr, Crow, Cval};
  clipper_csc::CscLists Mup, Cup;
  int64_t dropped_below = 0;  // entries below the diagonal, which the reference never reads: dropped, and reported
  std::string err = clipper_csc::check_csc("M", m, M);
  if (err.empty()) err = clipper_csc::check_csc("C", m, C);
  if (err.empty()) err = clipper_csc::upper_only("M", m, M, Mup, dropped_below);
  if (err.empty()) err = clipper_csc::upper_only("C", m, C, Cup, dropped_below);
  if (err.empty()) err = clipper_csc::check_values_csc("M", m, M, h->storage != CLIPPER_HIP_STORE_F64);
  if (err.empty()) err = clipper_csc::check_values_csc("C", m, C, false);
  if (!err.empty()) return fail(CLIPPER_HIP_E_INVALID, "%s", err.c_str());
  // (a warning, not an error — the call goes on and returns 0 unless something else fails: clipper_hip_last_error()
  // tells a caller who handed over both triangles, or only the lower one, what became of them)
  if (dropped_below > 0)
    (void)fail(0, "warning: %lld stored entries below the diagonal were ignored (the matrices are read through their upper "
                  "triangle, as the reference's selfadjointView<Upper> does: clipper.cpp:194-271)", static_cast<long long>(dropped_below));
  if (int rc = begin_matrix(h, m)) return rc;
  h->explicitC = !clipper_csc::is_pattern(m, M, C);
  plan_tiles(h);
  return csc_applies(h) ? sparse_to_slices(h, M) : sparse_to_dense(h, M, C);
}

// getMatrixData / getConstraintData: the dense (M, C), column-major m x m, identity on the diagonal
int get_dense(Ctx* h, double* M_out, double* C_out) {
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
                             : static_cast<double>(reinterpret_cast<const float*>(buf.data())[j * W + c]);
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
}

// x -> candidate 0 of table 0 of a shard (staged through the u0 buffer)
int stage_x(Ctx* h, Shard& s, const double* x) {
  HIPCHK(hipMemcpyAsync(s.u0, x, static_cast<size_t>(h->m) * sizeof(double), hipMemcpyHostToDevice, s.stream));
  hipLaunchKernelGGL(k_spread, dim3(static_cast<unsigned>(ceil_div(h->m, 256))), dim3(256), 0, s.stream, s.u0, h->m,
                     s.X[0]);
  h->u0_staged = false;
  return 0;
}

// yM = M_off x, yC = C_off x (the identity left out): one pair-mode mat-vec
int matvec(Ctx* h, const double* x, double* yM, double* yC) {
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  const int64_t m = h->m, W = h->W;
  int rc;
  for (auto& s : h->sh) {
    HIPCHK(hipSetDevice(s.device));
    if ((rc = stage_x(h, s, x))) return rc;
  }
  rc = h->csc_valid ? 0 : ensure_dense(h, true);
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
}

// The products of matvec through a ROW VIEW of the given rows: yM = M_off[:, rows] x[rows], yC likewise — what a pass
// of the solver computes when it streams the view instead of M. Builds the slices of M[rows, :] with the rectangular
// fill kernel from the staged points (the view of a later solve is built anew). For tests: equal to matvec of x with
// every other entry zeroed, up to the order of the partial sums.
int view_matvec(Ctx* h, const int32_t* rows, int64_t nrows, const double* x, double* yM, double* yC) {
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
  HIPCHK(v.rowmap[0].grow(static_cast<size_t>(h->mp)));
  HIPCHK(v.rowmap[1].grow(static_cast<size_t>(h->mp)));
  HIPCHK(hipMemcpyAsync(v.rowmap[0], rows, static_cast<size_t>(nrows) * sizeof(int32_t), hipMemcpyHostToDevice, s.stream));
  if ((rc = emit_rect(h, s, v.st, v.rowmap[0], nrows, -1, -1, true, 3, "row view"))) return rc;
  if ((rc = stage_x(h, s, x))) return rc;
  launch_slices_plain(h, s, store_view(v.st, v.rowmap[0], nrows), s.X[0]);
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
}

// ---- measurement ---------------------------------------------------------------------------

// the mean time of one pair-mode mat-vec on shard 0 over `reps` launches (after 3 unmeasured ones)
int bench_matvec(Ctx* h, int reps, double* avg_us) {
  if (!h->has_matrix) return fail(CLIPPER_HIP_E_STATE, "no matrix has been built or set");
  if (!h->csc_valid)
    if (int rc = ensure_dense(h, true)) return rc;
  Shard& s = h->sh[0];
  HIPCHK(hipSetDevice(s.device));
  Event e0, e1;  // (gone on every path out of here)
  HIPCHK(e0.create());
  HIPCHK(e1.create());
  for (int w = 0; w < 3; ++w) launch_plain(h, s, s.X[0]);
  HIPCHK(hipEventRecord(e0, s.stream));
  for (int r = 0; r < reps; ++r) launch_plain(h, s, s.X[0]);
  HIPCHK(hipEventRecord(e1, s.stream));
  HIPCHK(hipStreamSynchronize(s.stream));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  *avg_us = static_cast<double>(ms) * 1e3 / reps;
  h->tm.gemv_bytes = algorithmic_gemv_bytes(h, /*dense=*/!h->csc_valid);
  return 0;
}

// `workgroups` workgroups of one wave, each holding `lds_bytes` of LDS, spinning for `milliseconds` on their own stream
int debug_occupy(int device, int workgroups, int lds_bytes, double milliseconds) {
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
}

}  // namespace
