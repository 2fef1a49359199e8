/*
 * clipper_hip.h — C ABI of the MI355X (gfx950) implementation of CLIPPER's dense-cluster
 * hot path. This is the drop-in boundary: plain pointers, sizes and PODs only, no C++
 * or framework types. The reference has no FFI of its own for this path (it is one C++
 * shared library, CMakeLists.txt:93); each entry point below names the reference member
 * function (file:line relative to /root/reference) whose work it takes over, and
 * clipper_amd/csrc/host/ holds the `clipper::CLIPPER` facade + `clipperpy` module that a
 * maintainer binds to it.
 *
 * Conventions
 *   - Matrices are column-major fp64 (Eigen default). A is column-major m x 2 int32.
 *   - Every function returns 0 on success, <0 on failure (CLIPPER_HIP_E_*); the message
 *     is available from clipper_hip_last_error() (thread-local). Nothing throws.
 *   - Calls are synchronous from the caller's view; one context = one problem instance,
 *     not thread-safe per context (same as clipper::CLIPPER), independent across contexts.
 *   - There is NO CPU fallback: without a usable HIP device every call fails loudly.
 *
 * Storage of the affinity matrix on device
 *   CLIPPER_HIP_STORE_F32_CSC (the default of every front end) and CLIPPER_HIP_STORE_F64_CSC
 *   hold ONLY the stored (nonzero) entries of M_off — both triangles, as the reference's
 *   Eigen::SparseMatrix does (include/clipper/types.h:15) — as per-column lists of (value,
 *   row byte) cut into slices of 64 columns x 128 rows, padded to groups of 4 entries and to
 *   nothing else (5.7 bytes per stored entry with fp32 values, 9.6 with fp64).
 *   The solver's passes stream the slices; a dense store is materialised only while a getter,
 *   the exact-DSD gather or an explicit C needs one and is dropped again. Column shards hold
 *   the slices of their own columns. The values, the fp64 products and every decision are
 *   those of the dense storage of the same value type; only the zeros are skipped. These
 *   storages apply whenever C == pattern(M) (always on the scorePairwiseConsistency path,
 *   clipper.cpp:63-64); setMatrixData with any other C falls back to the dense store of the
 *   same value type. gemv_bytes reports the bytes the slices hold = what one pass streams.
 *   CLIPPER_HIP_STORE_F32 / _F64 keep M_off dense in HBM as column slices: a context that
 *   owns global columns [c0, c0+W) stores S[j][c] = M(j, c0+c) for all m rows j, row pitch W
 *   (multiple of 64 elements, zero padded): 4*m^2 (8*m^2) bytes. On the
 *   scorePairwiseConsistency path C is not stored: the mat-vec kernel derives C_off*x from
 *   the same pass over M. setMatrixData with any other C stores a second dense matrix.
 *   All vectors, accumulators, scalars and branch operands of the solver are fp64 in every
 *   mode; fp32 is a STORAGE type of M's entries only.
 */
#ifndef CLIPPER_HIP_H
#define CLIPPER_HIP_H

#include <stddef.h>

#include "clipper_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct clipper_hip_ctx clipper_hip_t;

enum {
  CLIPPER_HIP_STORE_F32 = 0,
  CLIPPER_HIP_STORE_F64 = 1,
  CLIPPER_HIP_STORE_F32_CSC = 2,
  CLIPPER_HIP_STORE_F64_CSC = 3
};

enum {
  CLIPPER_HIP_OK = 0,
  CLIPPER_HIP_E_INVALID = -1,  /* bad argument                       */
  CLIPPER_HIP_E_NOMEM = -2,    /* device or host allocation failed   */
  CLIPPER_HIP_E_HIP = -3,      /* HIP runtime error                  */
  CLIPPER_HIP_E_NODEVICE = -4, /* no gfx950 device visible           */
  CLIPPER_HIP_E_STATE = -5,    /* call out of order (no matrix yet)  */
  CLIPPER_HIP_E_COMM = -6,     /* RCCL error / communicator missing  */
  CLIPPER_HIP_E_SCOPE = -7,    /* not available in this configuration */
  CLIPPER_HIP_E_INTERNAL = -8  /* an unexpected C++ exception was caught at the boundary */
};

/* Timings of the most recent calls, from HIP events on the context's own stream. */
typedef struct clipper_hip_timings_t {
  double affinity_kernel_ms; /* affinity fill kernel(s) only                           */
  double affinity_total_ms;  /* H2D of D1,D2,A + gather + fill, host wall clock         */
  double solve_total_ms;     /* host wall clock of clipper_hip_solve                    */
  double gemv_avg_us;        /* mean duration of the mat-vec kernel (k_gemv: one pass over
                                M for a whole line-search window) over the last solve
                                (only when profiling is on; else 0)                     */
  double gemv_min_us;
  int64_t gemv_launches;     /* number of mat-vec launches that were timed              */
  double gemv_bytes;         /* algorithmic bytes of one launch: s*m*(owned columns) for a
                                dense store; for the compressed storage the bytes the slices
                                hold (headers, lengths, value and row quads) + their directory */
  double gemv_useful_bytes;  /* compressed storage: stored entries (both triangles, no quad
                                padding) x (value + row byte); dense store: = gemv_bytes     */
  double affinity_bytes;     /* bytes of M the last affinity build wrote (dense store or slices) */
  double exchange_avg_us;    /* column shards: mean duration of the sampled per-pass exchanges (reduce
                                launch + all-gather) of the last solve, HIP events on the solver
                                stream (profiling on; 0: none sampled / one shard)            */
  int64_t exchange_samples;
  double exchange_bytes;     /* bytes this rank contributes to one exchange                   */
} clipper_hip_timings_t;

/* The row view of the last solve (clipper_hip_set_row_view below). */
typedef struct clipper_hip_view_stats_t {
  int64_t builds;        /* row views built during the last solve                           */
  int64_t rows;          /* rows of the last one built (0: none)                            */
  int64_t bytes;         /* bytes its slices hold                                           */
  int64_t view_passes;   /* passes of the last solve that streamed a view instead of M      */
  int64_t passes;        /* all passes of the last solve                                    */
  double build_ms;       /* host wall clock spent building views (drain + compaction + fill + plan) */
  double view_pass_avg_us; /* mean duration of the sampled pass launches that streamed a view
                              (profiling on; 0 = none sampled)                               */
  int64_t view_pass_samples;
  int64_t resident_launches; /* launches of the resident solver on a view (k_rv_resident.hip.h) that RAN: the passes
                                on a view that ran inside one are counted in view_passes, not sampled   */
  int64_t resident_giveups;  /* launches of it that gave up and changed nothing (a unit that did not become resident
                                within the exchange's time-out — e.g. another tenant on the device —, a refused LDS
                                plan): the streaming launches did their work; the context then streams the views of
                                its next solves (1, 2, 4, ... 64 of them) before it tries again              */
  int64_t resident_iterations; /* solver iterations (one exchange each) that ran inside the launches that ran  */
  double resident_us;          /* their duration on the device's own wall clock: unit 0's first instruction to
                                  the last unit's commit (100 MHz ticks; free, always on)                      */
  double resident_event_us;    /* the same by HIP events around the launches (clipper_hip_set_profiling(h, 2):
                                  an event pair costs stream time, so not in a timed region); 0 = not timed   */
  int64_t resident_entries;    /* stored entries (quads x 4, padding included) of the view the last launch ran on */
  int64_t resident_units;      /* workgroups (one per CU: each holds its columns of the view in LDS) of that launch */
  /* the live sub-problem (csrc/k_subproblem.hip.h, clipper_hip_set_subproblem below) */
  int64_t sub_entries;         /* hand-overs of the last solve to the sub-problem of the associations that can still be selected */
  int64_t sub_leaves;          /* ... and hand-overs back (a column outside it could have come back to life)   */
  int64_t sub_passes;          /* passes of the last solve that ran on the sub-problem (not counted in view_passes) */
  int64_t sub_rows;            /* associations of the sub-problem (0: none was prepared)                       */
  int64_t sub_bytes;           /* bytes its slices hold                                                        */
  double sub_build_ms;         /* host wall clock spent preparing it (selection, gather, fill, plan)           */
  double sub_pass_avg_us;      /* mean duration of the sampled window passes on it (profiling on; 0 = none)    */
  int64_t sub_pass_samples;
  int64_t sub_dense;           /* 1: the sub-problem was mostly non-zero and was kept as a dense fp32 store (its passes: k_gemv) */
} clipper_hip_view_stats_t;

/* ---- life cycle --------------------------------------------------------------------- */

int clipper_hip_device_count(void);

/* One device holds the whole matrix. Replaces the construction of CLIPPER's members
 * M_, C_ (clipper.h:155-156). `storage` is CLIPPER_HIP_STORE_F32 / _F64. */
clipper_hip_t* clipper_hip_create(int device, int storage);

/* In-process column sharding: `nshards` slices driven by one host thread; devices[p] may
 * repeat (several logical shards on one GPU — used to test the sharded protocol on a
 * 1-GPU box). Slices exchange their (M_off*x, C_off*x) pieces by device-to-device copies. */
clipper_hip_t* clipper_hip_create_group(const int* devices, int nshards, int storage);

/* Multi-process column sharding, one process per GPU: this context is shard `rank` of
 * `world`. The per-pass exchange is an RCCL all-gather over xGMI; call
 * clipper_hip_comm_init before the first solve. */
clipper_hip_t* clipper_hip_create_rank(int device, int storage, int rank, int world);
/* ncclGetUniqueId into a 128-byte buffer (rank 0), to be broadcast by the launcher. */
int clipper_hip_comm_unique_id(void* id128);
/* ncclCommInitRank on this context's device with the broadcast id. */
int clipper_hip_comm_init(clipper_hip_t* h, const void* id128);
/* The same exchange through the CALLER instead of RCCL: once per pass the library hands `fn` this
 * rank's block (`bytes` bytes of host memory) and a buffer of world * bytes for the blocks of all
 * ranks, rank order (e.g. a torch.distributed / MPI all-gather). `fn` returns 0, or non-zero to
 * abort the solve with CLIPPER_HIP_E_COMM. Called from the thread that runs clipper_hip_solve.
 * One host round trip per pass: a portability and test back-end (it lets several processes share
 * ONE device), not a fast path. */
typedef int (*clipper_hip_allgather_fn)(void* user, const void* sendbuf, void* recvbuf, size_t bytes);
int clipper_hip_comm_init_callback(clipper_hip_t* h, clipper_hip_allgather_fn fn, void* user);

void clipper_hip_destroy(clipper_hip_t* h);
const char* clipper_hip_last_error(void);

/* ---- affinity build ----------------------------------------------------------------- */

/* CLIPPER::scorePairwiseConsistency (clipper.cpp:21-65) with the built-in
 * EuclideanDistance invariant (euclidean_distance.cpp:13-31, Params .h:22-27).
 * D1: d x n1, D2: d x n2 column-major fp64 host buffers; A: column-major m x 2 int32
 * host buffer, or NULL / m == 0 for the all-to-all hypothesis (utils.h:61-71).
 * Host buffers are only read during the call. */
int clipper_hip_affinity_euclidean(clipper_hip_t* h, const double* D1, int d, int64_t n1,
                                   const double* D2, int64_t n2, const int32_t* A, int64_t m,
                                   double sigma, double epsilon, double mindist,
                                   double affinityeps);

/* Same with PointNormalDistance (pointnormal_distance.cpp:13-35, Params .h:25-31); d == 6. */
int clipper_hip_affinity_pointnormal(clipper_hip_t* h, const double* D1, int d, int64_t n1,
                                     const double* D2, int64_t n2, const int32_t* A, int64_t m,
                                     double sigp, double epsp, double sign, double epsn,
                                     double affinityeps);

/* The same work split at the PCIe boundary, so a caller (and bench.py) can keep the inputs
 * resident in HBM and time the device work alone:
 *   clipper_hip_stage_inputs   = clipper.cpp:24-25 (A or all-to-all) + H2D of D1, D2, A +
 *                                gather of the per-association point tables
 *   clipper_hip_affinity_*_staged = the pair loop clipper.cpp:31-56 + :61-64 on device.
 * clipper_hip_affinity_euclidean(...) == stage_inputs(...) then ..._euclidean_staged(...). */
int clipper_hip_stage_inputs(clipper_hip_t* h, const double* D1, int d, int64_t n1,
                             const double* D2, int64_t n2, const int32_t* A, int64_t m);
int clipper_hip_affinity_euclidean_staged(clipper_hip_t* h, double sigma, double epsilon,
                                          double mindist, double affinityeps);
int clipper_hip_affinity_pointnormal_staged(clipper_hip_t* h, double sigp, double epsp,
                                            double sign, double epsn, double affinityeps);

/* ---- user-defined invariants ------------------------------------------- */

/* A PairwiseInvariant written as HIP device source and compiled at run time (hiprtc, gfx950).
 * The source defines
 *   __device__ double clipper_invariant(const double* ai, const double* aj,
 *                                       const double* bi, const double* bj,
 *                                       const double* params);
 * ai, aj, bi, bj point to CLIPPER_D doubles each (the library defines `constexpr int CLIPPER_D = d;`
 * before the source); params to the up to CLIPPER_HIP_INVARIANT_MAX_PARAMS doubles of the fill.
 * Helper functions and the math of <hip/hip_runtime.h> may be used. The matrix is the host loop's
 * (clipper.cpp:31-64) for the same function: it is called for i < j with ai = D1[:, A(i,0)],
 * aj = D1[:, A(j,0)], bi = D2[:, A(i,1)], bj = D2[:, A(j,1)], never for two associations that share
 * an index; a score is kept only if score > affinityeps (NaN is not); M is symmetric, C = pattern(M). */
#define CLIPPER_HIP_INVARIANT_MAX_D 32
#define CLIPPER_HIP_INVARIANT_MAX_PARAMS 16
typedef struct clipper_hip_invariant clipper_hip_invariant_t;

/* Compiles `source` for datum dimension d (1 <= d <= CLIPPER_HIP_INVARIANT_MAX_D); needs no device.
 * A compile error returns CLIPPER_HIP_E_INVALID with the compiler's log (line numbers relative to
 * `source`, file name "invariant") in clipper_hip_last_error(); a library without libhiprtc returns
 * CLIPPER_HIP_E_SCOPE. The handle keeps the code object and loads it on a device at its first fill
 * there; it may serve any number of contexts (not concurrently with its own destruction). */
int clipper_hip_invariant_create(const char* source, int d, clipper_hip_invariant_t** out);
int clipper_hip_invariant_destroy(clipper_hip_invariant_t* inv);

/* The pair loop of clipper.cpp:31-56 + :61-64 with the compiled invariant over the staged inputs
 * (their d must be the invariant's: CLIPPER_HIP_E_INVALID otherwise). params: nparams doubles
 * (0 <= nparams <= CLIPPER_HIP_INVARIANT_MAX_PARAMS; the rest of the block reads 0), passed at fill
 * time, so that changing them compiles nothing. */
int clipper_hip_affinity_custom_staged(clipper_hip_t* h, const clipper_hip_invariant_t* inv,
                                       const double* params, int nparams, double affinityeps);
/* = clipper_hip_stage_inputs(...) then clipper_hip_affinity_custom_staged(...) */
int clipper_hip_affinity_custom(clipper_hip_t* h, const clipper_hip_invariant_t* inv, const double* D1, int d,
                                int64_t n1, const double* D2, int64_t n2, const int32_t* A, int64_t m,
                                const double* params, int nparams, double affinityeps);

/* rows of A_ (= dimension of M_); CLIPPER::getInitialAssociations (clipper.cpp:117-120) */
int64_t clipper_hip_num_associations(const clipper_hip_t* h);
int clipper_hip_get_associations(const clipper_hip_t* h, int32_t* A_out /* col-major m x 2 */);

/* ---- matrix get / set ---------------------------------------------------------------- */

/* CLIPPER::setMatrixData (clipper.cpp:149-158): dense column-major m x m host matrices;
 * only the strict upper triangle is used. Keeps the current association list if its
 * length is m (so getSelectedAssociations keeps working), else clears it. */
int clipper_hip_set_matrix(clipper_hip_t* h, const double* M, const double* C, int64_t m);

/* CLIPPER::setSparseMatrixData (clipper.cpp:162-166): CSC, int64 column pointers, int32 row
 * indices. The reference reads the upper triangle of what it is given (selfadjointView<Upper>,
 * clipper.cpp:194-271) and so does this: an entry (i, j) with i < j stands for the symmetric pair,
 * entries below the diagonal are NOT read (a full symmetric matrix counts through its upper half; a
 * lower-triangular one is an empty matrix, as in the reference). The same (row, column) stored twice
 * is an error with the compressed storage. The diagonal is implicit in this library: a stored
 * non-zero diagonal entry (outside the reference's contract, clipper.h:137-138; it would count once
 * on top of the identity there) is refused with CLIPPER_HIP_E_INVALID; explicit zeros are dropped.
 * When entries below the diagonal were ignored the call still returns 0 and clipper_hip_last_error() holds a
 * warning that says how many (a caller that stored both triangles, or only the lower one, can tell).
 * Values (both setters): a non-finite value above the diagonal of M or C, and with an fp32 storage a finite value of M
 * whose float cast is infinite, is refused with CLIPPER_HIP_E_INVALID naming the matrix and the entry (i, j); the matrix
 * held stays intact. A non-zero value that underflows in fp32 is held as FLT_MIN with its sign: C == pattern(M). */
int clipper_hip_set_sparse(clipper_hip_t* h, int64_t m, const int64_t* Mcolptr,
                           const int32_t* Mrow, const double* Mval, const int64_t* Ccolptr,
                           const int32_t* Crow, const double* Cval);

/* CLIPPER::getAffinityMatrix / getConstraintMatrix (clipper.cpp:131-145): dense symmetric
 * fp64 with the identity added. Either pointer may be NULL. Moves 8*m^2 bytes per matrix
 * over PCIe: for tests and interoperability, not for the hot loop. */
int clipper_hip_get_matrix(clipper_hip_t* h, double* M_out, double* C_out);

/* ---- solver -------------------------------------------------------------------------- */

/* CLIPPER::solve -> findDenseClique (clipper.cpp:69-78, 172-323). u0: m doubles (host),
 * required (the facade supplies utils::randvec when the caller gives none). u_out (m
 * doubles) may be NULL. Rounding is done on the host: NONZERO and DSD_HEU with the reference's
 * exact tie-breaking (utils.cpp:33-68); DSD (exact densest subgraph of the graph induced by
 * nnz(u), dsd.cpp:171-320, Goldberg's flow algorithm) gathers that sub-matrix from the device
 * first — on a multi-process shard it returns CLIPPER_HIP_E_SCOPE. */
int clipper_hip_solve(clipper_hip_t* h, const double* u0, const clipper_params_t* params,
                      double* u_out, clipper_solve_info_t* info);

/* Split form: clipper_hip_stage_u0 copies u0 to HBM; clipper_hip_solve_staged runs
 * findDenseClique on it (device loop + D2H of u + host rounding).
 * clipper_hip_solve(u0, ...) == stage_u0(u0) then solve_staged(...). */
int clipper_hip_stage_u0(clipper_hip_t* h, const double* u0);
int clipper_hip_solve_staged(clipper_hip_t* h, const clipper_params_t* params, double* u_out,
                             clipper_solve_info_t* info);

/* Solution::nodes (clipper.h:69); returns the count or <0. */
int clipper_hip_get_nodes(const clipper_hip_t* h, int32_t* nodes_out, int32_t capacity);
/* CLIPPER::getSelectedAssociations (clipper.cpp:124-127): column-major k x 2. */
int clipper_hip_get_selected_associations(const clipper_hip_t* h, int32_t* A_out,
                                          int32_t capacity);

/* dsd::solve(M_, S) (dsd.cpp:274-320, the reference's `clipper::dsd::solve`): exact densest
 * subgraph (Goldberg) of the current affinity matrix, restricted to the k nodes S (NULL / k <= 0:
 * all nodes). The induced sub-matrix is gathered from the device, the flow algorithm runs on the
 * host. Returns the number of nodes written to nodes_out (ascending) or <0. */
int clipper_hip_densest_subgraph(clipper_hip_t* h, const int32_t* S, int32_t k,
                                 int32_t* nodes_out, int32_t capacity);

/* ---- maximum clique of the consistency graph (maxclique::solve, maxclique.cpp:23-150) ------------------ */

/* The graph: vertices 0..m-1, edge (i, j), i != j, exactly when C(i, j) != 0 — the pattern of M for a scored
 * problem, the stored C after set_matrix / set_sparse with an explicit C; every storage gives the same graph.
 * Methods (= maxclique::Method, maxclique.h:15-19):
 *   EXACT  (ROBIN*) a maximum clique; the same list on every call, storage and launch geometry.
 *          HEU's clique when its size reaches the core bound K + 1.
 *   HEU    the greedy clique of DESIGN.md 9: every vertex seeds one (largest core number first), the largest wins
 *          (ties: the smallest seed).
 *   KCORE  (ROBIN) every vertex whose core number is the maximum K (an edgeless graph: all of them).
 * EXACT and HEU return no vertex on an edgeless graph (maxclique.cpp:114-118). The clique (ascending) becomes the
 * context's node list (clipper_hip_get_nodes, clipper_hip_get_selected_associations); nothing the solver keeps is
 * touched. time_limit_s > 0 bounds HEU's and EXACT's launches (checked between launches, each of which is a
 * bounded amount of work): when it runs out the best clique so far is returned and info->timed_out = 1; <= 0: no
 * limit. One-shard contexts only: column shards return CLIPPER_HIP_E_SCOPE. The adjacency bitsets take m^2 / 8
 * bytes of device memory for the call (CLIPPER_HIP_E_NOMEM when they do not fit). */
enum { CLIPPER_HIP_MC_EXACT = 0, CLIPPER_HIP_MC_HEU = 1, CLIPPER_HIP_MC_KCORE = 2 }; /* = maxclique::Method */
typedef struct clipper_maxclique_info_t {
  int32_t num_nodes;       /* vertices of the returned list                                               */
  int32_t max_core;        /* K                                                                            */
  int32_t heuristic_size;  /* HEU's clique (EXACT, HEU; 0 for KCORE / an edgeless graph)                    */
  int32_t timed_out;       /* 1: the time limit stopped the search                                         */
  int64_t edges;           /* undirected edges                                                             */
  int64_t roots_searched;  /* EXACT: roots whose branch and bound ran                                      */
  int64_t roots_pruned;    /* EXACT: roots their core number or neighbourhood size ruled out               */
  int64_t bb_nodes;        /* EXACT: branch-and-bound nodes (colourings)                                   */
  double seconds;          /* wall time of the call                                                        */
} clipper_maxclique_info_t;
int clipper_hip_max_clique(clipper_hip_t* h, int method, double time_limit_s, clipper_maxclique_info_t* info);
/* The seeded call (DESIGN.md 9 "Seeded calls"): clipper_hip_max_clique started from a clique the caller already has
 * good reason to believe in, such as the node list clipper_hip_solve left. seed: nseed distinct vertices in any order,
 * which need not form a clique (seed = NULL and nseed = -1: the context's node list); an index out of range or a
 * repeated one returns CLIPPER_HIP_E_INVALID naming its position, before any device work. The list is turned into a
 * maximal clique Q0 on the device: its vertices are taken by the number of neighbours they have in the list (ties:
 * smallest index) while they are adjacent to all taken so far, then the clique is extended over all vertices as HEU
 * extends one. HEU and EXACT start from Q0 as their incumbent: HEU returns its own clique only when it is larger than
 * Q0 (heuristic_size reports the larger size), EXACT a larger clique than both when there is one, and then the very
 * list clipper_hip_max_clique returns. The result is a function of the graph and of the list as a set. An empty list,
 * an edgeless graph and a Q0 of one (isolated) vertex give the unseeded call's result; KCORE ignores the list.
 * CLIPPER_HIP_MC_SEED_ONLY returns Q0 and runs neither HEU nor EXACT (no list or an edgeless graph: no vertex).
 * clipper_hip_max_clique and clipper_hip_batch_max_clique refuse that method. */
typedef struct clipper_maxclique_seed_info_t {
  int32_t seed_given;   /* distinct vertices handed in                    */
  int32_t seed_kept;    /* of them, in the seed clique                    */
  int32_t seed_size;    /* s = |Q0|                                       */
  int32_t winner;       /* 0: the search, 1: HEU's clique, 2: the seed clique */
} clipper_maxclique_seed_info_t;
enum { CLIPPER_HIP_MC_SEED_ONLY = 3 };  /* seeded entry points only: return Q0, run neither HEU nor EXACT */
int clipper_hip_max_clique_seeded(clipper_hip_t* h, int method, double time_limit_s, const int32_t* seed, int32_t nseed,
                                  clipper_maxclique_info_t* info, clipper_maxclique_seed_info_t* seed_info);
/* The core number of every vertex of the same graph (Batagelj-Zaversnik): m int32. */
int clipper_hip_core_numbers(clipper_hip_t* h, int32_t* core_out /* m */);

/* ---- the semidefinite relaxation (sdp::solve, sdp.cpp:109-303; CLIPPER::solveAsMSRCSDR, clipper.cpp:100-112) ---- */

/* maximize <M, X>  s.t.  tr X = 1, X psd, X_ij = 0 where C_ij = 0, X_ij >= 0 elsewhere; only the lower triangle of
 * M and C (diagonal included) is read and taken as symmetric. ADMM with a Jacobi eigensolver on the device, fp64,
 * one workgroup; by default n <= CLIPPER_HIP_SDP_MAX_N, larger problems return CLIPPER_HIP_E_SCOPE.
 * clipper_hip_sdp_set_route (below) opens n <= CLIPPER_HIP_SDP_WIDE_MAX_N through the wide route: the same
 * iteration, stopping rule and certificate for one problem at a time over the whole chip.
 * Stops when the primal residual ||X - Z||_F, the dual residual rho ||Z - Z_prev||_F and the gap between <M, X> and
 * the dual bound lambda_max(M - Y) are all within the Boyd tolerances of eps_abs / eps_rel, at max_iters, or when
 * time_limit_secs > 0 runs out (checked between launches). pobj / dobj follow SCS's sign (minimisation):
 * pobj = -<M, X>, dobj = -lambda_max(M - Y), a certified bound on the optimum in every outcome.
 * acceleration_interval, acceleration_lookback and eps_infeas are accepted and ignored (there is no Anderson
 * acceleration, and the problem is always feasible: e_i e_i^T with C(i, i) != 0; a C without a nonzero diagonal
 * entry is refused with CLIPPER_HIP_E_INVALID). */
#define CLIPPER_HIP_SDP_MAX_N 128       /* the workgroup route: the working matrix is one workgroup's LDS */
#define CLIPPER_HIP_SDP_WIDE_MAX_N 1024 /* the wide route: the working matrix is in device memory        */
enum { CLIPPER_HIP_SDP_ROUTE_WORKGROUP = 0,   /* default: n <= CLIPPER_HIP_SDP_MAX_N, one workgroup per problem           */
       CLIPPER_HIP_SDP_ROUTE_AUTO      = 1,   /* workgroup route for n <= 128, wide route up to CLIPPER_HIP_SDP_WIDE_MAX_N */
       CLIPPER_HIP_SDP_ROUTE_WIDE      = 2 }; /* wide route at every n <= CLIPPER_HIP_SDP_WIDE_MAX_N (tests and probes)   */
/* The route of clipper_hip_sdp, clipper_hip_sdp_solve, clipper_hip_sdp_solve_batch and clipper_hip_batch_sdp: one
 * process-wide atomic setting, read once at the start of a call. Under AUTO or WIDE the scope limit of those calls is
 * CLIPPER_HIP_SDP_WIDE_MAX_N. set_route returns the previous setting, or CLIPPER_HIP_E_INVALID for an unknown route
 * (the setting is then unchanged). The wide route needs 8 (5 n^2 + 5 np^2) bytes of device memory and a little more
 * (80 MB at n = 1024, np = n rounded up to even); CLIPPER_HIP_E_NOMEM when they are not free. Two calls on the same
 * input under the same setting give the same bits; the two routes agree to rounding, not bit for bit. */
int clipper_hip_sdp_set_route(int route);
int clipper_hip_sdp_route(void);
typedef struct clipper_sdp_params_t { /* = sdp::Params (sdp.h:40-52) */
  int32_t verbose;
  int32_t max_iters;               /* >= 1 */
  int32_t acceleration_interval;   /* ignored */
  int32_t acceleration_lookback;   /* ignored */
  float eps_abs;
  float eps_rel;
  float eps_infeas;                /* ignored */
  float time_limit_secs;           /* <= 0: none */
} clipper_sdp_params_t;
typedef struct clipper_sdp_info_t {
  int32_t iters;        /* ADMM iterations                                                          */
  int32_t converged;    /* 1: all three tolerances met                                               */
  int32_t timed_out;    /* 1: time_limit_secs stopped the iteration                                  */
  int32_t num_nodes;    /* rounded selection: |evec1_i| > thr                                        */
  int32_t sweeps;       /* Jacobi sweeps, all projections and certificates together                  */
  int32_t route;        /* the route this problem took: CLIPPER_HIP_SDP_ROUTE_WORKGROUP or _WIDE     */
  double pobj;          /* -<M, X>                                                                   */
  double dobj;          /* -lambda_max(M - Y)                                                        */
  double r_prim;        /* ||X - Z||_F                                                               */
  double r_dual;        /* rho ||Z - Z_prev||_F                                                      */
  double rho;           /* the final penalty                                                         */
  double thr;           /* max |evec1| / 2                                                           */
  double t_total;       /* seconds: the whole call                                                   */
  double t_setup;       /* seconds: gather / upload and initialisation                               */
  double t_solve;       /* seconds: the iteration and the final certificate                          */
  double t_extract;     /* seconds: the rounding and the copies out                                  */
} clipper_sdp_info_t;
/* On the context's M and C (each with its identity diagonal: what getAffinityMatrix / getConstraintMatrix return),
 * read from whichever device store holds them. The selected nodes (ascending) become the context's node list.
 * Optional outputs (NULL allowed), m = the context's size: X and Y (m x m), lambdas (m, ascending: the eigenvalues
 * of X), evec1 (m: the eigenvector of the largest, its largest-magnitude entry positive). One-shard contexts only:
 * column shards and multi-process contexts return CLIPPER_HIP_E_SCOPE. */
int clipper_hip_sdp(clipper_hip_t* h, const clipper_sdp_params_t* params, double* X_out, double* Y_out,
                    double* lambdas_out, double* evec1_out, clipper_sdp_info_t* info);
/* Stand-alone: M and C column-major n x n (host), lower triangles read. nodes_out (capacity n, may be NULL)
 * receives the selection; returns its size or <0. Other outputs as clipper_hip_sdp. A NaN or an infinity in the
 * lower triangle of M or C is refused with CLIPPER_HIP_E_INVALID before the device is touched, its row and column in
 * the message. */
int clipper_hip_sdp_solve(int device, const double* M, const double* C, int64_t n, const clipper_sdp_params_t* params,
                          double* X_out, double* Y_out, double* lambdas_out, double* evec1_out, int32_t* nodes_out,
                          clipper_sdp_info_t* info);
/* Many relaxations in one call, one workgroup per problem ("Batches"): the problems run side by side
 * on the chip in launches over the list of those still iterating. The problems that take the wide route (under
 * CLIPPER_HIP_SDP_ROUTE_AUTO those above CLIPPER_HIP_SDP_MAX_N, under _WIDE all) run after them, one after another on
 * the same stream, each with the chip to itself. Per problem every output and every field of its
 * info but the times is bit for bit what clipper_hip_sdp_solve returns for it alone with the same params and the same
 * route setting, whatever else the batch holds and wherever the problem stands in it. M and C: host, column-major n x n, lower triangles
 * read. Outputs optional (NULL allowed) as in clipper_hip_sdp_solve; nodes_out has capacity n and receives
 * infos[i].num_nodes nodes. Only evec1, the eigenvalues, the nodes and the control records come back from the device
 * unless a problem asks for X or Y.
 * The whole call is refused on the first bad problem, its index in the message, before anything touches the device:
 * count < 0, a NULL M or C, n < 1, a non-finite value in a lower triangle -> CLIPPER_HIP_E_INVALID; n above the route setting's limit (CLIPPER_HIP_SDP_MAX_N by
 * default) -> CLIPPER_HIP_E_SCOPE; params
 * as clipper_hip_sdp_solve. count == 0 succeeds and does nothing. A C without a nonzero diagonal entry fails the call
 * with CLIPPER_HIP_E_INVALID. time_limit_secs > 0 bounds the whole call (checked between rounds of launches): every
 * problem still iterating then reports timed_out = 1 and a certified dobj. t_total / t_setup / t_solve / t_extract of
 * every info are the call's. infos (count records) may be NULL. Returns 0 or <0. */
typedef struct clipper_sdp_problem_t {
  const double* M;
  const double* C;
  int64_t n;
  double* X_out;        /* n x n */
  double* Y_out;        /* n x n */
  double* lambdas_out;  /* n, ascending */
  double* evec1_out;    /* n */
  int32_t* nodes_out;   /* capacity n */
} clipper_sdp_problem_t;
int clipper_hip_sdp_solve_batch(int device, const clipper_sdp_problem_t* problems, int32_t count,
                                const clipper_sdp_params_t* params, clipper_sdp_info_t* infos);

/* ---- before the path: putative associations ------------------------------------------------ */

/* k nearest neighbours in P1 of every point of P0 (both d x n column-major as `clipper::Data`:
 * each point contiguous; d = 2 | 3; knn <= 16), squared L2 distances ascending, brute force on
 * the device — what the nanoflann kd-tree queries of benchmarks/bm_utils.cpp:147-176 return.
 * idx_out / sqd_out (may be NULL): n0 x knn row-major; -1 / 1e300 where P1 has fewer points.
 * Among exactly equal distances the lower index comes first. Stand-alone: needs no context. */
int clipper_hip_knn(int device, const double* P0, int64_t n0, const double* P1, int64_t n1, int d,
                    int knn, int32_t* idx_out, double* sqd_out);

/* The route of the d = 3 nearest-neighbour search behind clipper_hip_knn, clipper_hip_distance_based_correspondences,
 * clipper_hip_estimate_normals, clipper_hip_compute_fpfh and clipper_hip_fpfh_from_points ("The grid
 * route of the search"): one process-wide atomic setting, read once at the start of a search. The grid route bins the
 * searched cloud into a uniform grid on the device and visits rings of cells around each query; every list it returns
 * equals the brute-force route's entry for entry and bit for bit, for every finite input, so the setting changes the
 * time of a call and nothing else. d = 2 searches run brute force in every mode; clipper_hip_match_descriptors is not
 * concerned. set_search returns the previous mode, or CLIPPER_HIP_E_INVALID for an unknown one (the setting is then
 * unchanged); neither function needs a device. The grid route reports a device allocation failure as
 * CLIPPER_HIP_E_NOMEM. */
enum { CLIPPER_HIP_KNN_BRUTE = 0,   /* default: n0 * n1 distance evaluations                                    */
       CLIPPER_HIP_KNN_GRID  = 1,   /* the uniform grid wherever d == 3                                         */
       CLIPPER_HIP_KNN_AUTO  = 2 }; /* the grid when d == 3 and n1 >= CLIPPER_HIP_KNN_AUTO_MIN_N, else brute force */
#define CLIPPER_HIP_KNN_AUTO_MIN_N 24000 /* the smallest measured n1 at which the grid route is faster */
int clipper_hip_knn_set_search(int mode);
int clipper_hip_knn_search(void);
/* The calling thread's last search: the route it took, the grid's cells per axis, the number of queries and the
 * candidates visited, summed over the queries (all 0 but the route and the queries for brute force). route is -1
 * before the thread's first search. auto_min_n is CLIPPER_HIP_KNN_AUTO_MIN_N as the library was built. kernels_ms is
 * the device time between two events around the search's kernels (the grid route's includes the host's wait for the
 * bounding box in their middle); it is read when this function is called, after the searching call has returned. */
typedef struct clipper_hip_knn_stats_t {
  int32_t route;       /* CLIPPER_HIP_KNN_BRUTE or CLIPPER_HIP_KNN_GRID */
  int32_t dim[3];      /* cells along x, y, z                           */
  int64_t queries;     /* n0                                            */
  int64_t candidates;  /* distance evaluations of the grid route        */
  int64_t auto_min_n;
  double kernels_ms;
} clipper_hip_knn_stats_t;
int clipper_hip_knn_last_search(clipper_hip_knn_stats_t* out);

/* utils::distance_based_correspondences (benchmarks/bm_utils.cpp:147-232): associations
 * (i, nn_k(i)) within `radius`, i ascending / neighbours by distance; with enforce_1to1 one row
 * per point of P1 (ascending) — its closest claimant. A_out: column-major n x 2 with n = the
 * return value (<0: error); capacity in rows (n0*knn always suffices). */
int64_t clipper_hip_distance_based_correspondences(int device, const double* P0, int64_t n0,
                                                   const double* P1, int64_t n1, int d, int knn,
                                                   double radius, int enforce_1to1,
                                                   int32_t* A_out, int64_t capacity);

/* Putative associations from FEATURE DESCRIPTORS (FPFH 33, FCGF / SpinNet / Predator 32 numbers per point): every
 * point of F0 is matched to its knn nearest descriptors of F1 by brute force on the device, with the same contract
 * as clipper_hip_knn (fp64 squared L2 distances added in coordinate order, ascending, the lower index first among
 * equal distances), for 1 <= d <= 64. Row (i, nn_k(i)), k < knn, is kept iff all of: nn_k(i) exists; max_sqdist <= 0
 * or sqd_k(i) <= max_sqdist; ratio <= 0 or F1 has a single point or sqd_0(i) < ratio^2 * sqd_1(i) (Lowe's test on
 * squared distances, strict); mutual == 0 or i is among the knn nearest descriptors of F0 to nn_k(i). */
typedef struct {
  int32_t knn;          /* 1..8 neighbours per point of F0 */
  int32_t mutual;       /* 0 | 1 */
  double  ratio;        /* 0 = off; else in (0, 1), needs knn == 1 */
  double  max_sqdist;   /* <= 0 = off */
} clipper_match_params_t;

/* F0: d x n0, F1: d x n1 column-major as `clipper::Data` (each descriptor contiguous); every value finite. A_out:
 * column-major n x 2 as `clipper::Association` with n = the return value (<0: error), i ascending then k ascending —
 * clipper_hip_stage_inputs takes it unchanged; capacity in rows (n0*knn always suffices). sqd_out (may be NULL): the
 * squared distance of each row. nn_idx_out / nn_sqd_out (may be NULL): the forward lists before the filters, n0 x knn
 * row-major, -1 / 1e300 where F1 has fewer points. Stand-alone: needs no context. */
int64_t clipper_hip_match_descriptors(int device, const double* F0, int64_t n0, const double* F1, int64_t n1, int d,
                                      const clipper_match_params_t* params,
                                      int32_t* A_out, double* sqd_out, int64_t capacity,
                                      int32_t* nn_idx_out, double* nn_sqd_out);

/* SURFACE NORMALS and FPFH DESCRIPTORS of a point cloud on the device: the two inputs at the front of the pipeline
 * (the normals for PointNormalDistance, the 33-number descriptors for the matcher above). The neighbourhood of point i of the
 * cloud P (3 x n column-major as `clipper::Data`) is the first knn entries of the list the nearest-neighbour search above
 * gives for i in P itself (fp64, ascending by (distance, index)): the point is in its own list, recognised by its
 * index. With radius > 0 only entries with sqd <= radius * radius are kept (the product evaluated once in fp64: a
 * point exactly on the radius is kept). cnt(i) is the number of kept entries. */
typedef struct {
  int32_t knn;       /* 3..32 entries of the list, the point itself included */
  int32_t reserved;
  double  radius;    /* <= 0 = off; finite */
} clipper_neighborhood_t;

/* N_out (3 x n): per point the unit eigenvector of the smallest eigenvalue of the two-pass centred covariance of its
 * kept neighbours (cyclic Jacobi in fp64); (0, 0, 1) where cnt < 3. Sign: towards `viewpoint` (3 doubles,
 * n . (v - p) >= 0), or with viewpoint NULL the component of largest magnitude positive. count_out (n, may be NULL):
 * cnt. Every coordinate must be finite. Stand-alone: needs no context. 0, or <0: error. */
int clipper_hip_estimate_normals(int device, const double* P, int64_t n, const clipper_neighborhood_t* nb,
                                 const double* viewpoint, double* N_out, int32_t* count_out);

/* Fast Point Feature Histograms (Rusu et al. 2009) from points and unit normals N (3 x n; squared length within
 * [0.99, 1.01]). F_out: 33 x n column-major (each descriptor contiguous: what the matcher above takes with
 * d = 33): three groups of 11 bins (theta, alpha, phi of the Darboux frame), SPFH(i) plus the SPFH of the kept
 * neighbours weighted by 1 / sqd in list order, each group of the weighted part scaled to 100. spfh_out (33 x n, may
 * be NULL): SPFH, integer counts times 100 / (cnt - 1). count_out (n, may be NULL): cnt. The contract in full:
 * DESIGN.md section 9. */
int clipper_hip_compute_fpfh(int device, const double* P, const double* N, int64_t n, const clipper_neighborhood_t* nb,
                             double* F_out, double* spfh_out, int32_t* count_out);

/* Both stages in one call: one upload, one search at the larger knn, the normals stay on the device. F_out and N_out
 * (3 x n, may be NULL) equal those of the two calls above bit for bit. */
int clipper_hip_fpfh_from_points(int device, const double* P, int64_t n, const clipper_neighborhood_t* normal_nb,
                                 const double* viewpoint, const clipper_neighborhood_t* feature_nb,
                                 double* F_out, double* N_out);

/* ICP: the LOCAL REFINEMENT of a registration on the device, and how good an alignment is. The source cloud P_src
 * (3 x n_src column-major as `clipper::Data`) is moved by T (column-major 4 x 4) onto the target P_tgt (3 x n_tgt);
 * the correspondence of a moved point q is the K = 1 entry of the nearest-neighbour search above in the target (fp64,
 * ties by (distance, index); the route of clipper_hip_knn_set_search, with the target's grid built once per call and
 * kept over the iterations); it is an inlier iff sqd <= max_distance * max_distance. fitness = inliers / n_src,
 * inlier_rmse = sqrt(sum sqd / inliers). Every sum has one fixed order of addition and nothing is fused, so the results
 * are functions of the inputs alone: the same on both search routes and from run to run (the rules in full:
 * clipper_amd/csrc/icp_rules.hpp). Stand-alone: needs no context. */
enum { CLIPPER_ICP_POINT_TO_POINT = 0,   /* Arun / Horn on the inliers                                            */
       CLIPPER_ICP_POINT_TO_PLANE = 1,   /* linearised (q - b) . n over the target's normals, Cayley rotation      */
       CLIPPER_ICP_GENERALIZED    = 2 }; /* plane-to-plane over per-point covariances: clipper_hip_icp_generalized */
enum { CLIPPER_ICP_CONVERGED      = 0,   /* fitness and rmse both changed by less than their bounds               */
       CLIPPER_ICP_MAX_ITERATIONS = 1,
       CLIPPER_ICP_TOO_FEW        = 2,   /* fewer than 3 (point-to-point, generalized) or 6 (point-to-plane) inliers */
       CLIPPER_ICP_DEGENERATE     = 3 }; /* the inliers do not determine the step (rank-deficient system)         */
typedef struct clipper_icp_params_t {
  int32_t method;          /* CLIPPER_ICP_POINT_TO_POINT | CLIPPER_ICP_POINT_TO_PLANE; clipper_hip_icp_generalized: CLIPPER_ICP_GENERALIZED */
  int32_t max_iterations;  /* 0..1000 (facades default to 30); 0 = evaluate only */
  double  max_distance;    /* positive and finite */
  double  rel_fitness;     /* >= 0 (facades default to 1e-6) */
  double  rel_rmse;        /* >= 0 (facades default to 1e-6) */
} clipper_icp_params_t;
typedef struct clipper_icp_info_t {
  int32_t iterations;   /* updates of T behind the last history row */
  int32_t status;       /* CLIPPER_ICP_* */
  int64_t count;        /* inliers, fitness and inlier_rmse under T_out */
  double  fitness;
  double  inlier_rmse;
  int32_t route;        /* CLIPPER_HIP_KNN_BRUTE or CLIPPER_HIP_KNN_GRID: the search route taken */
  int32_t dim[3];       /* cells per axis of the target's grid (0 0 0 for brute force) */
  int64_t candidates;   /* points visited by the grid's queries, summed over all iterations (0 for brute force) */
  double  device_ms;    /* between two events around the loop */
} clipper_icp_info_t;

/* N_tgt (3 x n_tgt unit normals; squared length within [0.99, 1.01]): NULL unless point-to-plane. T_init: NULL =
 * identity; finite, bottom row 0 0 0 1. Iteration k evaluates (count, fitness, rmse) under the current T, writes row k of
 * `history` (max_iterations + 1 rows of 3 doubles, may be NULL; rows never reached are 0) and stops CONVERGED when
 * k >= 1 and |fitness_k - fitness_(k-1)| < rel_fitness and |rmse_k - rmse_(k-1)| < rel_rmse, else TOO_FEW, else
 * MAX_ITERATIONS at k == max_iterations, else DEGENERATE when the step is undetermined; otherwise T <- dT T. T_out is
 * the T the last row was evaluated under. Every status returns 0 with a finite T_out; <0: error (bad arguments are
 * refused before any device work; CLIPPER_ICP_GENERALIZED is refused with the name of the call below). info may be NULL. */
int clipper_hip_icp(int device, const double* P_src, int64_t n_src, const double* P_tgt, const double* N_tgt,
                    int64_t n_tgt, const double* T_init, const clipper_icp_params_t* params, double* T_out,
                    clipper_icp_info_t* info, double* history);

/* GENERALIZED ICP (Segal et al.: the plane-to-plane metric) over per-point covariances: the correspondence, the inlier
 * test, the history, the stop rule and every status are clipper_hip_icp's; an inlier pair (q, b) with the covariances
 * C_a of its source point and C_b of its target point weighs its difference d = q - b by M = (C_b + R C_a R^T)^-1, R the
 * rotation of the current T, and the step solves J^T M J xi = -J^T M d for the rotation and shift of point-to-plane
 * (the order of every product: clipper_amd/csrc/icp_rules.hpp). C_src (6 x n_src) and C_tgt (6 x n_tgt): per point
 * xx, xy, xz, yy, yz, zz, contiguous per point, e.g. from clipper_hip_estimate_covariances; every entry finite and every
 * matrix positive definite (its three leading minors > 0 in fp64), else refused before any device work with the point
 * named. params->method must be CLIPPER_ICP_GENERALIZED. TOO_FEW: fewer than 3 inliers. A pair whose C_b + R C_a R^T
 * rounds to a singular matrix leaves a non-number in the sums, which ends the call DEGENERATE with the previous T. */
int clipper_hip_icp_generalized(int device, const double* P_src, const double* C_src, int64_t n_src, const double* P_tgt,
                                const double* C_tgt, int64_t n_tgt, const double* T_init, const clipper_icp_params_t* params,
                                double* T_out, clipper_icp_info_t* info, double* history);

/* ROBUST LOSSES AND TRIMMED ICP: clipper_hip_icp and clipper_hip_icp_generalized with a defence against bad pairs. Every
 * argument they share means what it means there. A pair within max_distance has the squared residual e: sqd
 * (point-to-point), ((q - b) . n)^2 (point-to-plane), d^T M d (generalized), and with k2 = scale * scale the weight
 *   NONE 1;  HUBER e <= k2 ? 1 : scale / sqrt(e);  CAUCHY 1 / (1 + e / k2);  TUKEY e < k2 ? (1 - e / k2)^2 : 0;
 *   GEMAN_MCCLURE (k2 / (k2 + e))^2
 * which multiplies every term the pair adds to the step's sums (point-to-point's centroids divide by the sum of the
 * weights). count, fitness, rmse, the history and the stop rule stay head counts and plain distances. TRIMMING
 * (trim < 1): each iteration, with `within` the points within max_distance, keep = (int64_t)(trim * (double)within) and
 * tau the keep-th smallest sqd among them (an exact rank select on the device), a point is kept iff it is within
 * max_distance and sqd <= tau: every point equal to tau is kept; keep == 0 keeps nothing and the call ends TOO_FEW.
 * count, fitness, rmse and the history are then over the kept points, and the loss acts on them alone. trim == 1
 * selects nothing. With NONE and trim 1 every bit returned equals the plain call's. A round whose weights are all zero
 * ends the call DEGENERATE with the previous T. TUKEY and GEMAN_MCCLURE redescend: a pair far beyond the scale weighs
 * (next to) nothing, so from a start far from the answer they may not converge where HUBER, CAUCHY and trimming do
 * (DESIGN.md section 9). The rules in full: clipper_amd/csrc/icp_rules.hpp. */
enum { CLIPPER_ICP_LOSS_NONE = 0, CLIPPER_ICP_LOSS_HUBER = 1, CLIPPER_ICP_LOSS_CAUCHY = 2, CLIPPER_ICP_LOSS_TUKEY = 3,
       CLIPPER_ICP_LOSS_GEMAN_MCCLURE = 4 };
typedef struct clipper_icp_robust_t {
  int32_t loss;      /* CLIPPER_ICP_LOSS_* */
  int32_t reserved;  /* 0 */
  double  scale;     /* of the residual (a distance), positive and finite; not read with CLIPPER_ICP_LOSS_NONE */
  double  trim;      /* in (0, 1]; 1 = no trimming */
} clipper_icp_robust_t;
typedef struct clipper_icp_robust_info_t { /* of the last history row */
  int64_t within;      /* points within max_distance, before trimming */
  double  weight_sum;  /* the sum of the weights of the kept pairs: point-to-point alone (the other two layouts do not
                          carry it): 0 for point-to-plane and generalized */
  double  trim_sqd;    /* tau; max_distance^2 with trim == 1, 0 when nothing was kept */
} clipper_icp_robust_info_t;

/* robust: never NULL; loss outside 0..4, reserved != 0, a scale that is not positive and finite with a loss, and a trim
 * outside (0, 1] are refused before any device work, the value named. robust_info may be NULL. */
int clipper_hip_icp_robust(int device, const double* P_src, int64_t n_src, const double* P_tgt, const double* N_tgt,
                           int64_t n_tgt, const double* T_init, const clipper_icp_params_t* params,
                           const clipper_icp_robust_t* robust, double* T_out, clipper_icp_info_t* info,
                           clipper_icp_robust_info_t* robust_info, double* history);
int clipper_hip_icp_generalized_robust(int device, const double* P_src, const double* C_src, int64_t n_src,
                                       const double* P_tgt, const double* C_tgt, int64_t n_tgt, const double* T_init,
                                       const clipper_icp_params_t* params, const clipper_icp_robust_t* robust, double* T_out,
                                       clipper_icp_info_t* info, clipper_icp_robust_info_t* robust_info, double* history);

/* The covariances clipper_hip_icp_generalized takes: C_out (6 x n), per point of the cloud P (3 x n) the matrix
 * I - (1 - epsilon) nv nv^T (eigenvalues epsilon, 1, 1) as xx, xy, xz, yy, yz, zz, nv being the unit eigenvector of the
 * smallest eigenvalue of the covariance of the point's neighbourhood: clipper_hip_estimate_normals' neighbourhood and
 * eigenvector, without its sign rule (the sign cancels). The identity where cnt < 3. epsilon in (0, 1] (facades
 * default to 1e-3). count_out (n, may be NULL): cnt. Stand-alone: needs no context. 0, or <0: error. */
int clipper_hip_estimate_covariances(int device, const double* P, int64_t n, const clipper_neighborhood_t* nb, double epsilon,
                                     double* C_out, int32_t* count_out);

/* fitness, inlier_rmse and count of the alignment T (NULL = identity), as iteration 0 of clipper_hip_icp computes them
 * (any of the three may be NULL). corr_out (n_src, may be NULL): the target index of each source point's
 * correspondence, -1 where it is no inlier. */
int clipper_hip_evaluate_registration(int device, const double* P_src, int64_t n_src, const double* P_tgt, int64_t n_tgt,
                                      const double* T, double max_distance, double* fitness, double* inlier_rmse,
                                      int64_t* count, int32_t* corr_out);

/* RANSAC OVER PUTATIVE ASSOCIATIONS: a consensus estimate of the rigid transform with D2[:, A(k,1)] ~ T D1[:, A(k,0)]
 * from the m associations A (column-major m x 2), on the device. D1: 3 x n1, D2: 3 x n2, column-major. Hypothesis h
 * draws n_sample distinct associations by a counter-based integer draw (a function of seed, h and the attempt alone),
 * is dropped when an edge of its sample has zero length in either cloud or the squared lengths differ by more than
 * edge_similarity^2, is fitted as clipper_hip_estimate_rigid_transform fits, and scores the NUMBER of associations with
 * |T p - b|^2 <= max_distance^2; the best is the largest count, among equal counts the smallest h. Hypotheses run in
 * rounds of hypotheses_per_round; after a round the call stops CONVERGED when evaluated >=
 * clipper_hip_ransac_needed(best count, m, n_sample, confidence), MAX_HYPOTHESES when evaluated >= max_hypotheses,
 * NO_MODEL (T_out the identity) when the hypotheses run out with a best count below 3. The winner is polished up to
 * refine_iterations times by ICP's point-to-point step over its inliers, a step being kept while the count does not
 * fall. Every floating-point sum has one fixed order and nothing is fused, and the score is an integer: what the call
 * returns is a function of its inputs alone (the rules in full: clipper_amd/csrc/ransac_rules.hpp).
 * Stand-alone: needs no context. */
typedef struct clipper_ransac_params_t {
  double  max_distance;          /* positive and finite */
  double  edge_similarity;       /* [0, 1); facades default to 0.9 */
  double  confidence;            /* (0, 1); facades default to 0.999 */
  int64_t max_hypotheses;        /* 1 .. 2^31 - 1; facades default to 100000 */
  int32_t hypotheses_per_round;  /* 256 .. 65536, a multiple of 256; facades default to 4096 */
  int32_t n_sample;              /* 3 .. 8; facades default to 3 */
  int32_t refine_iterations;     /* 0 .. 10; facades default to 1 */
  int32_t reserved;              /* 0 */
  uint64_t seed;
} clipper_ransac_params_t;
enum { CLIPPER_RANSAC_CONVERGED = 0, CLIPPER_RANSAC_MAX_HYPOTHESES = 1, CLIPPER_RANSAC_NO_MODEL = 2 };
typedef struct clipper_ransac_info_t {
  int32_t status;           /* CLIPPER_RANSAC_* */
  int32_t refined;          /* accepted polish steps */
  int64_t evaluated;        /* hypotheses formed: a multiple of hypotheses_per_round */
  int64_t checked;          /* of those, the ones that passed both checks and were scored */
  int64_t best_hypothesis;  /* the winner's number (-1: NO_MODEL) */
  int64_t best_count;       /* its count, before the polish */
  int64_t count;            /* inliers, fitness = count / m and inlier_rmse = sqrt(sum sqd / count) under T_out */
  double  fitness;
  double  inlier_rmse;
  int32_t sample[8];        /* the winner's sample: rows of A, -1 past n_sample */
  double  device_ms;        /* between two events around the device work */
} clipper_ransac_info_t;

/* T_out: column-major 4 x 4. inlier_out (m flags, may be NULL): the associations within max_distance under T_out.
 * Refused (CLIPPER_HIP_E_INVALID, before any device work, the offending value named): a parameter outside its range,
 * m < n_sample, a row of A outside the clouds, a non-finite coordinate of a point that A refers to. */
int clipper_hip_ransac_correspondences(int device, const double* D1, int64_t n1, const double* D2, int64_t n2,
                                       const int32_t* A, int64_t m, const clipper_ransac_params_t* params,
                                       double* T_out, uint8_t* inlier_out, clipper_ransac_info_t* info);
/* The stop rule, host only: ceil(log(1 - confidence) / log(1 - (count / m)^n_sample)); 1 when (count / m)^n_sample >= 1,
 * INT64_MAX when 1 - (count / m)^n_sample rounds to 1. <0 (CLIPPER_HIP_E_INVALID): an argument out of range (count in
 * 0..m, m >= 1, n_sample in 3..8, confidence in (0, 1)). */
int64_t clipper_hip_ransac_needed(int64_t count, int64_t m, int32_t n_sample, double confidence);

/* VOXEL DOWN-SAMPLING: the step in front of the normals, on the device. The cloud P (3 x n column-major as
 * `clipper::Data`, n >= 0) is cut into cubes of edge voxel_size whose origin is the cloud's own minimum corner lo (the
 * exact per-axis minimum; not Open3D's min - voxel_size / 2): the voxel of x on axis a is floor((x_a - lo_a) * inv)
 * with inv = 1.0 / voxel_size, the cell number (v_z * dim_y + v_y) * dim_x + v_x. One output row per occupied voxel, in
 * ascending cell number (lexicographic in z, y, x): the centroid of the voxel's points and, with normals N (3 x n, may
 * be NULL; finite), the sum of their normals made a unit vector, (0, 0, 1) where they cancel. Every sum takes a
 * voxel's members in ascending original index, in chunks of 512 added up one after the other from +0.0 over
 * (x - lo), the chunk sums in chunk order, and nothing is fused or atomic: the result is a function of the inputs
 * alone, the same from run to run (the rules in full: clipper_amd/csrc/voxel_rules.hpp).
 * P_out, N_out (3 x n), count_out (n): room for n rows, the first *n_out are written (count_out: the members per
 * row); trace_out (n): for every input point its output row. Every output but n_out may be NULL; N_out needs N.
 * Refused (CLIPPER_HIP_E_INVALID, before any device work): a voxel_size that is not finite and > 0, a non-finite
 * coordinate or normal, more than 2^21 voxels along an axis, n >= 2^31. Stand-alone: needs no context. */
typedef struct clipper_voxel_info_t {
  int32_t dim[3];      /* voxels along x, y, z                                                     */
  int32_t passes;      /* 8-bit passes of the radix sort: ceil(bitlength(dim_x dim_y dim_z - 1) / 8) */
  int32_t sort_tile;   /* pairs per workgroup of a sort pass                                       */
  int32_t chunk;       /* 512                                                                      */
  int32_t max_count;   /* the members of the fullest voxel                                         */
  int32_t reserved;
  double  kernels_ms;  /* between two events around the kernels                                    */
  double  sort_ms;     /* of that, between two events around the passes of the sort (0 without one) */
} clipper_voxel_info_t;
int clipper_hip_voxel_downsample(int device, const double* P, const double* N, int64_t n, double voxel_size,
                                 double* P_out, double* N_out, int32_t* count_out, int32_t* trace_out, int64_t* n_out,
                                 clipper_voxel_info_t* info);

/* CLOUDS ON THE DEVICE: the front end from raw scan to refined transform without crossing the bus between its stages.
 * clipper_hip_cloud_t owns n points (3 x n fp64, n >= 0) on one device and what the stages below have computed about
 * it: unit normals, descriptors (any 1 <= d <= 64; FPFH has 33), SPFH, covariances, the neighbour counts of each stage,
 * the members and the trace of the voxel stage that made it, and, built at the first search AGAINST it and kept, the
 * search grid (CLIPPER_HIP_KNN_GRID route) or the bounding box (brute-force route). clipper_hip_pairs_t owns an
 * association list on the device: m x 2 int32 column-major as `clipper::Association`, one squared distance per row
 * where it came from the matcher.
 * Every stage on handles runs the same device code as its host-buffer call above on the same route
 * (clipper_hip_knn_set_search is read per call) and gives the same bits; only the copies and the host's filters are
 * gone. What comes from the host is checked where it enters (create, set_descriptors) with the checks of the
 * host-buffer calls, before any device work: finite coordinates, normals of squared length within [0.99, 1.01],
 * n < 2^31. A stage that needs an attachment the cloud does not have returns CLIPPER_HIP_E_STATE. Creators return 0 and
 * hand the handle out through their last pointer argument (NULL on failure); destroy takes NULL. All work runs on the
 * default stream, and every call has waited for it when it returns. A handle is NOT safe for concurrent mutation:
 * stages attach to it and searches build what it keeps; calls on one handle must not overlap.
 * Not built: RANSAC on handles, the all-to-all hypothesis from clouds (pairs with m = 0 are refused at staging),
 * column-sharded and multi-process contexts (CLIPPER_HIP_E_SCOPE), batches of clouds in one call, fp32 clouds, d = 2. */
typedef struct clipper_hip_cloud clipper_hip_cloud_t;
typedef struct clipper_hip_pairs clipper_hip_pairs_t;
enum { CLIPPER_HIP_CLOUD_POINTS = 0,            /* 3 x n double                                              */
       CLIPPER_HIP_CLOUD_NORMALS = 1,           /* 3 x n double                                              */
       CLIPPER_HIP_CLOUD_DESCRIPTORS = 2,       /* d x n double (FPFH: 33 x n)                               */
       CLIPPER_HIP_CLOUD_SPFH = 3,              /* 33 x n double                                             */
       CLIPPER_HIP_CLOUD_COVARIANCES = 4,       /* 6 x n double                                              */
       CLIPPER_HIP_CLOUD_NORMAL_COUNTS = 5,     /* n int32: cnt of estimate_normals                          */
       CLIPPER_HIP_CLOUD_FPFH_COUNTS = 6,       /* n int32: cnt of compute_fpfh                              */
       CLIPPER_HIP_CLOUD_COVARIANCE_COUNTS = 7, /* n int32: cnt of estimate_covariances                      */
       CLIPPER_HIP_CLOUD_VOXEL_COUNTS = 8,      /* n int32: the members of each voxel (a voxel-made cloud)   */
       CLIPPER_HIP_CLOUD_VOXEL_TRACE = 9 };     /* trace_n int32: the row of every point of the voxel stage's input */
typedef struct clipper_hip_cloud_info_t {
  int64_t n;
  int64_t trace_n;          /* entries of CLIPPER_HIP_CLOUD_VOXEL_TRACE (0: none)                 */
  int32_t device;
  int32_t has_normals;
  int32_t descriptor_dim;   /* 0: no descriptors                                                  */
  int32_t has_spfh;
  int32_t has_covariances;
  int32_t has_voxel_counts;
  int32_t grid_builds;      /* how often the search grid over this cloud was built: 0 or 1        */
  int32_t grid_dim[3];      /* its cells along x, y, z (0 before it is built)                     */
} clipper_hip_cloud_info_t;

/* P: 3 x n column-major as `clipper::Data` (may be NULL with n == 0); N: unit normals, 3 x n, or NULL. */
int clipper_hip_cloud_create(int device, const double* P, const double* N, int64_t n, clipper_hip_cloud_t** out);
void clipper_hip_cloud_destroy(clipper_hip_cloud_t* cloud);
int64_t clipper_hip_cloud_count(const clipper_hip_cloud_t* cloud);   /* n, or <0: error */
/* `what`: one of CLIPPER_HIP_CLOUD_*; `out`: room for what the enumerator's comment says. An attachment that was never
 * computed: CLIPPER_HIP_E_STATE. */
int clipper_hip_cloud_download(const clipper_hip_cloud_t* cloud, int what, void* out);
int clipper_hip_cloud_info(const clipper_hip_cloud_t* cloud, clipper_hip_cloud_info_t* out);
/* Descriptors from elsewhere (FCGF, SpinNet, Predator: a network's), F: d x n column-major, every value finite,
 * 1 <= d <= 64; they replace the cloud's descriptors. The rows are padded for the matcher on the device, once. */
int clipper_hip_cloud_set_descriptors(clipper_hip_cloud_t* cloud, const double* F, int d);

/* A: m x 2 column-major, no negative index (the ranges are checked against the clouds where the pairs are used);
 * sqd: m, or NULL (clipper_hip_pairs_download then takes no sqd_out). m >= 0. */
int clipper_hip_pairs_create(int device, const int32_t* A, const double* sqd, int64_t m, clipper_hip_pairs_t** out);
void clipper_hip_pairs_destroy(clipper_hip_pairs_t* pairs);
int64_t clipper_hip_pairs_count(const clipper_hip_pairs_t* pairs);   /* m, or <0: error */
int clipper_hip_pairs_has_sqd(const clipper_hip_pairs_t* pairs);     /* 1: one squared distance per row, 0: none; <0: error */
int clipper_hip_pairs_download(const clipper_hip_pairs_t* pairs, int32_t* A_out, double* sqd_out);

/* clipper_hip_voxel_downsample on a cloud: *out is a NEW cloud whose points are the centroids and, when `in` has
 * normals, whose normals are the normalised normal sums; the members per voxel (VOXEL_COUNTS) and, with want_trace,
 * the trace (VOXEL_TRACE) are attached to it. One host read in the middle (the number of rows). `in` is not const: a
 * cloud that a stage made gets its corners folded on the device at its first down-sampling, and keeps them. */
int clipper_hip_cloud_voxel_downsample(clipper_hip_cloud_t* in, double voxel_size, int want_trace,
                                       clipper_hip_cloud_t** out, clipper_voxel_info_t* info);
/* clipper_hip_estimate_normals / _compute_fpfh / _fpfh_from_points / _estimate_covariances on a cloud: the result is
 * attached to it (normals and NORMAL_COUNTS; descriptors, SPFH and FPFH_COUNTS; both; covariances and
 * COVARIANCE_COUNTS). compute_fpfh needs normals (CLIPPER_HIP_E_STATE). Every stage searches the cloud in itself anew
 * (the lists are not kept); on the grid route the search queries the cloud's kept grid, built at first use. */
int clipper_hip_cloud_estimate_normals(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* nb, const double* viewpoint);
int clipper_hip_cloud_compute_fpfh(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* nb);
int clipper_hip_cloud_fpfh_from_points(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* normal_nb,
                                       const double* viewpoint, const clipper_neighborhood_t* feature_nb);
int clipper_hip_cloud_estimate_covariances(clipper_hip_cloud_t* cloud, const clipper_neighborhood_t* nb, double epsilon);
/* clipper_hip_match_descriptors on two clouds' descriptors (the same d; CLIPPER_HIP_E_STATE without), with the filters
 * run on the device: *out holds the rows of the host-buffer call, row for row and bit for bit, i ascending then k
 * ascending, with their squared distances. nn_idx_out / nn_sqd_out (may be NULL): the forward lists, n0 x knn. */
int clipper_hip_cloud_match(const clipper_hip_cloud_t* c0, const clipper_hip_cloud_t* c1, const clipper_match_params_t* params,
                            clipper_hip_pairs_t** out, int32_t* nn_idx_out, double* nn_sqd_out);
/* clipper_hip_stage_inputs from device data: D1 / D2 are the clouds' points (d = 3) or, with_normals, each point
 * followed by its normal (d = 6, for the PointNormalDistance fill); A is `pairs` (m >= 1, every index within its
 * cloud). The point tables are gathered with device-to-device traffic only; the pairs come down once (the solver's
 * rounding reads A on the host). The _staged fills and solves then run unchanged. One-shard contexts on the clouds'
 * device only (CLIPPER_HIP_E_SCOPE / CLIPPER_HIP_E_INVALID). */
int clipper_hip_stage_inputs_clouds(clipper_hip_t* h, const clipper_hip_cloud_t* c0, const clipper_hip_cloud_t* c1,
                                    const clipper_hip_pairs_t* pairs, int with_normals);
/* The k points idx names (each within the cloud), in the order of the list, to `out` (3 x k): what
 * clipper_hip_estimate_rigid_transform fits. */
int clipper_hip_cloud_gather_points(const clipper_hip_cloud_t* cloud, const int32_t* idx, int64_t k, double* out);
/* clipper_hip_icp / _icp_generalized / _icp_robust / _icp_generalized_robust on two clouds: params->method picks
 * point-to-point, point-to-plane (needs the target's normals) or generalized (needs both clouds' covariances), else
 * CLIPPER_HIP_E_STATE; robust and robust_info may be NULL (the plain rounds). The target's grid (or, on the
 * brute-force route, its bounding box) is built at the first call against `tgt` and KEPT: a second ICP, evaluation or
 * grid-route stage search against the same cloud builds nothing (clipper_hip_cloud_info: grid_builds stays 1). */
int clipper_hip_cloud_icp(const clipper_hip_cloud_t* src, clipper_hip_cloud_t* tgt, const double* T_init,
                          const clipper_icp_params_t* params, const clipper_icp_robust_t* robust, double* T_out,
                          clipper_icp_info_t* info, clipper_icp_robust_info_t* robust_info, double* history);
int clipper_hip_cloud_evaluate_registration(const clipper_hip_cloud_t* src, clipper_hip_cloud_t* tgt, const double* T,
                                            double max_distance, double* fitness, double* inlier_rmse, int64_t* count,
                                            int32_t* corr_out);

/* Line-search window: how many consecutive step sizes alpha, alpha*beta, ... of the
 * backtracking line search (clipper.cpp:234-251) one pass over M evaluates at once. The
 * trial sequence, the accepted trial and the result are those of the reference for every
 * window; only the number of passes over M changes. 0 = automatic (6 for m >= 8500 on slices,
 * m >= 6000 on a dense store; 4 for m >= 2000; else 1);
 * 1, 4, 6 or 8 forces a size (also: environment CLIPPER_HIP_WINDOW). Takes effect at the next
 * affinity build / set_matrix. clipper_hip_window returns the size in use. */
int clipper_hip_set_window(clipper_hip_t* h, int window);
int clipper_hip_window(const clipper_hip_t* h);

/* The resident solver: when the slices of the current matrix fit the LDS of the workgroups that
 * share them (m up to a few thousand, one device, C == pattern(M), automatic window), the whole of
 * findDenseClique (clipper.cpp:172-323) runs as ONE launch that keeps M on chip; otherwise — and
 * always with mode 1, or CLIPPER_HIP_RESIDENT=0 in the environment — as the streaming launches
 * (decision + pass, tail) per iteration. Same trial sequence and result either way. Mode 1 takes
 * effect at the next solve; back to 0 at the next affinity build / set_matrix (the plan is made there).
 * clipper_hip_last_solver: what the last solve ran on, 0 = streaming launches, 1 = resident. */
int clipper_hip_set_resident(clipper_hip_t* h, int mode);
int clipper_hip_last_solver(const clipper_hip_t* h);

/* The row view. Row r of every line-search candidate max(u + alpha g, 0) (clipper.cpp:235-236) is
 * exactly zero unless u[r] > 0 or g[r] > 0, and such a row adds exact zeros to M x: once the
 * projected gradient ascent has driven most of u to zero (a few iterations on registration data)
 * a pass needs only the rows that are still live. With M in slices (C == pattern(M)) the solver then
 * builds the slices of M[live rows, :] — scored again from the staged points on the
 * scorePairwiseConsistency path with a built-in invariant, filtered out of M's own slices for a
 * matrix that was handed over (setMatrixData / setSparseMatrixData, custom invariants) — and
 * streams THOSE while the device-side check "no live row outside the view" holds; any pass for
 * which it does not hold streams M itself. Same trial sequence, same sums up to the
 * order of the partial sums. mode 0 = automatic, 1 = never (also: CLIPPER_HIP_ROW_VIEW=0).
 * A view small enough for the LDS of the chip (at most 1024 rows, a few MB: the headline problem's 524
 * rows x 10 000 columns) is not streamed at all: the iterations on it run as ONE launch of workgroups that
 * each keep complete columns of the view on chip, until the solve ends or a row outside the view becomes
 * live (csrc/k_rv_resident.hip.h); mode 2 (also: CLIPPER_HIP_VIEW_RESIDENT=0) keeps the views but streams them. */
int clipper_hip_set_row_view(clipper_hip_t* h, int mode);
int clipper_hip_get_view_stats(const clipper_hip_t* h, clipper_hip_view_stats_t* out);

/* The live sub-problem: once a row view exists and the penalty d is large, no association outside a small set S (the
 * view's rows and the few columns with many entries among them) can get a positive gradient again — by a bound on
 * clipper.cpp:238-241 that the decision checks for every candidate it plans — and the solve continues on the
 * associations of S as a problem of its own (csrc/k_subproblem.hip.h): the same launches on M[S,S]. Exact: what is left
 * out is provably zero. mode 0 = automatic (one shard, built-in invariants, m >= 12 000: smaller problems' views are taken
 * by the resident solver), 1 = never (also: CLIPPER_HIP_SUBPROBLEM=0), 2 = automatic, but M[S,S] always as slices (a
 * sub-problem that is mostly non-zero — the inlier block — is otherwise kept as a dense fp32 store; also
 * CLIPPER_HIP_SUB_DENSE=0). */
int clipper_hip_set_subproblem(clipper_hip_t* h, int mode);

/* The products of clipper_hip_matvec through a row view built for the given rows (ascending association
 * indices): yM = M_off[:, rows] x[rows], yC likewise — what a pass of the solver computes when it
 * streams the view. For tests of the view's storage and of the rectangular fill kernel that writes it. */
int clipper_hip_view_matvec(clipper_hip_t* h, const int32_t* rows, int64_t nrows, const double* x,
                            double* yM, double* yC);

/* How the current matrix is stored: CLIPPER_HIP_STORE_F32_CSC only while the compressed copy is
 * in use (one shard, C == pattern(M)); a context created with it otherwise reports _F32. */
int clipper_hip_storage_in_use(const clipper_hip_t* h);

/* One pass of the mat-vec kernel: yM = M_off*x, yC = C_off*x (the products at
 * clipper.cpp:194,202,205,219,240-241,268,271). x, yM, yC: m doubles on the host. */
int clipper_hip_matvec(clipper_hip_t* h, const double* x, double* yM, double* yC);

/* ---- measurement ---------------------------------------------------------------------- */

/* When on (1), sampled mat-vec launches of a solve are bracketed by HIP events on the stream they
 * run on; clipper_hip_get_timings then reports their mean / min duration. 2: also an event pair around
 * every launch of the resident solver on a row view (clipper_hip_view_stats_t::resident_event_us). */
int clipper_hip_set_profiling(clipper_hip_t* h, int on);
int clipper_hip_get_timings(const clipper_hip_t* h, clipper_hip_timings_t* out);
/* Launches the mat-vec kernel `reps` times back to back on resident data and returns the
 * mean kernel time in microseconds (events on the launch stream). */
int clipper_hip_bench_matvec(clipper_hip_t* h, int reps, double* avg_us);
/* Device name, CU count, HBM bytes (for bench.py's report). */
/* ---- host-side neighbours of the path (no device work) -----------------
 * utils::read_ply (benchmarks/bm_utils.cpp:24-79): x, y, z of the `vertex` element of an ascii or
 * binary PLY file -> pts_out, column-major 3 x n (one datum per column, as invariants::Data).
 * pts_out == NULL: returns the vertex count only. Returns n or a negative status. */
int64_t clipper_hip_read_ply_xyz(const char* path, double* pts_out, int64_t capacity);
/* utils::generate_synthetic_correspondences (bm_utils.cpp:277-341): m putative associations with
 * outlier ratio rho — ni = round(m (1 - rho)) inliers drawn without replacement from the p good
 * associations Agood (column-major p x 2), placed LAST; m - ni outliers sampled uniformly without
 * repetition from all n0 * n1 pairs that are not in Agood, placed FIRST. A_out: m x 2, Agt_out:
 * ni x 2 (capacity m x 2), both column-major; *ni_out = ni. The reference seeds a mt19937 from
 * random_device; here the seed is an argument (mt19937_64), so a call is reproducible.
 * CLIPPER_HIP_E_STATE when Agood holds fewer than ni associations (the reference returns {}). */
int clipper_hip_generate_synthetic_correspondences(int64_t n0, int64_t n1, const int32_t* Agood,
                                                   int64_t p, int64_t m, double rho, uint64_t seed,
                                                   int32_t* A_out, int32_t* Agt_out,
                                                   int64_t* ni_out);
/* utils::get_precision_recall (bm_utils.cpp:345-371): TP counted row by row of A (na x 2) against
 * the set of rows of Agt (ngt x 2); (0, 0) when either is empty. */
int clipper_hip_precision_recall(const int32_t* A, int64_t na, const int32_t* Agt, int64_t ngt,
                                 double* precision, double* recall);
/* Least-squares rigid transform T (column-major 4 x 4) with D2[:, A(i,1)] ~ R D1[:, A(i,0)] + t over
 * the k >= 3 associations A (column-major k x 2): centroids, 3 x 3 cross-covariance, SVD, reflection
 * fix (Arun / Horn) — the consumer of the selected associations in examples/python/ex4_bunny.ipynb.
 * D1: 3 x n1, D2: 3 x n2, column-major. */
int clipper_hip_estimate_rigid_transform(const double* D1, int64_t n1, const double* D2, int64_t n2,
                                         const int32_t* A, int64_t k, double* T_out);

/* Measurement only (context created with CLIPPER_HIP_STAMPS=1 in the environment): per workgroup of
 * the last pass launch {start, decision done, end, info} on the 100 MHz device wall clock. */
int clipper_hip_debug_stamps(clipper_hip_t* h, int64_t* out, int capacity);

/* Test infrastructure: occupies `workgroups` wave slots with `lds_bytes` of LDS each on `device` for `milliseconds`
 * (a kernel that sleeps) and returns when it is over — "another tenant on the device" for the tests of the resident
 * solvers' time-outs (tests/test_gpu_rv_resident.py runs it in a second process). */
int clipper_hip_debug_occupy(int device, int workgroups, int lds_bytes, double milliseconds);

/* Test infrastructure: the work budgets of the maximum-clique launches, process-wide (host_maxclique.hpp): a peel
 * launch ends after `peel_budget` row-word operations at a round's end, a HEU / EXACT wave after `wave_budget`, and the
 * host resumes either with the next launch. Values <= 0 restore the constants (2^24 and 2^18). A smaller budget cuts the
 * same work into more launches and changes no result: the tests run the resume paths with budgets of 1 and 64. */
int clipper_hip_debug_mc_budgets(long long peel_budget, long long wave_budget);
/* Test infrastructure: the kernel launches of the context's last lone maximum-clique call (clipper_hip_max_clique,
 * clipper_hip_max_clique_seeded, clipper_hip_core_numbers); 0 before the first. */
int clipper_hip_debug_mc_launches(const clipper_hip_t* h);

/* Test infrastructure: the selection of the live sub-problem (csrc/k_subproblem.hip.h) by itself. What a selection
 * leaves behind: cnt[c] = 4 x the quads column c holds in the slices of the row view (at least its stored entries among
 * the view's rows; 0 for m <= c < mp), n0 = min(floor((0.4 s) s), 2e9), S = the view's rows and every column with
 * cnt > n0 (flags[0, mp)), its ascending list colmap[0, nS), the inverse pos[0, mp) (-1 outside S), ncol = the largest
 * cnt outside S, entries = the sum of cnt over S. */
typedef struct {
  int64_t mp;       /* the padded length of cnt, flags and pos */
  int64_t nS;
  int64_t entries;
  int64_t nrows;    /* rows of the view */
  int32_t ncol;
  int32_t n0;
  double s;         /* sum(u) as the selection read it */
  /* clipper_hip_debug_sub_last alone (0 from clipper_hip_debug_sub_select): */
  double N_used;    /* N of the decision's bound, max(1, ncol) + (nS - nrows); 0 when no sub-problem was built */
  int32_t built;    /* a sub-problem was built from this selection */
  int32_t entered;  /* ... and the solve was handed over to it */
} clipper_hip_sub_selection_t;
/* On a context whose matrix lives in slices and was scored from staged points with a built-in invariant: builds the row
 * view of `rows` (ascending association indices, as clipper_hip_view_matvec does) and runs exactly the launches a solve
 * makes to select S, with sum(u) = s (finite, >= 0). cnt, flags and pos take `capacity` >= mp = m rounded up to 64
 * elements, colmap as well (nS of them are written); any of the four may be NULL. */
int clipper_hip_debug_sub_select(clipper_hip_t* h, const int32_t* rows, int64_t nrows, double s, int64_t capacity,
                                 int32_t* cnt, uint8_t* flags, int32_t* colmap, int32_t* pos,
                                 clipper_hip_sub_selection_t* out);
/* The last selection the last solve made (CLIPPER_HIP_E_STATE: it made none, or clipper_hip_debug_sub_select has
 * overwritten it since): the same lists and record, the view's rows at that moment (rows: `capacity` elements, out->nrows
 * written), the sum(u) the kernel read, N as handed to the decision, and whether the sub-problem was built and entered. */
int clipper_hip_debug_sub_last(clipper_hip_t* h, int64_t capacity, int32_t* cnt, uint8_t* flags, int32_t* colmap,
                               int32_t* pos, int32_t* rows, clipper_hip_sub_selection_t* out);
/* The size threshold of the live sub-problem (12 000, or CLIPPER_HIP_SUBPROBLEM_MIN_M as the process started),
 * process-wide: full problems below it are not handed over. A value <= 0 restores the initial one. */
int clipper_hip_debug_sub_min_m(long long min_m);

/* Test infrastructure: what this process's library holds right now, as its owning types count it
 * (csrc/host_buf.hpp): out[0] live device buffers, out[1] their bytes, out[2] live pinned host buffers, out[3] live
 * events, out[4] allocations and event creations made so far. Touches no device. */
int clipper_hip_debug_live_resources(int64_t out[5]);

int clipper_hip_device_info(const clipper_hip_t* h, char* name64, int* cus, int64_t* hbm_bytes);

/* ---- batched solves: many independent small problems in one call -----------------
 * A batch owns one child context per problem slot (kept and reused from call to call) on one device
 * and ONE stream. A call scores every problem (the fills queued back to back, one wait for all of
 * them), plans each problem exactly as a lone context would, runs every problem whose plan is resident
 * (m <= 2048 on the slice storages) side by side in a few launches of k_solve_resident_batch, and solves
 * the others — no resident plan, a dense storage, a launch that gave up or was refused — alone on their
 * child context afterwards. Per problem the results are bit for bit those of clipper_hip_solve on a lone
 * context of the same storage with the same inputs, u0 and params whenever both took the same route
 * (clipper_hip_batch_route(i) == clipper_hip_last_solver of the lone context); only
 * clipper_solve_info_t::seconds differs: it is the wall time of the whole batched call.
 * The invariant is a built-in one (EuclideanDistance, PointNormalDistance) or a user-defined one
 * (clipper_hip_batch_solve_custom: one launch of its batched fill kernel scores every problem).
 * Not a batch: explicit matrices (set_matrix / set_sparse), column shards, multi-process ranks. */
typedef struct clipper_hip_batch clipper_hip_batch_t;
typedef struct {                /* one problem; host buffers, read during the call only */
  const double* D1; int64_t n1;  /* d x n1 column-major */
  const double* D2; int64_t n2;  /* d x n2 column-major */
  const int32_t* A; int64_t m;   /* m x 2 column-major; NULL or m = 0: all-to-all (n1 * n2) */
  const double* u0;              /* m doubles (n1 * n2 when all-to-all), required */
} clipper_batch_problem_t;
/* storage: CLIPPER_HIP_STORE_* (the slice storages are the ones with a resident route). The batch is returned in
 * *out (a status like every other entry point: the handle type is not one the C ABI's guards return). */
int clipper_hip_batch_create(int device, int storage, clipper_hip_batch_t** out);
void clipper_hip_batch_destroy(clipper_hip_batch_t* b);
/* Invalid input in any problem (d, sizes, an association out of range, a missing u0) fails the whole
 * call with CLIPPER_HIP_E_INVALID before any device work; the message names the problem's index and the
 * batch stays usable. n = 0 is valid. The results of the previous call are dropped either way. */
int clipper_hip_batch_solve_euclidean(clipper_hip_batch_t* b, const clipper_batch_problem_t* p, int32_t n,
                                      int d, double sigma, double epsilon, double mindist, const clipper_params_t* prm);
/* PointNormalDistance: every D is 6 x n (xyz + unit normal). */
int clipper_hip_batch_solve_pointnormal(clipper_hip_batch_t* b, const clipper_batch_problem_t* p, int32_t n,
                                        double sigp, double epsp, double sign, double epsn, const clipper_params_t* prm);
/* A user-defined invariant (clipper_hip_invariant_create): every problem's D1, D2 are inv->d x n; params: nparams
 * doubles (0..CLIPPER_HIP_INVARIANT_MAX_PARAMS). Contract, checks and results as clipper_hip_batch_solve_euclidean's,
 * against a lone clipper_hip_affinity_custom + clipper_hip_solve. inv == NULL or nparams out of range is refused
 * before the batch is looked at. */
int clipper_hip_batch_solve_custom(clipper_hip_batch_t* b, const clipper_hip_invariant_t* inv,
                                   const clipper_batch_problem_t* p, int32_t n, const double* params, int nparams,
                                   const clipper_params_t* prm);
/* Problem i of the last call: u (its m doubles; may be NULL) and the solve info; returns m. */
int clipper_hip_batch_get_solution(const clipper_hip_batch_t* b, int32_t i, double* u_out, clipper_solve_info_t* info);
/* Its selected nodes (ascending as the rounding leaves them, as clipper_hip_get_nodes); returns their count. */
int clipper_hip_batch_get_nodes(const clipper_hip_batch_t* b, int32_t i, int32_t* nodes_out, int32_t capacity);
/* Its selected associations, column-major k x 2 (as clipper_hip_get_selected_associations); returns k. */
int clipper_hip_batch_get_selected_associations(const clipper_hip_batch_t* b, int32_t i, int32_t* A_out, int32_t capacity);
/* 1 = solved in a batched resident launch, 0 = solved alone on its child context. */
int clipper_hip_batch_route(const clipper_hip_batch_t* b, int32_t i);
/* The last call: launches of k_solve_resident_batch, problems solved batched, problems solved alone.
 * Any pointer may be NULL. */
int clipper_hip_batch_get_stats(const clipper_hip_batch_t* b, int32_t* launches, int32_t* n_batched, int32_t* n_alone);
/* The last call's host wall time split (ms): staging + fills + plans, the batched launches (queued to
 * finished), the problems solved alone, rounding. Any pointer may be NULL. */
int clipper_hip_batch_get_split(const clipper_hip_batch_t* b, double* fill_ms, double* launch_ms, double* alone_ms,
                                double* round_ms);
/* The semidefinite relaxation (clipper_hip_sdp) of every problem of the batch's last solve call, all in the launches
 * of one batched call (clipper_hip_sdp_solve_batch's): each child's M and C with their identity diagonals, read from
 * the store that holds them. infos: one record per problem of that solve (may be NULL). Per problem the results are
 * bit for bit those of clipper_hip_sdp on a lone context scored from the same inputs on the same storage. Each
 * problem's selection becomes its node list: clipper_hip_batch_get_nodes / _get_selected_associations return it
 * (and clipper_hip_batch_get_solution's num_nodes is its size); the solver state of the children is untouched.
 * CLIPPER_HIP_E_STATE before any solve; CLIPPER_HIP_E_SCOPE naming the first problem with m above the route setting's
 * limit (CLIPPER_HIP_SDP_MAX_N by default; the problems above it take the wide route under CLIPPER_HIP_SDP_ROUTE_AUTO)
 * (nothing has run then, and the batch stays usable). */
int clipper_hip_batch_sdp(clipper_hip_batch_t* b, const clipper_sdp_params_t* params, clipper_sdp_info_t* infos);
/* The maximum clique (clipper_hip_max_clique, DESIGN.md 9 "Batches") of every problem of the batch's last solve call,
 * side by side in a handful of launches: the graph of problem i is the pattern of its child's M, read from the store
 * that holds it (the slices where they are valid, else the dense store). infos: one record per problem of that solve
 * (may be NULL). Per problem and for every method the node list, max_core, heuristic_size, edges and num_nodes equal
 * those of clipper_hip_max_clique on a lone context scored from the same inputs on the same storage, whatever else
 * the batch holds, wherever the problem stands in it and however the launches are cut; roots_searched, roots_pruned
 * and bb_nodes depend on the schedule and are only reported; seconds is the wall time of the whole call. The clique
 * (ascending) becomes the problem's node list: clipper_hip_batch_get_nodes / _get_selected_associations return it,
 * clipper_hip_batch_get_solution's num_nodes is its size; nothing the solver keeps is touched.
 * Routes: problems with m <= 2048 (the batch's resident limit, on all four storages) run in the batched launches,
 * their graphs out of ONE device slab whose size is checked against the free memory before anything runs
 * (CLIPPER_HIP_E_NOMEM with the figures; the batch stays usable); larger problems run afterwards, one by one, each as
 * clipper_hip_max_clique runs a lone context.
 * time_limit_s > 0 bounds the whole call, checked between launches: problems still searching when it runs out return
 * their best clique so far with timed_out = 1 (HEU's first launch always leaves one, as in the lone call), problems
 * that had finished keep timed_out = 0 and their exact result. A problem of the lone route gets the time that remains; when
 * none remains it still builds its graph and core numbers and makes ONE launch of HEU (the least a call does) and
 * returns that launch's best clique with timed_out = 1 (unless that launch finished HEU and no search was left).
 * CLIPPER_HIP_E_STATE before any solve, CLIPPER_HIP_E_INVALID for an unknown method; a batch of 0 problems returns 0. */
int clipper_hip_batch_max_clique(clipper_hip_batch_t* b, int method, double time_limit_s,
                                 clipper_maxclique_info_t* infos /* one per problem of the last solve, or NULL */);
/* clipper_hip_max_clique_seeded for every problem of the batch's last solve call, in the same launches as the
 * unseeded batched call plus one for the seed cliques. Problem i's vertex list is seeds[offsets[i] .. offsets[i + 1])
 * (offsets: one entry per problem and one more; an empty list: that problem runs unseeded); seeds = offsets = NULL:
 * every problem's own node list, as the last solve (or a later relaxation or clique call) left it. Per problem the list
 * and both records' fields are those of the lone seeded call on a lone context, the schedule-dependent counters
 * excepted. An invalid index returns CLIPPER_HIP_E_INVALID naming the problem and the position before any device
 * work; the batch stays usable. seed_infos: one record per problem, or NULL. */
int clipper_hip_batch_max_clique_seeded(clipper_hip_batch_t* b, int method, double time_limit_s, const int32_t* seeds,
                                        const int64_t* offsets, clipper_maxclique_info_t* infos,
                                        clipper_maxclique_seed_info_t* seed_infos);
/* The last clipper_hip_batch_max_clique: kernel launches of the batched route, problems that ran in them, problems
 * that ran alone. Any pointer may be NULL. */
int clipper_hip_batch_max_clique_stats(const clipper_hip_batch_t* b, int32_t* launches, int32_t* n_batched,
                                       int32_t* n_alone);
/* Problem i of the last clipper_hip_batch_sdp: X and Y (m x m), lambdas (m, ascending), evec1 (m); any may be NULL.
 * X and Y stay on the device until the next solve or relaxation of the batch. Returns m or <0. */
int clipper_hip_batch_get_sdp(const clipper_hip_batch_t* b, int32_t i, double* X_out, double* Y_out,
                              double* lambdas_out, double* evec1_out);

#ifdef __cplusplus
}
#endif
#endif /* CLIPPER_HIP_H */
