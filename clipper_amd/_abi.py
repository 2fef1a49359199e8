"""ctypes binding of the C ABI in include/clipper_hip.h (clipper_amd/lib/libclipper_hip.so).

This is the thinnest possible Python view of the drop-in boundary: every method is one
C call. The user-facing Python surface of the reference (`clipperpy`, py_clipper.cpp) is
provided by the pybind11 module built from clipper_amd/csrc/host/; this module is what the
parity tests and bench.py drive so that they exercise exactly the exported symbols.

There is no fallback: if the shared library is missing or no HIP device is usable, the
constructors raise.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CLIPPER_HIP_LIB: alternate build of the same library (A/B measurements of kernel variants)
LIB_PATH = os.environ.get("CLIPPER_HIP_LIB") or os.path.join(_HERE, "lib", "libclipper_hip.so")

STORE_F32, STORE_F64, STORE_F32_CSC, STORE_F64_CSC = 0, 1, 2, 3
ROUNDING_NONZERO, ROUNDING_DSD, ROUNDING_DSD_HEU = 0, 1, 2
MC_EXACT, MC_HEU, MC_KCORE = 0, 1, 2  # CLIPPER_HIP_MC_* = maxclique::Method
MC_SEED_ONLY = 3  # CLIPPER_HIP_MC_SEED_ONLY: the seeded entry points only
SDP_MAX_N = 128  # CLIPPER_HIP_SDP_MAX_N
SDP_WIDE_MAX_N = 1024  # CLIPPER_HIP_SDP_WIDE_MAX_N
SDP_ROUTE_WORKGROUP, SDP_ROUTE_AUTO, SDP_ROUTE_WIDE = 0, 1, 2  # CLIPPER_HIP_SDP_ROUTE_*
KNN_BRUTE, KNN_GRID, KNN_AUTO = 0, 1, 2  # CLIPPER_HIP_KNN_*: the route of the d = 3 nearest-neighbour search
INVARIANT_MAX_D, INVARIANT_MAX_PARAMS = 32, 16  # CLIPPER_HIP_INVARIANT_MAX_D / _MAX_PARAMS

# every symbol include/clipper_hip.h declares (checked by tests/test_abi_exports.py)
EXPORTED_SYMBOLS = [
    "clipper_hip_device_count", "clipper_hip_create", "clipper_hip_create_group",
    "clipper_hip_create_rank", "clipper_hip_comm_unique_id", "clipper_hip_comm_init",
    "clipper_hip_destroy", "clipper_hip_last_error", "clipper_hip_affinity_euclidean",
    "clipper_hip_affinity_pointnormal", "clipper_hip_num_associations",
    "clipper_hip_get_associations", "clipper_hip_set_matrix", "clipper_hip_set_sparse",
    "clipper_hip_get_matrix", "clipper_hip_solve", "clipper_hip_get_nodes",
    "clipper_hip_get_selected_associations", "clipper_hip_matvec", "clipper_hip_set_profiling",
    "clipper_hip_set_window", "clipper_hip_window", "clipper_hip_densest_subgraph",
    "clipper_hip_set_resident", "clipper_hip_last_solver",
    "clipper_hip_set_row_view", "clipper_hip_get_view_stats", "clipper_hip_view_matvec", "clipper_hip_set_subproblem",
    "clipper_hip_storage_in_use", "clipper_hip_knn", "clipper_hip_distance_based_correspondences",
    "clipper_hip_get_timings", "clipper_hip_bench_matvec", "clipper_hip_device_info",
    "clipper_hip_stage_inputs", "clipper_hip_affinity_euclidean_staged",
    "clipper_hip_affinity_pointnormal_staged", "clipper_hip_stage_u0",
    "clipper_hip_solve_staged", "clipper_hip_debug_stamps", "clipper_hip_comm_init_callback",
    "clipper_hip_read_ply_xyz", "clipper_hip_generate_synthetic_correspondences",
    "clipper_hip_precision_recall", "clipper_hip_estimate_rigid_transform", "clipper_hip_debug_occupy",
    "clipper_hip_debug_live_resources", "clipper_hip_debug_mc_budgets", "clipper_hip_debug_mc_launches",
    "clipper_hip_debug_sub_select", "clipper_hip_debug_sub_last", "clipper_hip_debug_sub_min_m",
    "clipper_hip_max_clique", "clipper_hip_core_numbers", "clipper_hip_sdp", "clipper_hip_sdp_solve",
    "clipper_hip_batch_create", "clipper_hip_batch_destroy", "clipper_hip_batch_solve_euclidean",
    "clipper_hip_batch_solve_pointnormal", "clipper_hip_batch_get_solution", "clipper_hip_batch_get_nodes",
    "clipper_hip_batch_get_selected_associations", "clipper_hip_batch_route", "clipper_hip_batch_get_stats",
    "clipper_hip_batch_get_split", "clipper_hip_invariant_create", "clipper_hip_invariant_destroy",
    "clipper_hip_affinity_custom_staged", "clipper_hip_affinity_custom", "clipper_hip_batch_solve_custom",
    "clipper_hip_sdp_solve_batch", "clipper_hip_batch_sdp", "clipper_hip_batch_get_sdp",
    "clipper_hip_batch_max_clique", "clipper_hip_batch_max_clique_stats",
    "clipper_hip_max_clique_seeded", "clipper_hip_batch_max_clique_seeded",
    "clipper_hip_sdp_set_route", "clipper_hip_sdp_route", "clipper_hip_match_descriptors",
    "clipper_hip_estimate_normals", "clipper_hip_compute_fpfh", "clipper_hip_fpfh_from_points",
    "clipper_hip_knn_set_search", "clipper_hip_knn_search", "clipper_hip_knn_last_search",
    "clipper_hip_icp", "clipper_hip_evaluate_registration", "clipper_hip_voxel_downsample",
    "clipper_hip_icp_generalized", "clipper_hip_estimate_covariances",
    "clipper_hip_ransac_correspondences", "clipper_hip_ransac_needed",
    "clipper_hip_icp_robust", "clipper_hip_icp_generalized_robust",
    "clipper_hip_cloud_create", "clipper_hip_cloud_destroy", "clipper_hip_cloud_count", "clipper_hip_cloud_download",
    "clipper_hip_cloud_info", "clipper_hip_cloud_set_descriptors", "clipper_hip_pairs_create", "clipper_hip_pairs_destroy",
    "clipper_hip_pairs_count", "clipper_hip_pairs_has_sqd", "clipper_hip_pairs_download", "clipper_hip_cloud_voxel_downsample",
    "clipper_hip_cloud_estimate_normals", "clipper_hip_cloud_compute_fpfh", "clipper_hip_cloud_fpfh_from_points",
    "clipper_hip_cloud_estimate_covariances", "clipper_hip_cloud_match", "clipper_hip_stage_inputs_clouds",
    "clipper_hip_cloud_gather_points", "clipper_hip_cloud_icp", "clipper_hip_cloud_evaluate_registration",
]

# CLIPPER_HIP_CLOUD_*: what clipper_hip_cloud_download copies down
(CLOUD_POINTS, CLOUD_NORMALS, CLOUD_DESCRIPTORS, CLOUD_SPFH, CLOUD_COVARIANCES, CLOUD_NORMAL_COUNTS, CLOUD_FPFH_COUNTS,
 CLOUD_COVARIANCE_COUNTS, CLOUD_VOXEL_COUNTS, CLOUD_VOXEL_TRACE) = range(10)


# int fn(void* user, const void* sendbuf, void* recvbuf, size_t bytes) — clipper_hip_allgather_fn
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)


class ClipperError(RuntimeError):
    """a C ABI entry point returned a negative status (CLIPPER_HIP_E_*)"""


class Params(C.Structure):
    """clipper_params_t == clipper::Params (reference include/clipper/clipper.h:27-60)."""

    _fields_ = [
        ("tol_u", C.c_double), ("tol_F", C.c_double), ("tol_Fop", C.c_double),
        ("maxiniters", C.c_int32), ("maxoliters", C.c_int32), ("beta", C.c_double),
        ("maxlsiters", C.c_int32), ("eps", C.c_double), ("affinityeps", C.c_double),
        ("rescale_u0", C.c_int32), ("rounding", C.c_int32),
    ]

    def __init__(self, **kw):
        super().__init__()
        self.tol_u, self.tol_F, self.tol_Fop = 1e-8, 1e-9, 1e-10
        self.maxiniters, self.maxoliters = 200, 1000
        self.beta, self.maxlsiters = 0.25, 99
        self.eps, self.affinityeps = 1e-9, 1e-4
        self.rescale_u0, self.rounding = 1, ROUNDING_DSD_HEU
        for k, v in kw.items():
            setattr(self, k, v)


class SolveInfo(C.Structure):
    _fields_ = [
        ("score", C.c_double), ("seconds", C.c_double), ("d", C.c_double),
        ("ifinal", C.c_int32), ("num_nodes", C.c_int32),
        ("n_passes", C.c_int64), ("n_trials", C.c_int64),
    ]


class Timings(C.Structure):
    _fields_ = [
        ("affinity_kernel_ms", C.c_double), ("affinity_total_ms", C.c_double),
        ("solve_total_ms", C.c_double), ("gemv_avg_us", C.c_double),
        ("gemv_min_us", C.c_double), ("gemv_launches", C.c_int64), ("gemv_bytes", C.c_double),
        ("gemv_useful_bytes", C.c_double), ("affinity_bytes", C.c_double),
        ("exchange_avg_us", C.c_double), ("exchange_samples", C.c_int64), ("exchange_bytes", C.c_double),
    ]


class ViewStats(C.Structure):
    """clipper_hip_view_stats_t (include/clipper_hip.h): the row views of the last solve."""

    _fields_ = [
        ("builds", C.c_int64), ("rows", C.c_int64), ("bytes", C.c_int64),
        ("view_passes", C.c_int64), ("passes", C.c_int64), ("build_ms", C.c_double),
        ("view_pass_avg_us", C.c_double), ("view_pass_samples", C.c_int64),
        ("resident_launches", C.c_int64), ("resident_giveups", C.c_int64),
        ("resident_iterations", C.c_int64), ("resident_us", C.c_double), ("resident_event_us", C.c_double),
        ("resident_entries", C.c_int64), ("resident_units", C.c_int64),
        ("sub_entries", C.c_int64), ("sub_leaves", C.c_int64), ("sub_passes", C.c_int64),
        ("sub_rows", C.c_int64), ("sub_bytes", C.c_int64), ("sub_build_ms", C.c_double),
        ("sub_pass_avg_us", C.c_double), ("sub_pass_samples", C.c_int64), ("sub_dense", C.c_int64),
    ]


class SubSelection(C.Structure):
    """clipper_hip_sub_selection_t (include/clipper_hip.h): the record of a selection of the live sub-problem."""

    _fields_ = [
        ("mp", C.c_int64), ("nS", C.c_int64), ("entries", C.c_int64), ("nrows", C.c_int64),
        ("ncol", C.c_int32), ("n0", C.c_int32), ("s", C.c_double), ("N_used", C.c_double),
        ("built", C.c_int32), ("entered", C.c_int32),
    ]


class MaxCliqueInfo(C.Structure):
    """clipper_maxclique_info_t (include/clipper_hip.h): what clipper_hip_max_clique reports."""

    _fields_ = [
        ("num_nodes", C.c_int32), ("max_core", C.c_int32), ("heuristic_size", C.c_int32), ("timed_out", C.c_int32),
        ("edges", C.c_int64), ("roots_searched", C.c_int64), ("roots_pruned", C.c_int64), ("bb_nodes", C.c_int64),
        ("seconds", C.c_double),
    ]


class MaxCliqueSeedInfo(C.Structure):
    """clipper_maxclique_seed_info_t (include/clipper_hip.h): what a seeded max-clique call reports of its seed."""

    _fields_ = [("seed_given", C.c_int32), ("seed_kept", C.c_int32), ("seed_size", C.c_int32), ("winner", C.c_int32)]


class SdpParams(C.Structure):
    """clipper_sdp_params_t (include/clipper_hip.h) = sdp::Params. acceleration_interval, acceleration_lookback and
    eps_infeas are accepted and ignored."""

    _fields_ = [
        ("verbose", C.c_int32), ("max_iters", C.c_int32), ("acceleration_interval", C.c_int32),
        ("acceleration_lookback", C.c_int32), ("eps_abs", C.c_float), ("eps_rel", C.c_float),
        ("eps_infeas", C.c_float), ("time_limit_secs", C.c_float),
    ]

    def __init__(self, **kw):
        base = dict(verbose=0, max_iters=2000, acceleration_interval=10, acceleration_lookback=10, eps_abs=1e-3,
                    eps_rel=1e-3, eps_infeas=1e-7, time_limit_secs=0.0)
        base.update(kw)
        super().__init__(**base)


class SdpInfo(C.Structure):
    """clipper_sdp_info_t (include/clipper_hip.h): what clipper_hip_sdp / clipper_hip_sdp_solve report."""

    _fields_ = [
        ("iters", C.c_int32), ("converged", C.c_int32), ("timed_out", C.c_int32), ("num_nodes", C.c_int32),
        ("sweeps", C.c_int32), ("route", C.c_int32),
        ("pobj", C.c_double), ("dobj", C.c_double), ("r_prim", C.c_double), ("r_dual", C.c_double),
        ("rho", C.c_double), ("thr", C.c_double), ("t_total", C.c_double), ("t_setup", C.c_double),
        ("t_solve", C.c_double), ("t_extract", C.c_double),
    ]


class SdpProblem(C.Structure):
    """clipper_sdp_problem_t (include/clipper_hip.h): one problem of clipper_hip_sdp_solve_batch (host buffers)."""

    _fields_ = [
        ("M", C.POINTER(C.c_double)), ("C", C.POINTER(C.c_double)), ("n", C.c_int64),
        ("X_out", C.POINTER(C.c_double)), ("Y_out", C.POINTER(C.c_double)), ("lambdas_out", C.POINTER(C.c_double)),
        ("evec1_out", C.POINTER(C.c_double)), ("nodes_out", C.POINTER(C.c_int32)),
    ]


@dataclass
class SdpResult:
    """sdp::Solution (sdp.h:15-37) plus the certificate: Y (the dual of the constraints of C) and SdpInfo."""

    X: np.ndarray
    Y: np.ndarray
    lambdas: np.ndarray
    evec1: np.ndarray
    thr: float
    nodes: np.ndarray
    iters: int
    pobj: float
    dobj: float
    info: SdpInfo


def _sdp_result(n, X, Y, lam, ev, nodes, info) -> SdpResult:
    return SdpResult(X=X, Y=Y, lambdas=lam, evec1=ev, thr=info.thr, nodes=nodes, iters=info.iters, pobj=info.pobj,
                     dobj=info.dobj, info=info)


class KnnStats(C.Structure):
    """clipper_hip_knn_stats_t (include/clipper_hip.h): the calling thread's last nearest-neighbour search."""

    _fields_ = [("route", C.c_int32), ("dim", C.c_int32 * 3), ("queries", C.c_int64), ("candidates", C.c_int64),
                ("auto_min_n", C.c_int64), ("kernels_ms", C.c_double)]


class MatchParams(C.Structure):
    """clipper_match_params_t"""
    _fields_ = [("knn", C.c_int32), ("mutual", C.c_int32), ("ratio", C.c_double), ("max_sqdist", C.c_double)]


class Neighborhood(C.Structure):
    """clipper_neighborhood_t: the first knn entries of a point's nearest-neighbour list in its own cloud (the point
    included), with radius > 0 only those within it"""
    _fields_ = [("knn", C.c_int32), ("reserved", C.c_int32), ("radius", C.c_double)]

    def __init__(self, knn=16, radius=0.0):
        super().__init__(int(knn), 0, float(radius))


FPFH_DIM = 33  # numbers per FPFH descriptor

ICP_POINT_TO_POINT, ICP_POINT_TO_PLANE, ICP_GENERALIZED = 0, 1, 2  # CLIPPER_ICP_*: clipper_icp_params_t.method
ICP_CONVERGED, ICP_MAX_ITERATIONS, ICP_TOO_FEW, ICP_DEGENERATE = 0, 1, 2, 3  # clipper_icp_info_t.status


class IcpParams(C.Structure):
    """clipper_icp_params_t"""
    _fields_ = [("method", C.c_int32), ("max_iterations", C.c_int32), ("max_distance", C.c_double),
                ("rel_fitness", C.c_double), ("rel_rmse", C.c_double)]

    def __init__(self, method=ICP_POINT_TO_POINT, max_distance=0.0, max_iterations=30, rel_fitness=1e-6, rel_rmse=1e-6):
        super().__init__(int(method), int(max_iterations), float(max_distance), float(rel_fitness), float(rel_rmse))


class IcpInfo(C.Structure):
    """clipper_icp_info_t: how an ICP ended (status: ICP_*), the alignment's count / fitness / inlier_rmse under T_out,
    the search route taken with the target grid's cells per axis and the candidates visited over all iterations, and
    the device time of the loop. `history` is attached by the Python facade: (iterations + 1) x 3 rows of (count,
    fitness, rmse)."""
    _fields_ = [("iterations", C.c_int32), ("status", C.c_int32), ("count", C.c_int64), ("fitness", C.c_double),
                ("inlier_rmse", C.c_double), ("route", C.c_int32), ("dim", C.c_int32 * 3), ("candidates", C.c_int64),
                ("device_ms", C.c_double)]


# CLIPPER_ICP_LOSS_*: clipper_icp_robust_t.loss
ICP_LOSS_NONE, ICP_LOSS_HUBER, ICP_LOSS_CAUCHY, ICP_LOSS_TUKEY, ICP_LOSS_GEMAN_MCCLURE = 0, 1, 2, 3, 4


class IcpRobust(C.Structure):
    """clipper_icp_robust_t: the loss (ICP_LOSS_*), its scale (a distance; not read without a loss) and the trimmed
    fraction kept of the points within max_distance (1 = no trimming)"""
    _fields_ = [("loss", C.c_int32), ("reserved", C.c_int32), ("scale", C.c_double), ("trim", C.c_double)]

    def __init__(self, loss=ICP_LOSS_NONE, scale=0.0, trim=1.0):
        super().__init__(int(loss), 0, float(scale), float(trim))


class IcpRobustInfo(C.Structure):
    """clipper_icp_robust_info_t, of the last history row: the points within max_distance before trimming, the sum of
    the weights (point-to-point; 0 otherwise) and the trimming threshold tau"""
    _fields_ = [("within", C.c_int64), ("weight_sum", C.c_double), ("trim_sqd", C.c_double)]


RANSAC_CONVERGED, RANSAC_MAX_HYPOTHESES, RANSAC_NO_MODEL = 0, 1, 2  # CLIPPER_RANSAC_*: clipper_ransac_info_t.status


class RansacParams(C.Structure):
    """clipper_ransac_params_t"""
    _fields_ = [("max_distance", C.c_double), ("edge_similarity", C.c_double), ("confidence", C.c_double),
                ("max_hypotheses", C.c_int64), ("hypotheses_per_round", C.c_int32), ("n_sample", C.c_int32),
                ("refine_iterations", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64)]

    def __init__(self, max_distance=0.0, n_sample=3, edge_similarity=0.9, max_hypotheses=100000, confidence=0.999, seed=0,
                 refine_iterations=1, hypotheses_per_round=4096):
        super().__init__(float(max_distance), float(edge_similarity), float(confidence), int(max_hypotheses),
                         int(hypotheses_per_round), int(n_sample), int(refine_iterations), 0, int(seed) & (2 ** 64 - 1))


class RansacInfo(C.Structure):
    """clipper_ransac_info_t: how the rounds ended (status: RANSAC_*), the accepted polish steps, the hypotheses formed
    and the ones scored, the winner's number, count and sample, the count / fitness / inlier_rmse under T_out and the
    device time. `inliers` (a boolean mask over the associations) is attached by the Python facade."""
    _fields_ = [("status", C.c_int32), ("refined", C.c_int32), ("evaluated", C.c_int64), ("checked", C.c_int64),
                ("best_hypothesis", C.c_int64), ("best_count", C.c_int64), ("count", C.c_int64), ("fitness", C.c_double),
                ("inlier_rmse", C.c_double), ("sample", C.c_int32 * 8), ("device_ms", C.c_double)]


class VoxelInfo(C.Structure):
    """clipper_voxel_info_t: the grid of a voxel_down_sample (voxels per axis), the 8-bit passes of its radix sort, the
    pairs per workgroup of a pass, the chunk length of the sums (512), the members of the fullest voxel, the device time
    between two events around the kernels and, of that, the time of the sort's passes."""
    _fields_ = [("dim", C.c_int32 * 3), ("passes", C.c_int32), ("sort_tile", C.c_int32), ("chunk", C.c_int32),
                ("max_count", C.c_int32), ("reserved", C.c_int32), ("kernels_ms", C.c_double), ("sort_ms", C.c_double)]


class CloudInfo(C.Structure):
    """clipper_hip_cloud_info_t: what a cloud on the device holds: its points, the entries of the voxel trace, its
    device, which attachments exist (descriptor_dim 0: no descriptors), how often the search grid over it was built
    (0 or 1: it is kept) and that grid's cells per axis."""
    _fields_ = [("n", C.c_int64), ("trace_n", C.c_int64), ("device", C.c_int32), ("has_normals", C.c_int32),
                ("descriptor_dim", C.c_int32), ("has_spfh", C.c_int32), ("has_covariances", C.c_int32),
                ("has_voxel_counts", C.c_int32), ("grid_builds", C.c_int32), ("grid_dim", C.c_int32 * 3)]


class BatchProblem(C.Structure):
    """clipper_batch_problem_t (include/clipper_hip.h): one problem of a batched solve (host buffers)."""

    _fields_ = [
        ("D1", C.POINTER(C.c_double)), ("n1", C.c_int64),
        ("D2", C.POINTER(C.c_double)), ("n2", C.c_int64),
        ("A", C.POINTER(C.c_int32)), ("m", C.c_int64),
        ("u0", C.POINTER(C.c_double)),
    ]


@dataclass
class Solution:
    """clipper::Solution (clipper.h:65-73) plus the counters this build reports."""

    t: float = 0.0
    ifinal: int = 0
    nodes: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    u0: np.ndarray = field(default_factory=lambda: np.zeros(0))
    u: np.ndarray = field(default_factory=lambda: np.zeros(0))
    score: float = 0.0
    d: float = 0.0
    n_passes: int = 0
    n_trials: int = 0


_lib = None


def load_library(path: str = LIB_PATH):
    """dlopen the product library and declare the prototypes. Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    L = C.CDLL(path)
    dp, ip, i64, vp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int64, C.c_void_p
    L.clipper_hip_device_count.restype = C.c_int
    L.clipper_hip_create.argtypes = [C.c_int, C.c_int]
    L.clipper_hip_create.restype = vp
    L.clipper_hip_create_group.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    L.clipper_hip_create_group.restype = vp
    L.clipper_hip_create_rank.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.clipper_hip_create_rank.restype = vp
    L.clipper_hip_comm_unique_id.argtypes = [vp]
    L.clipper_hip_comm_init.argtypes = [vp, vp]
    L.clipper_hip_destroy.argtypes = [vp]
    L.clipper_hip_destroy.restype = None
    L.clipper_hip_last_error.restype = C.c_char_p
    L.clipper_hip_affinity_euclidean.argtypes = [
        vp, dp, C.c_int, i64, dp, i64, ip, i64, C.c_double, C.c_double, C.c_double, C.c_double]
    L.clipper_hip_affinity_pointnormal.argtypes = [
        vp, dp, C.c_int, i64, dp, i64, ip, i64, C.c_double, C.c_double, C.c_double, C.c_double,
        C.c_double]
    L.clipper_hip_stage_inputs.argtypes = [vp, dp, C.c_int, i64, dp, i64, ip, i64]
    L.clipper_hip_affinity_euclidean_staged.argtypes = [vp] + [C.c_double] * 4
    L.clipper_hip_affinity_pointnormal_staged.argtypes = [vp] + [C.c_double] * 5
    L.clipper_hip_stage_u0.argtypes = [vp, dp]
    L.clipper_hip_solve_staged.argtypes = [vp, C.POINTER(Params), dp, C.POINTER(SolveInfo)]
    L.clipper_hip_num_associations.argtypes = [vp]
    L.clipper_hip_num_associations.restype = i64
    L.clipper_hip_get_associations.argtypes = [vp, ip]
    L.clipper_hip_set_matrix.argtypes = [vp, dp, dp, i64]
    L.clipper_hip_set_sparse.argtypes = [vp, i64, C.POINTER(i64), ip, dp, C.POINTER(i64), ip, dp]
    L.clipper_hip_get_matrix.argtypes = [vp, dp, dp]
    L.clipper_hip_solve.argtypes = [vp, dp, C.POINTER(Params), dp, C.POINTER(SolveInfo)]
    L.clipper_hip_get_nodes.argtypes = [vp, ip, C.c_int32]
    L.clipper_hip_get_selected_associations.argtypes = [vp, ip, C.c_int32]
    L.clipper_hip_matvec.argtypes = [vp, dp, dp, dp]
    L.clipper_hip_densest_subgraph.argtypes = [vp, ip, C.c_int32, ip, C.c_int32]
    L.clipper_hip_set_window.argtypes = [vp, C.c_int]
    L.clipper_hip_window.argtypes = [vp]
    L.clipper_hip_set_resident.argtypes = [vp, C.c_int]
    L.clipper_hip_last_solver.argtypes = [vp]
    L.clipper_hip_storage_in_use.argtypes = [vp]
    L.clipper_hip_set_row_view.argtypes = [vp, C.c_int]
    L.clipper_hip_set_subproblem.argtypes = [vp, C.c_int]
    L.clipper_hip_get_view_stats.argtypes = [vp, C.POINTER(ViewStats)]
    L.clipper_hip_view_matvec.argtypes = [vp, ip, i64, dp, dp, dp]
    u8p = C.POINTER(C.c_uint8)
    L.clipper_hip_debug_sub_select.argtypes = [vp, ip, i64, C.c_double, i64, ip, u8p, ip, ip, C.POINTER(SubSelection)]
    L.clipper_hip_debug_sub_last.argtypes = [vp, i64, ip, u8p, ip, ip, ip, C.POINTER(SubSelection)]
    L.clipper_hip_debug_sub_min_m.argtypes = [C.c_longlong]
    L.clipper_hip_knn.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int, C.c_int, ip, dp]
    L.clipper_hip_distance_based_correspondences.argtypes = [
        C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int, C.c_int, C.c_double, C.c_int, ip, C.c_int64]
    L.clipper_hip_distance_based_correspondences.restype = C.c_int64
    L.clipper_hip_match_descriptors.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int, C.POINTER(MatchParams),
                                                ip, dp, C.c_int64, ip, dp]
    L.clipper_hip_match_descriptors.restype = C.c_int64
    nbp = C.POINTER(Neighborhood)
    L.clipper_hip_estimate_normals.argtypes = [C.c_int, dp, C.c_int64, nbp, dp, dp, ip]
    L.clipper_hip_compute_fpfh.argtypes = [C.c_int, dp, dp, C.c_int64, nbp, dp, dp, ip]
    L.clipper_hip_fpfh_from_points.argtypes = [C.c_int, dp, C.c_int64, nbp, dp, nbp, dp, dp]
    L.clipper_hip_icp.argtypes = [C.c_int, dp, C.c_int64, dp, dp, C.c_int64, dp, C.POINTER(IcpParams), dp,
                                  C.POINTER(IcpInfo), dp]
    L.clipper_hip_icp_generalized.argtypes = [C.c_int, dp, dp, C.c_int64, dp, dp, C.c_int64, dp, C.POINTER(IcpParams), dp,
                                              C.POINTER(IcpInfo), dp]
    L.clipper_hip_icp_robust.argtypes = [C.c_int, dp, C.c_int64, dp, dp, C.c_int64, dp, C.POINTER(IcpParams),
                                         C.POINTER(IcpRobust), dp, C.POINTER(IcpInfo), C.POINTER(IcpRobustInfo), dp]
    L.clipper_hip_icp_generalized_robust.argtypes = [C.c_int, dp, dp, C.c_int64, dp, dp, C.c_int64, dp, C.POINTER(IcpParams),
                                                     C.POINTER(IcpRobust), dp, C.POINTER(IcpInfo), C.POINTER(IcpRobustInfo),
                                                     dp]
    L.clipper_hip_estimate_covariances.argtypes = [C.c_int, dp, C.c_int64, nbp, C.c_double, dp, ip]
    L.clipper_hip_evaluate_registration.argtypes = [C.c_int, dp, C.c_int64, dp, C.c_int64, dp, C.c_double,
                                                    C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64), ip]
    L.clipper_hip_voxel_downsample.argtypes = [C.c_int, dp, dp, C.c_int64, C.c_double, dp, dp, ip, ip,
                                               C.POINTER(C.c_int64), C.POINTER(VoxelInfo)]
    if hasattr(L, "clipper_hip_cloud_create"):  # (absent from an older build named by CLIPPER_HIP_LIB: the A/B tools)
        vpp = C.POINTER(vp)
        L.clipper_hip_cloud_create.argtypes = [C.c_int, dp, dp, i64, vpp]
        L.clipper_hip_cloud_destroy.argtypes = [vp]
        L.clipper_hip_cloud_destroy.restype = None
        L.clipper_hip_cloud_count.argtypes = [vp]
        L.clipper_hip_cloud_count.restype = i64
        L.clipper_hip_cloud_download.argtypes = [vp, C.c_int, vp]
        L.clipper_hip_cloud_info.argtypes = [vp, C.POINTER(CloudInfo)]
        L.clipper_hip_cloud_set_descriptors.argtypes = [vp, dp, C.c_int]
        L.clipper_hip_pairs_create.argtypes = [C.c_int, ip, dp, i64, vpp]
        L.clipper_hip_pairs_destroy.argtypes = [vp]
        L.clipper_hip_pairs_destroy.restype = None
        L.clipper_hip_pairs_count.argtypes = [vp]
        L.clipper_hip_pairs_count.restype = i64
        L.clipper_hip_pairs_has_sqd.argtypes = [vp]
        L.clipper_hip_pairs_download.argtypes = [vp, ip, dp]
        L.clipper_hip_cloud_voxel_downsample.argtypes = [vp, C.c_double, C.c_int, vpp, C.POINTER(VoxelInfo)]
        L.clipper_hip_cloud_estimate_normals.argtypes = [vp, nbp, dp]
        L.clipper_hip_cloud_compute_fpfh.argtypes = [vp, nbp]
        L.clipper_hip_cloud_fpfh_from_points.argtypes = [vp, nbp, dp, nbp]
        L.clipper_hip_cloud_estimate_covariances.argtypes = [vp, nbp, C.c_double]
        L.clipper_hip_cloud_match.argtypes = [vp, vp, C.POINTER(MatchParams), vpp, ip, dp]
        L.clipper_hip_stage_inputs_clouds.argtypes = [vp, vp, vp, vp, C.c_int]
        L.clipper_hip_cloud_gather_points.argtypes = [vp, ip, i64, dp]
        L.clipper_hip_cloud_icp.argtypes = [vp, vp, dp, C.POINTER(IcpParams), C.POINTER(IcpRobust), dp, C.POINTER(IcpInfo),
                                            C.POINTER(IcpRobustInfo), dp]
        L.clipper_hip_cloud_evaluate_registration.argtypes = [vp, vp, dp, C.c_double, C.POINTER(C.c_double),
                                                              C.POINTER(C.c_double), C.POINTER(C.c_int64), ip]
    L.clipper_hip_set_profiling.argtypes = [vp, C.c_int]
    L.clipper_hip_get_timings.argtypes = [vp, C.POINTER(Timings)]
    L.clipper_hip_bench_matvec.argtypes = [vp, C.c_int, dp]
    L.clipper_hip_device_info.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int), C.POINTER(i64)]
    L.clipper_hip_debug_stamps.argtypes = [vp, C.POINTER(i64), C.c_int]
    L.clipper_hip_comm_init_callback.argtypes = [vp, ALLGATHER_FN, vp]
    L.clipper_hip_read_ply_xyz.argtypes = [C.c_char_p, dp, i64]
    L.clipper_hip_read_ply_xyz.restype = i64
    L.clipper_hip_generate_synthetic_correspondences.argtypes = [i64, i64, ip, i64, i64, C.c_double, C.c_uint64,
                                                                 ip, ip, C.POINTER(i64)]
    L.clipper_hip_precision_recall.argtypes = [ip, i64, ip, i64, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.clipper_hip_estimate_rigid_transform.argtypes = [dp, i64, dp, i64, ip, i64, dp]
    if hasattr(L, "clipper_hip_ransac_correspondences"):  # (absent from an older build named by CLIPPER_HIP_LIB)
        L.clipper_hip_ransac_correspondences.argtypes = [C.c_int, dp, i64, dp, i64, ip, i64, C.POINTER(RansacParams), dp,
                                                         C.POINTER(C.c_uint8), C.POINTER(RansacInfo)]
        L.clipper_hip_ransac_needed.argtypes = [i64, i64, C.c_int32, C.c_double]
        L.clipper_hip_ransac_needed.restype = i64
    L.clipper_hip_debug_occupy.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double]
    if hasattr(L, "clipper_hip_debug_live_resources"):  # (absent from an older build named by CLIPPER_HIP_LIB: the A/B tools)
        L.clipper_hip_debug_live_resources.argtypes = [C.POINTER(i64)]
    L.clipper_hip_debug_mc_budgets.argtypes = [C.c_longlong, C.c_longlong]
    L.clipper_hip_debug_mc_launches.argtypes = [vp]
    L.clipper_hip_max_clique.argtypes = [vp, C.c_int, C.c_double, C.POINTER(MaxCliqueInfo)]
    L.clipper_hip_core_numbers.argtypes = [vp, ip]
    L.clipper_hip_sdp.argtypes = [vp, C.POINTER(SdpParams), dp, dp, dp, dp, C.POINTER(SdpInfo)]
    L.clipper_hip_sdp_solve.argtypes = [C.c_int, dp, dp, C.c_int64, C.POINTER(SdpParams), dp, dp, dp, dp, ip,
                                        C.POINTER(SdpInfo)]
    L.clipper_hip_sdp_solve_batch.argtypes = [C.c_int, C.POINTER(SdpProblem), C.c_int32, C.POINTER(SdpParams),
                                              C.POINTER(SdpInfo)]
    L.clipper_hip_batch_sdp.argtypes = [vp, C.POINTER(SdpParams), C.POINTER(SdpInfo)]
    L.clipper_hip_batch_get_sdp.argtypes = [vp, C.c_int32, dp, dp, dp, dp]
    L.clipper_hip_sdp_set_route.argtypes = [C.c_int]
    L.clipper_hip_sdp_route.argtypes = []
    L.clipper_hip_knn_set_search.argtypes = [C.c_int]
    L.clipper_hip_knn_search.argtypes = []
    L.clipper_hip_knn_last_search.argtypes = [C.POINTER(KnnStats)]
    L.clipper_hip_batch_max_clique.argtypes = [vp, C.c_int, C.c_double, C.POINTER(MaxCliqueInfo)]
    L.clipper_hip_batch_max_clique_stats.argtypes = [vp, ip, ip, ip]
    L.clipper_hip_max_clique_seeded.argtypes = [vp, C.c_int, C.c_double, ip, C.c_int32, C.POINTER(MaxCliqueInfo),
                                                C.POINTER(MaxCliqueSeedInfo)]
    L.clipper_hip_batch_max_clique_seeded.argtypes = [vp, C.c_int, C.c_double, ip, C.POINTER(C.c_int64),
                                                      C.POINTER(MaxCliqueInfo), C.POINTER(MaxCliqueSeedInfo)]
    L.clipper_hip_batch_create.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    L.clipper_hip_batch_destroy.argtypes = [vp]
    L.clipper_hip_batch_destroy.restype = None
    L.clipper_hip_batch_solve_euclidean.argtypes = [vp, C.POINTER(BatchProblem), C.c_int32, C.c_int] + \
        [C.c_double] * 3 + [C.POINTER(Params)]
    L.clipper_hip_batch_solve_pointnormal.argtypes = [vp, C.POINTER(BatchProblem), C.c_int32] + \
        [C.c_double] * 4 + [C.POINTER(Params)]
    L.clipper_hip_batch_solve_custom.argtypes = [vp, vp, C.POINTER(BatchProblem), C.c_int32, dp, C.c_int,
                                                 C.POINTER(Params)]
    L.clipper_hip_batch_get_solution.argtypes = [vp, C.c_int32, dp, C.POINTER(SolveInfo)]
    L.clipper_hip_batch_get_nodes.argtypes = [vp, C.c_int32, ip, C.c_int32]
    L.clipper_hip_batch_get_selected_associations.argtypes = [vp, C.c_int32, ip, C.c_int32]
    L.clipper_hip_batch_route.argtypes = [vp, C.c_int32]
    L.clipper_hip_batch_get_stats.argtypes = [vp, ip, ip, ip]
    L.clipper_hip_batch_get_split.argtypes = [vp, dp, dp, dp, dp]
    L.clipper_hip_invariant_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.clipper_hip_invariant_destroy.argtypes = [vp]
    L.clipper_hip_affinity_custom_staged.argtypes = [vp, vp, dp, C.c_int, C.c_double]
    L.clipper_hip_affinity_custom.argtypes = [vp, vp, dp, C.c_int, i64, dp, i64, ip, i64, dp, C.c_int, C.c_double]
    _lib = L
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def _i64p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int64))


def _f64_colmajor(D):
    return np.asfortranarray(np.asarray(D, dtype=np.float64))


def _assoc_colmajor(A):
    A = np.asarray(A)
    if A.size == 0:
        return None, 0
    A = np.asfortranarray(A.astype(np.int32, copy=False))
    if A.ndim != 2 or A.shape[1] != 2:
        raise ValueError("A must be m x 2")
    return A, A.shape[0]


def _params_array(params):
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1))
    return p, (_dp(p) if p.size else None)


class HipInvariant:
    """A user-defined invariant compiled for datum dimension d (clipper_hip_invariant_create): HIP device source that
    defines `__device__ double clipper_invariant(const double* ai, const double* aj, const double* bi,
    const double* bj, const double* params)`. Needs no device; a compile error raises ClipperError with the compiler's
    log. Usable as a context manager; close() releases the code object and its modules."""

    def __init__(self, source: str, d: int):
        self.L = load_library()
        self.source, self.d = source, int(d)
        h = C.c_void_p()
        rc = self.L.clipper_hip_invariant_create(source.encode(), self.d, C.byref(h))
        if rc < 0:
            raise ClipperError(f"clipper_hip error {rc}: {self.L.clipper_hip_last_error().decode()}")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.clipper_hip_invariant_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipClipper:
    """One problem instance on the GPU(s); method names follow clipperpy.CLIPPER."""

    def __init__(self, params: Params | None = None, device: int = 0, storage: int = STORE_F32,
                 group: list[int] | None = None, rank: int | None = None, world: int = 1):
        self.L = load_library()
        self.params = params or Params()
        if group is not None:
            arr = (C.c_int * len(group))(*group)
            h = self.L.clipper_hip_create_group(arr, len(group), storage)
        elif rank is not None:
            h = self.L.clipper_hip_create_rank(device, storage, rank, world)
        else:
            h = self.L.clipper_hip_create(device, storage)
        if not h:
            raise RuntimeError("clipper_hip_create failed: " + self.last_error())
        self.h = C.c_void_p(h)
        self.storage = storage
        self.soln = Solution()

    def last_error(self) -> str:
        return self.L.clipper_hip_last_error().decode()

    def close(self):
        if getattr(self, "h", None):
            self.L.clipper_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):  # raises ClipperError (a RuntimeError) for a negative status
        if rc < 0:
            raise ClipperError(f"clipper_hip error {rc}: {self.last_error()}")
        return rc

    # ---- communicator (multi-process shards) ----------------------------------------------
    def unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        self._check(self.L.clipper_hip_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes):
        buf = C.create_string_buffer(uid, 128)
        self._check(self.L.clipper_hip_comm_init(self.h, buf))

    # ---- affinity --------------------------------------------------------------------------
    def score_pairwise_consistency_euclidean(self, D1, D2, A=(), sigma=0.01, epsilon=0.06,
                                             mindist=0.0):
        D1, D2 = _f64_colmajor(D1), _f64_colmajor(D2)
        if D1.shape[0] != D2.shape[0]:
            raise ValueError("D1 and D2 must have the same number of rows")
        Ac, m = _assoc_colmajor(A)
        self._check(self.L.clipper_hip_affinity_euclidean(
            self.h, _dp(D1), D1.shape[0], D1.shape[1], _dp(D2), D2.shape[1],
            _ip(Ac) if Ac is not None else None, m, sigma, epsilon, mindist,
            self.params.affinityeps))

    def score_pairwise_consistency_pointnormal(self, D1, D2, A=(), sigp=0.5, epsp=0.5, sign=0.10,
                                               epsn=0.35):
        D1, D2 = _f64_colmajor(D1), _f64_colmajor(D2)
        if D1.shape[0] != 6 or D2.shape[0] != 6:
            raise ValueError("PointNormalDistance data are 6 x n (xyz + unit normal)")
        Ac, m = _assoc_colmajor(A)
        self._check(self.L.clipper_hip_affinity_pointnormal(
            self.h, _dp(D1), D1.shape[0], D1.shape[1], _dp(D2), D2.shape[1],
            _ip(Ac) if Ac is not None else None, m, sigp, epsp, sign, epsn,
            self.params.affinityeps))

    # split forms: inputs resident in HBM, device work callable (and timeable) on its own
    def stage_inputs(self, D1, D2, A=()):
        D1, D2 = _f64_colmajor(D1), _f64_colmajor(D2)
        if D1.shape[0] != D2.shape[0]:
            raise ValueError("D1 and D2 must have the same number of rows")
        Ac, m = _assoc_colmajor(A)
        self._check(self.L.clipper_hip_stage_inputs(
            self.h, _dp(D1), D1.shape[0], D1.shape[1], _dp(D2), D2.shape[1],
            _ip(Ac) if Ac is not None else None, m))

    def stage_inputs_clouds(self, c0, c1, pairs, with_normals: bool = False):
        """stage_inputs from two DeviceClouds and a DevicePairs (clipper_hip_stage_inputs_clouds): D1 / D2 are the
        clouds' points, with_normals each point followed by its normal (d = 6, for affinity_pointnormal_staged)"""
        self._check(self.L.clipper_hip_stage_inputs_clouds(self.h, c0.h, c1.h, pairs.h, int(bool(with_normals))))

    def affinity_euclidean_staged(self, sigma=0.01, epsilon=0.06, mindist=0.0):
        self._check(self.L.clipper_hip_affinity_euclidean_staged(
            self.h, sigma, epsilon, mindist, self.params.affinityeps))

    def affinity_pointnormal_staged(self, sigp=0.5, epsp=0.5, sign=0.10, epsn=0.35):
        self._check(self.L.clipper_hip_affinity_pointnormal_staged(
            self.h, sigp, epsp, sign, epsn, self.params.affinityeps))

    def affinity_custom(self, inv: HipInvariant, D1, D2, A=(), params=()):
        """scorePairwiseConsistency with a user-defined invariant (clipper_hip_affinity_custom)"""
        D1, D2 = _f64_colmajor(D1), _f64_colmajor(D2)
        if D1.shape[0] != D2.shape[0]:
            raise ValueError("D1 and D2 must have the same number of rows")
        Ac, m = _assoc_colmajor(A)
        p, pp = _params_array(params)
        self._check(self.L.clipper_hip_affinity_custom(
            self.h, inv.h, _dp(D1), D1.shape[0], D1.shape[1], _dp(D2), D2.shape[1],
            _ip(Ac) if Ac is not None else None, m, pp, p.size, self.params.affinityeps))

    def affinity_custom_staged(self, inv: HipInvariant, params=()):
        p, pp = _params_array(params)
        self._check(self.L.clipper_hip_affinity_custom_staged(self.h, inv.h, pp, p.size, self.params.affinityeps))

    def stage_u0(self, u0):
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        if u0.shape != (self.m,):
            raise ValueError(f"u0 must have shape ({self.m},)")
        self._u0 = u0
        self._check(self.L.clipper_hip_stage_u0(self.h, _dp(u0)))

    def solve_staged(self):
        n = self.m
        u = np.zeros(n)
        info = SolveInfo()
        self._check(self.L.clipper_hip_solve_staged(self.h, C.byref(self.params), _dp(u),
                                                    C.byref(info)))
        nodes = np.zeros(max(info.num_nodes, 1), dtype=np.int32)
        k = self._check(self.L.clipper_hip_get_nodes(self.h, _ip(nodes), nodes.size))
        self.soln = Solution(t=info.seconds, ifinal=info.ifinal, nodes=nodes[:k].copy(),
                             u0=getattr(self, "_u0", np.zeros(0)), u=u, score=info.score,
                             d=info.d, n_passes=info.n_passes, n_trials=info.n_trials)
        return self.soln

    @property
    def m(self) -> int:
        return int(self.L.clipper_hip_num_associations(self.h))

    def get_initial_associations(self):
        A = np.zeros((self.m, 2), dtype=np.int32, order="F")
        self._check(self.L.clipper_hip_get_associations(self.h, _ip(A)))
        return np.ascontiguousarray(A)

    # ---- matrices --------------------------------------------------------------------------
    def set_matrix_data(self, M, Cm):
        M, Cm = _f64_colmajor(M), _f64_colmajor(Cm)
        if M.shape != Cm.shape or M.shape[0] != M.shape[1]:
            raise ValueError("M and C must be square and of equal size")
        self._check(self.L.clipper_hip_set_matrix(self.h, _dp(M), _dp(Cm), M.shape[0]))

    def set_sparse_matrix_data(self, m, Mcolptr, Mrow, Mval, Ccolptr, Crow, Cval):
        a = lambda x, t: np.ascontiguousarray(x, dtype=t)
        Mcp, Mr, Mv = a(Mcolptr, np.int64), a(Mrow, np.int32), a(Mval, np.float64)
        Ccp, Cr, Cv = a(Ccolptr, np.int64), a(Crow, np.int32), a(Cval, np.float64)
        self._check(self.L.clipper_hip_set_sparse(self.h, m, _i64p(Mcp), _ip(Mr), _dp(Mv),
                                                  _i64p(Ccp), _ip(Cr), _dp(Cv)))

    def get_affinity_matrix(self):
        m = self.m
        M = np.zeros((m, m), order="F")
        self._check(self.L.clipper_hip_get_matrix(self.h, _dp(M), None))
        return M

    def get_constraint_matrix(self):
        m = self.m
        Cm = np.zeros((m, m), order="F")
        self._check(self.L.clipper_hip_get_matrix(self.h, None, _dp(Cm)))
        return Cm

    def matvec(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        yM, yC = np.zeros_like(x), np.zeros_like(x)
        self._check(self.L.clipper_hip_matvec(self.h, _dp(x), _dp(yM), _dp(yC)))
        return yM, yC

    # ---- solver ----------------------------------------------------------------------------
    def solve(self, u0):
        u0 = np.ascontiguousarray(u0, dtype=np.float64)
        n = self.m
        if n > 0 and u0.shape != (n,):
            raise ValueError(f"u0 must have shape ({n},)")
        u = np.zeros(max(n, 1))[:n]
        info = SolveInfo()
        self._check(self.L.clipper_hip_solve(self.h, _dp(u0), C.byref(self.params), _dp(u),
                                             C.byref(info)))
        nodes = np.zeros(max(info.num_nodes, 1), dtype=np.int32)
        k = self._check(self.L.clipper_hip_get_nodes(self.h, _ip(nodes), nodes.size))
        self.soln = Solution(t=info.seconds, ifinal=info.ifinal, nodes=nodes[:k].copy(), u0=u0,
                             u=u, score=info.score, d=info.d, n_passes=info.n_passes,
                             n_trials=info.n_trials)
        return self.soln

    def get_solution(self):
        return self.soln

    def get_selected_associations(self):
        k = len(self.soln.nodes)
        buf = np.zeros(2 * max(k, 1), dtype=np.int32)
        kk = self._check(self.L.clipper_hip_get_selected_associations(self.h, _ip(buf), max(k, 1)))
        if kk == 0:
            return np.zeros((0, 2), dtype=np.int32)
        return np.stack([buf[:kk], buf[kk:2 * kk]], axis=1)

    # ---- measurement ------------------------------------------------------------------------
    def densest_subgraph(self, S=None) -> np.ndarray:
        """dsd::solve(M_, S): exact densest subgraph of the current affinity matrix (all nodes, or
        restricted to the node list S)."""
        n = int(self.L.clipper_hip_num_associations(self.h))
        out = np.zeros(max(n, 1), dtype=np.int32)
        if S is None:
            k = self.L.clipper_hip_densest_subgraph(self.h, None, 0, _ip(out), len(out))
        else:
            Sa = np.ascontiguousarray(S, dtype=np.int32)
            k = self.L.clipper_hip_densest_subgraph(self.h, _ip(Sa), len(Sa), _ip(out), len(out))
        self._check(min(k, 0))
        return out[:k].copy()

    def max_clique(self, method: int = MC_EXACT, time_limit: float = 0.0, seed=None):
        """maxclique::solve on the consistency graph (C != 0): MC_EXACT (ROBIN*), MC_HEU or MC_KCORE (ROBIN).
        Returns (nodes ascending, MaxCliqueInfo); the nodes become the context's selection. time_limit in seconds
        (<= 0: none). seed: a list of distinct vertices the search starts from (clipper_hip_max_clique_seeded;
        "solution": the context's node list, e.g. the last solve's); with one the call returns
        (nodes, MaxCliqueInfo, MaxCliqueSeedInfo), and method may be MC_SEED_ONLY."""
        info = MaxCliqueInfo()
        sinfo = None
        if seed is None:
            self._check(self.L.clipper_hip_max_clique(self.h, int(method), float(time_limit), C.byref(info)))
        else:
            sinfo = MaxCliqueSeedInfo()
            if isinstance(seed, str):
                if seed != "solution":
                    raise ValueError('seed: a vertex list or "solution"')
                sp, ns = None, -1
            else:
                sa = np.ascontiguousarray(seed, dtype=np.int32).ravel()
                sp, ns = _ip(sa), int(sa.size)
            self._check(self.L.clipper_hip_max_clique_seeded(self.h, int(method), float(time_limit), sp, ns,
                                                             C.byref(info), C.byref(sinfo)))
        out = np.zeros(max(info.num_nodes, 1), dtype=np.int32)
        k = self.L.clipper_hip_get_nodes(self.h, _ip(out), len(out))
        self._check(min(k, 0))
        nodes = out[:k].copy()
        # clipper.cpp:92-96: the solution of a max-clique call
        self.soln = Solution(t=info.seconds, ifinal=0, nodes=nodes, u=np.zeros(self.m), score=-1.0)
        return (nodes, info) if sinfo is None else (nodes, info, sinfo)

    def sdp(self, params: SdpParams | None = None):
        """sdp::solve on the context's M and C (identity diagonals): CLIPPER::solveAsMSRCSDR on the device.
        Returns (nodes ascending, SdpResult); the nodes become the context's selection."""
        params = params if params is not None else SdpParams()
        n = int(self.m)
        X, Y = np.zeros((n, n)), np.zeros((n, n))
        lam, ev = np.zeros(n), np.zeros(n)
        info = SdpInfo()
        self._check(self.L.clipper_hip_sdp(self.h, C.byref(params), _dp(X), _dp(Y), _dp(lam), _dp(ev), C.byref(info)))
        out = np.zeros(max(info.num_nodes, 1), dtype=np.int32)
        k = self.L.clipper_hip_get_nodes(self.h, _ip(out), len(out))
        self._check(min(k, 0))
        nodes = out[:k].copy()
        # clipper.cpp:108-112: the solution of an SDP call
        self.soln = Solution(t=info.t_total, ifinal=0, nodes=nodes, u=np.zeros(self.m), score=-1.0)
        return nodes, _sdp_result(n, X, Y, lam, ev, nodes, info)

    def mc_launches(self) -> int:
        """Test infrastructure: the kernel launches of this context's last max_clique or core_numbers call."""
        return int(self._check(self.L.clipper_hip_debug_mc_launches(self.h)))

    def core_numbers(self) -> np.ndarray:
        """The core number of every vertex of the consistency graph."""
        n = int(self.L.clipper_hip_num_associations(self.h))
        out = np.zeros(max(n, 1), dtype=np.int32)
        self._check(self.L.clipper_hip_core_numbers(self.h, _ip(out)))
        return out[:n].copy()

    def set_window(self, window: int):
        """Line-search window (0 = automatic, 1 | 4 | 6 | 8); effective from the next build."""
        self._check(self.L.clipper_hip_set_window(self.h, int(window)))

    @property
    def window(self) -> int:
        return int(self.L.clipper_hip_window(self.h))

    def set_resident(self, mode: int):
        """0 = the resident (one-launch) solver where the slices fit on chip, 1 = never."""
        self._check(self.L.clipper_hip_set_resident(self.h, int(mode)))

    @property
    def last_solver(self) -> int:
        """What the last solve ran on: 0 = streaming launches, 1 = resident."""
        return int(self.L.clipper_hip_last_solver(self.h))

    def set_row_view(self, mode: int):
        """0 = build row views of M[live rows, :] during a solve where that pays, 1 = never."""
        self._check(self.L.clipper_hip_set_row_view(self.h, int(mode)))

    def set_subproblem(self, mode: int):
        """0 = hand a solve over to the live sub-problem (the associations that can still be selected) where that is
        provably exact and pays, 1 = never."""
        self._check(self.L.clipper_hip_set_subproblem(self.h, int(mode)))

    def view_matvec(self, rows, x):
        """(M_off[:, rows] x[rows], C_off[:, rows] x[rows]) through a row view built for `rows`."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        x = np.ascontiguousarray(x, dtype=np.float64)
        yM, yC = np.zeros(self.m), np.zeros(self.m)
        self._check(self.L.clipper_hip_view_matvec(self.h, _ip(rows), rows.size, _dp(x), _dp(yM), _dp(yC)))
        return yM, yC

    def _sub_selection(self, call, with_rows):
        cap = (self.m + 63) // 64 * 64
        cnt, colmap, pos, rows = (np.full(cap, -7, dtype=np.int32) for _ in range(4))
        flags = np.full(cap, 7, dtype=np.uint8)
        rec = SubSelection()
        self._check(call(cap, _ip(cnt), flags.ctypes.data_as(C.POINTER(C.c_uint8)), _ip(colmap), _ip(pos), _ip(rows), C.byref(rec)))
        mp = int(rec.mp)
        out = dict(cnt=cnt[:mp].copy(), flags=flags[:mp].copy(), colmap=colmap[:rec.nS].copy(), pos=pos[:mp].copy(),
                   mp=mp, nS=int(rec.nS), ncol=int(rec.ncol), n0=int(rec.n0), entries=int(rec.entries), s=float(rec.s),
                   nrows=int(rec.nrows))
        if with_rows:
            out.update(rows=rows[:rec.nrows].copy(), N_used=float(rec.N_used), built=bool(rec.built), entered=bool(rec.entered))
        return out

    def debug_sub_select(self, rows, s: float) -> dict:
        """Test infrastructure: the selection of the live sub-problem alone, on a row view built for `rows` (ascending)
        with sum(u) = s: cnt, flags, pos over [0, mp), colmap over [0, nS), and the record's nS, ncol, n0, entries."""
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        return self._sub_selection(lambda cap, cnt, flags, colmap, pos, _rows, rec: self.L.clipper_hip_debug_sub_select(
            self.h, _ip(rows), rows.size, float(s), cap, cnt, flags, colmap, pos, rec), False)

    def debug_sub_last(self) -> dict:
        """Test infrastructure: the last selection of the last solve — the same, and the view's rows at that moment, the
        sum(u) the kernel read, N as handed to the decision, whether the sub-problem was built and entered."""
        return self._sub_selection(lambda cap, *a: self.L.clipper_hip_debug_sub_last(self.h, cap, *a), True)

    def view_stats(self) -> ViewStats:
        t = ViewStats()
        self._check(self.L.clipper_hip_get_view_stats(self.h, C.byref(t)))
        return t

    @property
    def storage_in_use(self) -> int:
        return int(self.L.clipper_hip_storage_in_use(self.h))

    def set_profiling(self, on):
        """False / True, or 2: also HIP events around the launches of the resident solver on a view."""
        self._check(self.L.clipper_hip_set_profiling(self.h, int(on)))

    def timings(self) -> Timings:
        t = Timings()
        self._check(self.L.clipper_hip_get_timings(self.h, C.byref(t)))
        return t

    def bench_matvec(self, reps: int = 20) -> float:
        us = C.c_double()
        self._check(self.L.clipper_hip_bench_matvec(self.h, reps, C.byref(us)))
        return us.value

    def comm_init_callback(self, allgather):
        """exchange through `allgather(block: np.ndarray[float64]) -> np.ndarray` (the blocks of all
        ranks, rank order, concatenated) instead of RCCL — e.g. a torch.distributed gloo all-gather"""
        def thunk(user, send, recv, nbytes):
            try:
                n = nbytes // 8
                blk = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_double)), shape=(n,))
                out = np.ascontiguousarray(allgather(blk.copy()), dtype=np.float64)
                np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_double)), shape=(out.size,))[:] = out
                return 0
            except Exception:      # never unwind through the C frames
                import traceback
                traceback.print_exc()
                return 1
        self._xchg = ALLGATHER_FN(thunk)   # keep the trampoline alive
        self._check(self.L.clipper_hip_comm_init_callback(self.h, self._xchg, None))

    def debug_stamps(self):
        """per workgroup of the last pass launch: (start, decision done, end, info); needs
        CLIPPER_HIP_STAMPS=1 in the environment when the context is created"""
        rows = 16384 if os.environ.get("CLIPPER_HIP_STAMPS") == "2" else 4096
        out = np.zeros(rows * 4, dtype=np.int64)
        self._check(self.L.clipper_hip_debug_stamps(self.h, out.ctypes.data_as(C.POINTER(C.c_int64)), out.size))
        return out.reshape(rows, 4)

    def device_info(self):
        name = C.create_string_buffer(64)
        cus, hbm = C.c_int(), C.c_int64()
        self._check(self.L.clipper_hip_device_info(self.h, name, C.byref(cus), C.byref(hbm)))
        return name.value.decode(), cus.value, hbm.value


# ---- host-side neighbours of the path, through the C ABI (no device needed) ----------------------

def _status(rc):
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    return rc


def read_ply_xyz(path: str) -> np.ndarray:
    """utils::read_ply: vertex positions as a 3 x n float64 array (one datum per column)"""
    L = load_library()
    n = _status(L.clipper_hip_read_ply_xyz(path.encode(), None, 0))
    pts = np.zeros((n, 3), dtype=np.float64)
    _status(L.clipper_hip_read_ply_xyz(path.encode(), _dp(pts), n))
    return np.ascontiguousarray(pts.T)


def generate_synthetic_correspondences(n0: int, n1: int, Agood, m: int, rho: float, seed: int):
    """utils::generate_synthetic_correspondences -> (A m x 2, Agt ni x 2)"""
    L = load_library()
    Agood = np.asarray(Agood, dtype=np.int32).reshape(-1, 2)
    p = Agood.shape[0]
    gcm = np.ascontiguousarray(Agood.T).reshape(-1)
    A = np.zeros(2 * m, dtype=np.int32)
    Agt = np.zeros(2 * m, dtype=np.int32)
    ni = C.c_int64()
    _status(L.clipper_hip_generate_synthetic_correspondences(n0, n1, _ip(gcm), p, m, rho, seed, _ip(A), _ip(Agt),
                                                             C.byref(ni)))
    k = ni.value
    return A.reshape(2, m).T.copy(), Agt[:2 * k].reshape(2, k).T.copy()


def precision_recall(A, Agt):
    """utils::get_precision_recall"""
    L = load_library()
    A = np.asarray(A, dtype=np.int32).reshape(-1, 2)
    Agt = np.asarray(Agt, dtype=np.int32).reshape(-1, 2)
    a, g = np.ascontiguousarray(A.T).reshape(-1), np.ascontiguousarray(Agt.T).reshape(-1)
    p, r = C.c_double(), C.c_double()
    _status(L.clipper_hip_precision_recall(_ip(a) if a.size else None, A.shape[0], _ip(g) if g.size else None,
                                           Agt.shape[0], C.byref(p), C.byref(r)))
    return p.value, r.value


def estimate_rigid_transform(D1, D2, A) -> np.ndarray:
    """4 x 4 T with D2[:, A[i,1]] ~ R D1[:, A[i,0]] + t (D1, D2: 3 x n)"""
    L = load_library()
    D1, D2 = _f64_colmajor(D1), _f64_colmajor(D2)
    A = np.asarray(A, dtype=np.int32).reshape(-1, 2)
    a = np.ascontiguousarray(A.T).reshape(-1)
    T = np.zeros(16, dtype=np.float64)
    _status(L.clipper_hip_estimate_rigid_transform(_dp(D1), D1.shape[1], _dp(D2), D2.shape[1], _ip(a), A.shape[0],
                                                   _dp(T)))
    return T.reshape(4, 4).T.copy()


def ransac_correspondences(D1, D2, A, max_distance, n_sample=3, edge_similarity=0.9, max_hypotheses=100000,
                           confidence=0.999, seed=0, refine_iterations=1, hypotheses_per_round=4096, device=0):
    """clipper_hip_ransac_correspondences: the rigid transform most of the associations A (m x 2) between D1 and D2
    (3 x n, columns = points, the layouts of estimate_rigid_transform) agree on, by RANSAC on the device. Returns
    (T 4 x 4, info): info.status is RANSAC_*, info.inliers the boolean mask of the associations within max_distance
    under T."""
    L = load_library()
    D1, D2 = _f64_colmajor(D1), _f64_colmajor(D2)
    if D1.ndim != 2 or D1.shape[0] != 3 or D2.ndim != 2 or D2.shape[0] != 3:
        raise ValueError("D1 and D2 must be 3 x n")
    A = np.asarray(A, dtype=np.int32).reshape(-1, 2)
    a = np.ascontiguousarray(A.T).reshape(-1)
    prm = RansacParams(max_distance, n_sample, edge_similarity, max_hypotheses, confidence, seed, refine_iterations,
                       hypotheses_per_round)
    T = np.zeros(16, dtype=np.float64)
    mask = np.zeros(max(A.shape[0], 1), dtype=np.uint8)
    info = RansacInfo()
    _status(L.clipper_hip_ransac_correspondences(device, _dp(D1), D1.shape[1], _dp(D2), D2.shape[1], _ip(a), A.shape[0],
                                                 C.byref(prm), _dp(T), mask.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                 C.byref(info)))
    info.inliers = mask[:A.shape[0]].astype(bool)
    return T.reshape(4, 4).T.copy(), info


def ransac_needed(count: int, m: int, n_sample: int = 3, confidence: float = 0.999) -> int:
    """clipper_hip_ransac_needed: the hypotheses after which RANSAC stops CONVERGED with `count` inliers among m"""
    return int(_status(load_library().clipper_hip_ransac_needed(count, m, n_sample, confidence)))


def device_count() -> int:
    return int(load_library().clipper_hip_device_count())


def debug_occupy(device: int, workgroups: int, lds_bytes: int, milliseconds: float) -> None:
    """Test infrastructure: `workgroups` wave slots with `lds_bytes` of LDS each are held for `milliseconds`
    (blocks until the kernel is over): another tenant on the device."""
    rc = load_library().clipper_hip_debug_occupy(device, workgroups, lds_bytes, float(milliseconds))
    if rc < 0:
        raise ClipperError(f"clipper_hip_debug_occupy: {rc} ({_last_error()})")


def debug_mc_budgets(peel: int = 0, wave: int = 0) -> None:
    """Test infrastructure: the row-word budgets of the maximum-clique launches (peel; HEU / EXACT wave), process-wide;
    values <= 0 restore the library's constants. A smaller budget means more launches and the same results."""
    rc = load_library().clipper_hip_debug_mc_budgets(int(peel), int(wave))
    if rc < 0:
        raise ClipperError(f"clipper_hip_debug_mc_budgets: {rc} ({_last_error()})")


def debug_sub_min_m(min_m: int = 0) -> None:
    """Test infrastructure: the size threshold of the live sub-problem, process-wide; a value <= 0 restores the initial
    one (12 000, or CLIPPER_HIP_SUBPROBLEM_MIN_M as the process started)."""
    rc = load_library().clipper_hip_debug_sub_min_m(int(min_m))
    if rc < 0:
        raise ClipperError(f"clipper_hip_debug_sub_min_m: {rc} ({_last_error()})")


def debug_live_resources() -> dict:
    """Test infrastructure: what the library holds in this process right now (device buffers, their bytes, pinned
    buffers, events) and the allocations and event creations it has made so far."""
    out = (C.c_int64 * 5)()
    rc = load_library().clipper_hip_debug_live_resources(out)
    if rc < 0:
        raise ClipperError(f"clipper_hip_debug_live_resources: {rc} ({_last_error()})")
    return dict(zip(("device_buffers", "device_bytes", "pinned_buffers", "events", "allocations"), map(int, out)))


def _last_error() -> str:
    L = load_library()
    return (L.clipper_hip_last_error() or b"").decode()


def knn(P0, P1, knn: int, device: int = 0):
    """k nearest neighbours in P1 (d x n1) of every point of P0 (d x n0), columns = points as
    `clipper::Data`. Returns (idx n0 x knn int32, sqd n0 x knn)."""
    L = load_library()
    P0c, P1c = _f64_colmajor(P0), _f64_colmajor(P1)
    d, n0 = P0c.shape
    n1 = P1c.shape[1]
    idx = np.zeros((n0, knn), dtype=np.int32)
    sqd = np.zeros((n0, knn), dtype=np.float64)
    rc = L.clipper_hip_knn(device, _dp(P0c), n0, _dp(P1c), n1, d, knn, _ip(idx), _dp(sqd))
    if rc != 0:
        raise RuntimeError(f"clipper_hip error {rc}: {_last_error()}")
    return idx, sqd


def knn_set_search(mode: int) -> int:
    """clipper_hip_knn_set_search: the process-wide route of the d = 3 nearest-neighbour search behind knn,
    distance_based_correspondences, estimate_normals, compute_fpfh and fpfh_from_points (KNN_BRUTE, the default;
    KNN_GRID; KNN_AUTO). Returns the previous mode. Every route returns the same lists, bit for bit; d = 2 searches
    run brute force in every mode."""
    prev = load_library().clipper_hip_knn_set_search(int(mode))
    if prev < 0:
        raise ClipperError(f"clipper_hip error {prev}: {_last_error()}")
    return prev


def knn_search() -> int:
    """clipper_hip_knn_search: the current mode."""
    return load_library().clipper_hip_knn_search()


def knn_last_search() -> KnnStats:
    """clipper_hip_knn_last_search: the route the calling thread's last search took, the grid's cells per axis, the
    number of queries and the candidates visited (0 for brute force); route is -1 before the first search.
    auto_min_n: the searched-cloud size from which KNN_AUTO takes the grid; kernels_ms: the device time between two
    events around the search's kernels."""
    st = KnnStats()
    rc = load_library().clipper_hip_knn_last_search(C.byref(st))
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    return st


def sdp_set_route(route: int) -> int:
    """clipper_hip_sdp_set_route: the process-wide route of the sdp entry points (SDP_ROUTE_*); returns the previous
    setting. SDP_ROUTE_AUTO and SDP_ROUTE_WIDE open n <= SDP_WIDE_MAX_N through the wide route."""
    prev = load_library().clipper_hip_sdp_set_route(int(route))
    if prev < 0:
        raise ClipperError(f"clipper_hip error {prev}: {_last_error()}")
    return prev


def sdp_route() -> int:
    """clipper_hip_sdp_route: the current setting."""
    return load_library().clipper_hip_sdp_route()


def sdp_solve(M, C_, params: SdpParams | None = None, device: int = 0) -> SdpResult:
    """sdp::solve(M, C, params) on the device: n x n M and C (n <= 128, or <= 1024 under sdp_set_route), only their
    lower triangles read."""
    L = load_library()
    Mc = np.asfortranarray(np.asarray(M, dtype=np.float64))
    Cc = np.asfortranarray(np.asarray(C_, dtype=np.float64))
    n = Mc.shape[0]
    if Mc.shape != (n, n) or Cc.shape != (n, n):
        raise ValueError("M and C must be square and of the same size")
    params = params if params is not None else SdpParams()
    X, Y = np.zeros((n, n)), np.zeros((n, n))
    lam, ev = np.zeros(n), np.zeros(n)
    nodes = np.zeros(max(n, 1), dtype=np.int32)
    info = SdpInfo()
    k = L.clipper_hip_sdp_solve(device, _dp(Mc), _dp(Cc), n, C.byref(params), _dp(X), _dp(Y), _dp(lam), _dp(ev),
                                _ip(nodes), C.byref(info))
    if k < 0:
        raise ClipperError(f"clipper_hip error {k}: {_last_error()}")
    return _sdp_result(n, X, Y, lam, ev, nodes[:k].copy(), info)


def sdp_solve_batch(problems, params: SdpParams | None = None, device: int = 0, want_xy: bool = True) -> list:
    """sdp::solve on every (M, C) of `problems` in one call, one workgroup per problem (clipper_hip_sdp_solve_batch):
    per problem the SdpResult of sdp_solve on it alone, bit for bit (the times excepted: they are the call's).
    want_xy = False leaves X and Y on the device (empty arrays in the results)."""
    L = load_library()
    params = params if params is not None else SdpParams()
    count = len(problems)
    arr = (SdpProblem * max(count, 1))()
    keep = []
    for i, pr in enumerate(problems):
        if len(pr) != 2:
            raise ValueError(f"problem {i}: expected (M, C)")
        Mc = np.asfortranarray(np.asarray(pr[0], dtype=np.float64))
        Cc = np.asfortranarray(np.asarray(pr[1], dtype=np.float64))
        n = Mc.shape[0] if Mc.ndim == 2 else -1
        if Mc.ndim != 2 or Mc.shape != (n, n) or Cc.shape != (n, n):
            raise ValueError(f"problem {i}: M and C must be square and of the same size")
        X, Y = (np.zeros((n, n)), np.zeros((n, n))) if want_xy else (np.zeros((0, 0)), np.zeros((0, 0)))
        lam, ev, nodes = np.zeros(n), np.zeros(n), np.zeros(max(n, 1), dtype=np.int32)
        keep.append((Mc, Cc, X, Y, lam, ev, nodes))
        arr[i] = SdpProblem(_dp(Mc), _dp(Cc), n, _dp(X) if want_xy else None, _dp(Y) if want_xy else None, _dp(lam),
                            _dp(ev), _ip(nodes))
    infos = (SdpInfo * max(count, 1))()
    rc = L.clipper_hip_sdp_solve_batch(device, arr, count, C.byref(params), infos)
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    out = []
    for i, (Mc, Cc, X, Y, lam, ev, nodes) in enumerate(keep):
        info = SdpInfo.from_buffer_copy(infos[i])
        out.append(_sdp_result(Mc.shape[0], X, Y, lam, ev, nodes[:info.num_nodes].copy(), info))
    return out


def distance_based_correspondences(P0, P1, knn: int, radius: float, enforce_1to1: bool,
                                   device: int = 0) -> np.ndarray:
    """utils::distance_based_correspondences of the reference benchmark (bm_utils.cpp:147-232) on
    the device. P0: d x n0, P1: d x n1 (columns = points). Returns the associations n x 2."""
    L = load_library()
    P0c, P1c = _f64_colmajor(P0), _f64_colmajor(P1)
    d, n0 = P0c.shape
    n1 = P1c.shape[1]
    cap = n0 * knn
    buf = np.zeros(2 * max(cap, 1), dtype=np.int32)
    n = L.clipper_hip_distance_based_correspondences(device, _dp(P0c), n0, _dp(P1c), n1, d, knn,
                                                     float(radius), int(bool(enforce_1to1)),
                                                     _ip(buf), cap)
    if n < 0:
        raise RuntimeError(f"clipper_hip error {n}: {_last_error()}")
    n = int(n)
    return np.stack([buf[:n], buf[n:2 * n]], axis=1).astype(np.int32)


def match_descriptors(F0, F1, knn: int = 1, mutual: bool = True, ratio: float = 0.0, max_sqdist: float = 0.0,
                      device: int = 0, return_lists: bool = False):
    """clipper_hip_match_descriptors: putative associations from feature descriptors on the device. F0: d x n0,
    F1: d x n1 (columns = descriptors, as `clipper::Data`), 1 <= d <= 64. Every point of F0 is matched to its knn
    nearest descriptors of F1; `mutual` keeps a pair only if it is also found the other way round, `ratio` (0 = off,
    needs knn == 1) is Lowe's test sqd_0 < ratio^2 sqd_1, `max_sqdist` (<= 0 = off) bounds the squared distance.
    Returns (A n x 2 int32, sqd n), and with return_lists also the forward lists (idx n0 x knn int32, sqd n0 x knn)
    before the filters."""
    L = load_library()
    F0c, F1c = _f64_colmajor(F0), _f64_colmajor(F1)
    if F0c.ndim != 2 or F1c.ndim != 2 or F0c.shape[0] != F1c.shape[0]:
        raise ValueError("F0 and F1 must be d x n0 and d x n1")
    d, n0 = F0c.shape
    n1 = F1c.shape[1]
    prm = MatchParams(int(knn), int(bool(mutual)), float(ratio), float(max_sqdist))
    cap = max(n0 * max(int(knn), 0), 0)
    buf = np.zeros(2 * max(cap, 1), dtype=np.int32)
    sqd = np.zeros(max(cap, 1), dtype=np.float64)
    idx = np.zeros((n0, max(int(knn), 0)), dtype=np.int32) if return_lists else None
    lsq = np.zeros((n0, max(int(knn), 0)), dtype=np.float64) if return_lists else None
    n = L.clipper_hip_match_descriptors(device, _dp(F0c), n0, _dp(F1c), n1, d, C.byref(prm), _ip(buf), _dp(sqd), cap,
                                        _ip(idx) if return_lists else None, _dp(lsq) if return_lists else None)
    if n < 0:
        raise ClipperError(f"clipper_hip error {n}: {_last_error()}")
    n = int(n)
    A = np.stack([buf[:n], buf[n:2 * n]], axis=1).astype(np.int32)
    return (A, sqd[:n].copy(), idx, lsq) if return_lists else (A, sqd[:n].copy())


def _cloud(P, what="P"):
    Pc = _f64_colmajor(P)
    if Pc.ndim != 2 or Pc.shape[0] != 3:
        raise ValueError(f"{what} must be 3 x n")
    return Pc


def _viewpoint(viewpoint):
    if viewpoint is None:
        return None, None
    v = np.ascontiguousarray(np.asarray(viewpoint, dtype=np.float64).reshape(-1))
    if v.size != 3:
        raise ValueError("viewpoint must have 3 coordinates")
    return v, _dp(v)


def estimate_normals(P, knn: int = 16, radius: float = 0.0, viewpoint=None, device: int = 0, return_counts: bool = False):
    """clipper_hip_estimate_normals: unit surface normals of the cloud P (3 x n, columns = points as `clipper::Data`) on
    the device. A point's neighbourhood is the first knn (3..32) entries of its nearest-neighbour list in P, itself
    included, with radius > 0 only those within it; fewer than 3 neighbours give (0, 0, 1). The sign points towards
    `viewpoint` (3 numbers), or without one makes the largest component positive. Returns N (3 x n), with
    return_counts also the neighbours kept per point (n int32)."""
    L = load_library()
    Pc = _cloud(P)
    n = Pc.shape[1]
    nb = Neighborhood(knn, radius)
    v, vptr = _viewpoint(viewpoint)
    N = np.zeros((3, n), dtype=np.float64, order="F")
    cnt = np.zeros(max(n, 1), dtype=np.int32)
    rc = L.clipper_hip_estimate_normals(device, _dp(Pc), n, C.byref(nb), vptr, _dp(N), _ip(cnt))
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    return (N, cnt[:n]) if return_counts else N


def compute_fpfh(P, N, knn: int = 32, radius: float = 0.0, device: int = 0, return_spfh: bool = False):
    """clipper_hip_compute_fpfh: FPFH descriptors of the cloud P with unit normals N (both 3 x n) on the device, over
    the neighbourhood (knn, radius) as estimate_normals defines it. Returns F (33 x n, columns = descriptors: what
    match_descriptors takes), with return_spfh also (SPFH 33 x n, the neighbours kept per point n int32)."""
    L = load_library()
    Pc, Nc = _cloud(P), _cloud(N, "N")
    n = Pc.shape[1]
    if Nc.shape[1] != n:
        raise ValueError("P and N must hold the same number of points")
    nb = Neighborhood(knn, radius)
    F = np.zeros((FPFH_DIM, n), dtype=np.float64, order="F")
    S = np.zeros((FPFH_DIM, n), dtype=np.float64, order="F") if return_spfh else None
    cnt = np.zeros(max(n, 1), dtype=np.int32) if return_spfh else None
    rc = L.clipper_hip_compute_fpfh(device, _dp(Pc), _dp(Nc), n, C.byref(nb), _dp(F), _dp(S) if return_spfh else None,
                                    _ip(cnt) if return_spfh else None)
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    return (F, S, cnt[:n]) if return_spfh else F


def fpfh_from_points(P, normal_knn: int = 16, normal_radius: float = 0.0, viewpoint=None, knn: int = 32,
                     radius: float = 0.0, device: int = 0):
    """clipper_hip_fpfh_from_points: estimate_normals and compute_fpfh in one call (one upload, one search at the
    larger knn, the normals stay on the device). Returns (F 33 x n, N 3 x n): the two calls' bits."""
    L = load_library()
    Pc = _cloud(P)
    n = Pc.shape[1]
    nnb, fnb = Neighborhood(normal_knn, normal_radius), Neighborhood(knn, radius)
    v, vptr = _viewpoint(viewpoint)
    F = np.zeros((FPFH_DIM, n), dtype=np.float64, order="F")
    N = np.zeros((3, n), dtype=np.float64, order="F")
    rc = L.clipper_hip_fpfh_from_points(device, _dp(Pc), n, C.byref(nnb), vptr, C.byref(fnb), _dp(F), _dp(N))
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    return F, N


def _transform_arg(T, name):
    """a 4 x 4 transform as the column-major 16 doubles of the C ABI (None: NULL, the identity)"""
    if T is None:
        return None, None
    T = np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{name} must be 4 x 4")
    t = np.ascontiguousarray(T.T).reshape(-1)
    return t, _dp(t)


def _icp_call(fn, lead, T_init, method, max_distance, max_iterations, rel_fitness, rel_rmse, robust=None, robust_slots=None):
    """One ICP call of the C ABI. fn: the C function; lead: its arguments in front of T_init (the device and the clouds,
    or two handles; a pointer made by _dp keeps its array alive); robust: (loss, scale, trim) or None; robust_slots:
    whether fn takes the robust settings and their info at all (default: as robust is given; clipper_hip_cloud_icp takes
    NULL for both). Returns (T 4 x 4, info) with info.history attached, and for a robust call within, weight_sum and
    trim_sqd of clipper_icp_robust_info_t."""
    t0, t0p = _transform_arg(T_init, "T_init")
    prm = IcpParams(method, max_distance, max_iterations, rel_fitness, rel_rmse)
    rb, rinfo = (IcpRobust(*robust), IcpRobustInfo()) if robust is not None else (None, None)
    T = np.zeros(16, dtype=np.float64)
    info = IcpInfo()
    hist = np.zeros((max(int(max_iterations), 0) + 1, 3), dtype=np.float64)
    rbp, rip = (C.byref(rb), C.byref(rinfo)) if robust is not None else (None, None)
    slots = (robust is not None) if robust_slots is None else robust_slots
    mid, tail = ((rbp,), (rip,)) if slots else ((), ())
    rc = fn(*lead, t0p, C.byref(prm), *mid, _dp(T), C.byref(info), *tail, _dp(hist))
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    info.history = hist[:info.iterations + 1].copy()
    if robust is not None:
        info.within, info.weight_sum, info.trim_sqd = int(rinfo.within), float(rinfo.weight_sum), float(rinfo.trim_sqd)
    return T.reshape(4, 4).T.copy(), info


def _icp_clouds(device, P_src, P_tgt, N_tgt):
    """the leading arguments of clipper_hip_icp and clipper_hip_icp_robust"""
    Ps, Pt = _cloud(P_src, "P_src"), _cloud(P_tgt, "P_tgt")
    Nt = None if N_tgt is None else _cloud(N_tgt, "N_tgt")
    if Nt is not None and Nt.shape[1] != Pt.shape[1]:
        raise ValueError("P_tgt and N_tgt must hold the same number of points")
    return device, _dp(Ps), Ps.shape[1], _dp(Pt), None if Nt is None else _dp(Nt), Pt.shape[1]


def _gicp_clouds(device, P_src, C_src, P_tgt, C_tgt):
    """the leading arguments of clipper_hip_icp_generalized and clipper_hip_icp_generalized_robust"""
    Ps, Pt = _cloud(P_src, "P_src"), _cloud(P_tgt, "P_tgt")
    Cs, Ct = _covariances(C_src, "C_src", Ps.shape[1]), _covariances(C_tgt, "C_tgt", Pt.shape[1])
    return device, _dp(Ps), _dp(Cs), Ps.shape[1], _dp(Pt), _dp(Ct), Pt.shape[1]


def icp(P_src, P_tgt, T_init=None, method: int = ICP_POINT_TO_POINT, N_tgt=None, max_distance: float = 0.0,
        max_iterations: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, device: int = 0):
    """clipper_hip_icp: refine the alignment T_init (4 x 4, None = identity) of the source cloud P_src onto the target
    P_tgt (both 3 x n, columns = points as `clipper::Data`) on the device. method: ICP_POINT_TO_POINT, or
    ICP_POINT_TO_PLANE over the target's unit normals N_tgt (3 x n_tgt). A correspondence is the nearest target point
    of a moved source point, an inlier within max_distance. Returns (T 4 x 4, info): info.status is ICP_*,
    info.history the (iterations + 1) x 3 rows of (count, fitness, rmse), one per evaluated T."""
    return _icp_call(load_library().clipper_hip_icp, _icp_clouds(device, P_src, P_tgt, N_tgt), T_init, method, max_distance,
                     max_iterations, rel_fitness, rel_rmse)


def _covariances(Cv, name, n):
    """per-point covariances as the 6 x n column-major array of the C ABI (each point's six numbers contiguous)"""
    Cv = np.asarray(Cv, dtype=np.float64)
    if Cv.ndim != 2 or Cv.shape[0] != 6:
        raise ValueError(f"{name} must be 6 x n (xx, xy, xz, yy, yz, zz per column)")
    if Cv.shape[1] != n:
        raise ValueError(f"{name} must hold one matrix per point")
    return np.asfortranarray(Cv)


def estimate_covariances(P, knn: int = 20, radius: float = 0.0, epsilon: float = 1e-3, device: int = 0,
                         return_counts: bool = False):
    """clipper_hip_estimate_covariances: the per-point covariances of generalized ICP for the cloud P (3 x n, columns =
    points) on the device: I - (1 - epsilon) nv nv^T (eigenvalues epsilon, 1, 1) with nv the normal estimate_normals
    finds over the same neighbourhood (knn 3..32 the point included, radius > 0 keeps only those within it); the
    identity below 3 neighbours. Returns C (6 x n: xx, xy, xz, yy, yz, zz per column), with return_counts also the
    neighbours kept per point (n int32)."""
    L = load_library()
    Pc = _cloud(P)
    n = Pc.shape[1]
    nb = Neighborhood(knn, radius)
    Cv = np.zeros((6, n), dtype=np.float64, order="F")
    cnt = np.zeros(max(n, 1), dtype=np.int32)
    rc = L.clipper_hip_estimate_covariances(device, _dp(Pc), n, C.byref(nb), float(epsilon), _dp(Cv), _ip(cnt))
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    return (Cv, cnt[:n]) if return_counts else Cv


def icp_generalized(P_src, C_src, P_tgt, C_tgt, T_init=None, max_distance: float = 0.0, max_iterations: int = 30,
                    rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, device: int = 0):
    """clipper_hip_icp_generalized: icp with the plane-to-plane metric of generalized ICP over the per-point
    covariances C_src (6 x n_src) and C_tgt (6 x n_tgt), e.g. estimate_covariances' (positive definite, else refused).
    P_src, P_tgt: 3 x n, columns = points. Returns (T 4 x 4, info) as icp does."""
    return _icp_call(load_library().clipper_hip_icp_generalized, _gicp_clouds(device, P_src, C_src, P_tgt, C_tgt), T_init,
                     ICP_GENERALIZED, max_distance, max_iterations, rel_fitness, rel_rmse)


def icp_robust(P_src, P_tgt, T_init=None, method: int = ICP_POINT_TO_POINT, N_tgt=None, max_distance: float = 0.0,
               max_iterations: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, loss: int = ICP_LOSS_NONE,
               scale: float = 0.0, trim: float = 1.0, device: int = 0):
    """clipper_hip_icp_robust: icp with a robust loss (ICP_LOSS_*, `scale` a distance) weighing every pair by its
    residual, and / or trimming: each iteration keeps the fraction `trim` of the points within max_distance with the
    smallest distances (ties at the threshold all kept). count, fitness, rmse and the history are over the kept points.
    Returns (T 4 x 4, info) as icp does, info also carrying within, weight_sum and trim_sqd of the last row."""
    return _icp_call(load_library().clipper_hip_icp_robust, _icp_clouds(device, P_src, P_tgt, N_tgt), T_init, method,
                     max_distance, max_iterations, rel_fitness, rel_rmse, (loss, scale, trim))


def icp_generalized_robust(P_src, C_src, P_tgt, C_tgt, T_init=None, max_distance: float = 0.0, max_iterations: int = 30,
                           rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, loss: int = ICP_LOSS_NONE, scale: float = 0.0,
                           trim: float = 1.0, device: int = 0):
    """clipper_hip_icp_generalized_robust: icp_generalized with icp_robust's loss and trimming; the residual a loss
    weighs is d^T M d of the pair. Returns (T 4 x 4, info) as icp_robust does."""
    return _icp_call(load_library().clipper_hip_icp_generalized_robust, _gicp_clouds(device, P_src, C_src, P_tgt, C_tgt), T_init,
                     ICP_GENERALIZED, max_distance, max_iterations, rel_fitness, rel_rmse, (loss, scale, trim))


def _evaluate_call(fn, lead, n_src, T, max_distance, return_correspondences):
    """One evaluation of a registration by the C ABI: fn and its arguments in front of T as _icp_call's. Returns
    (fitness, inlier_rmse, count), with return_correspondences also the n_src correspondences."""
    t, tp = _transform_arg(T, "T")
    fit, rmse, cnt = C.c_double(), C.c_double(), C.c_int64()
    corr = np.zeros(max(n_src, 1), dtype=np.int32) if return_correspondences else None
    rc = fn(*lead, tp, float(max_distance), C.byref(fit), C.byref(rmse), C.byref(cnt),
            _ip(corr) if return_correspondences else None)
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    out = (fit.value, rmse.value, cnt.value)
    return out + (corr[:n_src],) if return_correspondences else out


def evaluate_registration(P_src, P_tgt, T=None, max_distance: float = 0.0, device: int = 0, return_correspondences: bool = False):
    """clipper_hip_evaluate_registration: (fitness, inlier_rmse, count) of the alignment T (4 x 4, None = identity) of
    P_src onto P_tgt (3 x n), as iteration 0 of icp computes them; with return_correspondences also the target index
    of every source point's correspondence (n_src int32, -1 = no inlier)."""
    L = load_library()
    Ps, Pt = _cloud(P_src, "P_src"), _cloud(P_tgt, "P_tgt")
    return _evaluate_call(L.clipper_hip_evaluate_registration, (device, _dp(Ps), Ps.shape[1], _dp(Pt), Pt.shape[1]), Ps.shape[1],
                          T, max_distance, return_correspondences)


def voxel_down_sample(P, voxel_size: float, N=None, device: int = 0, return_counts: bool = False,
                      return_trace: bool = False, return_info: bool = False):
    """clipper_hip_voxel_downsample: one point per occupied voxel of edge voxel_size of the cloud P (3 x n, columns =
    points as `clipper::Data`), on the device: the centroid of the voxel's points, in ascending cell number
    (lexicographic in z, y, x; the grid's origin is the cloud's minimum corner). With normals N (3 x n) also the
    normalised sum of each voxel's normals, (0, 0, 1) where they cancel. Returns P_out (3 x n_out), then in this order
    N_out (3 x n_out, when N is given), the members per voxel (n_out int32, with return_counts), for every input point
    its output column (n int32, with return_trace) and the VoxelInfo (with return_info); a tuple when more than one.
    The result is a function of the inputs alone: tests/voxel_model.py reproduces its bits."""
    L = load_library()
    Pc = _cloud(P)
    n = Pc.shape[1]
    Nc = None if N is None else _cloud(N, "N")
    if Nc is not None and Nc.shape[1] != n:
        raise ValueError("P and N must hold the same number of points")
    Po = np.zeros((3, max(n, 1)), dtype=np.float64, order="F")
    No = np.zeros((3, max(n, 1)), dtype=np.float64, order="F") if Nc is not None else None
    cnt = np.zeros(max(n, 1), dtype=np.int32) if return_counts else None
    trace = np.zeros(max(n, 1), dtype=np.int32) if return_trace else None
    n_out, info = C.c_int64(0), VoxelInfo()
    rc = L.clipper_hip_voxel_downsample(device, _dp(Pc), None if Nc is None else _dp(Nc), n, float(voxel_size), _dp(Po),
                                        None if No is None else _dp(No), None if cnt is None else _ip(cnt),
                                        None if trace is None else _ip(trace), C.byref(n_out), C.byref(info))
    if rc < 0:
        raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
    m = int(n_out.value)
    out = [np.asfortranarray(Po[:, :m])]
    if No is not None:
        out.append(np.asfortranarray(No[:, :m]))
    if return_counts:
        out.append(cnt[:m].copy())
    if return_trace:
        out.append(trace[:n].copy())
    if return_info:
        out.append(info)
    return out[0] if len(out) == 1 else tuple(out)


class _Handle:
    """an owning handle of the C ABI: close() (idempotent), a context manager, and a __del__ that tolerates the
    interpreter shutting down; using it after close() raises ClipperError instead of handing NULL to the library"""
    _destroy = ""
    _what = "handle"

    def __init__(self, h):
        self.L = load_library()
        self._h = h

    @property
    def h(self):
        if not getattr(self, "_h", None):
            raise ClipperError(f"this {self._what} is closed")
        return self._h

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            getattr(self.L, self._destroy)(h)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # (module globals may be gone at interpreter shutdown)
            pass

    def _check(self, rc):
        if rc < 0:
            raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
        return rc


class DevicePairs(_Handle):
    """clipper_hip_pairs_t: an association list on the device (m x 2 int32, with one squared distance per row where it
    came from DeviceCloud.match). DevicePairs(A[, sqd]) uploads one; len() is m; download() brings it back."""
    _destroy, _what = "clipper_hip_pairs_destroy", "DevicePairs"

    def __init__(self, A=None, sqd=None, device: int = 0, _h=False):
        super().__init__(_h or None)
        if _h is not False:  # (a handle a call of the library made: adopted)
            return
        Ac, m = _assoc_colmajor(() if A is None else A)
        sq = None if sqd is None else np.ascontiguousarray(sqd, dtype=np.float64).reshape(-1)
        if sq is not None and sq.size != m:
            raise ValueError("sqd must hold one squared distance per row of A")
        h = C.c_void_p()
        self._check(self.L.clipper_hip_pairs_create(device, _ip(Ac) if Ac is not None else None,
                                                    None if sq is None else _dp(sq), m, C.byref(h)))
        self._h = h

    def __len__(self):
        return int(self._check(self.L.clipper_hip_pairs_count(self.h)))

    @property
    def has_sqd(self) -> bool:
        """whether the pairs carry one squared distance per row (clipper_hip_pairs_has_sqd)"""
        return bool(self._check(self.L.clipper_hip_pairs_has_sqd(self.h)))

    def download(self, with_sqd: bool | None = None):
        """A (m x 2 int32), or (A, sqd) with with_sqd (default: whenever the pairs carry distances)"""
        m = len(self)
        buf = np.zeros(2 * max(m, 1), dtype=np.int32)
        sqd = np.zeros(max(m, 1), dtype=np.float64)
        if with_sqd is None:
            with_sqd = self.has_sqd
        self._check(self.L.clipper_hip_pairs_download(self.h, _ip(buf), _dp(sqd) if with_sqd else None))
        A = np.stack([buf[:m], buf[m:2 * m]], axis=1).astype(np.int32)
        return (A, sqd[:m].copy()) if with_sqd else A


class DeviceCloud(_Handle):
    """clipper_hip_cloud_t: a point cloud that lives on the device, carrying what the stages compute about it. P: 3 x n
    (columns = points as `clipper::Data`), normals: 3 x n unit normals or None. The methods mirror the stand-alone
    calls of this module and give their bits; nothing crosses the bus but what is asked for. Not safe for concurrent
    mutation. Usable as a context manager; close() frees the device memory (twice is harmless)."""
    _destroy, _what = "clipper_hip_cloud_destroy", "DeviceCloud"

    def __init__(self, P=None, normals=None, device: int = 0, _h=False):
        super().__init__(_h or None)
        if _h is not False:  # (a handle a call of the library made: adopted)
            return
        Pc = _cloud(np.zeros((3, 0)) if P is None else P)
        n = Pc.shape[1]
        Nc = None if normals is None else _cloud(normals, "normals")
        if Nc is not None and Nc.shape[1] != n:
            raise ValueError("P and normals must hold the same number of points")
        h = C.c_void_p()
        self._check(self.L.clipper_hip_cloud_create(device, _dp(Pc) if n else None, None if Nc is None else _dp(Nc), n,
                                                    C.byref(h)))
        self._h = h

    def __len__(self):
        return int(self._check(self.L.clipper_hip_cloud_count(self.h)))

    def info(self) -> CloudInfo:
        out = CloudInfo()
        self._check(self.L.clipper_hip_cloud_info(self.h, C.byref(out)))
        return out

    def _download(self, what, rows, dtype=np.float64, count=None):
        n = len(self) if count is None else count
        shape = (rows, max(n, 1)) if rows else (max(n, 1),)
        out = np.zeros(shape, dtype=dtype, order="F")
        self._check(self.L.clipper_hip_cloud_download(self.h, what, out.ctypes.data_as(C.c_void_p)))
        return np.asfortranarray(out[:, :n]) if rows else out[:n].copy()

    def points(self):
        return self._download(CLOUD_POINTS, 3)

    def normals(self):
        return self._download(CLOUD_NORMALS, 3)

    def descriptors(self):
        return self._download(CLOUD_DESCRIPTORS, max(int(self.info().descriptor_dim), 1))

    def spfh(self):
        return self._download(CLOUD_SPFH, FPFH_DIM)

    def covariances(self):
        return self._download(CLOUD_COVARIANCES, 6)

    def counts(self, what: int):
        """the int32 attachment `what`: CLOUD_NORMAL_COUNTS, _FPFH_COUNTS, _COVARIANCE_COUNTS, _VOXEL_COUNTS, _VOXEL_TRACE"""
        return self._download(what, 0, np.int32, int(self.info().trace_n) if what == CLOUD_VOXEL_TRACE else None)

    def set_descriptors(self, F):
        Fc = _f64_colmajor(F)
        if Fc.ndim != 2 or Fc.shape[1] != len(self):
            raise ValueError("F must be d x n")
        self._check(self.L.clipper_hip_cloud_set_descriptors(self.h, _dp(Fc), Fc.shape[0]))
        return self

    def voxel_down_sample(self, voxel_size: float, return_trace: bool = False, return_info: bool = False):
        """a NEW DeviceCloud of the centroids (and the normalised normal sums); counts(CLOUD_VOXEL_COUNTS) and, with
        return_trace, counts(CLOUD_VOXEL_TRACE) are attached to it"""
        h, info = C.c_void_p(), VoxelInfo()
        self._check(self.L.clipper_hip_cloud_voxel_downsample(self.h, float(voxel_size), int(bool(return_trace)), C.byref(h),
                                                              C.byref(info)))
        out = DeviceCloud(_h=h)
        return (out, info) if return_info else out

    def estimate_normals(self, knn: int = 16, radius: float = 0.0, viewpoint=None):
        v, vptr = _viewpoint(viewpoint)
        nb = Neighborhood(knn, radius)
        self._check(self.L.clipper_hip_cloud_estimate_normals(self.h, C.byref(nb), vptr))
        return self

    def compute_fpfh(self, knn: int = 32, radius: float = 0.0):
        nb = Neighborhood(knn, radius)
        self._check(self.L.clipper_hip_cloud_compute_fpfh(self.h, C.byref(nb)))
        return self

    def fpfh_from_points(self, normal_knn: int = 16, normal_radius: float = 0.0, viewpoint=None, knn: int = 32,
                         radius: float = 0.0):
        v, vptr = _viewpoint(viewpoint)
        nnb, fnb = Neighborhood(normal_knn, normal_radius), Neighborhood(knn, radius)
        self._check(self.L.clipper_hip_cloud_fpfh_from_points(self.h, C.byref(nnb), vptr, C.byref(fnb)))
        return self

    def estimate_covariances(self, knn: int = 20, radius: float = 0.0, epsilon: float = 1e-3):
        nb = Neighborhood(knn, radius)
        self._check(self.L.clipper_hip_cloud_estimate_covariances(self.h, C.byref(nb), float(epsilon)))
        return self

    def match(self, other: "DeviceCloud", knn: int = 1, mutual: bool = True, ratio: float = 0.0, max_sqdist: float = 0.0,
              return_lists: bool = False):
        """match_descriptors of this cloud's descriptors against `other`'s, the filters run on the device: DevicePairs,
        with return_lists also the forward lists (idx n0 x knn int32, sqd n0 x knn)"""
        prm = MatchParams(int(knn), int(bool(mutual)), float(ratio), float(max_sqdist))
        n0 = len(self)
        idx = np.zeros((n0, max(int(knn), 0)), dtype=np.int32) if return_lists else None
        lsq = np.zeros((n0, max(int(knn), 0)), dtype=np.float64) if return_lists else None
        h = C.c_void_p()
        self._check(self.L.clipper_hip_cloud_match(self.h, other.h, C.byref(prm), C.byref(h),
                                                   _ip(idx) if return_lists else None, _dp(lsq) if return_lists else None))
        pairs = DevicePairs(_h=h)
        return (pairs, idx, lsq) if return_lists else pairs

    def gather_points(self, idx):
        """the points idx names, 3 x k, in the order of the list"""
        ic = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
        out = np.zeros((3, max(ic.size, 1)), dtype=np.float64, order="F")
        self._check(self.L.clipper_hip_cloud_gather_points(self.h, _ip(ic), ic.size, _dp(out)))
        return np.asfortranarray(out[:, :ic.size])

    def icp(self, target: "DeviceCloud", T_init=None, method: int = ICP_POINT_TO_POINT, max_distance: float = 0.0,
            max_iterations: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, loss: int | None = None,
            scale: float = 0.0, trim: float = 1.0):
        """icp / icp_generalized (and, with a loss given — ICP_LOSS_NONE for trimming alone — their robust forms) of this
        cloud onto `target`, whose search grid is built at the first call and kept. Returns (T 4 x 4, info) as they do."""
        return _icp_call(self.L.clipper_hip_cloud_icp, (self.h, target.h), T_init, method, max_distance, max_iterations,
                         rel_fitness, rel_rmse, None if loss is None else (loss, scale, trim), robust_slots=True)

    def evaluate_registration(self, target: "DeviceCloud", T=None, max_distance: float = 0.0,
                              return_correspondences: bool = False):
        return _evaluate_call(self.L.clipper_hip_cloud_evaluate_registration, (self.h, target.h), len(self), T, max_distance,
                              return_correspondences)


class HipBatch:
    """Many independent problems solved in one call (clipper_hip_batch_*). Each problem is a tuple
    (D1, D2, A[, u0]) as HipClipper.score_pairwise_consistency_* and HipClipper.solve take them; A = () means
    all-to-all. A missing u0 is an error (the batch does not draw one). Per problem the result equals a lone
    HipClipper solve of the same storage on the same route (route(i) == that solve's last_solver), bit for bit,
    except Solution.t: the wall time of the whole call."""

    def __init__(self, storage: int = STORE_F32_CSC, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        self.b = None
        if self.L.clipper_hip_batch_create(device, storage, C.byref(h)) < 0 or not h.value:
            raise ClipperError(f"clipper_hip_batch_create failed: {_last_error()}")
        self.b = h.value
        self.n = 0

    def close(self):
        if getattr(self, "b", None):
            self.L.clipper_hip_batch_destroy(self.b)
            self.b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise ClipperError(f"clipper_hip error {rc}: {_last_error()}")
        return rc

    def _problems(self, problems, rows=None):
        keep, arr = [], (BatchProblem * max(len(problems), 1))()
        d = None
        for i, pr in enumerate(problems):
            if len(pr) not in (3, 4):
                raise ValueError(f"problem {i}: expected (D1, D2, A[, u0])")
            D1, D2 = _f64_colmajor(pr[0]), _f64_colmajor(pr[1])
            Ac, m = _assoc_colmajor(pr[2])
            u0 = np.ascontiguousarray(pr[3], dtype=np.float64) if len(pr) == 4 and pr[3] is not None else None
            if D1.shape[0] != D2.shape[0]:
                raise ValueError(f"problem {i}: D1 and D2 must have the same number of rows")
            if d is None:
                d = D1.shape[0]
            elif D1.shape[0] != d:
                raise ValueError(f"problem {i}: every problem of a batch has the same dimension")
            mm = m if (Ac is not None and m > 0) else D1.shape[1] * D2.shape[1]
            if u0 is not None and u0.shape != (mm,):
                raise ValueError(f"problem {i}: u0 must have shape ({mm},)")
            keep.append((D1, D2, Ac, u0))
            arr[i] = BatchProblem(_dp(D1), D1.shape[1], _dp(D2), D2.shape[1],
                                  _ip(Ac) if Ac is not None else None, m, _dp(u0) if u0 is not None else None)
        return arr, keep, (d if d is not None else (rows or 3))

    def _collect(self, n, keep):
        out = []
        for i in range(n):
            info = SolveInfo()
            m = self._check(self.L.clipper_hip_batch_get_solution(self.b, i, None, C.byref(info)))
            u = np.zeros(max(m, 1))[:m]
            self._check(self.L.clipper_hip_batch_get_solution(self.b, i, _dp(u), C.byref(info)))
            nodes = np.zeros(max(info.num_nodes, 1), dtype=np.int32)
            k = self._check(self.L.clipper_hip_batch_get_nodes(self.b, i, _ip(nodes), nodes.size))
            u0 = keep[i][3] if keep[i][3] is not None else np.zeros(0)
            out.append(Solution(t=info.seconds, ifinal=info.ifinal, nodes=nodes[:k].copy(), u0=u0, u=u,
                                score=info.score, d=info.d, n_passes=info.n_passes, n_trials=info.n_trials))
        self.n = n
        return out

    def solve_euclidean(self, problems, sigma=0.01, epsilon=0.06, mindist=0.0, params: Params | None = None):
        params = params or Params()
        arr, keep, d = self._problems(problems)
        self._check(self.L.clipper_hip_batch_solve_euclidean(self.b, arr, len(problems), d, sigma, epsilon, mindist,
                                                             C.byref(params)))
        return self._collect(len(problems), keep)

    def solve_custom(self, inv: HipInvariant, problems, params=(), solver_params: Params | None = None):
        """the problems scored by a user-defined invariant (clipper_hip_batch_solve_custom): every D is inv.d x n;
        params: the invariant's parameters (at most INVARIANT_MAX_PARAMS doubles)"""
        solver_params = solver_params or Params()
        arr, keep, _ = self._problems(problems, rows=inv.d)
        for i, k in enumerate(keep):
            if k[0].shape[0] != inv.d:
                raise ValueError(f"problem {i}: the invariant is compiled for d = {inv.d}, D1 has {k[0].shape[0]} rows")
        p, pp = _params_array(params)
        self._check(self.L.clipper_hip_batch_solve_custom(self.b, inv.h, arr, len(problems), pp, p.size,
                                                          C.byref(solver_params)))
        return self._collect(len(problems), keep)

    def solve_pointnormal(self, problems, sigp=0.5, epsp=0.5, sign=0.10, epsn=0.35, params: Params | None = None):
        params = params or Params()
        arr, keep, _ = self._problems(problems, rows=6)
        self._check(self.L.clipper_hip_batch_solve_pointnormal(self.b, arr, len(problems), sigp, epsp, sign, epsn,
                                                               C.byref(params)))
        return self._collect(len(problems), keep)

    def sdp(self, params: SdpParams | None = None, want_xy: bool = True) -> list:
        """The semidefinite relaxation of every problem of the last solve call, in one batched call
        (clipper_hip_batch_sdp): per problem the SdpResult HipClipper.sdp gives on a lone context, bit for bit. Each
        problem's selection becomes its node list (selected_associations(i) follows it)."""
        params = params if params is not None else SdpParams()
        infos = (SdpInfo * max(self.n, 1))()
        self._check(self.L.clipper_hip_batch_sdp(self.b, C.byref(params), infos))
        out = []
        for i in range(self.n):
            info = SdpInfo.from_buffer_copy(infos[i])
            n = self._check(self.L.clipper_hip_batch_get_sdp(self.b, i, None, None, None, None))
            X, Y = (np.zeros((n, n)), np.zeros((n, n))) if want_xy else (np.zeros((0, 0)), np.zeros((0, 0)))
            lam, ev = np.zeros(n), np.zeros(n)
            self._check(self.L.clipper_hip_batch_get_sdp(self.b, i, _dp(X) if want_xy else None,
                                                         _dp(Y) if want_xy else None, _dp(lam), _dp(ev)))
            nodes = np.zeros(max(info.num_nodes, 1), dtype=np.int32)
            k = self._check(self.L.clipper_hip_batch_get_nodes(self.b, i, _ip(nodes), nodes.size))
            out.append(_sdp_result(n, X, Y, lam, ev, nodes[:k].copy(), info))
        return out

    def max_clique(self, method: int = MC_EXACT, time_limit: float = 0.0, seeds=None) -> list:
        """The maximum clique (HipClipper.max_clique) of every problem of the last solve call, in one batched call
        (clipper_hip_batch_max_clique): per problem (nodes ascending, MaxCliqueInfo), the nodes and max_core,
        heuristic_size, edges, num_nodes those of a lone context. Each clique becomes its problem's node list
        (get_nodes(i), selected_associations(i)). time_limit in seconds bounds the whole call (<= 0: none).
        seeds: one vertex list per problem (an empty one: that problem runs unseeded) or "solution" (every problem's own
        node list); with them (clipper_hip_batch_max_clique_seeded) each problem's tuple ends with its
        MaxCliqueSeedInfo, and method may be MC_SEED_ONLY."""
        infos = (MaxCliqueInfo * max(self.n, 1))()
        if seeds is None:
            self._check(self.L.clipper_hip_batch_max_clique(self.b, int(method), float(time_limit), infos))
            return [(self.get_nodes(i), MaxCliqueInfo.from_buffer_copy(infos[i])) for i in range(self.n)]
        sinfos = (MaxCliqueSeedInfo * max(self.n, 1))()
        if isinstance(seeds, str):
            if seeds != "solution":
                raise ValueError('seeds: one vertex list per problem or "solution"')
            sp, op = None, None
        else:
            if len(seeds) != self.n:
                raise ValueError(f"{len(seeds)} seed lists for {self.n} problems")
            lists = [np.asarray(s, dtype=np.int32).ravel() for s in seeds]
            flat = np.ascontiguousarray(np.concatenate(lists + [np.zeros(1, np.int32)]))
            offs = np.zeros(self.n + 1, dtype=np.int64)
            offs[1:] = np.cumsum([len(s) for s in lists])
            sp, op = _ip(flat), offs.ctypes.data_as(C.POINTER(C.c_int64))
        self._check(self.L.clipper_hip_batch_max_clique_seeded(self.b, int(method), float(time_limit), sp, op, infos,
                                                               sinfos))
        return [(self.get_nodes(i), MaxCliqueInfo.from_buffer_copy(infos[i]),
                 MaxCliqueSeedInfo.from_buffer_copy(sinfos[i])) for i in range(self.n)]

    def max_clique_stats(self):
        """(kernel launches of the batched route, problems that ran in them, problems that ran alone) of the last
        max_clique call"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.L.clipper_hip_batch_max_clique_stats(self.b, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def get_nodes(self, i: int):
        """problem i's node list as the last solve, relaxation or clique call left it (ascending)"""
        info = SolveInfo()
        self._check(self.L.clipper_hip_batch_get_solution(self.b, i, None, C.byref(info)))
        nodes = np.zeros(max(info.num_nodes, 1), dtype=np.int32)
        k = self._check(self.L.clipper_hip_batch_get_nodes(self.b, i, _ip(nodes), nodes.size))
        return nodes[:k].copy()

    def route(self, i: int) -> int:
        """1 = solved in a batched resident launch, 0 = solved alone on its child context"""
        return self._check(self.L.clipper_hip_batch_route(self.b, i))

    def selected_associations(self, i: int):
        info = SolveInfo()
        self._check(self.L.clipper_hip_batch_get_solution(self.b, i, None, C.byref(info)))
        k = max(info.num_nodes, 1)
        buf = np.zeros(2 * k, dtype=np.int32)
        kk = self._check(self.L.clipper_hip_batch_get_selected_associations(self.b, i, _ip(buf), k))
        return np.stack([buf[:kk], buf[kk:2 * kk]], axis=1)

    def stats(self):
        """(launches, problems solved batched, problems solved alone) of the last call"""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.L.clipper_hip_batch_get_stats(self.b, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def split(self):
        """host wall time of the last call (ms): staging + fills + plans, batched launches, solved alone, rounding"""
        v = [C.c_double() for _ in range(4)]
        self._check(self.L.clipper_hip_batch_get_split(self.b, *[C.byref(x) for x in v]))
        return dict(zip(("fill_ms", "launch_ms", "alone_ms", "round_ms"), (x.value for x in v)))
