"""The stand-alone entry points of the C ABI (a device number and host arrays, no context) as one table: each with
valid arguments at n = 8 points and with one invalid argument, called through ctypes as a C caller would. Shared by
tests/test_standalone_entries_cpu.py (the argument checks come first, then the device) and
tests/test_gpu_standalone_entries.py (a device number out of range)."""
import ctypes as C

import numpy as np

from clipper_amd import _abi as abi

N = 8
_rng = np.random.default_rng(8)
_P = np.asfortranarray(_rng.random((3, N)))                  # 3 x n, columns = points
_Q = np.asfortranarray(_rng.random((3, N)))
_NRM = np.asfortranarray(np.tile(np.array([[0.0], [0.0], [1.0]]), (1, N)))
_F = np.asfortranarray(_rng.random((33, N)))
_M = np.asfortranarray(np.eye(N) + 0.5 * (np.ones((N, N)) - np.eye(N)))
_ONES = np.asfortranarray(np.ones((N, N)))

dp, ip = abi._dp, abi._ip


def _knn(L, device, bad):
    idx, sqd = np.zeros((N, 17), np.int32), np.zeros((N, 17))
    return L.clipper_hip_knn(device, dp(_P), N, dp(_Q), N, 3, 17 if bad else 2, ip(idx), dp(sqd))


def _correspondences(L, device, bad):
    A = np.zeros(2 * N * 17, np.int32)
    return L.clipper_hip_distance_based_correspondences(device, dp(_P), N, dp(_Q), N, 3, 17 if bad else 2, 0.5, 1, ip(A), N * 17)


def _match(L, device, bad):
    prm = abi.MatchParams(0 if bad else 1, 1, 0.0, 0.0)
    A, sqd = np.zeros(2 * N, np.int32), np.zeros(N)
    return L.clipper_hip_match_descriptors(device, dp(_F), N, dp(_F), N, 33, C.byref(prm), ip(A), dp(sqd), N, None, None)


def _normals(L, device, bad):
    nb = abi.Neighborhood(2 if bad else 4)
    out, cnt = np.zeros((3, N), order="F"), np.zeros(N, np.int32)
    return L.clipper_hip_estimate_normals(device, dp(_P), N, C.byref(nb), None, dp(out), ip(cnt))


def _fpfh(L, device, bad):
    nb = abi.Neighborhood(2 if bad else 4)
    out = np.zeros((33, N), order="F")
    return L.clipper_hip_compute_fpfh(device, dp(_P), dp(_NRM), N, C.byref(nb), dp(out), None, None)


def _fpfh_from_points(L, device, bad):
    nnb, fnb = abi.Neighborhood(4), abi.Neighborhood(2 if bad else 4)
    out = np.zeros((33, N), order="F")
    return L.clipper_hip_fpfh_from_points(device, dp(_P), N, C.byref(nnb), None, C.byref(fnb), dp(out), None)


def _icp(L, device, bad):
    prm = abi.IcpParams(max_distance=0.0 if bad else 0.5, max_iterations=2)
    T, info = np.zeros(16), abi.IcpInfo()
    return L.clipper_hip_icp(device, dp(_P), N, dp(_Q), None, N, None, C.byref(prm), dp(T), C.byref(info), None)


def _evaluate(L, device, bad):
    return L.clipper_hip_evaluate_registration(device, dp(_P), N, dp(_Q), N, None, 0.0 if bad else 0.5, None, None, None, None)


def _sdp(L, device, bad):
    prm, info = abi.SdpParams(), abi.SdpInfo()
    nodes = np.zeros(N, np.int32)
    return L.clipper_hip_sdp_solve(device, None if bad else dp(_M), dp(_ONES), N, C.byref(prm), None, None, None, None,
                                   ip(nodes), C.byref(info))


def _sdp_batch(L, device, bad):
    prm, info = abi.SdpParams(), abi.SdpInfo()
    nodes = np.zeros(N, np.int32)
    prob = abi.SdpProblem(dp(_M), dp(_ONES), N, None, None, None, None, ip(nodes))
    return L.clipper_hip_sdp_solve_batch(device, C.byref(prob), -1 if bad else 1, C.byref(prm), C.byref(info))


def _batch_create(L, device, bad):
    out = C.c_void_p()
    rc = L.clipper_hip_batch_create(device, abi.STORE_F32_CSC, None if bad else C.byref(out))
    if out.value:                                             # (a device took it: nothing is left behind)
        L.clipper_hip_batch_destroy(out)
    return rc


# (entry point, the call, what the call with the invalid argument says: every one of them CLIPPER_HIP_E_INVALID)
ENTRIES = [
    ("clipper_hip_knn", _knn, "knn must be in 1..16"),
    ("clipper_hip_distance_based_correspondences", _correspondences, "knn must be in 1..16"),
    ("clipper_hip_match_descriptors", _match, "knn must be in 1..8 (knn = 0)"),
    ("clipper_hip_estimate_normals", _normals, "neighbourhood: knn must be in 3..32 (knn = 2)"),
    ("clipper_hip_compute_fpfh", _fpfh, "neighbourhood: knn must be in 3..32 (knn = 2)"),
    ("clipper_hip_fpfh_from_points", _fpfh_from_points, "feature neighbourhood: knn must be in 3..32 (knn = 2)"),
    ("clipper_hip_icp", _icp, "icp: max_distance must be positive and finite"),
    ("clipper_hip_evaluate_registration", _evaluate, "evaluate_registration: max_distance must be positive and finite"),
    ("clipper_hip_sdp_solve", _sdp, "sdp: M and C are required"),
    ("clipper_hip_sdp_solve_batch", _sdp_batch, "sdp batch: count = -1"),
    ("clipper_hip_batch_create", _batch_create, "invalid argument"),
]

E_INVALID, E_NODEVICE = -1, -4


def call(entry, device, bad=False):
    """(status, message) of one entry of the table"""
    L = abi.load_library()
    rc = int(entry[1](L, device, bad))
    return rc, L.clipper_hip_last_error().decode()
