"""Host-side pieces either side of the hot path for the 3-D registration use case:
a PLY point reader, the putative-association generator of the reference's bunny example, and the
rigid-transform estimate that consumes the selected associations. Plain numpy, except for what searches nearest
neighbours on the device: the two association generators (ground_truth_associations, match_descriptors) and the
stage in front of them, raw cloud -> normals -> FPFH descriptors (estimate_normals, compute_fpfh) — the path
between them is clipper_hip_affinity_* / clipper_hip_solve.

Reference sites (relative to /root/reference): the data-set recipe restates
examples/python/ex4_bunny.ipynb cell 2 (sample the model, ground-truth transform, uniform noise in
a sigma-cube, outlier points uniform in a ball, nia correct + noa wrong associations); the
transform estimate is the closed form of Arun et al. that cell 6 obtains from open3d's
TransformationEstimationPointToPoint and benchmarks/bm_utils.cpp uses through Eigen::umeyama
(without scaling); the error measures are cell 7's."""
from __future__ import annotations

import contextlib
import struct

import numpy as np

_PLY_TYPES = {"char": "b", "int8": "b", "uchar": "B", "uint8": "B", "short": "h", "int16": "h",
              "ushort": "H", "uint16": "H", "int": "i", "int32": "i", "uint": "I", "uint32": "I",
              "float": "f", "float32": "f", "double": "d", "float64": "d"}


def read_ply_xyz(path: str) -> np.ndarray:
    """Vertex positions (n, 3) float64 of an ascii or binary PLY file (x, y, z properties of the
    `vertex` element; other properties and elements are skipped; list properties in the vertex
    element are not supported)."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError("not a PLY file")
        fmt, nvert, props, in_vertex = None, 0, [], False
        seen_vertex = False
        while True:
            line = f.readline()
            if not line:
                raise ValueError("PLY header not terminated")
            tok = line.decode("ascii", "replace").split()
            if not tok:
                continue
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    if seen_vertex:
                        raise ValueError("two vertex elements")
                    nvert, seen_vertex = int(tok[2]), True
                elif not seen_vertex:
                    raise ValueError("elements before `vertex` are not supported")
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError("list property in the vertex element")
                props.append((tok[2], _PLY_TYPES[tok[1]]))
            elif tok[0] == "end_header":
                break
        names = [p[0] for p in props]
        if not all(k in names for k in "xyz"):
            raise ValueError("vertex element has no x, y, z")
        if fmt == "ascii":
            rows = [f.readline().split() for _ in range(nvert)]
            arr = np.array([[float(r[names.index(k)]) for k in "xyz"] for r in rows], dtype=np.float64)
            for c, k in enumerate("xyz"):      # through the declared type, as a binary file would carry it
                arr[:, c] = arr[:, c].astype(dict(props)[k]).astype(np.float64)
        elif fmt in ("binary_little_endian", "binary_big_endian"):
            end = "<" if fmt == "binary_little_endian" else ">"
            dt = np.dtype([(n, end + t) for n, t in props])
            raw = np.frombuffer(f.read(dt.itemsize * nvert), dtype=dt, count=nvert)
            arr = np.stack([raw[k].astype(np.float64) for k in "xyz"], axis=1)
        else:
            raise ValueError(f"unknown PLY format {fmt!r}")
    return arr


def write_ply_xyz(path: str, pts: np.ndarray) -> None:
    """Binary little-endian PLY with float x, y, z (round-trip partner of read_ply_xyz)."""
    pts = np.asarray(pts, dtype="<f4")
    with open(path, "wb") as f:
        f.write(b"ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(pts))
        f.write(b"property float x\nproperty float y\nproperty float z\nend_header\n")
        f.write(pts.tobytes())


def random_rotation(rng: np.random.Generator) -> np.ndarray:
    """Uniformly distributed rotation matrix (QR of a Gaussian matrix, sign-fixed)."""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def uniform_in_ball(rng: np.random.Generator, n: int, radius: float) -> np.ndarray:
    """n points uniformly distributed in a 3-D ball."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (radius * rng.random(n) ** (1.0 / 3.0))[:, None]


def make_registration_dataset(model_points: np.ndarray, m: int, n1: int, n2o: int, outrat: float,
                              sigma: float, T_21: np.ndarray, seed: int = 0):
    """Two views of a model and m putative associations between them.

    model_points (N, 3): the full model; n1 points are sampled for view 1, transformed by T_21
    (4x4) into view 2 and perturbed by noise uniform in [-sigma/2, sigma/2]^3; n2o outlier points
    (uniform in a unit ball around view 2's centroid) are appended to view 2. The association list
    holds nia = m - round(m*outrat) correct pairs (i, i) followed by noa wrong pairs (i, j != i),
    all distinct. Returns D1 (3, n1), D2 (3, n1 + n2o) float64, A (m, 2) int32, Agt (nia, 2)."""
    rng = np.random.default_rng(seed)
    n2 = n1 + n2o
    noa = int(round(m * outrat))
    nia = m - noa
    if nia > n1:
        raise ValueError("more inlier associations than model points")
    if noa > n1 * n2 - n1:
        raise ValueError("more outlier associations than wrong pairs exist")
    pick = rng.choice(len(model_points), n1, replace=False)
    D1 = np.asarray(model_points, dtype=np.float64)[pick].T
    D2 = T_21[:3, :3] @ D1 + T_21[:3, 3:4]
    D2 = D2 + rng.uniform(-sigma / 2.0, sigma / 2.0, size=D2.shape)
    O2 = uniform_in_ball(rng, n2o, 1.0).T + D2.mean(axis=1, keepdims=True)
    D2 = np.hstack([D2, O2])
    good = rng.choice(n1, nia, replace=False)
    Agt = np.stack([good, good], axis=1).astype(np.int32)
    bad, seen = [], set()
    while len(bad) < noa:
        i, j = int(rng.integers(n1)), int(rng.integers(n2))
        if i == j or (i, j) in seen:
            continue
        seen.add((i, j))
        bad.append((i, j))
    A = np.concatenate([Agt, np.array(bad, dtype=np.int32).reshape(-1, 2)]).astype(np.int32)
    return np.ascontiguousarray(D1), np.ascontiguousarray(D2), A, Agt


def estimate_rigid_transform(D1: np.ndarray, D2: np.ndarray, A: np.ndarray) -> np.ndarray:
    """Least-squares rigid transform T (4x4) with D2[:, A[k,1]] ~ R D1[:, A[k,0]] + t over the
    associations A (k x 2): centroids, 3x3 cross-covariance, SVD, reflection fix."""
    A = np.asarray(A)
    if A.shape[0] < 3:
        raise ValueError("at least 3 associations are needed")
    P, Q = D1[:, A[:, 0]], D2[:, A[:, 1]]
    cp, cq = P.mean(axis=1, keepdims=True), Q.mean(axis=1, keepdims=True)
    H = (Q - cq) @ (P - cp).T
    U, _, Vt = np.linalg.svd(H)
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = (cq - R @ cp).ravel()
    return T


def ransac_correspondences(D1: np.ndarray, D2: np.ndarray, A: np.ndarray, max_distance: float, n_sample: int = 3,
                           edge_similarity: float = 0.9, max_hypotheses: int = 100000, confidence: float = 0.999,
                           seed: int = 0, refine_iterations: int = 1, hypotheses_per_round: int = 4096, device: int = 0):
    """RANSAC over the putative associations A (m x 2), on the GPU (clipper_hip_ransac_correspondences): the rigid
    transform T (4 x 4) with D2[:, A[k,1]] ~ R D1[:, A[k,0]] + t that most associations agree on within max_distance.
    D1, D2: 3 x n as for estimate_rigid_transform. A hypothesis fits n_sample associations whose edge lengths agree
    within edge_similarity in both clouds; its score is its inlier count; the rounds of hypotheses_per_round stop at
    `confidence` or at max_hypotheses; the winner is polished refine_iterations times over its inliers. The same
    inputs and seed give the same bytes. Returns (T, info): info.status (clipper_amd._abi.RANSAC_*), info.inliers (a
    boolean mask over A), info.count, info.fitness, info.inlier_rmse, info.best_hypothesis, info.best_count,
    info.sample, info.evaluated, info.checked, info.refined."""
    from . import _abi as abi
    return abi.ransac_correspondences(np.asarray(D1, dtype=np.float64), np.asarray(D2, dtype=np.float64), A, max_distance,
                                      n_sample=n_sample, edge_similarity=edge_similarity, max_hypotheses=max_hypotheses,
                                      confidence=confidence, seed=seed, refine_iterations=refine_iterations,
                                      hypotheses_per_round=hypotheses_per_round, device=device)


def transform_error(T: np.ndarray, That: np.ndarray):
    """(rotation error [rad], translation error) of an estimate against the truth."""
    E = np.linalg.inv(T) @ That
    c = min(max((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0), 1.0)
    return abs(float(np.arccos(c))), float(np.linalg.norm(E[:3, 3]))


def precision_recall(Ain: np.ndarray, Agt: np.ndarray):
    """Fraction of selected associations that are correct / of correct ones that were selected."""
    sel = {tuple(r) for r in np.asarray(Ain).tolist()}
    gt = {tuple(r) for r in np.asarray(Agt).tolist()}
    hit = len(sel & gt)
    return (hit / len(sel) if sel else 0.0), (hit / len(gt) if gt else 0.0)


# ---- the reference benchmark's putative-association recipe (benchmarks/main.cpp:156-166) --------

def scale_to_cube(pts: np.ndarray, s: float = 1.0) -> np.ndarray:
    """bm_utils.cpp:110-115: uniform scale so that the longest bounding-box edge is `s`."""
    d = pts.max(axis=0) - pts.min(axis=0)
    return pts * (s / d.max())


def bounded_normal_noise(rng: np.random.Generator, n: int, sigma: float, beta: float) -> np.ndarray:
    """bm_utils.cpp:117-143: N(0, sigma^2 I) conditioned on ||v|| <= beta (batched rejection)."""
    eta = rng.normal(0.0, sigma, (n, 3))
    bad = np.linalg.norm(eta, axis=1) > beta
    while bad.any():
        eta[bad] = rng.normal(0.0, sigma, (int(bad.sum()), 3))
        bad = np.linalg.norm(eta, axis=1) > beta
    return eta


_KNN_SEARCH = {"brute": 0, "grid": 1, "auto": 2}  # clipper_amd._abi.KNN_*


@contextlib.contextmanager
def _knn_search(search):
    """The process-wide route of the 3-D nearest-neighbour search (clipper_amd._abi.knn_set_search) set to `search`
    ("brute", "grid", "auto", or None to leave it alone) around one call, and put back as it was found."""
    from . import _abi as abi
    if search is None:
        yield
        return
    if search not in _KNN_SEARCH:
        raise ValueError(f"search must be one of {sorted(_KNN_SEARCH)} or None")
    prev = abi.knn_set_search(_KNN_SEARCH[search])
    try:
        yield
    finally:
        abi.knn_set_search(prev)


def ground_truth_associations(pcd0: np.ndarray, pcd1: np.ndarray, radius: float, device: int = 0, search: str | None = None):
    """main.cpp:85-91: one-to-one nearest-neighbour associations within `radius`, on the GPU
    (clipper_hip_distance_based_correspondences). pcd*: n x 3, rows = points. search: the route of the search for
    this call ("brute", "grid" or "auto"; None: the process's setting); the result does not depend on it."""
    from . import _abi as abi
    with _knn_search(search):
        return abi.distance_based_correspondences(pcd0.T, pcd1.T, 1, radius, True, device=device)


def __getattr__(name):
    """DeviceCloud and DevicePairs: clouds and association lists that live on the device, carrying what the stages
    below compute about them (clipper_amd._abi, which is loaded at first use like every device call of this module).
    They take and return the C ABI's layout, 3 x n with columns = points."""
    if name in ("DeviceCloud", "DevicePairs"):
        from . import _abi as abi
        return getattr(abi, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def match_descriptors(F0: np.ndarray, F1: np.ndarray, knn: int = 1, mutual: bool = True, ratio: float = 0.0,
                      max_sqdist: float = 0.0, device: int = 0):
    """Putative associations from feature descriptors, on the GPU (clipper_hip_match_descriptors).
    F0: n0 x d, F1: n1 x d, rows = descriptors (the layout feature extractors produce), d <= 64.
    Returns (A n x 2 int32, sqd n): see clipper_amd._abi.match_descriptors."""
    from . import _abi as abi
    return abi.match_descriptors(np.asarray(F0, dtype=np.float64).T, np.asarray(F1, dtype=np.float64).T, knn=knn,
                                 mutual=mutual, ratio=ratio, max_sqdist=max_sqdist, device=device)


def voxel_down_sample(P: np.ndarray, voxel_size: float, normals: np.ndarray | None = None, return_counts: bool = False,
                      return_trace: bool = False, device: int = 0):
    """One point per occupied voxel of edge voxel_size, on the GPU (clipper_hip_voxel_downsample): the step in front of
    estimate_normals. P: n x 3, rows = points. Returns the centroids of the occupied voxels (n_out x 3, in ascending
    cell number: lexicographic in z, y, x over a grid whose origin is the cloud's minimum corner), then in this order:
    with `normals` (n x 3) the normalised sum of each voxel's normals (n_out x 3; (0, 0, 1) where they cancel), with
    return_counts the points per voxel (n_out int32), with return_trace every input point's output row (n int32); a
    tuple when more than one. The result is a function of the inputs alone: the same bits from run to run."""
    from . import _abi as abi
    out = abi.voxel_down_sample(np.asarray(P, dtype=np.float64).T, voxel_size,
                                N=None if normals is None else np.asarray(normals, dtype=np.float64).T, device=device,
                                return_counts=return_counts, return_trace=return_trace)
    out = list(out) if isinstance(out, tuple) else [out]
    for k in range(1 if normals is None else 2):
        out[k] = np.ascontiguousarray(out[k].T)
    return out[0] if len(out) == 1 else tuple(out)


def estimate_normals(P: np.ndarray, knn: int = 16, radius: float = 0.0, viewpoint=None, device: int = 0,
                     search: str | None = None) -> np.ndarray:
    """Unit surface normals of a cloud, on the GPU (clipper_hip_estimate_normals). P: n x 3, rows = points. A point's
    neighbourhood is its knn (3..32) nearest points, itself included, with radius > 0 only those within it; the sign
    points towards `viewpoint`, or without one makes the largest component positive. Returns n x 3. search: as in
    ground_truth_associations."""
    from . import _abi as abi
    with _knn_search(search):
        N = abi.estimate_normals(np.asarray(P, dtype=np.float64).T, knn=knn, radius=radius, viewpoint=viewpoint, device=device)
    return np.ascontiguousarray(N.T)


def compute_fpfh(P: np.ndarray, N: np.ndarray | None = None, knn: int = 32, radius: float = 0.0, normal_knn: int = 16,
                 normal_radius: float = 0.0, viewpoint=None, device: int = 0, search: str | None = None) -> np.ndarray:
    """FPFH descriptors of a cloud, on the GPU. P: n x 3, rows = points; N: their unit normals n x 3, or None to
    estimate them in the same call over (normal_knn, normal_radius, viewpoint) (clipper_hip_fpfh_from_points; with N
    given: clipper_hip_compute_fpfh). Returns n x 33, rows = descriptors: what match_descriptors takes. search: as in
    ground_truth_associations."""
    from . import _abi as abi
    Pt = np.asarray(P, dtype=np.float64).T
    with _knn_search(search):
        if N is None:
            F, _ = abi.fpfh_from_points(Pt, normal_knn=normal_knn, normal_radius=normal_radius, viewpoint=viewpoint, knn=knn,
                                        radius=radius, device=device)
        else:
            F = abi.compute_fpfh(Pt, np.asarray(N, dtype=np.float64).T, knn=knn, radius=radius, device=device)
    return np.ascontiguousarray(F.T)


_ICP_METHODS = {"point": 0, "plane": 1}  # clipper_amd._abi.ICP_POINT_TO_POINT / ICP_POINT_TO_PLANE
_ICP_LOSSES = {"none": 0, "huber": 1, "cauchy": 2, "tukey": 3, "geman_mcclure": 4}  # clipper_amd._abi.ICP_LOSS_*


def _icp_robust_args(loss, scale, trim):
    """None when (loss, scale, trim) are the defaults: the call then takes the plain entry point. Else the keywords of
    the robust one."""
    if loss not in _ICP_LOSSES:
        raise ValueError(f"loss must be one of {sorted(_ICP_LOSSES)}")
    if loss == "none" and scale == 0.0 and trim == 1.0:
        return None
    return dict(loss=_ICP_LOSSES[loss], scale=scale, trim=trim)


def icp(src: np.ndarray, tgt: np.ndarray, T_init: np.ndarray | None = None, method: str = "point",
        normals: np.ndarray | None = None, max_distance: float = 0.0, max_iterations: int = 30, rel_fitness: float = 1e-6,
        rel_rmse: float = 1e-6, device: int = 0, search: str | None = None, loss: str = "none", scale: float = 0.0,
        trim: float = 1.0):
    """Local refinement of a registration, on the GPU (clipper_hip_icp): ICP from the alignment T_init (4 x 4, None =
    identity) of the cloud src onto tgt (n x 3, rows = points), e.g. the estimate_rigid_transform of a solve's selected
    associations. method "point" (point-to-point) or "plane" (point-to-plane over `normals`, the target's unit normals
    n_tgt x 3, e.g. estimate_normals(tgt)). A moved source point corresponds to its nearest target point and counts as
    an inlier within max_distance. Returns (T 4 x 4, info): info.status (clipper_amd._abi.ICP_*), info.iterations,
    info.count, info.fitness, info.inlier_rmse, info.history ((iterations + 1) x 3: count, fitness, rmse), info.route.
    search: as in ground_truth_associations; the result does not depend on it.
    Against bad pairs (partial overlap, clutter): loss "huber", "cauchy", "tukey" or "geman_mcclure" weighs every pair by
    its residual against `scale` (a distance), and trim < 1 keeps, each iteration, that fraction of the points within
    max_distance with the smallest distances (clipper_hip_icp_robust; info then also carries within, weight_sum and
    trim_sqd). "tukey" and "geman_mcclure" give pairs far beyond the scale no weight: start them close to the answer."""
    from . import _abi as abi
    if method not in _ICP_METHODS:
        raise ValueError(f"method must be one of {sorted(_ICP_METHODS)}")
    robust = _icp_robust_args(loss, scale, trim)
    kw = dict(T_init=T_init, method=_ICP_METHODS[method],
              N_tgt=None if normals is None else np.asarray(normals, dtype=np.float64).T, max_distance=max_distance,
              max_iterations=max_iterations, rel_fitness=rel_fitness, rel_rmse=rel_rmse, device=device, **(robust or {}))
    with _knn_search(search):
        call = abi.icp if robust is None else abi.icp_robust
        return call(np.asarray(src, dtype=np.float64).T, np.asarray(tgt, dtype=np.float64).T, **kw)


def estimate_covariances(P: np.ndarray, knn: int = 20, radius: float = 0.0, epsilon: float = 1e-3, device: int = 0,
                         search: str | None = None) -> np.ndarray:
    """The per-point covariances of generalized ICP, on the GPU (clipper_hip_estimate_covariances). P: n x 3, rows =
    points. Per point I - (1 - epsilon) nv nv^T, nv the normal of estimate_normals' neighbourhood (knn, radius): a disc
    of thickness epsilon in the surface; the identity where fewer than 3 neighbours are kept. Returns n x 6: xx, xy,
    xz, yy, yz, zz per row. search: as in ground_truth_associations."""
    from . import _abi as abi
    if not (0.0 < epsilon <= 1.0):
        raise ValueError(f"epsilon must be in (0, 1] (epsilon = {epsilon})")
    with _knn_search(search):
        Cv = abi.estimate_covariances(np.asarray(P, dtype=np.float64).T, knn=knn, radius=radius, epsilon=epsilon, device=device)
    return np.ascontiguousarray(Cv.T)


def icp_generalized(src: np.ndarray, tgt: np.ndarray, T_init: np.ndarray | None = None,
                    source_covariances: np.ndarray | None = None, target_covariances: np.ndarray | None = None,
                    covariance_knn: int = 20, epsilon: float = 1e-3, max_distance: float = 0.0, max_iterations: int = 30,
                    rel_fitness: float = 1e-6, rel_rmse: float = 1e-6, device: int = 0, search: str | None = None,
                    loss: str = "none", scale: float = 0.0, trim: float = 1.0):
    """Generalized ICP (the plane-to-plane metric), on the GPU (clipper_hip_icp_generalized): icp's loop, correspondences
    and stop rule, with every inlier pair weighed by the inverse of the sum of its two covariances: what refines
    voxel-down-sampled scans, where no source point has an exact partner. src, tgt: n x 3, rows = points. The
    covariances (n x 6 rows of xx, xy, xz, yy, yz, zz) left None are estimated in the call by
    estimate_covariances(cloud, covariance_knn, epsilon=epsilon). Returns (T 4 x 4, info) as icp does. loss, scale,
    trim: as in icp (clipper_hip_icp_generalized_robust); the residual a loss weighs is d^T M d of the pair."""
    from . import _abi as abi
    robust = _icp_robust_args(loss, scale, trim)
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    covs = []
    for name, cloud, cv in (("source_covariances", src, source_covariances), ("target_covariances", tgt, target_covariances)):
        if cv is None:
            cv = estimate_covariances(cloud, knn=covariance_knn, epsilon=epsilon, device=device, search=search)
        cv = np.asarray(cv, dtype=np.float64)
        if cv.ndim != 2 or cv.shape != (len(cloud), 6):
            raise ValueError(f"{name} must be n x 6, one row per point")
        covs.append(cv.T)
    kw = dict(T_init=T_init, max_distance=max_distance, max_iterations=max_iterations, rel_fitness=rel_fitness, rel_rmse=rel_rmse,
              device=device, **(robust or {}))
    with _knn_search(search):
        call = abi.icp_generalized if robust is None else abi.icp_generalized_robust
        return call(src.T, covs[0], tgt.T, covs[1], **kw)


def evaluate_registration(src: np.ndarray, tgt: np.ndarray, T: np.ndarray | None = None, max_distance: float = 0.0,
                          device: int = 0, search: str | None = None, return_correspondences: bool = False):
    """How good the alignment T (4 x 4, None = identity) of src onto tgt (n x 3) is, on the GPU
    (clipper_hip_evaluate_registration): (fitness, inlier_rmse, count) over all source points, with
    return_correspondences also each source point's target index (-1: no target point within max_distance)."""
    from . import _abi as abi
    with _knn_search(search):
        return abi.evaluate_registration(np.asarray(src, dtype=np.float64).T, np.asarray(tgt, dtype=np.float64).T, T=T,
                                         max_distance=max_distance, device=device,
                                         return_correspondences=return_correspondences)


def generate_synthetic_correspondences(n0: int, n1: int, Agood: np.ndarray, m: int, rho: float,
                                       rng: np.random.Generator):
    """bm_utils.cpp:277-341: m putative associations with outlier ratio rho — round(m (1 - rho))
    inliers drawn without replacement from Agood (placed last), the rest sampled uniformly without
    repetition from all n0*n1 pairs that are not in Agood (placed first). Returns (A, Agt) or None
    when Agood holds too few associations."""
    if not 0.0 <= rho <= 1.0:
        raise ValueError("outlier ratio must be in [0, 1]")
    ni = int(round(m * (1.0 - rho)))
    no = m - ni
    if ni > len(Agood):
        return None
    Agt = np.asarray(Agood)[rng.permutation(len(Agood))[:ni]].astype(np.int32)
    good = np.asarray(Agood, dtype=np.int64)
    good_flat = set((good[:, 0] * n1 + good[:, 1]).tolist())
    out = np.zeros((no, 2), dtype=np.int32)
    seen: set = set()
    k = 0
    while k < no:
        cand = rng.integers(0, n0 * n1, size=2 * (no - k) + 8)
        for flat in cand.tolist():
            if flat in seen:
                continue
            seen.add(flat)
            if flat in good_flat:
                continue
            out[k] = (flat // n1, flat % n1)
            k += 1
            if k == no:
                break
    return np.concatenate([out, Agt], axis=0), Agt
