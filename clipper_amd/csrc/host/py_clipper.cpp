// py_clipper.cpp — pybind11 module `clipperpy`: the reference's Python surface
// (bindings/python/py_clipper.cpp:116-233, trampolines.h:14-30) over the clipper:: facade of
// this build. Same module / submodule / class / method / field names and argument order.
//
// The reference converts numpy <-> Eigen with pybind11/eigen.h and `noconvert()` arguments
// (float64 data, int32 associations). Eigen is not available here, so small type casters do
// the same for the facade's containers: dtype must match when the argument is `noconvert`,
// any memory layout is accepted and copied to column-major.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <sstream>

#include "clipper/batch.h"
#include "clipper/clipper.h"
#include "clipper/device_cloud.h"
#include "clipper/invariants/device.h"
#include "clipper/registration.h"
#include "clipper/sdp.h"
#include "clipper/utils.h"

namespace py = pybind11;
using namespace pybind11::literals;

#ifndef CLIPPER_VERSION
#define CLIPPER_VERSION "0.2.4+mi355x.1"
#endif

// ------------------------------------------------------------------------------------------
// numpy <-> facade containers
// ------------------------------------------------------------------------------------------
namespace pybind11 {
namespace detail {

template <typename T>
struct dense_matrix_caster {
  using Mat = clipper::DenseMatrix<T>;
  static bool load_into(handle src, bool convert, Mat& out, int fixed_cols) {
    if (!src) return false;
    if (!convert && !isinstance<array_t<T>>(src)) return false;  // `noconvert`: dtype must match
    auto arr = array_t<T, array::f_style | array::forcecast>::ensure(src);
    if (!arr) return false;
    if (arr.ndim() == 1 && arr.shape(0) == 0) {  // empty -> 0 x cols
      out.resize(0, fixed_cols > 0 ? fixed_cols : 0);
      return true;
    }
    if (arr.ndim() != 2) return false;
    if (fixed_cols > 0 && arr.shape(1) != fixed_cols && arr.size() != 0) return false;
    out.resize(arr.shape(0), arr.shape(1));
    if (arr.size() > 0) std::memcpy(out.data(), arr.data(), sizeof(T) * static_cast<size_t>(arr.size()));
    return true;
  }
  static handle to_numpy(const Mat& m) {
    array_t<T, array::f_style> a({m.rows(), m.cols()});
    if (m.size() > 0) std::memcpy(a.mutable_data(), m.data(), sizeof(T) * static_cast<size_t>(m.size()));
    return a.release();
  }
};

template <>
struct type_caster<clipper::MatrixXd> {
  PYBIND11_TYPE_CASTER(clipper::MatrixXd, const_name("numpy.ndarray[numpy.float64[m, n]]"));
  bool load(handle src, bool convert) {
    return dense_matrix_caster<double>::load_into(src, convert, value, 0);
  }
  static handle cast(const clipper::MatrixXd& m, return_value_policy, handle) {
    return dense_matrix_caster<double>::to_numpy(m);
  }
};

template <>
struct type_caster<clipper::Association> {
  PYBIND11_TYPE_CASTER(clipper::Association, const_name("numpy.ndarray[numpy.int32[m, 2]]"));
  bool load(handle src, bool convert) {
    return dense_matrix_caster<int>::load_into(src, convert, value, 2);
  }
  static handle cast(const clipper::Association& m, return_value_policy, handle) {
    return dense_matrix_caster<int>::to_numpy(m);
  }
};

template <>
struct type_caster<clipper::VectorXd> {
  PYBIND11_TYPE_CASTER(clipper::VectorXd, const_name("numpy.ndarray[numpy.float64[m, 1]]"));
  bool load(handle src, bool convert) {
    if (!src) return false;
    if (!convert && !isinstance<array_t<double>>(src)) return false;
    auto arr = array_t<double, array::c_style | array::forcecast>::ensure(src);
    if (!arr) return false;
    if (arr.ndim() > 2) return false;
    if (arr.ndim() == 2 && arr.shape(0) != 1 && arr.shape(1) != 1 && arr.size() != 0) return false;
    value.resize(arr.size());
    if (arr.size() > 0) std::memcpy(value.data(), arr.data(), sizeof(double) * static_cast<size_t>(arr.size()));
    return true;
  }
  static handle cast(const clipper::VectorXd& v, return_value_policy, handle) {
    array_t<double> a(static_cast<py::ssize_t>(v.size()));
    if (v.size() > 0) std::memcpy(a.mutable_data(), v.data(), sizeof(double) * static_cast<size_t>(v.size()));
    return a.release();
  }
};

}  // namespace detail
}  // namespace pybind11

// ------------------------------------------------------------------------------------------
// trampolines (reference bindings/python/trampolines.h:14-30)
// ------------------------------------------------------------------------------------------
template <class InvariantBase = clipper::invariants::Invariant>
class PyInvariant : public InvariantBase {
 public:
  using InvariantBase::InvariantBase;
};

template <class PairwiseInvariantBase = clipper::invariants::PairwiseInvariant>
class PyPairwiseInvariant : public PyInvariant<PairwiseInvariantBase> {
 public:
  using PyInvariant<PairwiseInvariantBase>::PyInvariant;
  using Datum = clipper::invariants::Datum;
  double operator()(const Datum& ai, const Datum& aj, const Datum& bi, const Datum& bj) override {
    pybind11::gil_scoped_acquire acquire;  // the scoring loop may run without the GIL
    PYBIND11_OVERRIDE_PURE_NAME(double, PairwiseInvariantBase, "__call__", operator(), ai, aj, bi, bj);
  }
};

// non-pure variant for the built-ins (a Python subclass may or may not override __call__)
template <class Builtin>
class PyBuiltinInvariant : public Builtin {
 public:
  using Builtin::Builtin;
  using Datum = clipper::invariants::Datum;
  double operator()(const Datum& ai, const Datum& aj, const Datum& bi, const Datum& bj) override {
    pybind11::gil_scoped_acquire acquire;
    PYBIND11_OVERRIDE_NAME(double, Builtin, "__call__", operator(), ai, aj, bi, bj);
  }
};

// ------------------------------------------------------------------------------------------

void pybind_invariants(py::module& m) {
  m.doc() =
      "Invariants are quantities that do not change under the transformation between two sets "
      "of objects. They are used to build a consistency graph. Some built-in invariants are "
      "provided.";
  using namespace clipper::invariants;

  py::class_<Invariant, PyInvariant<>, std::shared_ptr<Invariant>>(m, "Invariant").def(py::init<>());
  py::class_<PairwiseInvariant, Invariant, PyPairwiseInvariant<>, std::shared_ptr<PairwiseInvariant>>(
      m, "PairwiseInvariant")
      .def(py::init<>())
      .def("__call__", &PairwiseInvariant::operator());

  py::class_<EuclideanDistance::Params>(m, "EuclideanDistanceParams")
      .def(py::init<>())
      .def("__repr__",
           [](const EuclideanDistance::Params& p) {
             std::ostringstream r;
             r << "<EuclideanDistanceParams : sigma=" << p.sigma << " epsilon=" << p.epsilon
               << " mindist=" << p.mindist << ">";
             return r.str();
           })
      .def_readwrite("sigma", &EuclideanDistance::Params::sigma)
      .def_readwrite("epsilon", &EuclideanDistance::Params::epsilon)
      .def_readwrite("mindist", &EuclideanDistance::Params::mindist);

  py::class_<EuclideanDistance, PairwiseInvariant, PyBuiltinInvariant<EuclideanDistance>,
             std::shared_ptr<EuclideanDistance>>(m, "EuclideanDistance")
      .def(py::init<const EuclideanDistance::Params&>());

  py::class_<PointNormalDistance::Params>(m, "PointNormalDistanceParams")
      .def(py::init<>())
      .def("__repr__",
           [](const PointNormalDistance::Params& p) {
             std::ostringstream r;
             r << "<PointNormalDistanceParams : sigp=" << p.sigp << " epsp=" << p.epsp
               << " sign=" << p.sign << " epsn=" << p.epsn << ">";
             return r.str();
           })
      .def_readwrite("sigp", &PointNormalDistance::Params::sigp)
      .def_readwrite("epsp", &PointNormalDistance::Params::epsp)
      .def_readwrite("sign", &PointNormalDistance::Params::sign)
      .def_readwrite("epsn", &PointNormalDistance::Params::epsn);

  py::class_<PointNormalDistance, PairwiseInvariant, PyBuiltinInvariant<PointNormalDistance>,
             std::shared_ptr<PointNormalDistance>>(m, "PointNormalDistance")
      .def(py::init<const PointNormalDistance::Params&>());

  // HIP device source, compiled at run time and evaluated on the GPU (include/clipper/invariants/device.h)
  py::class_<DeviceInvariant, PairwiseInvariant, std::shared_ptr<DeviceInvariant>>(m, "DeviceInvariant")
      .def(py::init<std::string, std::vector<double>>(), "source"_a, "params"_a = std::vector<double>())
      .def_property_readonly("source", &DeviceInvariant::source)
      .def_property_readonly("params", &DeviceInvariant::params);
}

void pybind_utils(py::module& m) {
  m.doc() = "Various convenience utilities for working with CLIPPER";
  m.def("create_all_to_all", clipper::utils::createAllToAll, "n1"_a, "n2"_a,
        "Create an all-to-all hypothesis for association. Useful for the case of no prior "
        "information or putative associations.");
  m.def("k2ij", clipper::utils::k2ij, "k"_a, "n"_a,
        "Maps a flat index k to coordinate of a square nxn symmetric matrix");
}

// what utils.icp and utils.icp_generalized return: (T 4 x 4, info)
static py::tuple icp_tuple(const clipper::registration::IcpResult& r) {
  clipper::MatrixXd T(4, 4), H(3, static_cast<std::ptrdiff_t>(r.history.size()));
  for (int i = 0; i < 16; ++i) T.data()[i] = r.T[i];
  for (size_t k = 0; k < r.history.size(); ++k)
    for (int c = 0; c < 3; ++c) H.data()[3 * k + c] = r.history[k][c];
  py::dict info;
  info["iterations"] = r.iterations;
  info["status"] = static_cast<int>(r.status);
  info["count"] = r.count;
  info["fitness"] = r.fitness;
  info["inlier_rmse"] = r.inlier_rmse;
  info["route"] = static_cast<int>(r.route);
  info["candidates"] = r.candidates;
  info["device_ms"] = r.device_ms;
  info["history"] = py::cast(H).attr("T");  // (iterations + 1) x 3: count, fitness, rmse
  return py::make_tuple(T, info);
}

// utils.icp_robust and utils.icp_generalized_robust: the same tuple, info also holding the robust call's three fields
static py::tuple icp_robust_tuple(const clipper::registration::IcpRobustResult& r) {
  py::tuple out = icp_tuple(r);
  py::dict info = out[1].cast<py::dict>();
  info["within"] = r.within;
  info["weight_sum"] = r.weight_sum;
  info["trim_sqd"] = r.trim_sqd;
  return out;
}

static clipper::registration::IcpRobust icp_robust_of(const std::string& loss, double scale, double trim) {
  namespace reg = clipper::registration;
  static const char* const names[] = {"none", "huber", "cauchy", "tukey", "geman_mcclure"};
  for (int l = 0; l < 5; ++l)
    if (loss == names[l]) return reg::IcpRobust{static_cast<reg::IcpLoss>(l), scale, trim};
  throw std::invalid_argument("loss must be one of \"none\", \"huber\", \"cauchy\", \"tukey\", \"geman_mcclure\"");
}

// the method string and the numeric keywords of an ICP binding as IcpParams. with_generalized: the call takes
// "generalized" besides "point" and "plane" (DeviceCloud.icp; the generalized bindings pass that name themselves)
static clipper::registration::IcpParams icp_params_of(const std::string& method, bool with_generalized, double max_distance,
                                                      int max_iterations, double rel_fitness, double rel_rmse) {
  namespace reg = clipper::registration;
  static const char* const names[] = {"point", "plane", "generalized"};
  for (int k = 0; k < (with_generalized ? 3 : 2); ++k)
    if (method == names[k])
      return reg::IcpParams{static_cast<reg::IcpMethod>(k), max_distance, max_iterations, rel_fitness, rel_rmse};
  throw std::invalid_argument(with_generalized ? "method must be \"point\", \"plane\" or \"generalized\""
                                               : "method must be \"point\" or \"plane\"");
}

PYBIND11_MODULE(clipperpy, m) {
  m.doc() = "A graph-theoretic framework for robust data association (MI355X hot path)";
  m.attr("__version__") = CLIPPER_VERSION;

  py::module m_invariants = m.def_submodule("invariants");
  pybind_invariants(m_invariants);

  py::module m_utils = m.def_submodule("utils");
  pybind_utils(m_utils);
  // putative associations from feature descriptors, on the device (include/clipper/registration.h)
  m_utils.def(
      "match_descriptors",
      [](const clipper::MatrixXd& F0, const clipper::MatrixXd& F1, int knn, bool mutual, double ratio,
         double max_sqdist) {
        clipper::registration::MatchParams prm;
        prm.knn = knn;
        prm.mutual = mutual;
        prm.ratio = ratio;
        prm.max_sqdist = max_sqdist;
        return clipper::registration::match_descriptors(F0, F1, prm);
      },
      "F0"_a, "F1"_a, "knn"_a = 1, "mutual"_a = true, "ratio"_a = 0.0, "max_sqdist"_a = 0.0,
      "Match feature descriptors (d x n0 and d x n1, one per column, d <= 64) into putative associations on the GPU: "
      "brute-force nearest neighbours with an optional mutual check, ratio test and distance bound.");

  // the step in front of the normals: one point per occupied voxel, on the device
  m_utils.def(
      "voxel_down_sample",
      [](const clipper::MatrixXd& P, double voxel_size, const clipper::MatrixXd& normals, bool return_counts, bool return_trace) {
        const clipper::registration::VoxelDownSampled r =
            clipper::registration::voxel_down_sample(P, voxel_size, normals, return_trace);
        py::list out;
        out.append(r.points);
        if (normals.cols() > 0) out.append(r.normals);
        if (return_counts) out.append(py::array_t<int32_t>(static_cast<py::ssize_t>(r.counts.size()), r.counts.data()));
        if (return_trace) out.append(py::array_t<int32_t>(static_cast<py::ssize_t>(r.trace.size()), r.trace.data()));
        return out.size() == 1 ? py::object(out[0]) : py::object(py::tuple(out));
      },
      "P"_a, "voxel_size"_a, "normals"_a = clipper::MatrixXd(3, 0), "return_counts"_a = false, "return_trace"_a = false,
      "One point per occupied voxel of edge voxel_size of the cloud P (3 x n, one point per column) on the GPU: the "
      "centroid of the voxel's points, in ascending cell number (z, y, x; the origin is the cloud's minimum corner). With "
      "normals (3 x n) also their normalised sum per voxel; with return_counts the points per voxel, with return_trace "
      "every input point's output column. The same bits from run to run.");

  // the stage in front of the matcher: raw cloud -> normals -> FPFH descriptors, on the device
  m_utils.def(
      "estimate_normals",
      [](const clipper::MatrixXd& P, int knn, double radius, const std::vector<double>& viewpoint) {
        if (!viewpoint.empty() && viewpoint.size() != 3) throw std::invalid_argument("viewpoint must have 3 coordinates");
        return clipper::registration::estimate_normals(P, clipper::registration::Neighborhood{knn, radius},
                                                       viewpoint.empty() ? nullptr : viewpoint.data());
      },
      "P"_a, "knn"_a = 16, "radius"_a = 0.0, "viewpoint"_a = std::vector<double>{},
      "Unit surface normals (3 x n) of the cloud P (3 x n, one point per column) on the GPU: per point the smallest "
      "eigenvector of the covariance of its knn nearest points (itself included; with radius > 0 only those within it), "
      "signed towards the viewpoint, or without one with its largest component positive.");
  m_utils.def(
      "compute_fpfh",
      [](const clipper::MatrixXd& P, const clipper::MatrixXd& N, int knn, double radius) {
        return clipper::registration::compute_fpfh(P, N, clipper::registration::Neighborhood{knn, radius});
      },
      "P"_a, "N"_a, "knn"_a = 32, "radius"_a = 0.0,
      "FPFH descriptors (33 x n, one per column: what match_descriptors takes) of the cloud P with unit normals N "
      "(both 3 x n) on the GPU.");

  // the step behind the solve: local refinement of the closed-form transform over the whole clouds, on the device
  m_utils.def(
      "icp",
      [](const clipper::MatrixXd& src, const clipper::MatrixXd& tgt, const clipper::MatrixXd& T_init, const std::string& method,
         const clipper::MatrixXd& normals, double max_distance, int max_iterations, double rel_fitness, double rel_rmse) {
        namespace reg = clipper::registration;
        const reg::IcpParams prm = icp_params_of(method, false, max_distance, max_iterations, rel_fitness, rel_rmse);
        if (T_init.rows() != 4 || T_init.cols() != 4) throw std::invalid_argument("T_init must be 4 x 4");
        const reg::IcpResult r = reg::icp(src, tgt, prm, T_init.data(), normals);
        return icp_tuple(r);
      },
      "src"_a, "tgt"_a, "T_init"_a, "method"_a = "point", "normals"_a = clipper::MatrixXd(3, 0), "max_distance"_a = 0.0,
      "max_iterations"_a = 30, "rel_fitness"_a = 1e-6, "rel_rmse"_a = 1e-6,
      "ICP on the GPU: refine the alignment T_init (4 x 4) of the cloud src onto tgt (3 x n, one point per column). method "
      "\"point\", or \"plane\" over the target's unit normals (3 x n_tgt). Returns (T, info): info holds iterations, status "
      "(0 converged, 1 max iterations, 2 too few inliers, 3 degenerate), count, fitness, inlier_rmse, route, candidates, "
      "device_ms and history ((iterations + 1) x 3: count, fitness, rmse).");
  // generalized ICP: the covariances of a cloud, and the refinement over them
  m_utils.def(
      "estimate_covariances",
      [](const clipper::MatrixXd& P, int knn, double radius, double epsilon) {
        return clipper::registration::estimate_covariances(P, clipper::registration::Neighborhood{knn, radius}, epsilon);
      },
      "P"_a, "knn"_a = 20, "radius"_a = 0.0, "epsilon"_a = 1e-3,
      "Per-point covariances (6 x n: xx, xy, xz, yy, yz, zz per column) of the cloud P (3 x n) on the GPU for "
      "icp_generalized: I - (1 - epsilon) n n^T over the normal n of the point's knn nearest points (itself included; "
      "with radius > 0 only those within it); the identity below 3 neighbours.");
  m_utils.def(
      "icp_generalized",
      [](const clipper::MatrixXd& src, const clipper::MatrixXd& src_cov, const clipper::MatrixXd& tgt,
         const clipper::MatrixXd& tgt_cov, const clipper::MatrixXd& T_init, double max_distance, int max_iterations,
         double rel_fitness, double rel_rmse) {
        namespace reg = clipper::registration;
        if (T_init.rows() != 4 || T_init.cols() != 4) throw std::invalid_argument("T_init must be 4 x 4");
        const reg::IcpParams prm = icp_params_of("generalized", true, max_distance, max_iterations, rel_fitness, rel_rmse);
        const reg::IcpResult r = reg::icp_generalized(src, src_cov, tgt, tgt_cov, prm, T_init.data());
        return icp_tuple(r);
      },
      "src"_a, "src_cov"_a, "tgt"_a, "tgt_cov"_a, "T_init"_a, "max_distance"_a = 0.0, "max_iterations"_a = 30,
      "rel_fitness"_a = 1e-6, "rel_rmse"_a = 1e-6,
      "Generalized ICP on the GPU: refine the alignment T_init (4 x 4) of src onto tgt (3 x n) with the plane-to-plane "
      "metric over the clouds' covariances (6 x n, e.g. estimate_covariances'). Returns (T, info) as icp does.");
  // robust losses and trimming: icp and icp_generalized with a defence against bad pairs
  m_utils.def(
      "icp_robust",
      [](const clipper::MatrixXd& src, const clipper::MatrixXd& tgt, const clipper::MatrixXd& T_init, const std::string& method,
         const clipper::MatrixXd& normals, double max_distance, int max_iterations, double rel_fitness, double rel_rmse,
         const std::string& loss, double scale, double trim) {
        namespace reg = clipper::registration;
        const reg::IcpParams prm = icp_params_of(method, false, max_distance, max_iterations, rel_fitness, rel_rmse);
        if (T_init.rows() != 4 || T_init.cols() != 4) throw std::invalid_argument("T_init must be 4 x 4");
        const reg::IcpRobustResult r = reg::icp_robust(src, tgt, prm, icp_robust_of(loss, scale, trim), T_init.data(), normals);
        return icp_robust_tuple(r);
      },
      "src"_a, "tgt"_a, "T_init"_a, "method"_a = "point", "normals"_a = clipper::MatrixXd(3, 0), "max_distance"_a = 0.0,
      "max_iterations"_a = 30, "rel_fitness"_a = 1e-6, "rel_rmse"_a = 1e-6, "loss"_a = "none", "scale"_a = 0.0, "trim"_a = 1.0,
      "icp with a robust loss (\"huber\", \"cauchy\", \"tukey\", \"geman_mcclure\"; scale: a distance) weighing every pair by "
      "its residual, and / or trimming: each iteration keeps the fraction trim of the points within max_distance with the "
      "smallest distances. Returns (T, info) as icp does, info also holding within, weight_sum and trim_sqd. \"tukey\" and "
      "\"geman_mcclure\" give pairs far beyond the scale no weight: start them close to the answer.");
  m_utils.def(
      "icp_generalized_robust",
      [](const clipper::MatrixXd& src, const clipper::MatrixXd& src_cov, const clipper::MatrixXd& tgt,
         const clipper::MatrixXd& tgt_cov, const clipper::MatrixXd& T_init, double max_distance, int max_iterations,
         double rel_fitness, double rel_rmse, const std::string& loss, double scale, double trim) {
        namespace reg = clipper::registration;
        if (T_init.rows() != 4 || T_init.cols() != 4) throw std::invalid_argument("T_init must be 4 x 4");
        const reg::IcpParams prm = icp_params_of("generalized", true, max_distance, max_iterations, rel_fitness, rel_rmse);
        const reg::IcpRobustResult r =
            reg::icp_generalized_robust(src, src_cov, tgt, tgt_cov, prm, icp_robust_of(loss, scale, trim), T_init.data());
        return icp_robust_tuple(r);
      },
      "src"_a, "src_cov"_a, "tgt"_a, "tgt_cov"_a, "T_init"_a, "max_distance"_a = 0.0, "max_iterations"_a = 30,
      "rel_fitness"_a = 1e-6, "rel_rmse"_a = 1e-6, "loss"_a = "none", "scale"_a = 0.0, "trim"_a = 1.0,
      "icp_generalized with icp_robust's loss and trimming; the residual a loss weighs is d^T M d of the pair.");
  m_utils.def(
      "evaluate_registration",
      [](const clipper::MatrixXd& src, const clipper::MatrixXd& tgt, const clipper::MatrixXd& T, double max_distance) {
        if (T.rows() != 4 || T.cols() != 4) throw std::invalid_argument("T must be 4 x 4");
        const clipper::registration::RegistrationQuality q = clipper::registration::evaluate_registration(src, tgt, T.data(), max_distance);
        return py::make_tuple(q.fitness, q.inlier_rmse, q.count);
      },
      "src"_a, "tgt"_a, "T"_a, "max_distance"_a,
      "(fitness, inlier_rmse, count) of the alignment T (4 x 4) of src onto tgt (3 x n) on the GPU: a source point is an "
      "inlier when its nearest target point lies within max_distance.");

  // the consensus estimator over putative associations, on the device
  m_utils.def(
      "ransac_correspondences",
      [](const clipper::MatrixXd& D1, const clipper::MatrixXd& D2, const clipper::Association& A, double max_distance,
         int n_sample, double edge_similarity, int64_t max_hypotheses, double confidence, uint64_t seed, int refine_iterations,
         int hypotheses_per_round, int device) {
        namespace reg = clipper::registration;
        reg::RansacParams prm;
        prm.max_distance = max_distance;
        prm.n_sample = n_sample;
        prm.edge_similarity = edge_similarity;
        prm.max_hypotheses = max_hypotheses;
        prm.confidence = confidence;
        prm.seed = seed;
        prm.refine_iterations = refine_iterations;
        prm.hypotheses_per_round = hypotheses_per_round;
        const reg::RansacInfo r = reg::ransac_correspondences(D1, D2, A, prm, device);
        clipper::MatrixXd T(4, 4);
        for (int i = 0; i < 16; ++i) T.data()[i] = r.T[i];
        py::array_t<bool> mask(static_cast<py::ssize_t>(r.inliers.size()));
        for (size_t k = 0; k < r.inliers.size(); ++k) mask.mutable_at(static_cast<py::ssize_t>(k)) = r.inliers[k] != 0;
        py::dict info;
        info["status"] = static_cast<int>(r.status);
        info["refined"] = r.refined;
        info["evaluated"] = r.evaluated;
        info["checked"] = r.checked;
        info["best_hypothesis"] = r.best_hypothesis;
        info["best_count"] = r.best_count;
        info["count"] = r.count;
        info["fitness"] = r.fitness;
        info["inlier_rmse"] = r.inlier_rmse;
        info["sample"] = std::vector<int32_t>(r.sample.begin(), r.sample.end());
        info["device_ms"] = r.device_ms;
        info["inliers"] = mask;
        return py::make_tuple(T, info);
      },
      "D1"_a, "D2"_a, "A"_a, "max_distance"_a, "n_sample"_a = 3, "edge_similarity"_a = 0.9, "max_hypotheses"_a = 100000,
      "confidence"_a = 0.999, "seed"_a = 0, "refine_iterations"_a = 1, "hypotheses_per_round"_a = 4096, "device"_a = 0,
      "RANSAC over the putative associations A (m x 2) between D1 and D2 (3 x n, one point per column) on the GPU: the "
      "rigid transform most associations agree on within max_distance. Returns (T, info): info holds status (0 converged, "
      "1 max hypotheses, 2 no model), inliers (a boolean mask over A), count, fitness, inlier_rmse, best_hypothesis, "
      "best_count, sample, evaluated, checked, refined and device_ms. The same inputs and seed give the same bytes.");

  // the route of the d = 3 nearest-neighbour search behind them ("The grid route of the search"): process-wide
  py::enum_<clipper::registration::KnnSearch>(m_utils, "KnnSearch")
      .value("Brute", clipper::registration::KnnSearch::Brute)
      .value("Grid", clipper::registration::KnnSearch::Grid)
      .value("Auto", clipper::registration::KnnSearch::Auto);
  m_utils.def("set_knn_search", &clipper::registration::setKnnSearch, "search"_a,
              "Select the route of the 3-D nearest-neighbour search: brute force (default), a uniform grid on the GPU, or "
              "the grid from a measured cloud size on. Every route returns the same lists, bit for bit.");
  m_utils.def("knn_search", &clipper::registration::knnSearch);

  // clouds and association lists that live on the device (include/clipper/device_cloud.h): the front end without
  // crossing the bus between its stages. close() frees the device memory (twice is harmless); a closed handle raises.
  {
    namespace reg = clipper::registration;
    py::class_<reg::DevicePairs>(m_utils, "DevicePairs")
        .def(py::init([](const clipper::Association& A, const std::vector<double>& sqd, int device) {
               return new reg::DevicePairs(A, sqd, device);
             }),
             "A"_a, "sqd"_a = std::vector<double>{}, "device"_a = 0)
        .def("__len__", &reg::DevicePairs::size)
        .def_property_readonly("has_sqd", &reg::DevicePairs::hasSqd)
        .def("download", [](const reg::DevicePairs& p) { return p.download(); })
        .def("download_with_sqd",
             [](const reg::DevicePairs& p) {
               std::vector<double> sqd;
               clipper::Association A = p.download(&sqd);
               return py::make_tuple(A, py::array_t<double>(static_cast<py::ssize_t>(sqd.size()), sqd.data()));
             })
        .def("close", &reg::DevicePairs::close)
        .def("__enter__", [](py::object self) { return self; })
        .def("__exit__", [](reg::DevicePairs& p, const py::args&) { p.close(); });
    py::class_<reg::DeviceCloud>(m_utils, "DeviceCloud")
        .def(py::init([](const clipper::MatrixXd& P, const clipper::MatrixXd& normals, int device) {
               return new reg::DeviceCloud(P, normals, device);
             }),
             "P"_a, "normals"_a = clipper::MatrixXd(3, 0), "device"_a = 0)
        .def("__len__", &reg::DeviceCloud::size)
        .def("points", &reg::DeviceCloud::points)
        .def("normals", &reg::DeviceCloud::normals)
        .def("descriptors", &reg::DeviceCloud::descriptors)
        .def("spfh", &reg::DeviceCloud::spfh)
        .def("covariances", &reg::DeviceCloud::covariances)
        .def("grid_builds", [](const reg::DeviceCloud& c) { return c.info().grid_builds; })
        .def("info",
             [](const reg::DeviceCloud& c) {
               const clipper_hip_cloud_info_t i = c.info();
               py::dict d;
               d["n"] = i.n;
               d["trace_n"] = i.trace_n;
               d["device"] = i.device;
               d["has_normals"] = i.has_normals != 0;
               d["descriptor_dim"] = i.descriptor_dim;
               d["has_spfh"] = i.has_spfh != 0;
               d["has_covariances"] = i.has_covariances != 0;
               d["has_voxel_counts"] = i.has_voxel_counts != 0;
               d["grid_builds"] = i.grid_builds;
               d["grid_dim"] = py::make_tuple(i.grid_dim[0], i.grid_dim[1], i.grid_dim[2]);
               return d;
             })
        .def("counts",
             [](const reg::DeviceCloud& c, const std::string& what) {
               static const char* const names[] = {"normals", "fpfh", "covariances", "voxel", "voxel_trace"};
               static const int whats[] = {CLIPPER_HIP_CLOUD_NORMAL_COUNTS, CLIPPER_HIP_CLOUD_FPFH_COUNTS,
                                           CLIPPER_HIP_CLOUD_COVARIANCE_COUNTS, CLIPPER_HIP_CLOUD_VOXEL_COUNTS,
                                           CLIPPER_HIP_CLOUD_VOXEL_TRACE};
               for (int k = 0; k < 5; ++k)
                 if (what == names[k]) {
                   const std::vector<int32_t> v = c.counts(whats[k]);
                   return py::array_t<int32_t>(static_cast<py::ssize_t>(v.size()), v.data());
                 }
               throw std::invalid_argument("what must be \"normals\", \"fpfh\", \"covariances\", \"voxel\" or \"voxel_trace\"");
             },
             "what"_a)
        .def("fpfh_from_points",
             [](reg::DeviceCloud& c, int normal_knn, double normal_radius, const std::vector<double>& viewpoint, int knn,
                double radius) {
               if (!viewpoint.empty() && viewpoint.size() != 3) throw std::invalid_argument("viewpoint must have 3 coordinates");
               c.computeFpfh(reg::Neighborhood{normal_knn, normal_radius}, viewpoint.empty() ? nullptr : viewpoint.data(),
                             reg::Neighborhood{knn, radius});
             },
             "normal_knn"_a = 16, "normal_radius"_a = 0.0, "viewpoint"_a = std::vector<double>{}, "knn"_a = 32, "radius"_a = 0.0)
        .def("evaluate_registration",
             [](const reg::DeviceCloud& c, reg::DeviceCloud& target, const py::object& T, double max_distance) {
               clipper::MatrixXd T0;
               if (!T.is_none()) {
                 T0 = T.cast<clipper::MatrixXd>();
                 if (T0.rows() != 4 || T0.cols() != 4) throw std::invalid_argument("T must be 4 x 4");
               }
               int64_t count = 0;
               const std::pair<double, double> fr = c.evaluateRegistration(target, T.is_none() ? nullptr : T0.data(), max_distance, &count);
               return py::make_tuple(fr.first, fr.second, count);
             },
             "target"_a, "T"_a = py::none(), "max_distance"_a = 0.0)
        .def("set_descriptors", [](reg::DeviceCloud& c, const clipper::MatrixXd& F) { c.setDescriptors(F); }, "F"_a)
        .def("voxel_down_sample",
             [](reg::DeviceCloud& c, double voxel_size, bool return_trace) {
               return new reg::DeviceCloud(c.voxelDownSample(voxel_size, return_trace));
             },
             "voxel_size"_a, "return_trace"_a = false, py::return_value_policy::take_ownership)
        .def("estimate_normals",
             [](reg::DeviceCloud& c, int knn, double radius, const std::vector<double>& viewpoint) {
               if (!viewpoint.empty() && viewpoint.size() != 3) throw std::invalid_argument("viewpoint must have 3 coordinates");
               c.estimateNormals(reg::Neighborhood{knn, radius}, viewpoint.empty() ? nullptr : viewpoint.data());
             },
             "knn"_a = 16, "radius"_a = 0.0, "viewpoint"_a = std::vector<double>{})
        .def("compute_fpfh", [](reg::DeviceCloud& c, int knn, double radius) { c.computeFpfh(reg::Neighborhood{knn, radius}); },
             "knn"_a = 32, "radius"_a = 0.0)
        .def("estimate_covariances",
             [](reg::DeviceCloud& c, int knn, double radius, double epsilon) {
               c.estimateCovariances(reg::Neighborhood{knn, radius}, epsilon);
             },
             "knn"_a = 20, "radius"_a = 0.0, "epsilon"_a = 1e-3)
        .def("match",
             [](const reg::DeviceCloud& c, const reg::DeviceCloud& other, int knn, bool mutual, double ratio, double max_sqdist) {
               reg::MatchParams prm;
               prm.knn = knn;
               prm.mutual = mutual;
               prm.ratio = ratio;
               prm.max_sqdist = max_sqdist;
               return new reg::DevicePairs(c.match(other, prm));
             },
             "other"_a, "knn"_a = 1, "mutual"_a = true, "ratio"_a = 0.0, "max_sqdist"_a = 0.0,
             py::return_value_policy::take_ownership)
        .def("gather_points", &reg::DeviceCloud::gatherPoints, "idx"_a)
        .def("icp",
             [](const reg::DeviceCloud& c, reg::DeviceCloud& target, const std::string& method, double max_distance,
                int max_iterations, const py::object& T_init, const py::object& loss, double scale, double trim) {
               const reg::IcpParams def;  // (this binding has no keywords for the stop bounds: the facade's defaults)
               const reg::IcpParams prm = icp_params_of(method, true, max_distance, max_iterations, def.rel_fitness, def.rel_rmse);
               clipper::MatrixXd T0;
               if (!T_init.is_none()) {
                 T0 = T_init.cast<clipper::MatrixXd>();
                 if (T0.rows() != 4 || T0.cols() != 4) throw std::invalid_argument("T_init must be 4 x 4");
               }
               const double* t0 = T_init.is_none() ? nullptr : T0.data();
               if (loss.is_none()) return icp_tuple(c.icp(target, prm, t0));
               return icp_robust_tuple(c.icp(target, prm, icp_robust_of(loss.cast<std::string>(), scale, trim), t0));
             },
             "target"_a, "method"_a = "point", "max_distance"_a = 0.0, "max_iterations"_a = 30, "T_init"_a = py::none(),
             "loss"_a = py::none(), "scale"_a = 0.0, "trim"_a = 1.0)
        .def("close", &reg::DeviceCloud::close)
        .def("__enter__", [](py::object self) { return self; })
        .def("__exit__", [](reg::DeviceCloud& c, const py::args&) { c.close(); });
  }

  // The reference fills `clipperpy.dsd` with pybind_utils (py_clipper.cpp:127-128; pybind_dsd is
  // never called), so that is what existing scripts see; the exact DSD solver is out of scope.
  py::module m_dsd = m.def_submodule("dsd");
  pybind_utils(m_dsd);

  py::enum_<clipper::maxclique::Method>(m, "MCMethod")
      .value("EXACT", clipper::maxclique::Method::EXACT)
      .value("HEU", clipper::maxclique::Method::HEU)
      .value("KCORE", clipper::maxclique::Method::KCORE);

  py::class_<clipper::maxclique::Params>(m, "MCParams")
      .def(py::init<>())
      .def("__repr__", [](const clipper::maxclique::Params&) { return "<CLIPPER Maximum Clique Parameters>"; })
      .def_readwrite("method", &clipper::maxclique::Params::method)
      .def_readwrite("threads", &clipper::maxclique::Params::threads)
      .def_readwrite("time_limit", &clipper::maxclique::Params::time_limit)
      .def_readwrite("verbose", &clipper::maxclique::Params::verbose)
      .def_readwrite("warm_start", &clipper::maxclique::Params::warm_start);

  py::class_<clipper::sdp::Params>(m, "SDPParams")
      .def(py::init<>())
      .def("__repr__", [](const clipper::sdp::Params&) { return "<CLIPPER SDP Parameters>"; })
      .def_readwrite("verbose", &clipper::sdp::Params::verbose)
      .def_readwrite("max_iters", &clipper::sdp::Params::max_iters)
      .def_readwrite("acceleration_interval", &clipper::sdp::Params::acceleration_interval)
      .def_readwrite("acceleration_lookback", &clipper::sdp::Params::acceleration_lookback)
      .def_readwrite("eps_abs", &clipper::sdp::Params::eps_abs)
      .def_readwrite("eps_rel", &clipper::sdp::Params::eps_rel)
      .def_readwrite("eps_infeas", &clipper::sdp::Params::eps_infeas)
      .def_readwrite("time_limit_secs", &clipper::sdp::Params::time_limit_secs);

  // clipperpy.sdp: sdp::solve (sdp.h) on the device, and its Solution
  py::class_<clipper::sdp::Solution>(m, "SDPSolution")
      .def(py::init<>())
      .def("__repr__", [](const clipper::sdp::Solution&) { return "<CLIPPER SDP Solution>"; })
      .def_readwrite("X", &clipper::sdp::Solution::X)
      .def_readwrite("lambdas", &clipper::sdp::Solution::lambdas)
      .def_readwrite("evec1", &clipper::sdp::Solution::evec1)
      .def_readwrite("thr", &clipper::sdp::Solution::thr)
      .def_readwrite("nodes", &clipper::sdp::Solution::nodes)
      .def_readwrite("iters", &clipper::sdp::Solution::iters)
      .def_readwrite("pobj", &clipper::sdp::Solution::pobj)
      .def_readwrite("dobj", &clipper::sdp::Solution::dobj)
      .def_readwrite("t", &clipper::sdp::Solution::t)
      .def_readwrite("t_parse", &clipper::sdp::Solution::t_parse)
      .def_readwrite("t_scs", &clipper::sdp::Solution::t_scs)
      .def_readwrite("t_scs_setup", &clipper::sdp::Solution::t_scs_setup)
      .def_readwrite("t_scs_solve", &clipper::sdp::Solution::t_scs_solve)
      .def_readwrite("t_scs_linsys", &clipper::sdp::Solution::t_scs_linsys)
      .def_readwrite("t_scs_cone", &clipper::sdp::Solution::t_scs_cone)
      .def_readwrite("t_scs_accel", &clipper::sdp::Solution::t_scs_accel)
      .def_readwrite("t_extract", &clipper::sdp::Solution::t_extract);
  py::module m_sdp = m.def_submodule("sdp");
  m_sdp.def("solve", py::overload_cast<const clipper::MatrixXd&, const clipper::MatrixXd&, const clipper::sdp::Params&>(
                         &clipper::sdp::solve),
            "M"_a, "C"_a, "params"_a = clipper::sdp::Params{});
  // the route of the device solver ("The wide route"): process-wide
  py::enum_<clipper::sdp::Route>(m_sdp, "Route")
      .value("Workgroup", clipper::sdp::Route::Workgroup)
      .value("Auto", clipper::sdp::Route::Auto)
      .value("Wide", clipper::sdp::Route::Wide);
  m_sdp.def("set_route", &clipper::sdp::setRoute, "route"_a);
  m_sdp.def("route", &clipper::sdp::route);
  // many problems in one call: lists of M and of C ("Batches")
  m_sdp.def("solve_batch",
            py::overload_cast<const std::vector<clipper::MatrixXd>&, const std::vector<clipper::MatrixXd>&,
                              const clipper::sdp::Params&>(&clipper::sdp::solve),
            "Ms"_a, "Cs"_a, "params"_a = clipper::sdp::Params{});

  py::enum_<clipper::Params::Rounding>(m, "Rounding")
      .value("NONZERO", clipper::Params::Rounding::NONZERO)
      .value("DSD", clipper::Params::Rounding::DSD)
      .value("DSD_HEU", clipper::Params::Rounding::DSD_HEU)
      .export_values();

  py::class_<clipper::Params>(m, "Params")
      .def(py::init<>())
      .def("__repr__", [](const clipper::Params&) { return "<CLIPPER Parameters>"; })
      .def_readwrite("tol_u", &clipper::Params::tol_u)
      .def_readwrite("tol_F", &clipper::Params::tol_F)
      .def_readwrite("tol_Fop", &clipper::Params::tol_Fop)
      .def_readwrite("maxiniters", &clipper::Params::maxiniters)
      .def_readwrite("maxoliters", &clipper::Params::maxoliters)
      .def_readwrite("beta", &clipper::Params::beta)
      .def_readwrite("maxlsiters", &clipper::Params::maxlsiters)
      .def_readwrite("eps", &clipper::Params::eps)
      .def_readwrite("affinityeps", &clipper::Params::affinityeps)
      .def_readwrite("rescale_u0", &clipper::Params::rescale_u0)
      .def_readwrite("rounding", &clipper::Params::rounding);

  py::class_<clipper::Solution>(m, "Solution")
      .def(py::init<>())
      .def("__repr__", [](const clipper::Solution&) { return "<CLIPPER Solution>"; })
      .def_readwrite("t", &clipper::Solution::t)
      .def_readwrite("ifinal", &clipper::Solution::ifinal)
      .def_readwrite("nodes", &clipper::Solution::nodes)
      .def_readwrite("u0", &clipper::Solution::u0)
      .def_readwrite("u", &clipper::Solution::u)
      .def_readwrite("score", &clipper::Solution::score);

  py::enum_<clipper::CLIPPER::Storage>(m, "Storage")
      .value("F32", clipper::CLIPPER::Storage::F32)
      .value("F64", clipper::CLIPPER::Storage::F64)
      .value("F32_CSC", clipper::CLIPPER::Storage::F32_CSC)
      .value("F64_CSC", clipper::CLIPPER::Storage::F64_CSC);

  py::class_<clipper::CLIPPER>(m, "CLIPPER")
      .def(py::init([](const clipper::invariants::PairwiseInvariantPtr& invariant,
                       const clipper::Params& params) {
        clipper::CLIPPER* c = new clipper::CLIPPER(invariant, params);
        // Python-extended invariants cannot be evaluated from several OpenMP threads
        // (reference py_clipper.cpp:199-209, pybind11 issue 813): a Python subclass is an
        // instance of one of the trampoline types.
        const bool python_subclass =
            static_cast<bool>(std::dynamic_pointer_cast<PyPairwiseInvariant<>>(invariant)) ||
            static_cast<bool>(std::dynamic_pointer_cast<
                              PyBuiltinInvariant<clipper::invariants::EuclideanDistance>>(invariant)) ||
            static_cast<bool>(std::dynamic_pointer_cast<
                              PyBuiltinInvariant<clipper::invariants::PointNormalDistance>>(invariant));
        c->setParallelize(!python_subclass);
        return c;
      }),
           // keep the Python invariant object (and with it a Python-side __call__ override) alive
           // for as long as the CLIPPER object holds its C++ half
           py::keep_alive<1, 2>())
      .def("__repr__", [](const clipper::CLIPPER&) { return "<CLIPPER>"; })
      .def("score_pairwise_consistency",
           static_cast<void (clipper::CLIPPER::*)(const clipper::invariants::Data&, const clipper::invariants::Data&,
                                                  const clipper::Association&)>(&clipper::CLIPPER::scorePairwiseConsistency),
           "D1"_a.noconvert(), "D2"_a.noconvert(), "A"_a.noconvert())
      .def("score_pairwise_consistency",
           static_cast<void (clipper::CLIPPER::*)(const clipper::registration::DeviceCloud&,
                                                  const clipper::registration::DeviceCloud&,
                                                  const clipper::registration::DevicePairs&)>(
               &clipper::CLIPPER::scorePairwiseConsistency),
           "c1"_a, "c2"_a, "pairs"_a,
           "The same from two utils.DeviceCloud and a utils.DevicePairs: staged and scored on the GPU from device data.")
      .def("solve", &clipper::CLIPPER::solve, "u0"_a.noconvert() = clipper::VectorXd())
      .def("solve_as_maximum_clique",
           [](clipper::CLIPPER& c, const clipper::maxclique::Params& params, const py::object& seed) {
             if (seed.is_none()) c.solveAsMaximumClique(params);
             else c.solveAsMaximumClique(params, seed.cast<std::vector<int>>());
           },
           "params"_a = clipper::maxclique::Params{}, "seed"_a = py::none())
      .def("solve_as_msrc_sdr", &clipper::CLIPPER::solveAsMSRCSDR, "params"_a = clipper::sdp::Params{})
      .def("set_device_sdp", &clipper::CLIPPER::setDeviceSdp, "on"_a)
      .def("get_initial_associations", &clipper::CLIPPER::getInitialAssociations)
      .def("get_selected_associations", &clipper::CLIPPER::getSelectedAssociations)
      .def("get_solution", &clipper::CLIPPER::getSolution)
      .def("get_affinity_matrix", &clipper::CLIPPER::getAffinityMatrix)
      .def("get_constraint_matrix", &clipper::CLIPPER::getConstraintMatrix)
      .def("set_matrix_data", &clipper::CLIPPER::setMatrixData, "M"_a.noconvert(), "C"_a.noconvert())
      .def("set_parallelize", &clipper::CLIPPER::setParallelize)
      // additions of this build
      .def("set_device", &clipper::CLIPPER::setDevice, "device"_a)
      .def("set_devices", &clipper::CLIPPER::setDevices, "devices"_a)
      .def("set_live_subproblem", &clipper::CLIPPER::setLiveSubproblem, "on"_a)
      .def("last_solve_passes_on_the_subproblem", &clipper::CLIPPER::lastSolvePassesOnTheSubproblem)
      .def("set_storage", &clipper::CLIPPER::setStorage, "storage"_a)
      .def("set_resident_solver", &clipper::CLIPPER::setResidentSolver, "on"_a)
      .def("set_row_views", &clipper::CLIPPER::setRowViews, "on"_a)
      .def("last_solve_passes_on_a_view", &clipper::CLIPPER::lastSolvePassesOnAView)
      .def("last_solve_was_resident", &clipper::CLIPPER::lastSolveWasResident)
      .def("get_path_stats", [](const clipper::CLIPPER& c) {
        const auto s = c.getPathStats();
        return py::dict("n_passes"_a = s.n_passes, "n_trials"_a = s.n_trials,
                        "affinity_kernel_ms"_a = s.affinity_kernel_ms, "d"_a = s.d);
      });

  // an addition of this build: many problems in one call (include/clipper/batch.h)
  py::class_<clipper::CLIPPERBatch>(m, "CLIPPERBatch")
      .def(py::init<const clipper::invariants::PairwiseInvariantPtr&, const clipper::Params&>(), "invariant"_a,
           "params"_a, py::keep_alive<1, 2>())
      // a batch scored by a DeviceInvariant (the constructor takes the built-ins only)
      .def_static("with_device_invariant", &clipper::CLIPPERBatch::withDeviceInvariant, "invariant"_a, "params"_a,
                  py::keep_alive<0, 1>())
      .def("__repr__", [](const clipper::CLIPPERBatch&) { return "<CLIPPERBatch>"; })
      .def("set_device", &clipper::CLIPPERBatch::setDevice, "device"_a)
      .def("set_storage", &clipper::CLIPPERBatch::setStorage, "storage"_a)
      // problems: a list of (D1, D2, A[, u0]) with the dtypes score_pairwise_consistency / solve take (no conversion)
      .def("solve", [](clipper::CLIPPERBatch& b, const py::sequence& problems) {
        std::vector<clipper::BatchProblem> ps(problems.size());
        auto load = [](const py::handle& h, auto& out, size_t i, const char* what) {
          py::detail::make_caster<std::decay_t<decltype(out)>> c;
          if (!c.load(h, false))
            throw py::type_error("problem " + std::to_string(i) + ": " + what + " has the wrong type or dtype");
          out = py::detail::cast_op<std::decay_t<decltype(out)>>(std::move(c));
        };
        for (size_t i = 0; i < ps.size(); ++i) {
          const py::tuple t = problems[i].cast<py::tuple>();
          if (t.size() != 3 && t.size() != 4)
            throw py::value_error("problem " + std::to_string(i) + ": expected (D1, D2, A[, u0])");
          load(t[0], ps[i].D1, i, "D1");
          load(t[1], ps[i].D2, i, "D2");
          load(t[2], ps[i].A, i, "A");
          if (t.size() == 4 && !t[3].is_none()) load(t[3], ps[i].u0, i, "u0");
        }
        return b.solve(ps);
      }, "problems"_a)
      .def("get_selected_associations", &clipper::CLIPPERBatch::getSelectedAssociations, "i"_a)
      .def("solved_batched", &clipper::CLIPPERBatch::solvedBatched, "i"_a)
      // the semidefinite relaxation of every problem of the last solve, in one batched call
      .def("solve_as_msrc_sdr", &clipper::CLIPPERBatch::solveAsMSRCSDR, "params"_a = clipper::sdp::Params{})
      .def("sdp_solutions", &clipper::CLIPPERBatch::sdpSolutions)
      // the maximum clique of every problem of the last solve, in one batched call
      .def("solve_as_maximum_clique", &clipper::CLIPPERBatch::solveAsMaximumClique,
           "params"_a = clipper::maxclique::Params{});
}
