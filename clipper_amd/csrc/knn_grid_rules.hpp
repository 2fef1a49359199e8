// knn_grid_rules.hpp — the rules of the uniform-grid route of the d = 3 nearest-neighbour search (DESIGN.md section 9,
// "The grid route of the search"), stated once for the kernels (k_knn_grid.hip.h) and the host: the cell of a
// coordinate, the order in which a candidate enters a list, the walk over one Chebyshev ring of cells, and when a
// query may stop. The lists the route returns are the brute-force route's (k_knn.hip.h) entry for entry and bit for
// bit: fp64 distances added in coordinate order with nothing fused, ascending by (distance, index), -1 / 1e300 where
// the searched cloud has fewer points. Plain sequential functions of one query; which work item holds what belongs to
// the kernels. Every expression rounds as written (the build runs with -ffp-contract=off). No HIP: builds with g++ as
// well (tests/cpp/test_knn_grid_rules.cpp restates build + query over these functions and compares with brute force).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KNN_GRID_HD __host__ __device__ __forceinline__
#else
#define KNN_GRID_HD inline
#endif

namespace clipper_hip {

constexpr double KNN_GRID_EMPTY = 1.0e300;  // the distance of an empty list entry, on every route

// The grid over the searched cloud: per axis the cloud's minimum, one factor and the number of slabs. The cells are
// numbered (z * dim[1] + y) * dim[0] + x, so that a run of cells along x is a run of cell numbers. The slab tables of
// the three axes stand one behind the other: axis a's entries are [off[a], off[a] + dim[a]).
struct KnnGrid {
  double lo[3];
  double inv[3];   // finite and >= 0 (host_knn_grid_plan.hpp); 0 on an axis with dim == 1
  int32_t dim[3];  // >= 1
  int32_t off[3];
};

// ---- the cell of a coordinate ---------------------------------------------------------------------------------------
// clamp(floor((x - lo) * inv), 0, dim - 1). Monotone non-decreasing in x, clamping included: the rounded subtraction,
// the rounded multiplication by inv >= 0 and floor are monotone, and so is the clamp. A coordinate below lo, one beyond
// the last slab and a product that is not a number all land in a border slab; nothing is out of range for any x.
KNN_GRID_HD int32_t knn_grid_cell(double x, double lo, double inv, int32_t dim) {
  const double c = floor((x - lo) * inv);
  if (!(c > 0.0)) return 0;
  const double last = static_cast<double>(dim - 1);
  return c > last ? dim - 1 : static_cast<int32_t>(c);
}

KNN_GRID_HD void knn_grid_cell3(const KnnGrid& g, const double (&p)[3], int32_t (&c)[3]) {
  for (int a = 0; a < 3; ++a) c[a] = knn_grid_cell(p[a], g.lo[a], g.inv[a], g.dim[a]);
}

KNN_GRID_HD int32_t knn_grid_cell_number(const KnnGrid& g, const int32_t (&c)[3]) {
  return (c[2] * g.dim[1] + c[1]) * g.dim[0] + c[0];
}

// ---- the distance: the contract's own arithmetic --------------------------------------------------------------------
KNN_GRID_HD double knn_grid_sqdist(const double (&q)[3], const double (&p)[3]) {
  double dist = 0.0;
  for (int k = 0; k < 3; ++k) {
    const double df = q[k] - p[k];
    dist = dist + df * df;
  }
  return dist;
}

// ---- candidate order ------------------------------------------------------------------------------------------------
// Candidates are not met in ascending index order, so (distance, index) is compared lexicographically: the brute-force
// rule ("strict <, the earlier one stays") would keep whichever of two tied points its cell happens to hold first.
// An empty entry is (1e300, -1): nothing at 1e300 or beyond ever enters, as in the brute-force route.
KNN_GRID_HD bool knn_grid_before(double d, int32_t j, double bd, int32_t bj) { return d < bd || (d == bd && j < bj); }

template <int K>
KNN_GRID_HD void knn_grid_clear(double (&bd)[K], int32_t (&bi)[K]) {
  for (int k = 0; k < K; ++k) {
    bd[k] = KNN_GRID_EMPTY;
    bi[k] = -1;
  }
}

// sorted insertion into the K best, every entry addressed by a constant (the kernel holds them in registers). The
// list is sorted, so "before entry k - 1" implies "before entry k": entry k takes the entry in front of it where the
// candidate goes before that one, the candidate where it goes before entry k only, and stays otherwise.
template <int K>
KNN_GRID_HD void knn_grid_insert(double (&bd)[K], int32_t (&bi)[K], double d, int32_t j) {
  bool at = knn_grid_before(d, j, bd[K - 1], bi[K - 1]);
  if (!at) return;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = K - 1; k > 0; --k) {
    const bool up = knn_grid_before(d, j, bd[k - 1], bi[k - 1]);
    bd[k] = up ? bd[k - 1] : (at ? d : bd[k]);
    bi[k] = up ? bi[k - 1] : (at ? j : bi[k]);
    at = up;
  }
  bd[0] = at ? d : bd[0];
  bi[0] = at ? j : bi[0];
}

// The brute-force routes' rule (k_knn.hip.h, k_match.hip.h): their candidates DO arrive in ascending index order, so
// "strict <, the earlier one stays in front" gives the same (distance, index) order for one comparison per entry
// instead of two; tests/cpp/test_knn_grid_rules.cpp holds the two rules against each other on such streams.
template <int K>
KNN_GRID_HD void knn_insert_first(double (&bd)[K], int32_t (&bi)[K], double dist, int32_t j) {
  if (dist < bd[K - 1]) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = K - 1; k >= 0; --k) {
      const bool here = (k == 0) || !(dist < bd[k - 1]);
      if (dist < bd[k]) {
        if (here) {
          bd[k] = dist;
          bi[k] = j;
        } else {
          bd[k] = bd[k - 1];
          bi[k] = bi[k - 1];
        }
      }
    }
  }
}

// ---- the walk over the rings -----------------------------------------------------------------------------------------
// Ring r of a query: the cells at Chebyshev distance exactly r from its cell qc that lie inside the grid, as runs of
// consecutive cell numbers along x. A row (y, z) on a face of the ring's cube holds one run, x0..x1; any other row
// the two cells at x = qc[0] -+ r. The walk is a cursor over (ring, z, y, run of the row), advanced one run at a time,
// so that a query is ONE loop whose step is either a candidate or an advance of the cursor, with one bound on its
// steps. Every coordinate of the cursor moves between integers clipped to the grid's dimensions.
struct KnnGridCursor {
  int32_t r, z, y, s;              // ring, row, run of the row (0 | 1)
  int32_t x0, x1, y0, y1, z0, z1;  // ring r's cube, clipped to the grid
};

KNN_GRID_HD void knn_grid_enter_ring(const KnnGrid& g, const int32_t (&qc)[3], int32_t r, KnnGridCursor& c) {
  c.r = r;
  c.x0 = qc[0] - r > 0 ? qc[0] - r : 0;
  c.x1 = qc[0] + r < g.dim[0] - 1 ? qc[0] + r : g.dim[0] - 1;
  c.y0 = qc[1] - r > 0 ? qc[1] - r : 0;
  c.y1 = qc[1] + r < g.dim[1] - 1 ? qc[1] + r : g.dim[1] - 1;
  c.z0 = qc[2] - r > 0 ? qc[2] - r : 0;
  c.z1 = qc[2] + r < g.dim[2] - 1 ? qc[2] + r : g.dim[2] - 1;
  c.z = c.z0;
  c.y = c.y0;
  c.s = 0;
}

KNN_GRID_HD bool knn_grid_ring_done(const KnnGridCursor& c) { return c.z > c.z1; }

// the run under the cursor, first..last inclusive (false: that run lies outside the grid), and the cursor moved on
KNN_GRID_HD bool knn_grid_next_run(const KnnGrid& g, const int32_t (&qc)[3], KnnGridCursor& c, int32_t& first, int32_t& last) {
  const bool face = c.z == qc[2] - c.r || c.z == qc[2] + c.r || c.y == qc[1] - c.r || c.y == qc[1] + c.r;
  const int32_t row = (c.z * g.dim[1] + c.y) * g.dim[0];
  const int32_t a = face ? c.x0 : (c.s == 0 ? qc[0] - c.r : qc[0] + c.r);
  const int32_t b = face ? c.x1 : a;
  first = row + a;
  last = row + b;
  const bool inside = a >= 0 && b <= g.dim[0] - 1;
  if (face || c.s == 1) {
    c.s = 0;
    if (c.y < c.y1) {
      ++c.y;
    } else {
      c.y = c.y0;
      ++c.z;
    }
  } else {
    c.s = 1;
  }
  return inside;
}

// the first ring whose cube covers the whole grid: the search ends behind it whatever the list holds
KNN_GRID_HD int32_t knn_grid_last_ring(const KnnGrid& g, const int32_t (&qc)[3]) {
  int32_t r = 0;
  for (int a = 0; a < 3; ++a) {
    if (qc[a] > r) r = qc[a];
    if (g.dim[a] - 1 - qc[a] > r) r = g.dim[a] - 1 - qc[a];
  }
  return r;
}

// ---- when a query may stop ------------------------------------------------------------------------------------------
// smin[off[a] + c]: the smallest a-coordinate among the points of slabs >= c; pmax[off[a] + c]: the largest among
// slabs <= c; +inf / -inf where those slabs hold no point. Both come from the data (suffix / prefix reductions).
//
// bound_r, a lower bound on the COMPUTED distance of every point outside the rings 0..r of the query. Such a point lies
// in a slab beyond the ring on some axis a. On the upper side its slab number exceeds cell(q_a), so by the monotony of
// knn_grid_cell x > q_a, and x >= s = smin[a][qc_a + r + 1] > q_a. The rounded subtraction is monotone:
// fl(q_a - x) <= fl(q_a - s) <= 0; so is the rounded square of a non-positive number (decreasing), and the rounded sum
// of non-negative terms is no smaller than any of them. So the point's computed distance is >= fl(fl(q_a - s)^2). The
// lower side mirrors it with pmax. bound_r is the smallest of the six; a face with no slab beyond it gives +inf.
KNN_GRID_HD double knn_grid_face(double q, double s) {
  const double df = q - s;
  return df * df;
}

KNN_GRID_HD double knn_grid_bound(const KnnGrid& g, const double (&q)[3], const int32_t (&qc)[3], int32_t r,
                                  const double* smin, const double* pmax) {
  double bound = INFINITY;
  for (int a = 0; a < 3; ++a) {
    const int32_t up = qc[a] + r + 1, dn = qc[a] - r - 1;
    if (up <= g.dim[a] - 1) {
      const double f = knn_grid_face(q[a], smin[g.off[a] + up]);
      if (f < bound) bound = f;
    }
    if (dn >= 0) {
      const double f = knn_grid_face(q[a], pmax[g.off[a] + dn]);
      if (f < bound) bound = f;
    }
  }
  return bound;
}

// After every cell within ring r has been visited: stop iff the list is full and its last distance is STRICTLY below
// the bound. On equality a point further out may tie with a lower index.
KNN_GRID_HD bool knn_grid_may_stop(int32_t last_index, double last_sqd, double bound) {
  return last_index >= 0 && last_sqd < bound;
}

// ---- one query, start to end ----------------------------------------------------------------------------------------
// range(first, last, t, e): the places t..e-1 of the points of cells first..last in the binned cloud; visit(t): the
// point at place t goes to knn_grid_insert. Returns the number of candidates visited. One loop: its steps are the
// candidates (at most n1: no cell is visited twice), the runs (at most two per row and ring) and the rings; max_steps
// restates that bound as an integer of the grid's dimensions, so that no table content can keep the loop running.
KNN_GRID_HD int64_t knn_grid_max_steps(const KnnGrid& g, int64_t n1) {
  const int64_t rings = (g.dim[0] > g.dim[1] ? (g.dim[0] > g.dim[2] ? g.dim[0] : g.dim[2]) : (g.dim[1] > g.dim[2] ? g.dim[1] : g.dim[2]));
  return n1 + rings * (2 * static_cast<int64_t>(g.dim[1]) * g.dim[2] + 1);
}

template <int K, class Range, class Visit>
KNN_GRID_HD int64_t knn_grid_query(const KnnGrid& g, const double (&q)[3], int64_t n1, const double* smin, const double* pmax,
                                   const double (&bd)[K], const int32_t (&bi)[K], Range range, Visit visit) {
  int32_t qc[3];
  knn_grid_cell3(g, q, qc);
  const int32_t rlast = knn_grid_last_ring(g, qc);
  const int64_t max_steps = knn_grid_max_steps(g, n1);
  KnnGridCursor c;
  knn_grid_enter_ring(g, qc, 0, c);
  int64_t seen = 0;
  int32_t t = 0, e = 0;
  bool done = false;
  for (int64_t step = 0; step < max_steps && !done; ++step) {
    if (t < e) {
      visit(t);
      ++t;
      ++seen;
    } else if (!knn_grid_ring_done(c)) {
      int32_t first, last;
      if (knn_grid_next_run(g, qc, c, first, last)) range(first, last, t, e);
    } else {
      done = c.r >= rlast || knn_grid_may_stop(bi[K - 1], bd[K - 1], knn_grid_bound(g, q, qc, c.r, smin, pmax));
      if (!done) knn_grid_enter_ring(g, qc, c.r + 1, c);
    }
  }
  return seen;
}

}  // namespace clipper_hip
