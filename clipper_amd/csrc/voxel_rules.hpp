// voxel_rules.hpp — the arithmetic of voxel down-sampling ("Voxel down-sampling"), stated once
// for the kernels (k_sort.hip.h, k_voxel.hip.h) and the host: the voxel of a point, the cell number and its limit, the
// digits and the number of passes of the radix sort, the order in which a voxel's members are added, the centroid and
// the normal of a voxel. Plain sequential functions of one point, one key or one list of members: which work item
// holds what belongs to the kernels. Every expression rounds as written (the build runs with -ffp-contract=off). No
// HIP: builds with g++ as well (tests/cpp/test_voxel_rules.cpp). tests/voxel_model.py restates the same contract in numpy.
//
// The grid's origin is the cloud's own minimum corner lo (the exact per-axis minimum), NOT Open3D's
// min - voxel_size / 2: with lo as the origin (x - lo) >= 0 for every point, and the voxel of the minimum is cell 0.
//
// Why the key is monotone: x - lo, the multiplication by inv > 0 and floor are each monotone (non-decreasing) in x,
// roundings included, so v_a(lo) = 0 <= v_a(x) <= v_a(hi) = dim_a - 1 for every point of the cloud; the clamp never
// acts and is there all the same. The key (v_z * dim_y + v_y) * dim_x + v_x is then the position of (z, y, x) in
// lexicographic order, and with every dim_a <= 2^21 it stays below 2^63.
#pragma once

#include <math.h>
#include <stdint.h>

#include "features_rules.hpp"

#define VOXEL_HD FEAT_HD

namespace clipper_hip {

constexpr int VOXEL_CHUNK = 512;                  // members per sequential sum (a rule of the contract, not a tuned value)
constexpr int32_t VOXEL_MAX_DIM = 1 << 21;        // voxels along one axis: three of them keep the key below 2^63
constexpr int SORT_DIGIT_BITS = 8;                // of the LSD radix sort
constexpr int SORT_RADIX = 1 << SORT_DIGIT_BITS;  // 256

// ---- the grid -------------------------------------------------------------------------------------------------------
struct VoxelGrid {
  double lo[3];    // the exact per-axis minimum of the cloud
  double inv;      // 1.0 / voxel_size, evaluated once
  int32_t dim[3];  // voxels along x, y, z: v_a(hi) + 1
};

// where a coordinate falls on its axis, before the clamp: floor((x - lo) * inv), as a double (it may be huge)
VOXEL_HD double voxel_coord(double x, double lo, double inv) { return floor((x - lo) * inv); }

// the voxel of a coordinate on an axis of dim cells
VOXEL_HD int32_t voxel_cell(double x, double lo, double inv, int32_t dim) {
  double v = voxel_coord(x, lo, inv);
  if (!(v >= 0.0)) v = 0.0;
  if (v > static_cast<double>(dim - 1)) v = static_cast<double>(dim - 1);
  return static_cast<int32_t>(v);
}

// The grid of a cloud with the corners lo, hi: false when an axis would hold more than VOXEL_MAX_DIM voxels (`axis`
// says which; also when the product is no number, e.g. an extent of 0 times an infinite inv).
VOXEL_HD bool voxel_plan(const double (&lo)[3], const double (&hi)[3], double voxel_size, VoxelGrid& g, int& axis) {
  g.inv = 1.0 / voxel_size;
  for (int a = 0; a < 3; ++a) {
    g.lo[a] = lo[a];
    const double d = voxel_coord(hi[a], lo[a], g.inv) + 1.0;
    if (!(d >= 1.0 && d <= static_cast<double>(VOXEL_MAX_DIM))) {
      axis = a;
      return false;
    }
    g.dim[a] = static_cast<int32_t>(d);
  }
  return true;
}

// the cell number: lexicographic in (z, y, x)
VOXEL_HD uint64_t voxel_key(const VoxelGrid& g, const double (&p)[3]) {
  const uint64_t vx = static_cast<uint64_t>(voxel_cell(p[0], g.lo[0], g.inv, g.dim[0]));
  const uint64_t vy = static_cast<uint64_t>(voxel_cell(p[1], g.lo[1], g.inv, g.dim[1]));
  const uint64_t vz = static_cast<uint64_t>(voxel_cell(p[2], g.lo[2], g.inv, g.dim[2]));
  return (vz * static_cast<uint64_t>(g.dim[1]) + vy) * static_cast<uint64_t>(g.dim[0]) + vx;
}

VOXEL_HD uint64_t voxel_cells(const VoxelGrid& g) {
  return static_cast<uint64_t>(g.dim[0]) * static_cast<uint64_t>(g.dim[1]) * static_cast<uint64_t>(g.dim[2]);
}

// ---- the sort -------------------------------------------------------------------------------------------------------
// passes over 8-bit digits that order every key below `cells`: ceil(bitlength(cells - 1) / 8); 0 for one cell, <= 8
VOXEL_HD int sort_passes(uint64_t cells) {
  uint64_t top = cells > 0 ? cells - 1 : 0;
  int bits = 0;
  while (top) {
    ++bits;
    top >>= 1;
  }
  return (bits + SORT_DIGIT_BITS - 1) / SORT_DIGIT_BITS;
}

VOXEL_HD uint32_t sort_digit(uint64_t key, int pass) {
  return static_cast<uint32_t>(key >> (SORT_DIGIT_BITS * pass)) & static_cast<uint32_t>(SORT_RADIX - 1);
}

// ---- the sums -------------------------------------------------------------------------------------------------------
// A voxel's members are taken in ascending original index and cut into chunks of VOXEL_CHUNK. One chunk: members
// [b, e) added one after the other from +0.0; get(k, v) fetches member k's three numbers (x - lo for the centroid, the
// normal for the normals).
template <class Get>
VOXEL_HD void voxel_chunk_sum(int64_t b, int64_t e, Get get, double (&s)[3]) {
  s[0] = 0.0;
  s[1] = 0.0;
  s[2] = 0.0;
  for (int64_t k = b; k < e; ++k) {
    double v[3];
    get(k, v);
    s[0] = s[0] + v[0];
    s[1] = s[1] + v[1];
    s[2] = s[2] + v[2];
  }
}

// the chunk sums of a voxel are added in chunk order from +0.0: tot = ((0 + s_0) + s_1) + ...
VOXEL_HD void voxel_add_chunk(double (&tot)[3], const double (&s)[3]) {
  tot[0] = tot[0] + s[0];
  tot[1] = tot[1] + s[1];
  tot[2] = tot[2] + s[2];
}

VOXEL_HD int64_t voxel_chunks(int64_t count) { return (count + VOXEL_CHUNK - 1) / VOXEL_CHUNK; }

// the whole sum of the members [0, count) by the two rules above (a sequential restatement: the host's, the tests')
template <class Get>
VOXEL_HD void voxel_sum(int64_t count, Get get, double (&tot)[3]) {
  tot[0] = 0.0;
  tot[1] = 0.0;
  tot[2] = 0.0;
  for (int64_t b = 0; b < count; b += VOXEL_CHUNK) {
    double s[3];
    voxel_chunk_sum(b, b + VOXEL_CHUNK < count ? b + VOXEL_CHUNK : count, get, s);
    voxel_add_chunk(tot, s);
  }
}

// the point of a voxel: the centroid of its members, from the sum of (x - lo)
VOXEL_HD void voxel_centroid(const VoxelGrid& g, const double (&tot)[3], int32_t count, double (&c)[3]) {
  const double w = static_cast<double>(count);
  for (int a = 0; a < 3; ++a) c[a] = g.lo[a] + tot[a] / w;
}

// the normal of a voxel: the sum of its members' normals made a unit vector, (0, 0, 1) when they cancel
// (estimate_normals' own fallback: the output stays acceptable to compute_fpfh)
VOXEL_HD void voxel_normal(const double (&s)[3], double (&nv)[3]) {
  const double l2 = feat_dot(s, s);
  if (l2 == 0.0) {
    nv[0] = 0.0;
    nv[1] = 0.0;
    nv[2] = 1.0;
    return;
  }
  const double len = sqrt(l2);
  for (int a = 0; a < 3; ++a) nv[a] = s[a] / len;
}

}  // namespace clipper_hip
