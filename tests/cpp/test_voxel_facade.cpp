// test_voxel_facade.cpp — clipper::registration::voxel_down_sample through the clipper:: facade: the cloud and its
// normals come from files (column-major 3 x n doubles), the points and normals (3 x n_out), the counts (n_out int32)
// and the trace (n int32) go to files for tests/test_gpu_voxel.py to compare with the C ABI's bits; a refusal arrives as
// std::invalid_argument with the library's message. Plain asserts (no gtest in the image). Built and run by
// tests/test_gpu_voxel.py.
//   test_voxel_facade n voxel_size P.f64 N.f64 P_out.f64 N_out.f64 counts.i32 trace.i32
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>

#include <clipper/registration.h>

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      std::exit(1);                                                         \
    }                                                                       \
  } while (0)

static clipper::invariants::Data read(const char* path, long n) {
  clipper::invariants::Data M(3, n);
  FILE* f = std::fopen(path, "rb");
  EXPECT(f != nullptr);
  EXPECT(std::fread(M.data(), sizeof(double), static_cast<size_t>(3 * n), f) == static_cast<size_t>(3 * n));
  std::fclose(f);
  return M;
}

template <class T>
static void write(const char* path, const T* p, size_t count) {
  FILE* f = std::fopen(path, "wb");
  EXPECT(f != nullptr);
  EXPECT(std::fwrite(p, sizeof(T), count, f) == count);
  std::fclose(f);
}

int main(int argc, char** argv) {
  EXPECT(argc == 9);
  const long n = std::atol(argv[1]);
  const double voxel_size = std::atof(argv[2]);
  const clipper::invariants::Data P = read(argv[3], n), N = read(argv[4], n);
  namespace reg = clipper::registration;

  const reg::VoxelDownSampled r = reg::voxel_down_sample(P, voxel_size, N, true);
  const long m = static_cast<long>(r.points.cols());
  EXPECT(r.points.rows() == 3 && m >= 1 && m <= n);
  EXPECT(r.normals.rows() == 3 && r.normals.cols() == m);
  EXPECT(static_cast<long>(r.counts.size()) == m && static_cast<long>(r.trace.size()) == n);
  EXPECT(r.dim[0] >= 1 && r.dim[1] >= 1 && r.dim[2] >= 1 && r.passes >= 0 && r.passes <= 8 && r.max_count >= 1);
  write(argv[5], r.points.data(), static_cast<size_t>(3 * m));
  write(argv[6], r.normals.data(), static_cast<size_t>(3 * m));
  write(argv[7], r.counts.data(), r.counts.size());
  write(argv[8], r.trace.data(), r.trace.size());

  // without normals and without the trace: the same points, nothing else
  const reg::VoxelDownSampled plain = reg::voxel_down_sample(P, voxel_size);
  EXPECT(plain.points.cols() == m && plain.normals.cols() == 0 && plain.trace.empty());
  for (long k = 0; k < 3 * m; ++k) EXPECT(plain.points.data()[k] == r.points.data()[k]);

  bool thrown = false;
  try {
    reg::voxel_down_sample(P, 0.0);
  } catch (const std::invalid_argument& e) {
    thrown = std::string(e.what()) == "voxel_size must be finite and greater than 0 (voxel_size = 0)";
  }
  EXPECT(thrown);
  std::printf("ALL VOXEL FACADE TESTS PASSED\n");
  return 0;
}
