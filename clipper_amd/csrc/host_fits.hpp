// host_fits.hpp — the build-until-it-fits loop of every compressed build, stated once.
// Host-only (no HIP): tests/cpp/test_until_fits.cpp builds it with g++.
//
// A build writes slices into arenas of unknown sufficient size: it is queued, waited for, its counters read; what
// overflowed has its arenas grown and is built again. Over n items (a lone build: n = 1):
//   round r = 0, 1, ...:  enqueue(i)          for every pending i, ascending
//                         wait()              once
//                         complete(i, again)  for every pending i, ascending
//                         pending := the items that said again
// until nothing is pending. A build that would be the (max_builds + 1)-th is not made: exhausted() is returned
// instead. A non-zero return of any callback ends the loop at once with that code.
#pragma once

#include <cstddef>
#include <vector>

namespace clipper_fits {

constexpr int MAX_BUILDS = 3;  // the first build of a size sizes the arenas, the second fits, the third is the margin

// int enqueue(size_t i); int wait(); int complete(size_t i, bool& again); int exhausted()
template <typename Enqueue, typename Wait, typename Complete, typename Exhausted>
int until_fits(size_t n, int max_builds, Enqueue enqueue, Wait wait, Complete complete, Exhausted exhausted) {
  size_t one = 0;
  std::vector<size_t> many;  // (n = 1: no allocation)
  size_t* pending = &one;
  if (n > 1) {
    many.resize(n);
    for (size_t i = 0; i < n; ++i) many[i] = i;
    pending = many.data();
  }
  for (int built = 0; n > 0; ++built) {
    if (built >= max_builds) return exhausted();
    for (size_t k = 0; k < n; ++k)
      if (int rc = enqueue(pending[k])) return rc;
    if (int rc = wait()) return rc;
    size_t kept = 0;
    for (size_t k = 0; k < n; ++k) {
      bool again = false;
      if (int rc = complete(pending[k], again)) return rc;
      if (again) pending[kept++] = pending[k];
    }
    n = kept;
  }
  return 0;
}

}  // namespace clipper_fits
