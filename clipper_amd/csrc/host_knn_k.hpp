// host_knn_k.hpp — the list length of a nearest-neighbour search as a template argument: which instantiated K serves a
// list of `len` entries (knn_list_k), and the step from a run-time K to the instantiation (dispatch_k, in the idiom of
// dispatch_vt). Every search kernel (k_knn_*, k_match_partial, k_knn_grid, k_feat_spfh) exists for powers of two only;
// each launch site names the set it instantiates, and a K outside it runs nothing. Pure host code: no HIP, builds with
// g++ (tests/cpp/test_knn_k.cpp).
#pragma once

#include <type_traits>

namespace clipper_hip {

// the smallest power-of-two multiple of kmin that holds len entries, kmax at the most (nearest-K lists are nested: a
// longer list holds the shorter one as its prefix). kmin and kmax are powers of two.
inline int knn_list_k(int len, int kmin, int kmax) {
  int k = kmin;
  while (k < len && k < kmax) k *= 2;
  return k;
}

// calls f(std::integral_constant<int, K>{}) if K is one of Ks; false, with nothing called, if it is not
template <int... Ks, typename F>
bool dispatch_k(int K, F&& f) {
  return ((K == Ks && (f(std::integral_constant<int, Ks>{}), true)) || ...);
}

}  // namespace clipper_hip
