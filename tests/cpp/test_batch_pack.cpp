// CPU test of the launch packer of batched solves (clipper_amd/csrc/host_batchpack.hpp): random problem lists —
// every packable problem in exactly one launch, never split, at most `cap` workgroups per launch, one instantiation
// per launch, groups in key order and problems in batch order inside a group, the same launches on a second call;
// problems with more units than a launch holds are handed back.
//   g++ -std=c++17 -O1 -I clipper_amd/csrc tests/cpp/test_batch_pack.cpp -o /tmp/t && /tmp/t
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "host_batchpack.hpp"

#define EXPECT(cond)                                                \
  do {                                                              \
    if (!(cond)) {                                                  \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

int main() {
  std::mt19937 g(7);
  const int keys[] = {11, 12, 14, 111, 112, 114};
  for (int trial = 0; trial < 2000; ++trial) {
    const int cap = 1 + static_cast<int>(g() % 300);
    const int n = static_cast<int>(g() % 400);
    std::vector<clipper_batch::PackItem> items(static_cast<size_t>(n));
    for (auto& it : items) {
      it.key = keys[g() % (trial % 3 == 0 ? 1 : 6)];
      it.units = 1 + static_cast<int>(g() % (g() % 4 == 0 ? 80 : 8));
    }
    std::vector<int> rejected;
    const auto L = clipper_batch::pack_launches(items, cap, &rejected);
    std::vector<int> seen(static_cast<size_t>(n), 0);
    for (int r : rejected) {
      EXPECT(items[static_cast<size_t>(r)].units > cap);
      ++seen[static_cast<size_t>(r)];
    }
    int prev_key = -1;
    for (const auto& l : L) {
      EXPECT(!l.items.empty());
      EXPECT(l.workgroups <= cap);
      EXPECT(l.key >= prev_key);
      prev_key = l.key;
      int wg = 0, prev = -1;
      for (int k : l.items) {
        EXPECT(items[static_cast<size_t>(k)].key == l.key);
        EXPECT(k > prev);  // batch order inside a launch
        prev = k;
        wg += items[static_cast<size_t>(k)].units;
        ++seen[static_cast<size_t>(k)];
      }
      EXPECT(wg == l.workgroups);
    }
    for (int s : seen) EXPECT(s == 1);  // every problem once: in one launch, or handed back
    const auto L2 = clipper_batch::pack_launches(items, cap);
    EXPECT(L2.size() == L.size());
    for (size_t j = 0; j < L.size(); ++j) EXPECT(L2[j].items == L[j].items && L2[j].key == L[j].key);
  }
  // 300 one-unit problems with 248 workgroups per launch: two launches, 248 + 52
  std::vector<clipper_batch::PackItem> ones(300, clipper_batch::PackItem{11, 1});
  const auto L = clipper_batch::pack_launches(ones, 248);
  EXPECT(L.size() == 2 && L[0].workgroups == 248 && L[1].workgroups == 52);
  EXPECT(clipper_batch::pack_launches({}, 248).empty());
  std::printf("batch pack ok\n");
  return 0;
}
