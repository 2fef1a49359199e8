// The plan of a seeded maximum-clique call (host_mcplan.hpp, DESIGN.md 9 "Seeded calls"): where the vertex lists sit,
// that a call without lists keeps the unseeded plan offset for offset, the check of a list and the winner rule.
// Host only: g++ -std=c++17 -I clipper_amd/csrc.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_mcplan.hpp"

namespace plan = clipper_mc_plan;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

int main() {
  const std::vector<int32_t> m = {1, 65, 200, 2048, 129};
  const size_t PB = 144, CB = 64, SB = 120;
  const plan::GraphPlan U = plan::make_graph_plan(m, 2048, PB, CB, SB);
  // no list, and lists that are all empty: the unseeded plan
  for (const std::vector<int32_t>& none : {std::vector<int32_t>{}, std::vector<int32_t>(m.size(), 0)}) {
    const plan::GraphPlan Z = plan::make_graph_plan(m, 2048, PB, CB, SB, none);
    CHECK(Z.bytes == U.bytes && Z.up_end == U.up_end && Z.work == U.work && Z.out_begin == U.out_begin);
    CHECK(Z.given_end == Z.ctl + m.size() * CB && U.given_end == Z.given_end);
    for (size_t i = 0; i < m.size(); ++i) {
      CHECK(Z.at[i].list == U.at[i].list && Z.at[i].pos == U.at[i].pos && Z.at[i].out == U.at[i].out);
      CHECK(Z.at[i].core == U.at[i].core && Z.at[i].deg == U.at[i].deg && Z.at[i].G == U.at[i].G);
    }
  }
  // lists: inside [ctl's end, given_end), 256-byte aligned, disjoint, in the first copy and before every list / pos
  const std::vector<int32_t> n = {1, 0, 200, 37, 0};
  const plan::GraphPlan S = plan::make_graph_plan(m, 2048, PB, CB, SB, n);
  size_t prev_end = S.ctl + m.size() * CB;
  for (size_t i = 0; i < m.size(); ++i) {
    if (n[i] == 0) continue;
    CHECK(S.at[i].given % plan::ARRAY_ALIGN == 0);
    CHECK(S.at[i].given >= prev_end);
    prev_end = S.at[i].given + static_cast<size_t>(n[i]) * 4;
    CHECK(prev_end <= S.given_end);
  }
  CHECK(S.given_end > S.ctl + m.size() * CB && S.given_end <= S.up_end && S.up_begin == U.up_begin);
  for (size_t i = 0; i < m.size(); ++i) {
    CHECK(S.at[i].list >= S.given_end && S.at[i].pos >= S.given_end && S.at[i].list % plan::ARRAY_ALIGN == 0);
    CHECK(S.at[i].G == U.at[i].G && S.at[i].degw == U.at[i].degw);  // (the device-only part does not move)
  }
  CHECK(S.bytes >= U.bytes && S.bytes <= U.bytes + 3 * (plan::ARRAY_ALIGN + 200 * 4));
  CHECK(S.probs == U.probs && S.src == U.src && S.ctl == U.ctl);

  // the check of a list
  const int32_t ok[] = {5, 0, 63, 64, 199};
  CHECK(plan::first_bad_seed(ok, 5, 200) == -1);
  CHECK(plan::first_bad_seed(ok, 0, 200) == -1 && plan::first_bad_seed(nullptr, 0, 0) == -1);
  CHECK(plan::first_bad_seed(ok, 5, 199) == 4);  // index m
  const int32_t neg[] = {3, -1, 4};
  CHECK(plan::first_bad_seed(neg, 3, 10) == 1);
  const int32_t dup[] = {3, 7, 9, 7, 3};
  CHECK(plan::first_bad_seed(dup, 5, 10) == 3);
  const int32_t one[] = {0};
  CHECK(plan::first_bad_seed(one, 1, 1) == -1 && plan::first_bad_seed(one, 1, 0) == 0);

  // the winner: the search above b; else the seed clique when s >= 2 and HEU did not beat it; else HEU's clique
  CHECK(plan::seeded_winner(5, 5, 6) == 0 && plan::seeded_winner(0, 5, 6) == 0 && plan::seeded_winner(3, 5, 6) == 0);
  CHECK(plan::seeded_winner(5, 5, 5) == 2 && plan::seeded_winner(2, 2, 2) == 2);
  CHECK(plan::seeded_winner(3, 5, 5) == 1 && plan::seeded_winner(0, 5, 5) == 1 && plan::seeded_winner(1, 4, 4) == 1);
  std::printf("mc seed plan ok\n");
  return 0;
}
