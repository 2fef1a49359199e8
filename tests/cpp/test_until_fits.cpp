// The build-until-it-fits driver (clipper_amd/csrc/host_fits.hpp) on scripted items: every callback call is logged and
// the whole log compared with the expected sequence. Built with plain g++ (tests/test_batch_cpu.py).
#include "host_fits.hpp"

#include <cstdio>
#include <cstdlib>
#include <new>
#include <string>
#include <utility>
#include <vector>

namespace {

int g_failures = 0;
long g_allocs = 0;  // calls of operator new, counted while the n = 1 cases run

void check(bool ok, const char* what, const std::string& got = "") {
  if (ok) return;
  ++g_failures;
  std::fprintf(stderr, "FAILED: %s%s%s\n", what, got.empty() ? "" : ": got ", got.c_str());
}

// A scripted run. again[i] = how many times item i says "again" (-1: always). fail_kind, fail_nth: the call (e / w / c) and its
// occurrence (0-based, counted over the whole run) that returns `code`. Log: "e<i>" "w" "c<i>", "|" between rounds,
// "X" for the exhaustion callable.
struct Run {
  std::vector<int> again;
  char fail_kind = 0;
  int fail_nth = 0, code = 0;
  std::string log;
  int waits = 0, exhausted = 0, seen_e = 0, seen_w = 0, seen_c = 0;
  std::vector<int> builds;

  int hit(char kind, int& seen) { return (kind == fail_kind && seen++ == fail_nth) ? code : 0; }
  char last = 0;  // the kind of the last call logged
  void add(const std::string& t) {
    if (!log.empty()) log += ' ';
    log += t;
    last = t[0];
  }
  int go(int max_builds) {
    builds.assign(again.size(), 0);
    return clipper_fits::until_fits(
        again.size(), max_builds,
        [&](size_t i) {
          if (last == 'c') add("|");  // (a new round)
          add("e" + std::to_string(i));
          ++builds[i];
          return hit('e', seen_e);
        },
        [&] {
          add("w");
          ++waits;
          return hit('w', seen_w);
        },
        [&](size_t i, bool& ag) {
          add("c" + std::to_string(i));
          ag = again[i] < 0 || builds[i] <= again[i];
          return hit('c', seen_c);
        },
        [&] {
          add("X");
          ++exhausted;
          return 77;
        });
  }
};

Run script(std::vector<int> again) {
  Run r;
  r.again = std::move(again);
  return r;
}

void expect(Run r, int max_builds, int want_rc, const std::string& want_log, const char* what) {
  const int rc = r.go(max_builds);
  check(rc == want_rc, what, "rc " + std::to_string(rc));
  check(r.log == want_log, what, "\"" + r.log + "\"");
}

}  // namespace

void* operator new(std::size_t n) {
  ++g_allocs;
  if (void* p = std::malloc(n ? n : 1)) return p;
  throw std::bad_alloc();
}
void operator delete(void* p) noexcept { std::free(p); }
void operator delete(void* p, std::size_t) noexcept { std::free(p); }

int main() {
  // one item that fits
  expect(script({0}), 3, 0, "e0 w c0", "one item that fits");
  // one item that overflows twice, then fits, under a limit of 3: exactly three builds
  expect(script({2}), 3, 0, "e0 w c0 | e0 w c0 | e0 w c0", "two overflows under a limit of 3");
  // one item that always overflows: the exhaustion callable once, after exactly max_builds builds, no further enqueue
  expect(script({-1}), 3, 77, "e0 w c0 | e0 w c0 | e0 w c0 X", "always overflowing, limit 3");
  expect(script({-1}), 4, 77, "e0 w c0 | e0 w c0 | e0 w c0 | e0 w c0 X", "always overflowing, limit 4");
  {
    Run r = script({-1});
    r.go(3);
    check(r.exhausted == 1 && r.builds[0] == 3 && r.waits == 3, "exhaustion: one call after three builds");
  }
  // five items, 1 and 3 again in round 0, 3 again in round 1: one wait per round
  {
    Run r = script({0, 1, 0, 2, 0});
    const int rc = r.go(3);
    check(rc == 0, "five items", "rc " + std::to_string(rc));
    check(r.log == "e0 e1 e2 e3 e4 w c0 c1 c2 c3 c4 | e1 e3 w c1 c3 | e3 w c3", "five items", "\"" + r.log + "\"");
    check(r.waits == 3 && r.exhausted == 0, "five items: one wait per round");
  }
  // a non-zero code from each callback, at the first and at a later position: returned, and the log ends there
  {
    struct Case { char kind; int nth; const char* log; };
    const Case cases[] = {
        {'e', 0, "e0"},
        {'e', 6, "e0 e1 e2 e3 e4 w c0 c1 c2 c3 c4 | e1 e3"},
        {'w', 0, "e0 e1 e2 e3 e4 w"},
        {'w', 1, "e0 e1 e2 e3 e4 w c0 c1 c2 c3 c4 | e1 e3 w"},
        {'c', 0, "e0 e1 e2 e3 e4 w c0"},
        {'c', 6, "e0 e1 e2 e3 e4 w c0 c1 c2 c3 c4 | e1 e3 w c1 c3"},
    };
    for (const Case& c : cases) {
      Run r = script({0, 1, 0, 2, 0});
      r.fail_kind = c.kind;
      r.fail_nth = c.nth;
      r.code = 40 + c.nth;
      const int rc = r.go(3);
      const std::string what = std::string("a code from ") + c.kind + " #" + std::to_string(c.nth);
      check(rc == 40 + c.nth, what.c_str(), "rc " + std::to_string(rc));
      check(r.log == c.log, what.c_str(), "\"" + r.log + "\"");
      check(r.exhausted == 0, what.c_str());
    }
  }
  // n = 0: nothing is called, wait included
  expect(script({}), 3, 0, "", "n = 0");
  expect(script({}), 0, 0, "", "n = 0 under a limit of 0");
  // n = 1 makes no heap allocation inside the driver
  {
    int builds = 0;
    const long before = g_allocs;
    const int rc = clipper_fits::until_fits(
        1, 3, [&](size_t) { return ++builds, 0; }, [] { return 0; },
        [&](size_t, bool& again) { return again = builds < 2, 0; }, [] { return 77; });
    const long after = g_allocs;
    check(rc == 0 && builds == 2, "n = 1, plain callbacks");
    check(after == before, "n = 1 allocates nothing", std::to_string(after - before) + " allocations");
  }
  if (g_failures) return 1;
  std::printf("until fits ok\n");
  return 0;
}
