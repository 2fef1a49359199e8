// CPU test of clipper_amd/csrc/host_buf.hpp (g++ only): the three owners over counting stubs of the runtime calls
// they make. The stubs record every allocation and free with the device that was current, and can make the n-th
// allocation fail. tests/test_host_buf.py builds and runs this, once more under the address and UB sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

// ---- the slice of the runtime API the header uses ---------------------------------------------------------------------
enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2, hipErrorInvalidValue = 1 };
typedef struct StubEvent* hipEvent_t;
constexpr unsigned hipHostMallocDefault = 0, hipHostMallocMapped = 2, hipHostMallocCoherent = 0x40000000;
constexpr unsigned hipEventDefault = 0, hipEventDisableTiming = 2;

namespace stub {
int device = 0;
long mallocs = 0, frees = 0, host_mallocs = 0, host_frees = 0, alias_asks = 0, ev_creates = 0, ev_destroys = 0;
long fail_at = -1;  // the allocation (device or pinned, counted together from 0) that fails
long alloc_no = 0;
size_t last_bytes = 0;
unsigned last_flags = 0;
std::map<void*, std::pair<int, size_t>> dev_live;  // pointer -> (device of allocation, bytes)
std::map<void*, size_t> host_live;
long wrong_device_frees = 0, unknown_frees = 0;
bool next_fails() { return alloc_no++ == fail_at; }
}  // namespace stub

hipError_t hipGetDevice(int* d) {
  *d = stub::device;
  return hipSuccess;
}
hipError_t hipSetDevice(int d) {
  stub::device = d;
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) {
  *p = nullptr;
  if (stub::next_fails()) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  stub::dev_live[*p] = {stub::device, bytes};
  stub::last_bytes = bytes;
  ++stub::mallocs;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  auto it = stub::dev_live.find(p);
  if (it == stub::dev_live.end()) {
    ++stub::unknown_frees;
    return hipErrorInvalidValue;
  }
  if (it->second.first != stub::device) ++stub::wrong_device_frees;
  stub::dev_live.erase(it);
  std::free(p);
  ++stub::frees;
  return hipSuccess;
}
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned flags) {
  *p = nullptr;
  if (stub::next_fails()) return hipErrorOutOfMemory;
  *p = std::malloc(bytes ? bytes : 1);
  stub::host_live[*p] = bytes;
  stub::last_bytes = bytes;
  stub::last_flags = flags;
  ++stub::host_mallocs;
  return hipSuccess;
}
hipError_t hipHostFree(void* p) {
  if (!stub::host_live.erase(p)) {
    ++stub::unknown_frees;
    return hipErrorInvalidValue;
  }
  std::free(p);
  ++stub::host_frees;
  return hipSuccess;
}
hipError_t hipHostGetDevicePointer(void** d, void* h, unsigned) {
  ++stub::alias_asks;
  *d = static_cast<char*>(h) + 1;  // (any address that is not the host's: the test only compares it)
  return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t* e) {
  *e = reinterpret_cast<hipEvent_t>(std::malloc(1));
  ++stub::ev_creates;
  return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
  stub::last_flags = flags;
  return hipEventCreate(e);
}
hipError_t hipEventDestroy(hipEvent_t e) {
  std::free(e);
  ++stub::ev_destroys;
  return hipSuccess;
}

#include "host_buf.hpp"

using clipper_hip_buf::DevBuf;
using clipper_hip_buf::Event;
using clipper_hip_buf::live;
using clipper_hip_buf::PinnedBuf;

static int failures = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++failures;                                                        \
    }                                                                    \
  } while (0)

static bool live_is(int64_t bufs, int64_t bytes, int64_t pinned, int64_t events) {
  return live().dev_bufs == bufs && live().dev_bytes == bytes && live().pinned_bufs == pinned && live().events == events;
}

static void test_grow() {
  DevBuf<double> b;
  CHECK(b.grow(100) == hipSuccess && b.p && b.cap == 100 && stub::last_bytes == 800 && stub::mallocs == 1);
  double* first = b.p;
  CHECK(b.grow(100) == hipSuccess && b.grow(7) == hipSuccess && b.grow(0) == hipSuccess);  // n <= cap: kept
  CHECK(b.p == first && b.cap == 100 && stub::mallocs == 1 && stub::frees == 0);
  CHECK(b.grow(101) == hipSuccess && b.cap == 101 && stub::last_bytes == 808);  // exactly n, no rounding
  CHECK(stub::mallocs == 2 && stub::frees == 1 && live_is(1, 808, 0, 0));
  double* q = b;  // the implicit conversion a launch uses
  CHECK(q == b.p && b + 1 == q + 1);
  DevBuf<void> bytes;
  CHECK(bytes.alloc(33) == hipSuccess && bytes.cap == 33 && stub::last_bytes == 33 && bytes.as<float>() == bytes.p);
  DevBuf<uint32_t> dir;  // a size that is no whole number of elements
  CHECK(dir.alloc_bytes(4 * 32 + 6) == hipSuccess && dir.cap == 33 && dir.bytes() == 134 && stub::last_bytes == 134);
  b.reset();
  CHECK(!b.p && b.cap == 0 && live_is(2, 33 + 134, 0, 0));
}

// the resident solver's exchange buffer at the parent: freed, set to null, the allocation fails, the capacity still
// says the old size, and the next plan of a smaller matrix launches on a null buffer
static void test_failed_growth() {
  DevBuf<unsigned long long> xb;
  CHECK(xb.grow(1000) == hipSuccess);
  stub::fail_at = stub::alloc_no;
  CHECK(xb.grow(2000) == hipErrorOutOfMemory);
  CHECK(xb.p == nullptr && xb.cap == 0 && xb.bytes() == 0 && live_is(0, 0, 0, 0));
  const long before = stub::mallocs;
  CHECK(xb.grow(500) == hipSuccess && xb.p != nullptr && xb.cap == 500 && stub::mallocs == before + 1);  // smaller: allocates
  PinnedBuf<uint8_t> plan;
  CHECK(plan.grow(64) == hipSuccess);
  stub::fail_at = stub::alloc_no;
  CHECK(plan.grow(128) == hipErrorOutOfMemory && !plan.p && !plan.dev && plan.cap == 0);
  CHECK(plan.grow(16) == hipSuccess && plan.p && plan.cap == 16);
  stub::fail_at = -1;
}

static void test_moves() {
  const long f0 = stub::frees;
  {
    DevBuf<int32_t> a;
    CHECK(a.alloc(10) == hipSuccess);
    int32_t* pa = a.p;
    DevBuf<int32_t> b(std::move(a));
    CHECK(!a.p && a.cap == 0 && b.p == pa && b.cap == 10);
    {
      DevBuf<int32_t> gone(std::move(a));  // a moved-from owner, moved again and destroyed: frees nothing
    }
    CHECK(stub::frees == f0);
    DevBuf<int32_t> c;
    CHECK(c.alloc(20) == hipSuccess);
    c = std::move(b);  // the target's old array goes, exactly once
    CHECK(stub::frees == f0 + 1 && c.p == pa && c.cap == 10 && !b.p && live_is(1, 40, 0, 0));
    c = std::move(c);  // (self-assignment keeps it)
    CHECK(c.p == pa && stub::frees == f0 + 1);
  }
  CHECK(stub::frees == f0 + 2 && live_is(0, 0, 0, 0) && stub::unknown_frees == 0);
  {
    Event e, f;
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && stub::last_flags == hipEventDisableTiming && f.create() == hipSuccess);
    const long d0 = stub::ev_destroys;
    Event g(std::move(e));
    CHECK(!e.e && g.e && live_is(0, 0, 0, 2));
    f = std::move(g);
    CHECK(stub::ev_destroys == d0 + 1 && live_is(0, 0, 0, 1));
    hipEvent_t raw = f;
    CHECK(raw == f.e);
  }
  CHECK(live_is(0, 0, 0, 0) && stub::ev_creates == stub::ev_destroys);
}

// bench_matvec at the parent: two events created, then early returns in front of their destruction
static int early_return(bool fail_midway) {
  Event e0, e1;
  if (e0.create() != hipSuccess || e1.create() != hipSuccess) return -1;
  DevBuf<double> tmp;
  if (tmp.alloc(16) != hipSuccess) return -1;
  if (fail_midway) return -2;  // (what HIPCHK does on an error)
  return 0;
}
static void test_early_returns_release() {
  const long c0 = stub::ev_creates, f0 = stub::frees;
  CHECK(early_return(true) == -2 && live_is(0, 0, 0, 0) && stub::ev_destroys == stub::ev_creates && stub::ev_creates == c0 + 2);
  CHECK(early_return(false) == 0 && live_is(0, 0, 0, 0) && stub::frees == f0 + 2);
}

static void test_device_of_free() {
  hipSetDevice(3);
  DevBuf<float> a;
  CHECK(a.alloc(8) == hipSuccess && a.device == 3);
  hipSetDevice(5);
  DevBuf<float> b;
  CHECK(b.alloc(8) == hipSuccess && b.device == 5);
  hipSetDevice(0);
  a.reset();
  CHECK(stub::device == 0);  // made current for the free, then put back
  CHECK(b.grow(9) == hipSuccess && b.device == 0);  // (replaced on the device that is current now)
  hipSetDevice(1);
  {
    DevBuf<float> c(std::move(b));
  }
  CHECK(stub::device == 1 && stub::wrong_device_frees == 0);
  hipSetDevice(0);
}

// P1 / P2 (and P1f / P2f) shared one capacity field at the parent: each buffer now answers for itself
static void test_independent_capacities() {
  DevBuf<double> P1, P2;
  CHECK(P1.grow(64) == hipSuccess);
  const long m0 = stub::mallocs;
  CHECK(P2.grow(64) == hipSuccess && stub::mallocs == m0 + 1 && P2.p && P2.p != P1.p);  // P1's capacity says nothing about P2
  CHECK(P1.grow(32) == hipSuccess && P2.grow(64) == hipSuccess && stub::mallocs == m0 + 1);
  CHECK(P2.grow(65) == hipSuccess && P1.cap == 64 && P2.cap == 65);
}

static void test_pinned() {
  const long asks = stub::alias_asks;
  PinnedBuf<int32_t> plain;
  CHECK(plain.alloc(4) == hipSuccess && plain.p && !plain.dev && stub::alias_asks == asks && stub::last_flags == hipHostMallocDefault);
  PinnedBuf<int32_t> mapped;
  CHECK(mapped.alloc(16, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess);
  CHECK(stub::last_flags == (hipHostMallocMapped | hipHostMallocCoherent) && stub::last_bytes == 64);
  CHECK(mapped.dev && mapped.dev != mapped.p && stub::alias_asks == asks + 1);
  int32_t* d = mapped.dev;
  CHECK(mapped.grow(16, hipHostMallocMapped) == hipSuccess && mapped.dev == d && stub::alias_asks == asks + 1);  // kept: not asked again
  CHECK(mapped.grow(17, hipHostMallocMapped) == hipSuccess && stub::alias_asks == asks + 2 && mapped.cap == 17);
  *mapped = 7;
  CHECK(mapped[0] == 7 && live_is(0, 0, 2, 0));
  PinnedBuf<int32_t> taken(std::move(mapped));
  CHECK(!mapped.p && !mapped.dev && taken.dev && live_is(0, 0, 2, 0));
  struct Rec { int32_t a, b; };
  PinnedBuf<Rec> rec;
  CHECK(rec.alloc_bytes(64, hipHostMallocMapped) == hipSuccess && stub::last_bytes == 64 && rec.cap == 8);
  rec->b = 5;
  CHECK(rec.p[0].b == 5);
}

int main() {
  test_grow();
  CHECK(live_is(0, 0, 0, 0));
  test_failed_growth();
  test_moves();
  test_early_returns_release();
  test_device_of_free();
  test_independent_capacities();
  test_pinned();
  CHECK(live_is(0, 0, 0, 0));
  CHECK(stub::dev_live.empty() && stub::host_live.empty() && stub::unknown_frees == 0 && stub::wrong_device_frees == 0);
  CHECK(stub::mallocs == stub::frees && stub::host_mallocs == stub::host_frees && stub::ev_creates == stub::ev_destroys);
  // "allocations so far": every success, and no failure
  CHECK(live().allocs == stub::mallocs + stub::host_mallocs + stub::ev_creates);
  if (failures) return 1;
  std::printf("host buf ok: %ld device, %ld pinned allocations, %ld events\n", stub::mallocs, stub::host_mallocs, stub::ev_creates);
  return 0;
}
