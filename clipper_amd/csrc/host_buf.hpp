// host_buf.hpp — the three owners of the host side: DevBuf<T> (device memory), PinnedBuf<T> (pinned host memory, with
// its device alias where it is mapped) and Event. Each is move-only, frees what it holds when it goes, and is the only
// place that calls the runtime's allocation, free and event-creation functions (tests/test_abi_exports.py scans for it).
// Depends on the HIP runtime API alone (tests/cpp/test_host_buf.cpp includes it over counting stubs).
// None of them zeroes or copies: every memset stays with its caller, in stream order.
#pragma once

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <utility>

namespace clipper_hip_buf {

// process-wide counts, moved only by the owners below (clipper_hip_debug_live_resources reads them)
struct LiveCounts {
  std::atomic<int64_t> dev_bufs{0}, dev_bytes{0}, pinned_bufs{0}, events{0}, allocs{0};
};
inline LiveCounts& live() {
  static LiveCounts c;
  return c;
}

template <class T>
struct elem_size { static constexpr size_t value = sizeof(T); };
template <>
struct elem_size<void> { static constexpr size_t value = 1; };  // a buffer of bytes

// makes `device` current for a scope (a free belongs on the device of its allocation); -1: leave it
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int device) {
    if (device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device) (void)hipSetDevice(device);
    else prev = -1;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// ---- device memory: an array of `cap` elements (bytes for T = void) on `device` ------------------------------------
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;     // whole elements
  size_t nbytes = 0;  // as allocated
  int device = -1;    // where it was allocated

  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap), nbytes(o.nbytes), device(o.device) { o.p = nullptr, o.cap = o.nbytes = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, cap = o.cap, nbytes = o.nbytes, device = o.device;
      o.p = nullptr, o.cap = o.nbytes = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  operator T*() const { return p; }
  T* get() const { return p; }
  template <class U>
  U* as() const { return reinterpret_cast<U*>(p); }
  size_t bytes() const { return nbytes; }

  void reset() {
    if (!p) return;
    {
      DeviceScope on(device);
      (void)hipFree(p);
    }
    live().dev_bufs--, live().dev_bytes -= static_cast<int64_t>(nbytes);
    p = nullptr, cap = nbytes = 0;
  }
  // frees what it holds, then allocates exactly n elements on the current device; {null, 0} on failure
  hipError_t alloc(size_t n) { return alloc_bytes(n * elem_size<T>::value); }
  // the same for a size that is no whole number of elements (a directory with a trailer)
  hipError_t alloc_bytes(size_t b) {
    reset();
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, b);
    if (e != hipSuccess) return e;
    p = static_cast<T*>(q), nbytes = b, cap = b / elem_size<T>::value;
    if (hipGetDevice(&device) != hipSuccess) device = -1;
    live().dev_bufs++, live().dev_bytes += static_cast<int64_t>(nbytes), live().allocs++;
    return hipSuccess;
  }
  // an array that only grows: kept while it holds n elements, else replaced (contents lost)
  hipError_t grow(size_t n) { return (p && n <= cap) ? hipSuccess : alloc(n); }
};

// ---- pinned host memory; `dev` is its device address where the flags map it ---------------------------------------
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  T* dev = nullptr;
  size_t cap = 0;  // elements

  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  PinnedBuf(PinnedBuf&& o) noexcept : p(o.p), dev(o.dev), cap(o.cap) { o.p = o.dev = nullptr, o.cap = 0; }
  PinnedBuf& operator=(PinnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = o.p, dev = o.dev, cap = o.cap;
      o.p = o.dev = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~PinnedBuf() { reset(); }

  operator T*() const { return p; }
  T* get() const { return p; }
  T* operator->() const { return p; }

  void reset() {
    if (!p) return;
    (void)hipHostFree(p);
    live().pinned_bufs--;
    p = dev = nullptr, cap = 0;
  }
  hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) { return alloc_bytes(n * elem_size<T>::value, flags); }
  hipError_t alloc_bytes(size_t b, unsigned flags = hipHostMallocDefault) {
    reset();
    void* q = nullptr;
    hipError_t e = hipHostMalloc(&q, b, flags);
    if (e != hipSuccess) return e;
    void* d = nullptr;
    if ((flags & hipHostMallocMapped) && (e = hipHostGetDevicePointer(&d, q, 0)) != hipSuccess) {
      (void)hipHostFree(q);
      return e;
    }
    p = static_cast<T*>(q), dev = static_cast<T*>(d), cap = b / elem_size<T>::value;
    live().pinned_bufs++, live().allocs++;
    return hipSuccess;
  }
  hipError_t grow(size_t n, unsigned flags = hipHostMallocDefault) {
    return (p && n <= cap) ? hipSuccess : alloc(n, flags);
  }
};

// ---- an event -------------------------------------------------------------------------------------------------------
struct Event {
  hipEvent_t e = nullptr;

  Event() = default;
  Event(const Event&) = delete;
  Event& operator=(const Event&) = delete;
  Event(Event&& o) noexcept : e(o.e) { o.e = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) {
      reset();
      e = o.e;
      o.e = nullptr;
    }
    return *this;
  }
  ~Event() { reset(); }

  operator hipEvent_t() const { return e; }

  void reset() {
    if (!e) return;
    (void)hipEventDestroy(e);
    live().events--;
    e = nullptr;
  }
  hipError_t create(unsigned flags = hipEventDefault) {
    reset();
    hipError_t r = flags == hipEventDefault ? hipEventCreate(&e) : hipEventCreateWithFlags(&e, flags);
    if (r != hipSuccess) {
      e = nullptr;
      return r;
    }
    live().events++, live().allocs++;
    return hipSuccess;
  }
};

}  // namespace clipper_hip_buf
