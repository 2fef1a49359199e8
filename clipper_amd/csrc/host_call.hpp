// host_call.hpp — the frame of a stand-alone call (one that takes a device number and host arrays and needs no
// context): the device made current, the device temporaries of the call, the copies up and down. Every entry point
// checks its own arguments first and the device after them. Part of clipper_hip.hip (one translation unit; included
// there after host_state.hpp, whose fail and HIPCHK it reports through).
#pragma once

namespace {

// the number of devices to ndev, or CLIPPER_HIP_E_NODEVICE
int visible_devices(int& ndev) {
  ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(CLIPPER_HIP_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
  return 0;
}

// the device of a call made current: 0, or CLIPPER_HIP_E_NODEVICE / CLIPPER_HIP_E_INVALID
int use_device(int device) {
  int ndev = 0;
  if (int rc = visible_devices(ndev)) return rc;
  if (device < 0 || device >= ndev) return fail(CLIPPER_HIP_E_INVALID, "device %d out of range (%d visible)", device, ndev);
  HIPCHK(hipSetDevice(device));
  return 0;
}

// device temporaries of one call, released when it goes out of scope: on every path (hipFree waits for the device, so
// nothing the call queued is in flight once they are gone: host arrays declared before it outlive every copy)
struct DevTemps {
  std::vector<DevBuf<void>> v;
  // n bytes on device dev (current): 0, or CLIPPER_HIP_E_NOMEM with the report made
  template <typename T>
  int alloc(int dev, T*& p, size_t n) {
    DevBuf<void> b;
    HIPCHK(b.alloc(std::max<size_t>(n, 16)));
    b.device = dev;
    p = b.as<T>();
    v.push_back(std::move(b));
    return 0;
  }
  // several at once, as (pointer, bytes) pairs in order: stops at the first that fails
  template <typename T, typename... More>
  int alloc(int dev, T*& p, size_t n, More&&... more) {
    if (int rc = alloc(dev, p, n)) return rc;
    return alloc(dev, std::forward<More>(more)...);
  }
};

// `count` elements up, queued on st
template <typename T>
int copy_up(T* dst, const T* src, size_t count, hipStream_t st) {
  HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, st));
  return 0;
}

// `count` elements down, queued on st, unless the caller left the destination out
template <typename T>
int copy_down(T* dst, const T* src, size_t count, hipStream_t st) {
  if (dst) HIPCHK(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyDeviceToHost, st));
  return 0;
}

}  // namespace
