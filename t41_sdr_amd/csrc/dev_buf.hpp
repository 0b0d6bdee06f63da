// t41_sdr_amd/csrc/dev_buf.hpp -- what both host sides (rx_ctx.hpp, tx_host.cpp) hold device memory and the current
// device with.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>

namespace t41 {

// device memory a context owns: freed with its holder (t41rx_destroy / t41tx_destroy: under the context's DeviceGuard)
struct HipFree {
  void operator()(void *p) const { (void)hipFree(p); }
};
template <class T>
using DevBuf = std::unique_ptr<T, HipFree>;

// hipMalloc into b; its previous buffer is freed first, and b stays empty when the allocation fails
template <class T>
hipError_t dev_alloc(DevBuf<T> &b, size_t bytes) {
  b.reset();
  void *p = nullptr;
  const hipError_t e = hipMalloc(&p, bytes);
  if (e == hipSuccess) b.reset(static_cast<T *>(p));
  return e;
}

// the context's device for the length of a call; the caller's device comes back behind it
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace t41
