// Host-only helpers of the fused Dense forwards' launchers (dense_forward.hip, dense_forward_fleet.hip,
// dense_forward_wide.hip): the current device, its CU count, and the dynamic-LDS high-water mark of a
// kernel's instances.  No device code.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>

namespace sml {

constexpr int DFW_MAXDEV = 64;

inline int dense_fwd_cur_device() {
  int dev = 0;
  return hipGetDevice(&dev) == hipSuccess && dev >= 0 && dev < DFW_MAXDEV ? dev : -1;
}

// CUs of the current device, asked once per device
inline int dense_fwd_cu_count() {
  static std::atomic<int> cus[DFW_MAXDEV];
  const int dev = dense_fwd_cur_device();
  int n = dev >= 0 ? cus[dev].load(std::memory_order_relaxed) : 0;
  if (n < 1) {
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev < 0 ? 0 : dev) != hipSuccess || n < 1) n = 256;
    if (dev >= 0) cus[dev].store(n, std::memory_order_relaxed);
  }
  return n;
}

// hipFuncAttributeMaxDynamicSharedMemorySize only grows: set once per device and instance for the
// largest plan seen.  One object per kernel template (N instances), so no two kernels share a mark.
template <int N>
struct DenseFwdLdsMark {
  std::atomic<int> have[DFW_MAXDEV][N];
  hipError_t ensure(const void* fn, int instance, int bytes) {
    const int dev = dense_fwd_cur_device();
    if (dev >= 0 && have[dev][instance].load(std::memory_order_relaxed) >= bytes) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0) have[dev][instance].store(bytes, std::memory_order_relaxed);
    return e;
  }
};

}  // namespace sml
