// The only place that launches a kernel.  Every entry point goes through sodt_launch<kernel>(): opt in to the dynamic LDS
// the launch asks for, launch, poll.  A non-zero status is SODT_ELAUNCH (the runtime refused); an entry point that launches
// several kernels returns at the first one and queues nothing behind it.
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/sodt_hip.h"

// Raise Kern's dynamic-LDS limit to `bytes` if it is not there yet; false, with the HIP error cleared, if the runtime refuses.
// The size reached is remembered per kernel instantiation and per process, not per device (one device per process here).
template <auto Kern>
bool sodt_lds_optin(int bytes) {
  static int have = 0;
  if (bytes <= have) return true;
  if (hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  have = bytes;
  return true;
}

template <auto Kern, class... A>
[[nodiscard]] int sodt_launch(dim3 grid, dim3 block, int dyn_lds, hipStream_t st, const A&... args) {
  if (dyn_lds > 0 && !sodt_lds_optin<Kern>(dyn_lds)) return SODT_ELAUNCH;
  hipLaunchKernelGGL(Kern, grid, block, dyn_lds, st, args...);
  return hipGetLastError() == hipSuccess ? SODT_OK : SODT_ELAUNCH;
}
