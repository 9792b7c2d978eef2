// Coordinate arithmetic shared by the bilinear resize kernels (multiscale.hip, tta.hip).
#pragma once
#include <hip/hip_runtime.h>

// align_corners=False (ATen's area_pixel_compute_source_index): source index and blend weight of output index o when `in`
// pixels become `out`.  src = (o + 0.5) * in / out - 0.5 clamped at 0 is n / d with n = max((2 o + 1) * in - out, 0),
// d = 2 * out: the index is the exact integer quotient, the weight the exact remainder over d (one rounding).
__device__ __forceinline__ void ms_coord2(int o, int in, int out, int& i0, float& l) {
  const int d = 2 * out;
  int n = (2 * o + 1) * in - out;
  n = n > 0 ? n : 0;
  i0 = n / d;
  l = (float)(n - i0 * d) / (float)d;
}

// i = q * d + r with 0 <= r < d, for 0 <= i < 2^20 and 1 <= d <= 2^10, rcp = 1.0f / d: the estimate is off by at most one
__device__ __forceinline__ void ms_divmod(int i, int d, float rcp, int& q, int& r) {
  q = (int)((float)i * rcp);
  r = i - q * d;
  if (r < 0) { q -= 1; r += d; }
  if (r >= d) { q += 1; r -= d; }
}
