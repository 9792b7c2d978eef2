// Detect's eval decode (models/model.py:59-66) of one raw value: the arithmetic sodt_detect_decode (head.hip) and
// sodt_detect_decode_tta (tta.hip) share, so that the two cannot drift.
#pragma once
#include "common.h"

// raw value of output column o at grid cell (y, x) of anchor a; anchor_grid is (na, 2) in pixels
__device__ __forceinline__ float detect_decode_value(float rawv, int o, int x, int y, int a, const float* __restrict__ anchor_grid,
                                                     float stride) {
  const float s = sigmoid_f(rawv);
  float v = s;
  if (o == 0) v = (s * 2.f - 0.5f + (float)x) * stride;
  else if (o == 1) v = (s * 2.f - 0.5f + (float)y) * stride;
  else if (o == 2) v = (s * 2.f) * (s * 2.f) * anchor_grid[a * 2];
  else if (o == 3) v = (s * 2.f) * (s * 2.f) * anchor_grid[a * 2 + 1];
  return v;
}
