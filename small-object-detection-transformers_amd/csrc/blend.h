// The bilinear blend of the pre-processing kernels (preprocess.hip, quad.hip),
//     (1 - ly) ((1 - lx) p00 + lx p01) + ly ((1 - lx) p10 + lx p11),
// with its roundings spelled out: three products are rounded, three multiply-adds are fused.  Under -ffp-contract=fast the
// compiler picks which products of such an expression it fuses per kernel; two kernels that must agree bit for bit
// (sodt_preprocess_u8_quad and sodt_preprocess_u8 on the materialised quad batch) share this one form instead.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float sodt_blend4(float ly, float lx, float p00, float p01, float p10, float p11) {
  const float top = fmaf(lx, p01, (1.f - lx) * p00);
  const float bot = fmaf(1.f - lx, p10, lx * p11);
  return fmaf(1.f - ly, top, ly * bot);
}
