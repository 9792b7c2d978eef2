// The super-resolution term of the training loss (Train.py:420-427, --super) straight from the uint8 batch:
//
//     'IR'      sr_loss = 0.5 * L1Loss()(output_sr, ir_image)
//     'RGB'     sr_loss = 0.5 * L1Loss()(output_sr, image)
//     'RGB+IR'  sr_loss = 0.1 * (L1Loss()(output_sr[:, 0:3], image) + L1Loss()(output_sr[:, 3:], ir_image[:, 0:1]))
//
// with image = imgs.float() / 255.0 (Train.py:364-365).  The torch spelling slices, subtracts, takes abs and mean twice and
// lets autograd run two sign * scale passes and a concatenation over a tensor that is 1 GiB at B = 4 @ 2048^2, against f32
// copies of the targets that nothing else needs at full resolution.  Here the forward is ONE pass over output_sr and the
// uint8 planes and the backward ONE pass that writes the gradient of output_sr; nothing of tensor size lives in between.
//
// Per element both form t = float(u8) / 255.0f and o - t in f32 exactly as torch does (unit_of: the correctly rounded
// quotient from two FMAs, equal to the IEEE division for all 256 inputs).  A block works inside one (image, channel) plane
// (blockIdx.y), so the target plane, the group (planes 0:3 or plane 3) and the alignment are block-uniform.  16-byte loads
// of output_sr against 4-byte loads of the uint8 target (16-byte ones of an f32 target), four of each in flight per
// thread; a plane whose size is not a multiple of four, or whose base is not aligned, takes the element-wise form of the
// same kernel (no second launch).
//
// Forward: |o - t| accumulates in f64 per thread, is reduced over the block in a fixed order and stored as the block's
// partial.  The block that draws the last ticket sums the partials of each group in block order, forms
// w * (s0 / n0 + s1 / n1) in f64 and writes one f32: no floating-point atomic anywhere, so equal inputs give equal bits.
// Backward: dsr = (float)(upstream * w / n_group) * sign(o - t), sign(0) = 0, upstream read from device memory (it carries
// the GradScaler scale, the world size and the --quad factor of Train.py:439-445).
// HBM-bound: 4 B + 1 B read per element forward, 4 B + 1 B read and 4 B written backward.
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

struct SrL1Args {
  const float* sr;
  const void* tgt[2];          // rgb, ir
  int C;                       // channels of output_sr
  int n_rgb;                   // its leading channels that are compared with rgb; the others with plane 0 of ir
  int c_tgt[2];                // channels of rgb / ir
  int P;                       // elements of one plane
  long units;                  // per plane: P / 4 chunks (VEC) or P elements
};

// float(k) / 255.0f, correctly rounded, for k = 0 .. 255: q = k * r with r = RN(1 / 255), one Newton correction with the exact
// remainder.  (Identical to the IEEE quotient for each of the 256 inputs; the division's expansion costs four times as much.)
__device__ __forceinline__ float unit_of(unsigned k) {
  const float kf = (float)k, r = 0x1.010102p-8f;
  const float q = kf * r;
  return fmaf(fmaf(-q, 255.0f, kf), r, q);
}

template <typename TT> struct Tgt;
template <> struct Tgt<unsigned char> {
  typedef uint32_t raw4;
  static __device__ __forceinline__ raw4 zero4() { return 0u; }
  static __device__ __forceinline__ raw4 load4(const unsigned char* p, long u) { return ((const uint32_t*)p)[u]; }
  static __device__ __forceinline__ void unpack4(raw4 v, float* t) {
    t[0] = unit_of(v & 255u); t[1] = unit_of((v >> 8) & 255u); t[2] = unit_of((v >> 16) & 255u); t[3] = unit_of(v >> 24);
  }
  static __device__ __forceinline__ float load1(const unsigned char* p, long i) { return unit_of(p[i]); }
};
template <> struct Tgt<float> {
  typedef float4 raw4;
  static __device__ __forceinline__ raw4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  static __device__ __forceinline__ raw4 load4(const float* p, long u) { return ((const float4*)p)[u]; }
  static __device__ __forceinline__ void unpack4(raw4 v, float* t) { t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w; }
  static __device__ __forceinline__ float load1(const float* p, long i) { return p[i]; }
};

// what a block needs to know about its plane
template <typename TT> struct Plane { const float* o; const TT* t; int group; };
template <typename TT> __device__ __forceinline__ Plane<TT> plane_of(const SrL1Args& a, int pl) {
  const int b = pl / a.C, ch = pl - b * a.C;
  const int from_ir = ch >= a.n_rgb;
  const long tplane = (long)b * a.c_tgt[from_ir] + (from_ir ? 0 : ch);
  Plane<TT> p;
  p.o = a.sr + (long)pl * a.P;
  p.t = (const TT*)a.tgt[from_ir] + tplane * a.P;
  p.group = (from_ir && a.n_rgb > 0) ? 1 : 0;
  return p;
}

__device__ __forceinline__ double block_sum(double v, double* s_w) {       // fixed order; the result is valid in thread 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();                                                         // (s_w may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
}

template <typename TT, bool VEC>
__global__ __launch_bounds__(256) void sr_l1_fwd_kernel(const SrL1Args a, const double w, const double n0, const double n1,
                                                       unsigned* __restrict__ ticket, double* __restrict__ part,
                                                       float* __restrict__ loss) {
  const Plane<TT> p = plane_of<TT>(a, blockIdx.y);
  const long stride = (long)gridDim.x * 256;
  double s = 0.0;
  for (long u0 = (long)blockIdx.x * 256 + threadIdx.x; u0 < a.units; u0 += 4 * stride) {
    if constexpr (VEC) {
      float4 ov[4];
      typename Tgt<TT>::raw4 tv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {                 // all eight loads before the first use; past the plane: 0 against 0
        const long u = u0 + k * stride;
        const bool in = u < a.units;
        ov[k] = in ? ((const float4*)p.o)[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        tv[k] = in ? Tgt<TT>::load4(p.t, u) : Tgt<TT>::zero4();
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float t[4];
        Tgt<TT>::unpack4(tv[k], t);
        s += ((double)fabsf(ov[k].x - t[0]) + (double)fabsf(ov[k].y - t[1])) +
             ((double)fabsf(ov[k].z - t[2]) + (double)fabsf(ov[k].w - t[3]));
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long i = u0 + k * stride;
        if (i < a.units) s += (double)fabsf(p.o[i] - Tgt<TT>::load1(p.t, i));
      }
    }
  }
  __shared__ double s_w[4];
  __shared__ int s_last;
  const double tot = block_sum(s, s_w);
  const unsigned nblk = gridDim.x * gridDim.y;
  if (threadIdx.x == 0) {
    // the partial is published before the ticket is drawn (release), and the block that draws the last one sees all of them
    // (acquire); partials are only ever touched by device-scope atomics
    __hip_atomic_store(&part[blockIdx.y * gridDim.x + blockIdx.x], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == nblk - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double g0 = 0.0, g1 = 0.0;
  for (unsigned i = threadIdx.x; i < nblk; i += 256) {             // block order: thread t takes t, t + 256, ...
    const double v = __hip_atomic_load(&part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int ch = (int)(i / gridDim.x) % a.C;
    if (a.n_rgb > 0 && ch >= a.n_rgb) g1 += v; else g0 += v;
  }
  g0 = block_sum(g0, s_w);
  g1 = block_sum(g1, s_w);
  if (threadIdx.x == 0) *loss = (float)(w * (g0 / n0 + (n1 > 0.0 ? g1 / n1 : 0.0)));
}

__device__ __forceinline__ float signed_coef(float d, float c) {       // c * sgn(d); sgn(0) = 0, a NaN stays one
  return d > 0.f ? c : d < 0.f ? -c : d == 0.f ? 0.f : d;
}

template <typename TT, bool VEC>
__global__ __launch_bounds__(256) void sr_l1_bwd_kernel(const SrL1Args a, const float* __restrict__ upstream, const double wn0,
                                                       const double wn1, float* __restrict__ dsr) {
  const Plane<TT> p = plane_of<TT>(a, blockIdx.y);
  float* __restrict__ d = dsr + (long)blockIdx.y * a.P;
  const float c = (float)((double)*upstream * (p.group ? wn1 : wn0));       // upstream * w / n_group, one rounding
  const long stride = (long)gridDim.x * 256;
  for (long u0 = (long)blockIdx.x * 256 + threadIdx.x; u0 < a.units; u0 += 4 * stride) {
    if constexpr (VEC) {
      float4 ov[4];
      typename Tgt<TT>::raw4 tv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long u = u0 + k * stride;
        const bool in = u < a.units;
        ov[k] = in ? ((const float4*)p.o)[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        tv[k] = in ? Tgt<TT>::load4(p.t, u) : Tgt<TT>::zero4();
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long u = u0 + k * stride;
        if (u >= a.units) break;
        float t[4];
        Tgt<TT>::unpack4(tv[k], t);
        ((float4*)d)[u] = make_float4(signed_coef(ov[k].x - t[0], c), signed_coef(ov[k].y - t[1], c),
                                      signed_coef(ov[k].z - t[2], c), signed_coef(ov[k].w - t[3], c));
      }
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const long i = u0 + k * stride;
        if (i < a.units) d[i] = signed_coef(p.o[i] - Tgt<TT>::load1(p.t, i), c);
      }
    }
  }
}

// the shape of both launches, and the weights of the three branches of Train.py:420-427
struct SrL1Plan { SrL1Args a; bool vec; unsigned bx, planes; double w, n0, n1; };

unsigned blocks_per_plane(int B, int C, long P, bool vec) {
  const long units = vec ? P / 4 : P, planes = (long)B * C;
  long bx = (units + 1023) / 1024;                       // four units per thread and trip
  const long cap = planes >= 2048 ? 1 : 2048 / planes;   // about eight blocks per CU in all; the rest is the blocks' stride
  if (bx > cap) bx = cap;
  return (unsigned)(bx < 1 ? 1 : bx);
}

bool shape_bad(int B, int C, int H, int W) {
  return B <= 0 || C <= 0 || H <= 0 || W <= 0 || (long)B * C > 65535 || (long)H * W >= (1L << 31);
}

bool make_plan(const float* sr, const void* rgb, const void* ir, int target_dtype, int mode, int B, int C, int c_rgb, int c_ir,
               int H, int W, SrL1Plan* pl) {
  if (!sr || shape_bad(B, C, H, W) || (target_dtype != SODT_F32 && target_dtype != SODT_U8)) return false;
  int n_rgb;
  if (mode == SODT_SR_IR) { if (C != 1 || !ir || c_ir < 1) return false; n_rgb = 0; pl->w = 0.5; }
  else if (mode == SODT_SR_RGB) { if (!rgb || c_rgb != C) return false; n_rgb = C; pl->w = 0.5; }
  else if (mode == SODT_SR_RGB_IR) { if (C != 4 || !rgb || c_rgb != 3 || !ir || c_ir < 1) return false; n_rgb = 3; pl->w = 0.1; }
  else return false;
  const long P = (long)H * W;
  const int tsz = target_dtype == SODT_U8 ? 1 : 4;
  if (((uintptr_t)sr & 3) || ((uintptr_t)rgb & (tsz - 1)) || ((uintptr_t)ir & (tsz - 1))) return false;
  // the vector form needs every plane to start on a 16-byte (output_sr, f32 target) / 4-byte (uint8 target) boundary
  const uintptr_t tal = target_dtype == SODT_U8 ? 3 : 15;
  pl->vec = (P & 3) == 0 && ((uintptr_t)sr & 15) == 0 && (!rgb || n_rgb == 0 || ((uintptr_t)rgb & tal) == 0) &&
            (!ir || n_rgb == C || ((uintptr_t)ir & tal) == 0);
  SrL1Args& a = pl->a;
  a.sr = sr; a.tgt[0] = rgb; a.tgt[1] = ir;
  a.C = C; a.n_rgb = n_rgb; a.c_tgt[0] = c_rgb; a.c_tgt[1] = c_ir;
  a.P = (int)P; a.units = pl->vec ? P / 4 : P;
  pl->planes = (unsigned)(B * C);
  pl->bx = blocks_per_plane(B, C, P, pl->vec);
  pl->n0 = (double)B * (n_rgb > 0 ? n_rgb : C) * (double)P;
  pl->n1 = n_rgb > 0 ? (double)B * (C - n_rgb) * (double)P : 0.0;
  return true;
}

}  // namespace

// [ticket (16 bytes)] [one f64 partial per block]; sized for the form with the most blocks
extern "C" int sodt_sr_l1_workspace_bytes(int B, int C, int H, int W, size_t* bytes) {
  if (!bytes || shape_bad(B, C, H, W)) return SODT_EINVAL;
  const long P = (long)H * W;
  unsigned bx = blocks_per_plane(B, C, P, false);
  if ((P & 3) == 0) { const unsigned bv = blocks_per_plane(B, C, P, true); if (bv > bx) bx = bv; }
  *bytes = 16 + sizeof(double) * (size_t)bx * (size_t)(B * C);
  return SODT_OK;
}

// (returns from the calling entry point)
#define SODT_SR_L1_DISPATCH(KERNEL, ...)                                                                                        \
  do {                                                                                                                          \
    const dim3 grid(pl.bx, pl.planes), block(256);                                                                              \
    if (target_dtype == SODT_U8)                                                                                                \
      return pl.vec ? sodt_launch<KERNEL<unsigned char, true>>(grid, block, 0, s, __VA_ARGS__)                                  \
                    : sodt_launch<KERNEL<unsigned char, false>>(grid, block, 0, s, __VA_ARGS__);                                \
    return pl.vec ? sodt_launch<KERNEL<float, true>>(grid, block, 0, s, __VA_ARGS__)                                            \
                  : sodt_launch<KERNEL<float, false>>(grid, block, 0, s, __VA_ARGS__);                                          \
  } while (0)

extern "C" int sodt_sr_l1_fwd(const float* sr, const void* rgb, const void* ir, int target_dtype, int mode, int B, int C,
                              int c_rgb, int c_ir, int H, int W, void* ws, size_t ws_bytes, float* loss, sodt_stream_t st) {
  SrL1Plan pl;
  if (!make_plan(sr, rgb, ir, target_dtype, mode, B, C, c_rgb, c_ir, H, W, &pl)) return SODT_EINVAL;
  if (!ws || ((uintptr_t)ws & 15) || !loss || ((uintptr_t)loss & 3)) return SODT_EINVAL;
  if (ws_bytes < 16 + sizeof(double) * (size_t)pl.bx * pl.planes) return SODT_EINVAL;
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(ws, 0, 16, s) != hipSuccess) return SODT_ELAUNCH;       // the ticket starts every call at zero
  unsigned* ticket = (unsigned*)ws;
  double* part = (double*)((char*)ws + 16);
  SODT_SR_L1_DISPATCH(sr_l1_fwd_kernel, pl.a, pl.w, pl.n0, pl.n1, ticket, part, loss);
}

extern "C" int sodt_sr_l1_bwd(const float* sr, const void* rgb, const void* ir, int target_dtype, int mode, int B, int C,
                              int c_rgb, int c_ir, int H, int W, const float* upstream, float* dsr, sodt_stream_t st) {
  SrL1Plan pl;
  if (!make_plan(sr, rgb, ir, target_dtype, mode, B, C, c_rgb, c_ir, H, W, &pl)) return SODT_EINVAL;
  if (!upstream || ((uintptr_t)upstream & 3) || !dsr || ((uintptr_t)dsr & 3)) return SODT_EINVAL;
  if (pl.vec && ((uintptr_t)dsr & 15)) {                  // an unaligned gradient buffer: the element-wise form
    pl.vec = false;
    pl.a.units = pl.a.P;
    pl.bx = blocks_per_plane(B, C, pl.a.P, false);
  }
  hipStream_t s = (hipStream_t)st;
  const double wn0 = pl.w / pl.n0, wn1 = pl.n1 > 0.0 ? pl.w / pl.n1 : 0.0;
  SODT_SR_L1_DISPATCH(sr_l1_bwd_kernel, pl.a, upstream, wn0, wn1, dsr);
}
#undef SODT_SR_L1_DISPATCH
