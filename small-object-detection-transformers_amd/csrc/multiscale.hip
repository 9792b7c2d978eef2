// Multi-scale training on the device: the input side of Train.py:396-402 fused with the pre-processing before it.
//
//     image = imgs.to(device).float() / 255.0                                                         Train.py:364-365
//     imgs  = F.interpolate(image, size=[i // down_factor ...], mode='bilinear', align_corners=True)   Train.py:371-374
//     imgs  = F.interpolate(imgs, size=ns, mode='bilinear', align_corners=False)                       Train.py:401-402
//
// for the RGB and the IR batch in ONE launch: uint8 planes in, f32 planes at the drawn size out, no global intermediate.
// Stage 1 (align_corners=True, a shrink) is the arithmetic of preprocess.hip: src = o * (in - 1) / (mid - 1).  Stage 2
// (align_corners=False, either direction) is ATen's area_pixel_compute_source_index: src = (o + 0.5) * mid / out - 0.5 clamped
// at 0, i.e. n / d with n = max((2 o + 1) * mid - out, 0), d = 2 * out.  Both take the source index and the blend weight from
// the exact integer quotient and remainder (one rounding, in the final division), and every stage-1 value an output pixel
// blends is formed and rounded in f32, as the reference's f32 intermediate is.
//
// A workgroup walks output tiles of up to 32 x 256 pixels.  Per tile it writes the coordinate tables of the tile's rows and
// columns to LDS (the integer divisions happen once per row / column, not per pixel), evaluates stage 1 ONCE for every
// intermediate pixel under the tile into an LDS patch (at S = 1536 from 512 a stage-1 pixel feeds nine outputs), and blends
// stage 2 out of the patch: one thread per four consecutive output pixels, one 16-byte store when aligned.  Where the second
// stage shrinks by more than four in area an output pixel's four stage-1 values cost less than the patch under it (and
// under a long enough shrink no patch fits the LDS): such launches skip the patch and form the four values per pixel.
#include "common.h"
#include "bilinear.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_TW = 256, MS_TH = 32;      // largest output tile (columns, rows)
constexpr int MS_PATCH = 4096;              // f32 stage-1 values of one tile (16 KB)
constexpr int MS_FW = 512, MS_FH = 128;     // largest patch width / height (coordinate-table entries)

struct MsArgs {
  const unsigned char* src[2]; float* dst[2];
  int planes[2];              // B * channels of the RGB / IR tensor
  int Hin, Win, Hmid, Wmid, Hout, Wout;
  int tw, th;                 // output tile (tw a multiple of 4)
  int fw_cap, fh_cap;         // bound of the patch under one tile; fw_cap == 0: no patch, stage 1 per output pixel
};

// float(k) / 255.0f, correctly rounded, for k = 0 .. 255 (srloss.hip: q = k * RN(1 / 255) and one Newton correction with the
// exact remainder; identical to the IEEE quotient for each of the 256 inputs at a quarter of its cost)
__device__ __forceinline__ float ms_unit(unsigned k) {
  const float kf = (float)k, r = 0x1.010102p-8f;
  const float q = kf * r;
  return fmaf(fmaf(-q, 255.0f, kf), r, q);
}

// stage 1, align_corners=True: source index and weight of intermediate index o (in -> mid pixels)
__device__ __forceinline__ void ms_coord1(int o, int in, int mid, int& i0, float& l) {
  const int d = mid > 1 ? mid - 1 : 1, n = mid > 1 ? o * (in - 1) : 0;      // src = n / d exactly
  i0 = n / d;
  l = (float)(n - i0 * d) / (float)d;
}

// stage 2, align_corners=False: ms_coord2 of bilinear.h (mid -> out pixels)

// the stage-1 value at rows (y0, y1, ly), columns (x0, x1, lx) of one uint8 plane
__device__ __forceinline__ float ms_value1(const unsigned char* sp, int Win, int y0, int y1, float ly, int x0, int x1, float lx) {
  const unsigned r0 = (unsigned)y0 * (unsigned)Win, r1 = (unsigned)y1 * (unsigned)Win;
  const float p00 = ms_unit(sp[r0 + x0]), p01 = ms_unit(sp[r0 + x1]);
  const float p10 = ms_unit(sp[r1 + x0]), p11 = ms_unit(sp[r1 + x1]);
  return (1.f - ly) * ((1.f - lx) * p00 + lx * p01) + ly * ((1.f - lx) * p10 + lx * p11);
}

// the stage-1 value of intermediate pixel (ym, xm), coordinates included (the launches without a patch)
__device__ __forceinline__ float ms_value1_at(const unsigned char* sp, const MsArgs& a, int ym, int xm) {
  int y0, x0;
  float ly, lx;
  ms_coord1(ym, a.Hin, a.Hmid, y0, ly);
  ms_coord1(xm, a.Win, a.Wmid, x0, lx);
  return ms_value1(sp, a.Win, y0, y0 + 1 < a.Hin ? y0 + 1 : a.Hin - 1, ly, x0, x0 + 1 < a.Win ? x0 + 1 : a.Win - 1, lx);
}

__global__ __launch_bounds__(MS_THREADS) void preprocess_u8_ms_kernel(const MsArgs a) {
  __shared__ float patch[MS_PATCH];
  __shared__ int oc_i[MS_TW], or_i[MS_TH], mc_i[MS_FW], mr_i[MS_FH];          // out column / row -> intermediate index,
  __shared__ float oc_l[MS_TW], or_l[MS_TH], mc_l[MS_FW], mr_l[MS_FH];        // patch column / row -> source index; weights
  const int tid = threadIdx.x;
  const int tiles_x = (a.Wout + a.tw - 1) / a.tw, tiles_y = (a.Hout + a.th - 1) / a.th;
  const long per_plane = (long)tiles_x * tiles_y;
  const long total = per_plane * (a.planes[0] + a.planes[1]);
  const bool use_patch = a.fw_cap > 0;
  for (long u = blockIdx.x; u < total; u += gridDim.x) {        // u depends on the block alone: every barrier below is uniform
    long pl = u / per_plane;
    const long t = u - pl * per_plane;
    const int ty = (int)(t / tiles_x), tx = (int)(t - (long)ty * tiles_x);
    const int which = pl >= a.planes[0];
    if (which) pl -= a.planes[0];
    const unsigned char* sp = a.src[which] + pl * (long)a.Hin * a.Win;
    float* dpl = a.dst[which] + pl * (long)a.Hout * a.Wout;
    const int ox_t = tx * a.tw, oy_t = ty * a.th;
    const int cols = a.Wout - ox_t < a.tw ? a.Wout - ox_t : a.tw;           // valid columns / rows of this tile
    const int rows = a.Hout - oy_t < a.th ? a.Hout - oy_t : a.th;
    __syncthreads();                                                        // the previous tile's readers are done
    // (A) stage-2 coordinates of the tile's columns and rows; a column past the row's end repeats the last one
    for (int c = tid; c < a.tw + a.th; c += MS_THREADS) {
      if (c < a.tw) {
        ms_coord2(ox_t + (c < cols ? c : cols - 1), a.Wmid, a.Wout, oc_i[c], oc_l[c]);
      } else {
        const int r = c - a.tw;
        ms_coord2(oy_t + (r < rows ? r : rows - 1), a.Hmid, a.Hout, or_i[r], or_l[r]);
      }
    }
    __syncthreads();
    const int xb = oc_i[0], yb = or_i[0];                                   // first intermediate column / row under the tile
    int fw = 0;
    if (use_patch) {
      // (B) stage-1 coordinates of the patch's columns and rows (the indices grow with the output index: the last one bounds them)
      const int xe = oc_i[cols - 1] + 1 < a.Wmid ? oc_i[cols - 1] + 1 : a.Wmid - 1;
      const int ye = or_i[rows - 1] + 1 < a.Hmid ? or_i[rows - 1] + 1 : a.Hmid - 1;
      fw = xe - xb + 1 < a.fw_cap ? xe - xb + 1 : a.fw_cap;                 // (the caps hold by construction: see the entry point)
      const int fh = ye - yb + 1 < a.fh_cap ? ye - yb + 1 : a.fh_cap;
      for (int c = tid; c < fw + fh; c += MS_THREADS) {
        if (c < fw) ms_coord1(xb + c, a.Win, a.Wmid, mc_i[c], mc_l[c]);
        else ms_coord1(yb + c - fw, a.Hin, a.Hmid, mr_i[c - fw], mr_l[c - fw]);
      }
      __syncthreads();
      // (C) stage 1, once per intermediate pixel under the tile
      const float rcp = 1.0f / (float)fw;
      for (int i = tid; i < fw * fh; i += MS_THREADS) {
        int fy, fx;
        ms_divmod(i, fw, rcp, fy, fx);
        const int y0 = mr_i[fy], x0 = mc_i[fx];
        patch[i] = ms_value1(sp, a.Win, y0, y0 + 1 < a.Hin ? y0 + 1 : a.Hin - 1, mr_l[fy], x0, x0 + 1 < a.Win ? x0 + 1 : a.Win - 1, mc_l[fx]);
      }
      __syncthreads();
    }
    // (D) stage 2: four consecutive output pixels per thread
    const int gq = (cols + 3) >> 2;
    const float rcq = 1.0f / (float)gq;
    for (int i = tid; i < rows * gq; i += MS_THREADS) {
      int r, g;
      ms_divmod(i, gq, rcq, r, g);
      const int c0 = g * 4;
      const int ym0 = or_i[r], ym1 = ym0 + 1 < a.Hmid ? ym0 + 1 : a.Hmid - 1;
      const float ly = or_l[r];
      float o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int xm0 = oc_i[c0 + k], xm1 = xm0 + 1 < a.Wmid ? xm0 + 1 : a.Wmid - 1;
        const float lx = oc_l[c0 + k];
        float m00, m01, m10, m11;
        if (use_patch) {
          const int q0 = (ym0 - yb) * fw - xb, q1 = (ym1 - yb) * fw - xb;
          m00 = patch[q0 + xm0]; m01 = patch[q0 + xm1];
          m10 = patch[q1 + xm0]; m11 = patch[q1 + xm1];
        } else {
          m00 = ms_value1_at(sp, a, ym0, xm0); m01 = ms_value1_at(sp, a, ym0, xm1);
          m10 = ms_value1_at(sp, a, ym1, xm0); m11 = ms_value1_at(sp, a, ym1, xm1);
        }
        o[k] = (1.f - ly) * ((1.f - lx) * m00 + lx * m01) + ly * ((1.f - lx) * m10 + lx * m11);
      }
      float* dp = dpl + (long)(oy_t + r) * a.Wout + ox_t + c0;
      if (c0 + 3 < cols && (((uintptr_t)dp) & 15) == 0) {
        *(float4*)dp = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < cols) dp[k] = o[k];
      }
    }
  }
}

// Largest index distance + 1 between the first intermediate pixel under output pixel o and the second under o + n - 1:
// floor(src(o + n - 1)) + 1 - floor(src(o)) + 1 <= (n - 1) * mid / out + 3, and never more than mid.
long ms_span(int n, int mid, int out) {
  const long s = (long)(n - 1) * mid / out + 3;
  return s < mid ? s : mid;
}

}  // namespace

extern "C" int sodt_preprocess_u8_ms(const unsigned char* rgb, const unsigned char* ir, float* out_rgb, float* out_ir, int B,
                                     int c_rgb, int c_ir, int Hin, int Win, int Hmid, int Wmid, int Hout, int Wout,
                                     sodt_stream_t st) {
  if (!rgb || !ir || !out_rgb || !out_ir || B <= 0 || c_rgb <= 0 || c_ir <= 0) return SODT_EINVAL;
  if (Hin <= 0 || Win <= 0 || Hmid <= 0 || Wmid <= 0 || Hout <= 0 || Wout <= 0 || Hmid > Hin || Wmid > Win) return SODT_EINVAL;
  const long lim = 1L << 31;
  // o * (in - 1) of stage 1; (2 o + 1) * mid and 2 * out of stage 2; the 32-bit pixel offset inside one source plane
  if ((long)Hin * Hmid >= lim || (long)Win * Wmid >= lim || 2L * Hout * Hmid >= lim || 2L * Wout * Wmid >= lim ||
      2L * Hout >= lim || 2L * Wout >= lim || (long)Hin * Win >= lim)
    return SODT_EINVAL;
  MsArgs a;
  a.src[0] = rgb; a.src[1] = ir; a.dst[0] = out_rgb; a.dst[1] = out_ir;
  a.planes[0] = B * c_rgb; a.planes[1] = B * c_ir;
  a.Hin = Hin; a.Win = Win; a.Hmid = Hmid; a.Wmid = Wmid; a.Hout = Hout; a.Wout = Wout;
  // The output tile: as large as the LDS patch under it allows, rows first.  No patch where the second stage shrinks by more
  // than four in area (an output pixel then needs fewer stage-1 values than lie under it) or where nothing fits.
  // The widest tile splits a row evenly (576 columns: 3 x 192, not 256 + 256 + 64), so every tile is a full one.
  const int tiles_w = (Wout + MS_TW - 1) / MS_TW, tw_max = ((Wout + tiles_w - 1) / tiles_w + 3) / 4 * 4;
  const int th_max = Hout < MS_TH ? Hout : MS_TH;
  int tw = tw_max, th = th_max;
  auto fits = [&](int w, int h) {
    const long fw = ms_span(w < Wout ? w : Wout, Wmid, Wout), fh = ms_span(h, Hmid, Hout);
    return fw <= MS_FW && fh <= MS_FH && fw * fh <= MS_PATCH;
  };
  bool patch = (long)Hmid * Wmid <= 4L * Hout * Wout;
  if (patch) {
    while (!fits(tw, th) && th > 1) th = (th + 1) / 2;
    while (!fits(tw, th) && tw > 4) tw = (tw / 2 + 3) / 4 * 4;
    patch = fits(tw, th);
  }
  if (!patch) { tw = tw_max; th = th_max; }
  a.tw = tw; a.th = th;
  a.fw_cap = patch ? (int)ms_span(tw < Wout ? tw : Wout, Wmid, Wout) : 0;
  a.fh_cap = patch ? (int)ms_span(th, Hmid, Hout) : 0;
  const long total = (long)((Wout + tw - 1) / tw) * ((Hout + th - 1) / th) * (a.planes[0] + a.planes[1]);
  const long blocks = total < 2048 ? total : 2048;
  return sodt_launch<preprocess_u8_ms_kernel>(dim3((unsigned)blocks), dim3(MS_THREADS), 0, (hipStream_t)st, a);
}
