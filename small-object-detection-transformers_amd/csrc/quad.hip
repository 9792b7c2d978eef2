// Quad collate on the device: LoadImagesAndLabels.collate_fn4 (basics/utils/datasets.py:637-664, --quad of Train.py:223) on the
// image side, alone and fused with the pre-processing after it.
//
//     per group g of four samples i = 4g .. 4g + 3, one draw random.random() < 0.5                      datasets.py:645-647
//       zoom: im = F.interpolate(img[i][None].float(), scale_factor=2., mode='bilinear', align_corners=False)[0].type(uint8)
//       tile: im = cat((cat((img[i], img[i+1]), 1), cat((img[i+2], img[i+3]), 1)), 2)                   datasets.py:654
//     image = imgs.to(device).float() / 255.0                                                            Train.py:364-365
//     imgs  = F.interpolate(image, size=[i // down_factor ...], mode='bilinear', align_corners=True)      Train.py:371-374
//
// Both kernels read a virtual pixel Q(g, c, y, x) of the 2H x 2W image of group g:
//   tile: source image 4g + (y >= H) + 2 (x >= W) at (y mod H, x mod W) - i+1 lies BELOW i, i+2 to the RIGHT;
//   zoom: (9 a + 3 b + 3 c + d) >> 4 on image 4g, a = in[y >> 1][x >> 1], b the vertical neighbour (row (y >> 1) - 1 for even
//         y, + 1 for odd y, clamped to the image), c the horizontal one by the same rule, d the diagonal one.  The half-pixel
//         2x zoom has the weights 1/4 and 3/4 only, every partial sum is an integer over 16 and exact in f32 in any order, and
//         the cast back to uint8 truncates: the integer form IS the reference's result, byte for byte.
// The mode of a group is bit g of zoom_mask, passed by value (no device table; hence at most 64 groups).  blockIdx.y is the
// group, so the mode is uniform in every workgroup and no wave mixes the two fetches.
//
// quad_u8_kernel materialises Q as uint8 (what SRLoss reads under --super, and what --multi-scale resizes): one thread
// makes 16 consecutive bytes of an output row - in tile mode one 16-byte load where the source is aligned and does not
// straddle the seam, in zoom mode from 2 x 10 source bytes - and stores them as 16 bytes where the row is aligned.
// preprocess_u8_quad_kernel is preprocess.hip's kernel with Q as its source: the same exact integer quotient / remainder
// for the align-corners coordinate, (float)k / 255.0f and the same blend with the same roundings (blend.h, shared: the two
// agree bit for bit on the materialised quad batch), one thread per four consecutive output pixels, one 16-byte store when
// aligned.  In zoom mode the four virtual pixels under an output pixel lie in a 3 x 3 source
// patch around ((y0 + 1) >> 1, (x0 + 1) >> 1): its nine bytes are fetched once.
#include "common.h"
#include "launch.h"
#include "blend.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int QD_THREADS = 256;
constexpr int QD_MAX_GROUPS = 64;           // bits of zoom_mask
constexpr long QD_MAX_BLOCKS = 256 * 32;

struct QuadArgs {
  const unsigned char* src[2];
  void* dst[2];               // uint8 (quad_u8_kernel) or f32 (preprocess_u8_quad_kernel) planes
  int ch[2];                  // channels of the RGB / IR tensor
  int H, W;                   // one source image
  int Hout, Wout;             // preprocess_u8_quad_kernel only
  unsigned long long zoom_mask;
};

__device__ __forceinline__ int qd_clamp(int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; }

// tile mode: offset of virtual pixel (y, x) from plane c of image 4g, in a (B, C, H, W) tensor
__device__ __forceinline__ long qd_tile_off(int y, int x, int H, int W, long img_stride) {
  const int below = y >= H, right = x >= W;
  return (long)(below + 2 * right) * img_stride + (long)(y - below * H) * W + (x - right * W);
}

__device__ __forceinline__ unsigned qd_zoom(unsigned a, unsigned b, unsigned c, unsigned d) { return (9u * a + 3u * b + 3u * c + d) >> 4; }

__global__ __launch_bounds__(QD_THREADS) void quad_u8_kernel(const QuadArgs a) {
  const int g = blockIdx.y;
  const bool zoom = (a.zoom_mask >> g) & 1ull;
  const int H = a.H, W = a.W, H2 = 2 * H, W2 = 2 * W;
  const int wq = (W2 + 15) >> 4;                          // 16-byte groups per output row
  const long per_plane = (long)H2 * wq;
  const long total = per_plane * (a.ch[0] + a.ch[1]);
  const long hw = (long)H * W;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    int c = (int)(idx / per_plane);
    const long rem = idx - c * per_plane;
    const int y = (int)(rem / wq), x0 = (int)(rem - (long)y * wq) * 16;
    const int which = c >= a.ch[0];
    if (which) c -= a.ch[0];
    const int C = a.ch[which];
    const unsigned char* sp = a.src[which] + ((long)(4 * g) * C + c) * hw;       // plane c of image 4g
    unsigned char* dp = (unsigned char*)a.dst[which] + ((long)g * C + c) * (4 * hw) + (long)y * W2 + x0;
    const long img_stride = (long)C * hw;
    unsigned w[4] = {0u, 0u, 0u, 0u};                     // the 16 bytes, little endian
    if (zoom) {
      const int ys = y >> 1, yn = qd_clamp(ys + ((y & 1) ? 1 : -1), H - 1);
      const unsigned char* ra = sp + (long)ys * W;
      const unsigned char* rb = sp + (long)yn * W;
      const int xs0 = x0 >> 1;                            // source columns xs0 - 1 .. xs0 + 8, clamped to the row
      unsigned pa[10], pb[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) {
        const int xc = qd_clamp(xs0 - 1 + k, W - 1);
        pa[k] = ra[xc];
        pb[k] = rb[xc];
      }
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const int k = 1 + (j >> 1);                       // pa[k] = in[ys][(x0 + j) >> 1] (or its clamp past the row's end)
        // the horizontal neighbour of an in-row pixel: k - 1 / k + 1 hold clamp(xs -/+ 1) because xs itself is inside the row
        const int kn = (j & 1) ? k + 1 : k - 1;
        w[j >> 2] |= qd_zoom(pa[k], pb[k], pa[kn], pb[kn]) << (8 * (j & 3));
      }
    } else {
      const bool one_half = x0 + 16 <= W || (x0 >= W && x0 + 16 <= W2);
      const unsigned char* s = sp + qd_tile_off(y, x0, H, W, img_stride);
      if (one_half && (((uintptr_t)s) & 15) == 0) {
        const uint4 v = *(const uint4*)s;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
          const int x = x0 + j < W2 ? x0 + j : W2 - 1;
          w[j >> 2] |= (unsigned)sp[qd_tile_off(y, x, H, W, img_stride)] << (8 * (j & 3));
        }
      }
    }
    if (x0 + 16 <= W2 && (((uintptr_t)dp) & 15) == 0) {
      *(uint4*)dp = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (x0 + j < W2) dp[j] = (unsigned char)(w[j >> 2] >> (8 * (j & 3)));
    }
  }
}

__global__ __launch_bounds__(QD_THREADS) void preprocess_u8_quad_kernel(const QuadArgs a) {
  const int g = blockIdx.y;
  const bool zoom = (a.zoom_mask >> g) & 1ull;
  const int H = a.H, W = a.W, Hin = 2 * H, Win = 2 * W;
  const int wq = (a.Wout + 3) >> 2;                       // 4-pixel groups per output row
  const long per_plane = (long)a.Hout * wq;
  const long total = per_plane * (a.ch[0] + a.ch[1]);
  const long hw = (long)H * W;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    int c = (int)(idx / per_plane);
    const long rem = idx - c * per_plane;
    const int oy = (int)(rem / wq), ox0 = (int)(rem - (long)oy * wq) * 4;
    const int which = c >= a.ch[0];
    if (which) c -= a.ch[0];
    const int C = a.ch[which];
    const unsigned char* sp = a.src[which] + ((long)(4 * g) * C + c) * hw;       // plane c of image 4g
    float* dp = (float*)a.dst[which] + ((long)g * C + c) * ((long)a.Hout * a.Wout) + (long)oy * a.Wout + ox0;
    const long img_stride = (long)C * hw;
    const int dy = a.Hout > 1 ? a.Hout - 1 : 1, ny = a.Hout > 1 ? oy * (Hin - 1) : 0;        // src = ny / dy exactly
    const int y0 = ny / dy;
    const float ly = (float)(ny - y0 * dy) / (float)dy;
    const int y1 = y0 + 1 < Hin ? y0 + 1 : Hin - 1;
    float o[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ox = ox0 + i < a.Wout ? ox0 + i : a.Wout - 1;
      const int dx = a.Wout > 1 ? a.Wout - 1 : 1, nx = a.Wout > 1 ? ox * (Win - 1) : 0;
      const int x0 = nx / dx;
      const float lx = (float)(nx - x0 * dx) / (float)dx;
      const int x1 = x0 + 1 < Win ? x0 + 1 : Win - 1;
      unsigned q00, q01, q10, q11;
      if (zoom) {
        // rows cy - 1 .. cy + 1 and columns cx - 1 .. cx + 1 (clamped) hold a and its neighbour for y0, y1 and x0, x1
        const int cy = (y0 + 1) >> 1, cx = (x0 + 1) >> 1;
        unsigned p[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const unsigned char* row = sp + (long)qd_clamp(cy - 1 + r, H - 1) * W;
#pragma unroll
          for (int k = 0; k < 3; ++k) p[r][k] = row[qd_clamp(cx - 1 + k, W - 1)];
        }
        // The zoom is separable before the shift: 9 a + 3 b + 3 c + d = sum_r wy[r] sum_k wx[k] p[r][k], weights 3 on a's row /
        // column and 1 on the neighbour's.  For the first index v0 of a pair a sits at patch entry 1 (v0 even, neighbour 0) or
        // 0 (v0 odd, neighbour 1): entry 2 never counts.  For v1 = v0 + 1 a sits at entry 1, neighbour 2 (v0 even) or 0 (v0
        // odd); a v1 clamped onto v0 repeats v0's weights.
        const bool xo = x0 & 1, yo = y0 & 1, xs = x1 == x0, ys = y1 == y0;
        const unsigned wx00 = xo ? 3u : 1u, wx01 = xo ? 1u : 3u;
        const unsigned wx10 = xs ? wx00 : xo ? 1u : 0u, wx11 = xs ? wx01 : 3u, wx12 = xs || xo ? 0u : 1u;
        const unsigned wy00 = yo ? 3u : 1u, wy01 = yo ? 1u : 3u;
        const unsigned wy10 = ys ? wy00 : yo ? 1u : 0u, wy11 = ys ? wy01 : 3u, wy12 = ys || yo ? 0u : 1u;
        unsigned h0[3], h1[3];                            // the patch's rows blended for column x0 / x1
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          h0[r] = wx00 * p[r][0] + wx01 * p[r][1];
          h1[r] = wx10 * p[r][0] + wx11 * p[r][1] + wx12 * p[r][2];
        }
        q00 = (wy00 * h0[0] + wy01 * h0[1]) >> 4;
        q01 = (wy00 * h1[0] + wy01 * h1[1]) >> 4;
        q10 = (wy10 * h0[0] + wy11 * h0[1] + wy12 * h0[2]) >> 4;
        q11 = (wy10 * h1[0] + wy11 * h1[1] + wy12 * h1[2]) >> 4;
      } else {
        q00 = sp[qd_tile_off(y0, x0, H, W, img_stride)];
        q01 = sp[qd_tile_off(y0, x1, H, W, img_stride)];
        q10 = sp[qd_tile_off(y1, x0, H, W, img_stride)];
        q11 = sp[qd_tile_off(y1, x1, H, W, img_stride)];
      }
      const float p00 = (float)q00 / 255.0f, p01 = (float)q01 / 255.0f;
      const float p10 = (float)q10 / 255.0f, p11 = (float)q11 / 255.0f;
      o[i] = sodt_blend4(ly, lx, p00, p01, p10, p11);
    }
    if (ox0 + 3 < a.Wout && (((uintptr_t)dp) & 15) == 0) {
      *(float4*)dp = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (ox0 + i < a.Wout) dp[i] = o[i];
    }
  }
}

// what both entries refuse: pointers, the batch, the group count, the sizes, the 32-bit offset inside one quad plane
bool qd_bad(const void* rgb, const void* ir, const void* out_rgb, const void* out_ir, int B, int c_rgb, int c_ir, int H, int W) {
  if (!rgb || !out_rgb || B < 4 || B / 4 > QD_MAX_GROUPS || c_rgb <= 0 || c_ir < 0 || (c_ir > 0 && (!ir || !out_ir))) return true;
  if (H <= 0 || W <= 0) return true;
  return 4L * H * W >= (1L << 31);
}

dim3 qd_grid(long units_per_group, int n) {
  long bx = (units_per_group + QD_THREADS - 1) / QD_THREADS;
  const long cap = QD_MAX_BLOCKS / n > 0 ? QD_MAX_BLOCKS / n : 1;
  if (bx > cap) bx = cap;
  return dim3((unsigned)bx, (unsigned)n);
}

}  // namespace

extern "C" int sodt_quad_u8(const unsigned char* rgb, const unsigned char* ir, unsigned char* out_rgb, unsigned char* out_ir,
                            int B, int c_rgb, int c_ir, int H, int W, unsigned long long zoom_mask, sodt_stream_t st) {
  if (qd_bad(rgb, ir, out_rgb, out_ir, B, c_rgb, c_ir, H, W)) return SODT_EINVAL;
  QuadArgs a;
  a.src[0] = rgb; a.src[1] = ir; a.dst[0] = out_rgb; a.dst[1] = out_ir;
  a.ch[0] = c_rgb; a.ch[1] = c_ir;
  a.H = H; a.W = W; a.Hout = 2 * H; a.Wout = 2 * W;
  a.zoom_mask = zoom_mask;
  const long units = 2L * H * ((2L * W + 15) / 16) * (c_rgb + c_ir);
  return sodt_launch<quad_u8_kernel>(qd_grid(units, B / 4), dim3(QD_THREADS), 0, (hipStream_t)st, a);
}

extern "C" int sodt_preprocess_u8_quad(const unsigned char* rgb, const unsigned char* ir, float* out_rgb, float* out_ir, int B,
                                       int c_rgb, int c_ir, int H, int W, int Hout, int Wout, unsigned long long zoom_mask,
                                       sodt_stream_t st) {
  if (qd_bad(rgb, ir, out_rgb, out_ir, B, c_rgb, c_ir, H, W)) return SODT_EINVAL;
  if (Hout <= 0 || Wout <= 0 || Hout > 2 * H || Wout > 2 * W) return SODT_EINVAL;
  if (2L * H * Hout >= (1L << 31) || 2L * W * Wout >= (1L << 31)) return SODT_EINVAL;
  QuadArgs a;
  a.src[0] = rgb; a.src[1] = ir; a.dst[0] = out_rgb; a.dst[1] = out_ir;
  a.ch[0] = c_rgb; a.ch[1] = c_ir;
  a.H = H; a.W = W; a.Hout = Hout; a.Wout = Wout;
  a.zoom_mask = zoom_mask;
  const long units = (long)Hout * ((Wout + 3) / 4) * (c_rgb + c_ir);
  return sodt_launch<preprocess_u8_quad_kernel>(qd_grid(units, B / 4), dim3(QD_THREADS), 0, (hipStream_t)st, a);
}
