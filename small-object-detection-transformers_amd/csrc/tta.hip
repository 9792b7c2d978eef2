// Test-time augmentation (basics/models/model.py:155-184, the `--augment` of basics/test.py): the two ends of the augmented
// forward that are not the plain forward itself.
//
//     xi  = scale_img(x.flip(fi) if fi else x, si, gs)              model.py:161-162, torch_utils.py:249-259
//           = F.pad(F.interpolate(img, size=(int(h * si), int(w * si)), mode='bilinear', align_corners=False), value=0.447)
//     yi[..., :4] /= si;  yi[..., 1] = img_size[0] - yi[..., 1]  |  yi[..., 0] = img_size[1] - yi[..., 0]      model.py:178-182
//
// tta_scale_kernel makes every augmented input of one call - all passes, RGB and IR - in ONE launch: f32 planes in, f32 planes
// at each pass's padded size out, every output element written (the pad as 0.447f), no memset, no intermediate.  The source
// coordinate is ms_coord2 of bilinear.h (exact integer quotient and remainder, one rounding in the weight); the flip is index
// arithmetic on that coordinate, so it happens before the resize as in the reference.  With the content size equal to the
// input's, every weight is exactly 0 and the result is the flipped copy bit for bit.
//
// A workgroup walks output tiles of up to 32 x 256 pixels (multiscale.hip's tile).  Per tile it writes the tables of the tile's
// rows and columns to LDS - both source indices, already flipped, and the weight; -1 marks a pad row / column - so the integer
// divisions happen once per row / column, and then one thread makes four consecutive output pixels from their sixteen source
// values and stores them with one 16-byte store where aligned.  The kernel is memory-bound: consecutive threads read
// neighbouring source pixels (a shrink by 0.67 touches every cache line of the source once per tile row pair).
//
// detect_decode_tta_kernel is detect_decode_kernel (head.hip, the same detect_decode_value) for one pass, writing rows
// row_off .. row_off + na * ny * nx of the concatenated z (B, rows_total, no) with the de-scale and the de-flip applied.
#include "common.h"
#include "bilinear.h"
#include "detect_decode.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int TTA_THREADS = 256;
constexpr int TTA_TW = 256, TTA_TH = 32;    // largest output tile (columns, rows)
constexpr float TTA_PAD = 0.447f;           // torch_utils.py:259: the imagenet mean

struct TtaPass {
  float* dst[2];
  int h, w, Hp, Wp, flip;
  int tw, th, tiles_x;        // output tile (tw a multiple of 4) and tiles per row of tiles
  long tiles;                 // tiles of one plane
  long first;                 // first work unit of this pass
};

struct TtaArgs {
  const float* src[2];
  int planes[2];              // B * channels of the RGB / IR tensor
  int H, W, npass;
  long total;                 // work units of the launch: (pass, plane, tile)
  TtaPass p[SODT_TTA_MAX_PASSES];
};

__global__ __launch_bounds__(TTA_THREADS) void tta_scale_kernel(const TtaArgs a) {
  __shared__ int c_i0[TTA_TW], c_i1[TTA_TW], r_i0[TTA_TH], r_i1[TTA_TH];      // source column / row of an output column / row
  __shared__ float c_l[TTA_TW], r_l[TTA_TH];                                  // (flip applied; -1: pad) and the blend weights
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W;
  for (long u = blockIdx.x; u < a.total; u += gridDim.x) {       // u depends on the block alone: every barrier below is uniform
    int k = 0;
    while (k + 1 < a.npass && u >= a.p[k + 1].first) ++k;
    const TtaPass& p = a.p[k];
    const long v = u - p.first;
    long pl = v / p.tiles;
    const long t = v - pl * p.tiles;
    const int ty = (int)(t / p.tiles_x), tx = (int)(t - (long)ty * p.tiles_x);
    const int which = pl >= a.planes[0];
    if (which) pl -= a.planes[0];
    const float* sp = a.src[which] + pl * (long)H * W;
    float* dpl = p.dst[which] + pl * (long)p.Hp * p.Wp;
    const int ox_t = tx * p.tw, oy_t = ty * p.th;
    const int cols = p.Wp - ox_t < p.tw ? p.Wp - ox_t : p.tw;              // valid columns / rows of this tile
    const int rows = p.Hp - oy_t < p.th ? p.Hp - oy_t : p.th;
    __syncthreads();                                                        // the previous tile's readers are done
    for (int c = tid; c < p.tw + p.th; c += TTA_THREADS) {
      if (c < p.tw) {                                                       // a column past the row's end repeats the last one
        const int ox = ox_t + (c < cols ? c : cols - 1);
        int i0 = -1, i1 = -1;
        float l = 0.f;
        if (ox < p.w) {
          ms_coord2(ox, W, p.w, i0, l);
          i1 = i0 + 1 < W ? i0 + 1 : W - 1;
          if (p.flip == 3) { i0 = W - 1 - i0; i1 = W - 1 - i1; }
        }
        c_i0[c] = i0; c_i1[c] = i1; c_l[c] = l;
      } else {
        const int r = c - p.tw;
        const int oy = oy_t + (r < rows ? r : rows - 1);
        int i0 = -1, i1 = -1;
        float l = 0.f;
        if (oy < p.h) {
          ms_coord2(oy, H, p.h, i0, l);
          i1 = i0 + 1 < H ? i0 + 1 : H - 1;
          if (p.flip == 2) { i0 = H - 1 - i0; i1 = H - 1 - i1; }
        }
        r_i0[r] = i0; r_i1[r] = i1; r_l[r] = l;
      }
    }
    __syncthreads();
    const int gq = (cols + 3) >> 2;
    const float rcq = 1.0f / (float)gq;
    for (int i = tid; i < rows * gq; i += TTA_THREADS) {
      int r, g;
      ms_divmod(i, gq, rcq, r, g);
      const int c0 = g * 4;
      const int y0 = r_i0[r], y1 = r_i1[r];
      const float ly = r_l[r];
      float o[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int x0 = c_i0[c0 + q], x1 = c_i1[c0 + q];
        const float lx = c_l[c0 + q];
        float val = TTA_PAD;
        if (y0 >= 0 && x0 >= 0) {
          const unsigned q0 = (unsigned)y0 * (unsigned)W, q1 = (unsigned)y1 * (unsigned)W;
          const float m00 = sp[q0 + x0], m01 = sp[q0 + x1], m10 = sp[q1 + x0], m11 = sp[q1 + x1];
          val = (1.f - ly) * ((1.f - lx) * m00 + lx * m01) + ly * ((1.f - lx) * m10 + lx * m11);
        }
        o[q] = val;
      }
      float* dp = dpl + (long)(oy_t + r) * p.Wp + ox_t + c0;
      if (c0 + 3 < cols && (((uintptr_t)dp) & 15) == 0) {
        *(float4*)dp = make_float4(o[0], o[1], o[2], o[3]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (c0 + q < cols) dp[q] = o[q];
      }
    }
  }
}

__global__ __launch_bounds__(256) void detect_decode_tta_kernel(const float* __restrict__ raw, const float* __restrict__ anchor_grid,
                                                               float* __restrict__ zout, int na, int ny, int nx, int no,
                                                               float stride, long row_off, long rows_total, float si, int flip,
                                                               float img_h, float img_w) {
  // blockIdx.y is the image; an image's na * ny * nx * no values fit 31 bits (the entry checks), so the index arithmetic is
  // 32-bit (the 64-bit quotients of the flat index cost more than the traffic)
  const unsigned per_image = (unsigned)na * ny * nx * no;
  const long b = blockIdx.y;
  const float* rp = raw + b * per_image;
  float* zp = zout + (b * rows_total + row_off) * no;
  for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < per_image; i += gridDim.x * 256u) {
    const unsigned cell = i / (unsigned)no, row = cell / (unsigned)nx, a = row / (unsigned)ny;
    const int o = (int)(i - cell * no), x = (int)(cell - row * nx), y = (int)(row - a * ny);
    float v = detect_decode_value(rp[i], o, x, y, (int)a, anchor_grid, stride);
    if (o < 4) {
      v = v / si;                                    // model.py:178, IEEE f32 division as ATen's CPU kernel does it
      if (o == 0 && flip == 3) v = img_w - v;        // model.py:182
      if (o == 1 && flip == 2) v = img_h - v;        // model.py:180
    }
    zp[i] = v;
  }
}

inline unsigned tta_blocks(long work, int cap = 4096) {
  long b = (work + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

}  // namespace

extern "C" int sodt_tta_scale(const float* rgb, const float* ir, int B, int c_rgb, int c_ir, int H, int W,
                              const sodt_tta_pass* passes, int npass, sodt_stream_t st) {
  if (!rgb || !passes || B <= 0 || c_rgb <= 0 || c_ir < 0 || H <= 0 || W <= 0) return SODT_EINVAL;
  if (c_ir > 0 && !ir) return SODT_EINVAL;
  if (npass <= 0 || npass > SODT_TTA_MAX_PASSES) return SODT_EINVAL;
  const long lim = 1L << 31;
  if ((long)H * W >= lim) return SODT_EINVAL;                                 // the 32-bit pixel offset inside one source plane
  TtaArgs a;
  a.src[0] = rgb; a.src[1] = ir;
  a.planes[0] = B * c_rgb; a.planes[1] = B * c_ir;
  a.H = H; a.W = W; a.npass = npass;
  long first = 0;
  for (int k = 0; k < npass; ++k) {
    const sodt_tta_pass& s = passes[k];
    if (!s.out_rgb || (c_ir > 0 && !s.out_ir)) return SODT_EINVAL;
    if (s.h <= 0 || s.w <= 0 || s.Hp <= 0 || s.Wp <= 0 || s.h > s.Hp || s.w > s.Wp) return SODT_EINVAL;
    if (s.flip != 0 && s.flip != 2 && s.flip != 3) return SODT_EINVAL;
    // (2 o + 1) * in and 2 * out of ms_coord2; the tile origin plus a tile stays an int
    if (2L * s.h * H >= lim || 2L * s.w * W >= lim || (long)s.Hp + TTA_TH >= lim || (long)s.Wp + TTA_TW >= lim) return SODT_EINVAL;
    TtaPass& p = a.p[k];
    p.dst[0] = s.out_rgb; p.dst[1] = s.out_ir;
    p.h = s.h; p.w = s.w; p.Hp = s.Hp; p.Wp = s.Wp; p.flip = s.flip;
    // the widest tile splits a row evenly (576 columns: 3 x 192, not 256 + 256 + 64), so every tile is a full one
    const int tiles_w = (s.Wp + TTA_TW - 1) / TTA_TW;
    p.tw = ((s.Wp + tiles_w - 1) / tiles_w + 3) / 4 * 4;
    p.th = s.Hp < TTA_TH ? s.Hp : TTA_TH;
    p.tiles_x = (s.Wp + p.tw - 1) / p.tw;
    p.tiles = (long)p.tiles_x * ((s.Hp + p.th - 1) / p.th);
    p.first = first;
    first += p.tiles * (a.planes[0] + a.planes[1]);
  }
  for (int k = npass; k < SODT_TTA_MAX_PASSES; ++k) a.p[k] = a.p[0];
  a.total = first;
  const long blocks = a.total < 2048 ? a.total : 2048;
  return sodt_launch<tta_scale_kernel>(dim3((unsigned)blocks), dim3(TTA_THREADS), 0, (hipStream_t)st, a);
}

extern "C" int sodt_detect_decode_tta(const float* raw, const float* anchor_grid, float* z, int B, int na, int ny, int nx,
                                      int no, float stride, long row_off, long rows_total, float si, int flip, int img_h,
                                      int img_w, sodt_stream_t st) {
  if (!raw || !anchor_grid || !z || B <= 0 || na <= 0 || ny <= 0 || nx <= 0 || no < 5) return SODT_EINVAL;
  const long lim = 1L << 31;
  const long cells = (long)na * ny;                                           // (each product checked before the next: no overflow)
  if (cells >= lim || cells * nx >= lim || cells * nx * no >= lim || B > 65535) return SODT_EINVAL;      // 32-bit index inside an image; grid.y
  const long per_image = cells * nx * no;
  if (row_off < 0 || rows_total <= 0 || cells * nx > rows_total || row_off > rows_total - cells * nx) return SODT_EINVAL;
  if (!(si > 0.f) || !(si <= 3.4e38f) || (flip != 0 && flip != 2 && flip != 3) || img_h <= 0 || img_w <= 0) return SODT_EINVAL;
  return sodt_launch<detect_decode_tta_kernel>(dim3(tta_blocks(per_image), (unsigned)B), dim3(256), 0, (hipStream_t)st,
                     raw, anchor_grid, z, na, ny, nx, no, stride, row_off, rows_total, si, flip, (float)img_h, (float)img_w);
}
