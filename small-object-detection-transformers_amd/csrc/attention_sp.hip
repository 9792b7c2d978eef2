// Shifted window attention (SW-MSA) on a ZERO-PADDED grid for gfx950: the attention core of a shifted Swin block whose
// H x W token grid is no multiple of its 8-token window (backbone_vit.py:1084-1125 with window_partition / window_unpartition
// :619-672 and the mask of :1058-1077).
//
// The reference rolls the UNPADDED grid by (-shift, -shift), zero-pads the rolled grid at the bottom / right to Hp x Wp AFTER
// norm1 (so a pad token's q / k / v are the qkv bias), partitions Hp x Wp into windows, attends with the relative-position
// bias and the 0 / -100 mask whose region ids come from the unpadded rolled grid (pad positions: id 0, the zero padding of the
// id image), un-partitions, crops to H x W and rolls back.  Here all of that is index arithmetic: qkv / out / dout / dqkv stay
// on the unpadded grid in natural token order, the padded grid is never materialised.  Per window the 64-entry map
// "window slot -> source token row, or pad" and the 64 region ids are formed once and kept in LDS; a pad key / value reads
// qkv_bias (narrowed to the run dtype as a stored qkv row would be), a pad query is not computed into memory (its output is
// cropped) and carries no gradient.  attention.hip derives both the roll and the region ids from the partition geometry,
// which is why its kernels cannot run this block with a padded H, W.
//
// One workgroup = NW waves = NW heads of one window (one 64-token tile); Q K^T and P V on MFMA 16x16 tiles through mma16<T>(),
// P through LDS, as attn_fwd_kernel / attn_bwd_kernel of attention.hip (single-tile case), from which the tile layout and the
// fragment helpers are copied.  The backward recomputes P from the saved log-sum-exp, walks the windows of a head group
// persistently with the relative-position-bias gradient summed in registers, writes dqkv for every real token and ADDS the
// k / v gradient of the pad keys to dqkv_bias: summed in registers over the windows a wave visits, reduced inside the wave, then
// one atomic per channel.
#include "common.h"
#include "launch.h"
#include "routes.h"
#include <type_traits>

namespace {

#define SP_LOG2E 1.4426950408889634f
constexpr int SP_WS = 8, SP_L2 = 2 * SP_WS - 1, SP_LT = SP_L2 * SP_L2;

// window slot n of window (b, wy, wx) of the padded, rolled grid -> token row of the unpadded grid (-1: pad) and mask region
__device__ __forceinline__ void sp_token(const SpGeo& g, int b, int wy, int wx, int n, int& row, int& rid) {
  const int iy = n >> 3, ix = n & 7;
  const int ys = wy * SP_WS + iy, xs = wx * SP_WS + ix;       // position in the rolled grid
  if (ys >= g.H || xs >= g.W) { row = -1; rid = 0; return; }
  int y = ys + g.shift, x = xs + g.shift;                     // roll by -shift: rolled[i] = grid[(i + shift) mod size]
  if (y >= g.H) y -= g.H;
  if (x >= g.W) x -= g.W;
  row = (b * g.H + y) * g.W + x;
  const int ry = ys < g.H - SP_WS ? 0 : (ys < g.H - g.shift ? 1 : 2);
  const int rx = xs < g.W - SP_WS ? 0 : (xs < g.W - g.shift ? 1 : 2);
  rid = ry * 3 + rx;
}

template <typename T, int HD>
struct Lay {
  static constexpr int E = TT<T>::SZ;
  static constexpr int KPL = TT<T>::KPL;
  static constexpr int QROW = HD * E + 16;     // [64 tokens][HD] tile row (bytes)
  static constexpr int TROW = 64 * E + 16;     // [64][64] tile row (bytes)
  static constexpr int QTILE = 64 * QROW;
  static constexpr int STILE = 64 * TROW;
  static constexpr int DCH = HD / KPL;         // 16-byte chunks per head row
  static constexpr int KBQ = (HD + TT<T>::MMA_K - 1) / TT<T>::MMA_K;   // mma steps over d
  static constexpr int KBT = 64 / TT<T>::MMA_K;                        // mma steps over 64 tokens
};

// MFMA operand fragment from a [rows][K] tile: lane reads 16 bytes at (row0 + (l&15), k = kb*MMA_K + KPL*(l>>4))
template <typename T>
__device__ __forceinline__ uint4 frag(const unsigned char* tile, int rowbytes, int row0, int kb, int klimit, int lane) {
  const int k = kb * TT<T>::MMA_K + TT<T>::KPL * (lane >> 4);
  if (k >= klimit) return make_uint4(0, 0, 0, 0);
  return *(const uint4*)(tile + (row0 + (lane & 15)) * rowbytes + k * TT<T>::SZ);
}

// fragment whose contraction index runs along the LDS ROWS of a [K rows][cols] tile (see attention.hip).  EXEC must be full.
template <typename T> __device__ __forceinline__ uint4 fragT(const unsigned char* tile, int rowbytes, int k0, int col0, int lane);
template <> __device__ __forceinline__ uint4 fragT<bf16>(const unsigned char* tile, int rowbytes, int k0, int col0, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const unsigned char* a = tile + (k0 + 8 * g + q) * rowbytes + (col0 + 4 * p) * 2;
  typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
  union { s16x4 v; uint2 u; } lo, hi;
  lo.v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a));
  hi.v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(a + 4 * rowbytes));
  return make_uint4(lo.u.x, lo.u.y, hi.u.x, hi.u.y);
}
template <> __device__ __forceinline__ uint4 fragT<float>(const unsigned char* tile, int rowbytes, int k0, int col0, int lane) {
  const unsigned char* a = tile + (k0 + 4 * (lane >> 4)) * rowbytes + (col0 + (lane & 15)) * 4;
  uint4 r;
  r.x = *(const uint32_t*)(a);
  r.y = *(const uint32_t*)(a + rowbytes);
  r.z = *(const uint32_t*)(a + 2 * rowbytes);
  r.w = *(const uint32_t*)(a + 3 * rowbytes);
  return r;
}

template <typename T> __device__ __forceinline__ void st_elem(unsigned char* p, float v) { *(T*)p = from_f<T>(v); }

// store 4 consecutive elements (accumulator rows 4g..4g+3 of one column) into a transposed tile
template <typename T> __device__ __forceinline__ void st4(unsigned char* p, const f32x4& v);
template <> __device__ __forceinline__ void st4<float>(unsigned char* p, const f32x4& v) {
  *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void st4<bf16>(unsigned char* p, const f32x4& v) {
  *(uint2*)p = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
}

// one 16-byte chunk of a pad token's q / k / v: KPL consecutive f32 of the qkv bias, narrowed to T
template <typename T> __device__ __forceinline__ uint4 bias_chunk(const float* __restrict__ p) {
  float f[TT<T>::KPL];
#pragma unroll
  for (int j = 0; j < TT<T>::KPL; ++j) f[j] = p[j];
  return pack<T>(f);
}

// ---------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------
template <typename T, int HD, int NW>
__global__ __launch_bounds__(NW * 64) void attn_sp_fwd_kernel(const T* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                             const float* __restrict__ bias_t, T* __restrict__ out,
                                                             float* __restrict__ lse, const SpGeo g) {
  using L = Lay<T, HD>;
  constexpr int E = L::E, KPL = L::KPL;
  constexpr int NT = NW * 64;
  __shared__ __attribute__((aligned(16))) unsigned char sQ[NW * L::QTILE];
  __shared__ __attribute__((aligned(16))) unsigned char sK[NW * L::QTILE];
  __shared__ __attribute__((aligned(16))) unsigned char sV[NW * L::QTILE];
  __shared__ __attribute__((aligned(16))) unsigned char sP[NW * L::STILE];
  __shared__ int sTok[64];                       // window slot -> token row, -1: pad
  __shared__ int sRid[64];                       // window slot -> mask region
  __shared__ float sBias[NW][SP_LT + 3];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int HG = g.heads / NW;
  int bid = blockIdx.x;
  const int hg = bid % HG; bid /= HG;
  const int wx = bid % g.nwx; bid /= g.nwx;
  const int wy = bid % g.nwy; const int b = bid / g.nwy;
  const int head = hg * NW + w;
  const int C3 = 3 * g.C;

  if (tid < 64) {
    int row, rid;
    sp_token(g, b, wy, wx, tid, row, rid);
    sTok[tid] = row; sRid[tid] = rid;
  }
  const float* bt = bias_t + (long)head * SP_LT;
  for (int i = lane; i < SP_LT; i += 64) sBias[w][i] = bt[i];
  __syncthreads();
  // ---- Q / K / V tiles: 64 slots x NW*HD; a pad slot reads the bias row
  constexpr int CPR = NW * L::DCH;
  for (int idx = tid; idx < 64 * CPR; idx += NT) {
    const int r = idx / CPR, cc = idx - r * CPR;
    const int h = cc / L::DCH, dc = cc - h * L::DCH;
    const int col = (hg * NW) * HD + cc * KPL;
    const int row = sTok[r];
    uint4 qv, kv, vv;
    if (row >= 0) {
      const T* src = qkv + (long)row * C3 + col;
      qv = *(const uint4*)(src); kv = *(const uint4*)(src + g.C); vv = *(const uint4*)(src + 2 * g.C);
    } else {
      qv = bias_chunk<T>(qkv_bias + col); kv = bias_chunk<T>(qkv_bias + g.C + col); vv = bias_chunk<T>(qkv_bias + 2 * g.C + col);
    }
    const int off = (h * 64 + r) * L::QROW + dc * 16;
    *(uint4*)(sQ + off) = qv; *(uint4*)(sK + off) = kv; *(uint4*)(sV + off) = vv;
  }
  __syncthreads();

  const int fr = lane & 15, fg = lane >> 4;
  const float scale = rsqrtf((float)HD);
  const unsigned char* myQ = sQ + w * L::QTILE;
  const unsigned char* myK = sK + w * L::QTILE;
  const unsigned char* myV = sV + w * L::QTILE;
  unsigned char* myP = sP + w * L::STILE;
  float m_row[4][4], l_row[4][4];

  // ---- S = Q K^T (per 16-row strip), bias, mask, softmax, P -> LDS
  int krid[4];
#pragma unroll
  for (int ns = 0; ns < 4; ++ns) krid[ns] = sRid[ns * 16 + fr];
#pragma unroll
  for (int ms = 0; ms < 4; ++ms) {
    f32x4 s[4];
#pragma unroll
    for (int ns = 0; ns < 4; ++ns) s[ns] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kb = 0; kb < L::KBQ; ++kb) {
      const uint4 fa = frag<T>(myQ, L::QROW, ms * 16, kb, HD, lane);
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        const uint4 fb = frag<T>(myK, L::QROW, ns * 16, kb, HD, lane);
        mma16<T>(s[ns], fa, fb);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qn = ms * 16 + fg * 4 + r;
      const int qiy = qn >> 3, qix = qn & 7, qrid = sRid[qn];
      float mx = -1e30f;
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        const int kn = ns * 16 + fr;
        float v = s[ns][r] * scale + sBias[w][(qiy - (kn >> 3) + SP_WS - 1) * SP_L2 + (qix - (kn & 7) + SP_WS - 1)];
        if (qrid != krid[ns]) v += -100.0f;
        s[ns][r] = v;
        mx = fmaxf(mx, v);
      }
      mx = group16_max(mx);
      float rs = 0.f;
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) { const float p = __expf(s[ns][r] - mx); s[ns][r] = p; rs += p; }
      rs = group16_sum(rs);
      m_row[ms][r] = mx; l_row[ms][r] = rs;
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) st_elem<T>(myP + qn * L::TROW + (ns * 16 + fr) * E, s[ns][r]);
    }
  }
  __syncthreads();
  // ---- O = P V
  f32x4 o[4][HD / 16];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int d = 0; d < HD / 16; ++d) o[i][d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < L::KBT; ++kb) {
    uint4 fb[HD / 16];
#pragma unroll
    for (int d = 0; d < HD / 16; ++d) fb[d] = fragT<T>(myV, L::QROW, kb * TT<T>::MMA_K, d * 16, lane);
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      const uint4 fa = frag<T>(myP, L::TROW, ms * 16, kb, 64, lane);
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) mma16<T>(o[ms][d], fa, fb[d]);
    }
  }
  __syncthreads();

  // ---- normalise, write lse, stage O through this head's Q tile, coalesced store of the real tokens (the crop)
  unsigned char* myO = sQ + w * L::QTILE;
#pragma unroll
  for (int ms = 0; ms < 4; ++ms)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qn = ms * 16 + fg * 4 + r;
      const float inv = 1.0f / l_row[ms][r];
      const int row = sTok[qn];
      if (fr == 0 && lse && row >= 0) lse[(long)row * g.heads + head] = m_row[ms][r] + __logf(l_row[ms][r]);
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) st_elem<T>(myO + qn * L::QROW + (d * 16 + fr) * E, o[ms][d][r] * inv);
    }
  __syncthreads();
  for (int idx = tid; idx < 64 * CPR; idx += NT) {
    const int r = idx / CPR, cc = idx - r * CPR;
    const int h = cc / L::DCH, dc = cc - h * L::DCH;
    const int row = sTok[r];
    if (row >= 0)
      *(uint4*)(out + (long)row * g.C + (hg * NW) * HD + cc * KPL) = *(const uint4*)(sQ + (h * 64 + r) * L::QROW + dc * 16);
  }
}

// ---------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------
template <typename T, int HD, int NW>
__global__ __launch_bounds__(NW * 64) void attn_sp_bwd_kernel(const T* __restrict__ qkv, const float* __restrict__ qkv_bias,
                                                             const float* __restrict__ bias_t, const T* __restrict__ d_out,
                                                             const float* __restrict__ lse, T* __restrict__ dqkv,
                                                             float* __restrict__ dqkv_bias, float* __restrict__ dbias_t,
                                                             const SpGeo g, int nwin) {
  using L = Lay<T, HD>;
  constexpr int E = L::E, KPL = L::KPL;
  constexpr int NT = NW * 64;
  constexpr int MK = TT<T>::MMA_K;
  // only row-major [slot][d] tiles are staged; every "transposed" MFMA operand is read with fragT
  __shared__ __attribute__((aligned(16))) unsigned char sQ[NW * L::QTILE], sK[NW * L::QTILE], sV[NW * L::QTILE],
      sDO[NW * L::QTILE];
  __shared__ __attribute__((aligned(16))) unsigned char sPT[NW * L::STILE], sDST[NW * L::STILE];   // [key][q]
  __shared__ float sDB[NW][SP_LT + 3];
  __shared__ float sBias[NW][SP_LT + 3];          // x log2 e
  __shared__ float sLse[NW][64];                  // x log2 e; a pad query: +1e30, so that its recomputed P is exactly 0
  __shared__ int sTok[64];
  __shared__ int sRid[64];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int fr = lane & 15, fg = lane >> 4;
  const int hg = blockIdx.y;
  const int head = hg * NW + w;
  const int C3 = 3 * g.C;
  const float scale = rsqrtf((float)HD);
  const float scale2 = scale * SP_LOG2E;
  constexpr int CPR = NW * L::DCH;

  for (int i = tid; i < NW * (SP_LT + 3); i += NT) (&sDB[0][0])[i] = 0.f;
  {
    const float* bt = bias_t + (long)head * SP_LT;
    for (int i = lane; i < SP_LT; i += 64) sBias[w][i] = bt[i] * SP_LOG2E;
  }

  unsigned char* myQ = sQ + w * L::QTILE; unsigned char* myK = sK + w * L::QTILE;
  unsigned char* myV = sV + w * L::QTILE; unsigned char* myDO = sDO + w * L::QTILE;
  unsigned char* myPT = sPT + w * L::STILE; unsigned char* myDST = sDST + w * L::STILE;

  // relative-position-bias gradient: dS summed in registers over every window this wave visits (the (q, key) -> table-entry
  // map is the same for all of them; a pad query's dS is exactly 0, a pad KEY's dS counts: the reference adds the table to it too)
  f32x4 dbacc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) dbacc[a][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  // k / v gradient of the pad keys, summed over this lane's accumulator rows (slots 16 ks + 4 fg + r) and over the windows
  float padk[HD / 16], padv[HD / 16];
#pragma unroll
  for (int d = 0; d < HD / 16; ++d) { padk[d] = 0.f; padv[d] = 0.f; }

  for (int item = blockIdx.x; item < nwin; item += gridDim.x) {
    int t = item;
    const int wx = t % g.nwx; t /= g.nwx;
    const int wy = t % g.nwy; const int b = t / g.nwy;

    __syncthreads();       // the previous window's tiles and slot map are no longer read
    if (tid < 64) {
      int row, rid;
      sp_token(g, b, wy, wx, tid, row, rid);
      sTok[tid] = row; sRid[tid] = rid;
    }
    __syncthreads();
    {
      const int row = sTok[lane];
      sLse[w][lane] = row >= 0 ? lse[(long)row * g.heads + head] * SP_LOG2E : 1e30f;
    }
    for (int idx = tid; idx < 64 * CPR; idx += NT) {
      const int r = idx / CPR, cc = idx - r * CPR;
      const int h = cc / L::DCH, dc = cc - h * L::DCH;
      const int col = (hg * NW) * HD + cc * KPL;
      const int row = sTok[r];
      uint4 qv, kv, vv, dv_ = make_uint4(0, 0, 0, 0);
      if (row >= 0) {
        const T* src = qkv + (long)row * C3 + col;
        qv = *(const uint4*)(src); kv = *(const uint4*)(src + g.C); vv = *(const uint4*)(src + 2 * g.C);
        dv_ = *(const uint4*)(d_out + (long)row * g.C + col);
      } else {
        qv = bias_chunk<T>(qkv_bias + col); kv = bias_chunk<T>(qkv_bias + g.C + col); vv = bias_chunk<T>(qkv_bias + 2 * g.C + col);
      }
      const int off = (h * 64 + r) * L::QROW + dc * 16;
      *(uint4*)(sQ + off) = qv; *(uint4*)(sK + off) = kv; *(uint4*)(sV + off) = vv; *(uint4*)(sDO + off) = dv_;
    }
    __syncthreads();

    // ---- phase A: per 16-query strip  S, dP -> P, dS ; P^T and dS^T to LDS (packed 4-q stores)
    int krid[4];
#pragma unroll
    for (int ns = 0; ns < 4; ++ns) krid[ns] = sRid[ns * 16 + fr];
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      f32x4 s[4], dp[4];
#pragma unroll
      for (int kb = 0; kb < L::KBQ; ++kb) {
        const uint4 fq = frag<T>(myQ, L::QROW, ms * 16, kb, HD, lane);
        const uint4 fo = frag<T>(myDO, L::QROW, ms * 16, kb, HD, lane);
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
          const uint4 fk = frag<T>(myK, L::QROW, ns * 16, kb, HD, lane);
          const uint4 fv = frag<T>(myV, L::QROW, ns * 16, kb, HD, lane);
          if (kb == 0) { s[ns] = mma16z<T>(fq, fk); dp[ns] = mma16z<T>(fo, fv); }
          else { mma16<T>(s[ns], fq, fk); mma16<T>(dp[ns], fo, fv); }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qn = ms * 16 + fg * 4 + r;
        const float lq = sLse[w][qn];
        const int qiy = qn >> 3, qix = qn & 7, qrid = sRid[qn];
        float dl = 0.f;
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
          const int kn = ns * 16 + fr;
          float v = fmaf(s[ns][r], scale2, sBias[w][(qiy - (kn >> 3) + SP_WS - 1) * SP_L2 + (qix - (kn & 7) + SP_WS - 1)]);
          if (qrid != krid[ns]) v += -100.0f * SP_LOG2E;
          const float p = __builtin_amdgcn_exp2f(v - lq);
          s[ns][r] = p;
          dl = fmaf(p, dp[ns][r], dl);
        }
        dl = group16_sum(dl);
#pragma unroll
        for (int ns = 0; ns < 4; ++ns) {
          const float ds = s[ns][r] * (dp[ns][r] - dl);
          dp[ns][r] = ds;
          dbacc[ms][ns][r] += ds;
        }
      }
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        st4<T>(myPT + (ns * 16 + fr) * L::TROW + (ms * 16 + fg * 4) * E, s[ns]);
        st4<T>(myDST + (ns * 16 + fr) * L::TROW + (ms * 16 + fg * 4) * E, dp[ns]);
      }
    }
    __syncthreads();

    // ---- phase B: dV = P^T dO ; dK = dS^T Q ; dQ = dS K   (contraction over LDS rows -> fragT)
    f32x4 dk[4][HD / 16], dv[4][HD / 16], dq[4][HD / 16];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) {
        dk[i][d] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[i][d] = f32x4{0.f, 0.f, 0.f, 0.f}; dq[i][d] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
    for (int kb = 0; kb < L::KBT; ++kb) {
      uint4 fdo[HD / 16], fqq[HD / 16], fkk[HD / 16];
#pragma unroll
      for (int d = 0; d < HD / 16; ++d) {
        fdo[d] = fragT<T>(myDO, L::QROW, kb * MK, d * 16, lane);
        fqq[d] = fragT<T>(myQ, L::QROW, kb * MK, d * 16, lane);
        fkk[d] = fragT<T>(myK, L::QROW, kb * MK, d * 16, lane);
      }
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        const uint4 fp = frag<T>(myPT, L::TROW, ks * 16, kb, 64, lane);
        const uint4 fs = frag<T>(myDST, L::TROW, ks * 16, kb, 64, lane);
        const uint4 fst = fragT<T>(myDST, L::TROW, kb * MK, ks * 16, lane);    // dS[q = ks strip][key block kb]
#pragma unroll
        for (int d = 0; d < HD / 16; ++d) {
          mma16<T>(dv[ks][d], fp, fdo[d]);
          mma16<T>(dk[ks][d], fs, fqq[d]);
          mma16<T>(dq[ks][d], fst, fkk[d]);
        }
      }
    }
    // the pad keys' gradient stays in registers (f32): it belongs to qkv.bias, not to a token
    if (wy == g.nwy - 1 || wx == g.nwx - 1) {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (sTok[ks * 16 + fg * 4 + r] < 0) {
#pragma unroll
            for (int d = 0; d < HD / 16; ++d) { padk[d] += dk[ks][d][r] * scale; padv[d] += dv[ks][d][r]; }
          }
    }
    __syncthreads();   // every wave is done reading sQ / sK / sV / sDO / sPT / sDST of this window
    // ---- dQ, dK, dV staged through sQ / sK / sV -> dqkv rows of the real tokens
#pragma unroll
    for (int ms = 0; ms < 4; ++ms)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int d = 0; d < HD / 16; ++d) {
          const int off = (ms * 16 + fg * 4 + r) * L::QROW + (d * 16 + fr) * E;
          st_elem<T>(myQ + off, dq[ms][d][r] * scale);
          st_elem<T>(myK + off, dk[ms][d][r] * scale);
          st_elem<T>(myV + off, dv[ms][d][r]);
        }
    __syncthreads();
    for (int idx = tid; idx < 64 * CPR; idx += NT) {
      const int r = idx / CPR, cc = idx - r * CPR;
      const int h = cc / L::DCH, dc = cc - h * L::DCH;
      const int row = sTok[r];
      if (row >= 0) {
        T* dst = dqkv + (long)row * C3 + (hg * NW) * HD + cc * KPL;
        const int off = (h * 64 + r) * L::QROW + dc * 16;
        *(uint4*)(dst) = *(const uint4*)(sQ + off);
        *(uint4*)(dst + g.C) = *(const uint4*)(sK + off);
        *(uint4*)(dst + 2 * g.C) = *(const uint4*)(sV + off);
      }
    }
  }

  // ---- pad keys: reduce over the four lane groups of the wave, then one atomic per channel (the q third is never touched)
#pragma unroll
  for (int d = 0; d < HD / 16; ++d) {
    float a = padk[d], c = padv[d];
    a += __shfl_xor(a, 16); a += __shfl_xor(a, 32);
    c += __shfl_xor(c, 16); c += __shfl_xor(c, 32);
    if (fg == 0) {
      if (a != 0.f) atomicAdd(dqkv_bias + g.C + head * HD + d * 16 + fr, a);
      if (c != 0.f) atomicAdd(dqkv_bias + 2 * g.C + head * HD + d * 16 + fr, c);
    }
  }
  // ---- bias-table gradient: registers -> LDS table -> global atomics, once for all the windows this wave handled
  __syncthreads();
#pragma unroll
  for (int ms = 0; ms < 4; ++ms)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qn = ms * 16 + fg * 4 + r;
      const int qiy = qn >> 3, qix = qn & 7;
#pragma unroll
      for (int ns = 0; ns < 4; ++ns) {
        const int kn = ns * 16 + fr;
        atomicAdd(&sDB[w][(qiy - (kn >> 3) + SP_WS - 1) * SP_L2 + (qix - (kn & 7) + SP_WS - 1)], dbacc[ms][ns][r]);
      }
    }
  __syncthreads();
  for (int i = lane; i < SP_LT; i += 64) {
    const float v = sDB[w][i];
    if (v != 0.f) atomicAdd(dbias_t + (long)head * SP_LT + i, v);
  }
}

template <typename T> constexpr int DTYPE = std::is_same<T, bf16>::value ? SODT_BF16 : SODT_F32;

template <typename T, int HD>
int launch_sp_fwd(const void* qkv, const float* qkv_bias, const float* bias_t, void* out, float* lse, const SpGeo& g, hipStream_t st) {
  constexpr int NW = attn_nw(DTYPE<T>, HD, false);
  const long nwg = (long)g.B * g.nwy * g.nwx * (g.heads / NW);
  return sodt_launch<attn_sp_fwd_kernel<T, HD, NW>>(dim3((unsigned)nwg), dim3(NW * 64), 0, st, (const T*)qkv, qkv_bias, bias_t,
                                                    (T*)out, lse, g);
}

template <typename T, int HD>
int launch_sp_bwd(const void* qkv, const float* qkv_bias, const float* bias_t, const void* dout, const float* lse, void* dqkv,
                  float* dqkv_bias, float* dbias_t, const SpGeo& g, hipStream_t st) {
  constexpr int NW = attn_nw(DTYPE<T>, HD, true);
  const int nwin = g.B * g.nwy * g.nwx;
  return sodt_launch<attn_sp_bwd_kernel<T, HD, NW>>(dim3(attn_sp_bwd_grid(nwin, g.heads / NW), g.heads / NW), dim3(NW * 64), 0, st,
                                                    (const T*)qkv, qkv_bias, bias_t, (const T*)dout, lse, (T*)dqkv, dqkv_bias,
                                                    dbias_t, g, nwin);
}

}  // namespace

extern "C" int sodt_window_attn_sp_fwd(const void* qkv, const float* qkv_bias, const float* bias_t, void* out, float* lse,
                                       int B, int H, int W, int C, int heads, int ws, int shift, int dtype, sodt_stream_t st_) {
  SpGeo g;
  if (!qkv || !qkv_bias || !bias_t || !out || !make_sp_geo(g, B, H, W, C, heads, ws, shift)) return SODT_EINVAL;
  const int hd = C / heads;
  if (!attn_sp_fwd_route(dtype, hd, g)) return SODT_EINVAL;
  hipStream_t st = (hipStream_t)st_;
  if (dtype == SODT_BF16)
    return hd == 16 ? launch_sp_fwd<bf16, 16>(qkv, qkv_bias, bias_t, out, lse, g, st)
                    : launch_sp_fwd<bf16, 32>(qkv, qkv_bias, bias_t, out, lse, g, st);
  return hd == 16 ? launch_sp_fwd<float, 16>(qkv, qkv_bias, bias_t, out, lse, g, st)
                  : launch_sp_fwd<float, 32>(qkv, qkv_bias, bias_t, out, lse, g, st);
}

extern "C" int sodt_window_attn_sp_bwd(const void* qkv, const float* qkv_bias, const float* bias_t, const void* out,
                                       const void* dout, const float* lse, void* dqkv, float* dqkv_bias, float* dbias_t,
                                       int B, int H, int W, int C, int heads, int ws, int shift, int dtype, sodt_stream_t st_) {
  SpGeo g;
  (void)out;     // single-tile windows: delta = rowsum(dO o O) is formed from the recomputed P
  if (!qkv || !qkv_bias || !bias_t || !dout || !lse || !dqkv || !dqkv_bias || !dbias_t ||
      !make_sp_geo(g, B, H, W, C, heads, ws, shift)) return SODT_EINVAL;
  const int hd = C / heads;
  if (!attn_sp_bwd_route(dtype, hd, g)) return SODT_EINVAL;
  hipStream_t st = (hipStream_t)st_;
  if (dtype == SODT_BF16)
    return hd == 16 ? launch_sp_bwd<bf16, 16>(qkv, qkv_bias, bias_t, dout, lse, dqkv, dqkv_bias, dbias_t, g, st)
                    : launch_sp_bwd<bf16, 32>(qkv, qkv_bias, bias_t, dout, lse, dqkv, dqkv_bias, dbias_t, g, st);
  return hd == 16 ? launch_sp_bwd<float, 16>(qkv, qkv_bias, bias_t, dout, lse, dqkv, dqkv_bias, dbias_t, g, st)
                  : launch_sp_bwd<float, 32>(qkv, qkv_bias, bias_t, dout, lse, dqkv, dqkv_bias, dbias_t, g, st);
}
