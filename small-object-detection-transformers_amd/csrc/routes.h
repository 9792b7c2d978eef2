// Which kernel runs: one pure function per routed entry point (sodt_gemm_nt, sodt_gemm_tn, the window-attention entries).
// Plain C++17 and nothing from HIP, so tests/host/attn_routes_main.cpp compiles it alone.  The launchers (gemm.hip, gemm3.hip,
// attention.hip) validate, ask here, and switch over the answer; geometry a decision needs (tile sizes, persistent grids)
// lives here with it.
#pragma once
#include "../../include/sodt_hip.h"

// ================================================================================= GEMM
// pipelined bf16 kernels (gemm3.hip): CU tile and the limits its LDS layout sets
constexpr int T3_BM = 256, T3_BN = 192, T3_BK = 64;
constexpr int T3_MAXKLEN = (8192 - 256) / 2;        // elements of one K-segment (the zero page a dead row's DMA walks is 8 KiB)
constexpr int T3_MAXBIAS = 3072;                    // f32 bias[N] kept in LDS

// eligibility of the pipelined NT kernel (bf16 only); the caller has validated pointers / alignment
inline bool nt3_eligible(const sodt_gemm_args& g) {
  switch (g.flags) {
    case 0: case SODT_EPI_BIAS: case SODT_EPI_RESID: case SODT_EPI_BIAS | SODT_EPI_RESID:
    case SODT_EPI_BIAS | SODT_EPI_GELU_DUAL: case SODT_EPI_DGELU: case SODT_EPI_BIAS | SODT_EPI_GELU: break;
    case SODT_EPI_RELU: case SODT_EPI_BIAS | SODT_EPI_RELU: case SODT_EPI_DRELU: break;      // the SR branch's convolutions (sr.py)
    case SODT_EPI_STATS:                           // the head's BatchNorm convolutions, thin outputs only (one column tile, NV = 2)
      if (g.N > 64 || !g.stats || g.oscatter) return false;
      break;
    case SODT_EPI_BIAS | SODT_EPI_DGELU_RC:
      if (g.K % (2 * T3_BK)) return false;         // both halves whole K-steps
      break;
    default: return false;
  }
  if (g.rmod > 0 || (g.oscatter && (g.flags != 0 || !g.a.spatial))) return false;
  // N: whole 192-column tiles, or (K >= 512) any multiple of 8 with the last tile partial - a narrow output (the 64-channel 3x3
  // convolutions of the SR branch, the 256-wide ones of its tail) is priced by the A stream, which this kernel moves by LDS-DMA
  // three stages ahead; the idle accumulator columns cost matrix cycles that are not the bound there
  const int kmin_partial = g.flags == SODT_EPI_STATS ? 192 : 512;     // (statistics: the alternative is the 128 x 128 K-loop kernel)
  if (g.N % 8 || (g.N % T3_BN && (g.K < kmin_partial || g.K > T3_MAXKLEN)) || g.K % T3_BK || g.K < 192 || g.M < T3_BM) return false;
  if ((g.flags & SODT_EPI_RESID) && (g.ldr % 8)) return false;
  if ((g.flags & (SODT_EPI_DGELU | SODT_EPI_DRELU)) && (g.ldaux % 8)) return false;
  if ((g.flags & SODT_EPI_BIAS) && g.N > T3_MAXBIAS) return false;
  if ((g.ldw % 8) || (g.ldc % 8)) return false;
  for (int i = 0; i < g.a.nseg; ++i)
    if (g.a.s[i].klen % T3_BK || g.a.s[i].klen > T3_MAXKLEN) return false;
  return true;
}

enum NtKind {
  NT_REFUSED,      // SODT_EPI_DGELU_RC where the pipelined kernel, the only one that has it, is not eligible
  NT_PIPE,         // gemm_nt3_kernel<cf, scatter, thin ? 2 : 3>
  NT_BS_STATS,     // gemm_bs_kernel<T, 128, true, -1, false>
  NT_BS_SIMPLE,    // gemm_bs_kernel<T, 128, false, cf, true>
  NT_BS_GENERIC,   // gemm_bs_kernel<T, 128, false, -1, false>
  NT_AS128,        // gemm_as_kernel<T, 128>
  NT_AS64,         // gemm_as_kernel<T, 64>
  NT_TILED         // gemm_nt_kernel<T, cf>
};
struct NtRoute {
  NtKind kind;
  int cf;          // the epilogue set the kernel is compiled for (-1: it reads g.flags at run time)
  bool thin;       // NT_PIPE: two accumulator column groups (N <= 64)
  bool scatter;    // NT_PIPE: output-row scatter
};

// the flag sets that have a branch-free instantiation of the tiled and the simple B-stationary kernel
inline int nt_static_cf(int flags) {
  switch (flags) {
    case 0: case SODT_EPI_BIAS: case SODT_EPI_RESID: case SODT_EPI_BIAS | SODT_EPI_RESID:
    case SODT_EPI_BIAS | SODT_EPI_GELU_DUAL: case SODT_EPI_DGELU: return flags;
    default: return -1;
  }
}

// g has passed sodt_gemm_nt's validation; dtype is SODT_BF16 or SODT_F32
inline NtRoute nt_route(const sodt_gemm_args& g, int dtype, int variant) {
  const bool bf = dtype == SODT_BF16;
  const bool pipe_ok = bf && nt3_eligible(g);
  if ((g.flags & SODT_EPI_DGELU_RC) && !pipe_ok) return {NT_REFUSED, -1, false, false};
  if (pipe_ok && (variant == SODT_VARIANT_AUTO || variant == SODT_VARIANT_NO_TN3)) {
    bool thin = g.N <= 64 && !g.oscatter;   // (the 64-channel 3x3 convolutions of the SR branch and the head)
    switch (g.flags) {
      case 0: case SODT_EPI_BIAS: case SODT_EPI_BIAS | SODT_EPI_RESID: case SODT_EPI_RESID: case SODT_EPI_BIAS | SODT_EPI_RELU:
      case SODT_EPI_DRELU: case SODT_EPI_STATS: break;
      default: thin = false;
    }
    return {NT_PIPE, g.flags, thin, g.oscatter != 0};
  }
  // short contraction -> a stationary kernel (row bytes a multiple of 128 so the XOR swizzle stays in-row)
  const int kpl = bf ? 8 : 4, KB = g.K * (bf ? 2 : 4);
  if (!(g.flags & SODT_EPI_DETECT) && (KB % 128) == 0 && KB <= 384 && variant != SODT_VARIANT_TILED) {
    // (the B-stationary kernel adds the residual before the generic epilogue: a ReLU / ReLU mask must come first, so not with both)
    const bool relu_resid = (g.flags & (SODT_EPI_RELU | SODT_EPI_DRELU)) && (g.flags & SODT_EPI_RESID);
    if ((g.N % kpl) == 0 && !(g.flags & SODT_EPI_OUT_F32) && variant != SODT_VARIANT_ASTAT && !relu_resid) {
      if (g.flags & SODT_EPI_STATS) return {NT_BS_STATS, -1, false, false};
      const int cf = g.a.nseg == 1 && !g.a.spatial && !g.oscatter ? nt_static_cf(g.flags) : -1;
      return {cf >= 0 ? NT_BS_SIMPLE : NT_BS_GENERIC, cf, false, false};
    }
    return {NT_AS128, -1, false, false};     // (NT_AS64 was the arm for KB > 384, which the test above excludes)
  }
  return {NT_TILED, g.oscatter ? -1 : nt_static_cf(g.flags), false, false};
}

// pipelined TN: K on the 256-wide side when that pads less (ties keep N there); mirrored by ops.tn_splits
inline bool tn3_swap(int N, int K) {
  const long a = (long)((N + 255) / 256) * 256 * ((K + 191) / 192) * 192;
  const long b = (long)((K + 255) / 256) * 256 * ((N + 191) / 192) * 192;
  return b < a;
}

enum TnKind {
  TN_PIPE,         // gemm_tn3_kernel<swap, spatial>
  TN_256x192,      // gemm_tn2_kernel<T>
  TN_TILED         // gemm_tn_kernel<T>
};
struct TnRoute {
  TnKind kind;
  bool swap, spatial;   // TN_PIPE
};

inline TnRoute tn_route(const sodt_gemm_tn_args& g, int dtype, int variant) {
  if (dtype == SODT_BF16 && variant == SODT_VARIANT_AUTO && (g.N % 8) == 0 && (g.K % 8) == 0 && g.M >= 1024)
    return {TN_PIPE, tn3_swap(g.N, g.K), g.x.spatial != 0};
  if (variant != SODT_VARIANT_TILED && (g.N <= 192 || g.K <= 192))   // short side <= 192: the tile reads each operand (almost) once
    return {TN_256x192, false, false};
  return {TN_TILED, false, false};
}

// ================================================================================= window attention
namespace {   // unnamed: AttnGeo is a kernel parameter, so its namespace is part of every attention kernel's symbol name
struct AttnGeo {
  int B, H, W, C, heads, ws, shift;
  int nwy, nwx, N, nqt;   // windows per column/row, tokens per window, 64-token tiles per window
};
}  // namespace

inline bool make_geo(AttnGeo& g, int B, int H, int W, int C, int heads, int ws, int shift) {
  if (B <= 0 || H <= 0 || W <= 0 || ws <= 0 || (H % ws) || (W % ws) || heads <= 0 || (C % heads)) return false;
  if ((ws * ws) % 64) return false;
  if (ws < 8 || (64 % ws && ws < 64) ) return false;           // a 64-token tile must cover whole window rows
  if (ws > 64) return false;
  if (shift < 0 || shift >= ws) return false;
  g.B = B; g.H = H; g.W = W; g.C = C; g.heads = heads; g.ws = ws; g.shift = shift;
  g.nwy = H / ws; g.nwx = W / ws; g.N = ws * ws; g.nqt = g.N / 64;
  return true;
}

// waves (= heads) per workgroup of the (dtype, head dim) instantiation; 0: not built
constexpr int attn_nw(int dtype, int hd, bool bwd) {
  const int i = hd == 16 ? 0 : hd == 32 ? 1 : hd == 64 ? 2 : -1;
  if (i < 0 || (dtype != SODT_BF16 && dtype != SODT_F32)) return 0;
  constexpr int tab[2][2][3] = {{{4, 2, 2}, {2, 2, 1}},      // f32: forward, backward
                                {{4, 4, 2}, {4, 2, 1}}};     // bf16
  return tab[dtype == SODT_BF16][bwd][i];
}
constexpr int attn_dch(int dtype, int hd) { return hd / (dtype == SODT_BF16 ? 8 : 4); }    // 16-byte chunks per head row
constexpr int attn_mma_k(int dtype) { return dtype == SODT_BF16 ? 32 : 16; }               // contraction depth of one mma16()
// the multi-tile forward kernel (mt) is built where DCH is 4..16; the two-pass kernels (mt2 forward, dkv + dq backward) need
// whole mma steps over the head dim as well
constexpr bool attn_mt1_built(int dtype, int hd) { return attn_dch(dtype, hd) >= 4 && attn_dch(dtype, hd) <= 16; }
constexpr bool attn_mt2_built(int dtype, int hd) { return hd % attn_mma_k(dtype) == 0 && attn_mt1_built(dtype, hd); }

enum AttnFwdKind { AF_FAST, AF_MT2, AF_MT, AF_GENERIC };
enum AttnBwdKind { AB_FAST2, AB_SINGLE, AB_DKV_DQ, AB_MT, AB_GENERIC };
// AB_DKV_DQ and AB_MT follow attn_delta_kernel; AB_MT is followed by attn_dq_finish_kernel
struct AttnRoute {
  int kind;        // AttnFwdKind / AttnBwdKind
  int nw;          // 0: refused (SODT_EINVAL)
};

inline AttnRoute attn_fwd_route(int dtype, int hd, const AttnGeo& g) {
  const int nw = attn_nw(dtype, hd, false);
  if (!nw || g.heads % nw) return {AF_GENERIC, 0};
  if (3 * attn_dch(dtype, hd) <= 12 && g.nqt == 1) return {AF_FAST, nw};
  if (g.nqt > 1 && (g.nqt % 4) == 0) {
    if (attn_mt2_built(dtype, hd) && g.shift == 0 && g.ws <= 32) return {AF_MT2, nw};
    if (attn_mt1_built(dtype, hd)) return {AF_MT, nw};
  }
  return {AF_GENERIC, nw};
}

inline AttnRoute attn_bwd_route(int dtype, int hd, const AttnGeo& g) {
  const int nw = attn_nw(dtype, hd, true);
  if (!nw || g.heads % nw) return {AB_GENERIC, 0};
  const bool pfok = 4 * attn_dch(dtype, hd) <= 16;         // q / k / v / dO fragments stay in registers
  if (pfok && g.nqt == 1) return {g.ws == 8 ? AB_FAST2 : AB_SINGLE, nw};
  if (g.nqt == 1) return {AB_GENERIC, nw};
  if (attn_mt2_built(dtype, hd) && g.shift == 0 && g.ws <= 32 && (g.nqt % 4) == 0 && (g.N % 128) == 0)
    return {AB_DKV_DQ, nw};                                 // two passes, no dQ atomics
  return {AB_MT, nw};
}

// the window-major backward (operands as the fused forward saves them): head dim 16, 8x8 windows
inline AttnRoute attn_bwd_wm_route(int dtype, int hd, const AttnGeo& g) {
  const int nw = hd == 16 ? attn_nw(dtype, hd, true) : 0;
  if (!nw || g.heads % nw || g.nqt != 1 || g.ws != 8) return {AB_FAST2, 0};
  return {AB_FAST2, nw};
}
// the same with q / k / v recomputed (bf16, C = 192, 12 heads)
inline AttnRoute attn_bwd_rc_route(int dtype, const AttnGeo& g) {
  if (dtype != SODT_BF16 || g.heads != 12 || g.C != 192 || g.nqt != 1 || g.ws != 8) return {AB_FAST2, 0};
  return {AB_FAST2, 4};
}

// ---- persistent grids
inline int attn_fwd_fast_grid(int nwin) { return nwin < 512 ? nwin : 512; }
// Grid of the persistent single-tile backward kernels: every workgroup ends with one flush of its bias-gradient table
// (225 global atomics per wave onto the 2,700 floats of the 12 heads).  With 1024 x (heads / NW) workgroups that was
// 2.7 M same-line device-scope atomics per launch - 0.2 ms, 40 % of the stage-1 launch (the loops themselves ran six
// rounds of 0.05 ms).  Launch only as many workgroups as are resident at once and let them walk more windows.
inline int bwd_persistent_grid(int nwin, int ngroups, int NW) {
  const int resident = 256 * (NW == 4 ? 2 : (NW == 2 ? 2 : 4));     // CUs x workgroups per CU (launch bounds / LDS)
  int gx = resident / (ngroups > 0 ? ngroups : 1);
  if (gx < 1) gx = 1;
  return nwin < gx ? nwin : gx;
}
// walkers in whole rounds of the 8 XCDs (see the kernel's id map); walkers beyond the window count only join the final
// (all-zero) bias-gradient flush
inline int attn_rc_grid(int nwin) {
  const int gx = bwd_persistent_grid(nwin, 12 / 4, 4);
  return gx >= 8 ? gx / 8 * 8 : 8;
}

// ================================================================================= shifted window attention on a zero-padded grid
// (attention_sp.hip: sodt_window_attn_sp_fwd / _bwd).  8x8 windows over the padded grid Hp x Wp of an H x W token grid that is
// no multiple of 8; the padded grid exists as index arithmetic only.
namespace {   // unnamed for the reason AttnGeo is
struct SpGeo {
  int B, H, W, C, heads, shift;
  int nwy, nwx;           // windows per column / row of the PADDED grid
};
}  // namespace

inline bool make_sp_geo(SpGeo& g, int B, int H, int W, int C, int heads, int ws, int shift) {
  if (B <= 0 || heads <= 0 || C <= 0 || (C % heads)) return false;
  if (ws != 8 || shift <= 0 || shift >= ws || H <= ws || W <= ws) return false;
  if ((H % ws) == 0 && (W % ws) == 0) return false;            // an unpadded grid is sodt_window_attn_fwd's
  g.B = B; g.H = H; g.W = W; g.C = C; g.heads = heads; g.shift = shift;
  g.nwy = (H + ws - 1) / ws; g.nwx = (W + ws - 1) / ws;
  return (long)B * g.nwy * g.nwx * 64 * heads < (1L << 31);    // token rows and the forward's grid (windows x head groups) are int
}

// one wave per (window, head), nw heads per workgroup; head dim 16 or 32 only.  nw == 0: refused (SODT_EINVAL)
inline int attn_sp_fwd_route(int dtype, int hd, const SpGeo& g) {
  const int nw = (hd == 16 || hd == 32) ? attn_nw(dtype, hd, false) : 0;
  return (nw && g.heads % nw == 0) ? nw : 0;
}
inline int attn_sp_bwd_route(int dtype, int hd, const SpGeo& g) {
  const int nw = (hd == 16 || hd == 32) ? attn_nw(dtype, hd, true) : 0;
  return (nw && g.heads % nw == 0) ? nw : 0;
}
// persistent grid of the backward: the workgroups resident at once (its LDS footprint allows one per CU)
inline int attn_sp_bwd_grid(int nwin, int ngroups) {
  int gx = 256 / (ngroups > 0 ? ngroups : 1);
  if (gx < 1) gx = 1;
  return nwin < gx ? nwin : gx;
}
