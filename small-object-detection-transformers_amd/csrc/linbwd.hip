// Backward of a square 192 -> 192 linear layer in ONE pass over dY (bf16):
//     dX[M][192]   = epi( dY[M][192] @ W )           W given as wT[k][n] = W[n][k], the [N][K] operand sodt_gemm_nt takes
//     dW[192][192] += dY^T @ X[M][192]               (f32)
//     dbias[192]   += column sums of dY              (f32, optional)
// The two launches this replaces (sodt_gemm_tn + sodt_gemm_nt at N = K = 192) each stream dY from HBM; here a 32-row stage of
// dY lands in LDS once and feeds both products.
//
// Structure (gfx950, one workgroup of 8 waves per M-slice, as gemm_tn3_kernel of gemm3.hip):
//   * wT (72 KiB) is loaded once into LDS, XOR-swizzled on the 16-byte chunk for ds_read_b128 (gemm_nt3_kernel's W image).
//   * dY and X rows arrive by LDS-DMA in 32-row stages (12 KiB + 12 KiB), three stages deep, two in flight; one raw barrier per
//     stage behind a counted vmcnt.  Both images are row-major [m][192], XOR-swizzled on the 32-byte unit (gemm_tn3_kernel's Q image).
//   * Per stage the wave grid 4(n) x 2(k) adds dY^T X into 3 x 6 accumulator tiles held across the whole slice (both operands through
//     ds_read_b64_tr_b16; dbias is one extra MFMA per tile row against a vector of ones), and waves 0-5 compute the 32 x 192 block
//     of dX: wave t owns output columns 32 t .. 32 t + 31 with the operands swapped and the W rows permuted inside the group, so a
//     lane ends with 8 consecutive columns of one row and stores 16 bytes straight from its registers (K ascending in 32-element
//     steps, the order of gemm_nt3_kernel).
//   * SODT_EPI_DGELU: the aux rows of stage s + 1 are fetched with inline-asm loads during stage s, queued BEHIND that stage's dX
//     stores and AHEAD of the DMA of stage s + 2, so every wait stays a counted one: the store count of a ragged stage varies, the
//     loads behind it do not.
//   * Each slice's partial dW tile (and dbias row) goes to the caller's scratch with plain stores; linbwd_reduce_kernel adds the
//     live slices in a fixed order (run-to-run deterministic).  Without a scratch that fits: f32 atomics.
// Cost: 144 + 144 MFMAs per stage and CU against 36 KiB of HBM traffic - memory-priced.
#include "gemm_epi.h"
#include "launch.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int LB_C = 192;
constexpr int LB_ROWB = LB_C * 2;                    // 384 bytes per LDS row
constexpr int LB_WBYTES = LB_C * LB_ROWB;            // 72 KiB: the resident wT image
constexpr int LB_ROWS = 32, LB_NST = 3;
constexpr int LB_IMG = LB_ROWS * LB_ROWB;            // 12 KiB per operand and stage
constexpr int LB_STAGE = 2 * LB_IMG;                 // dY image, then X image
constexpr int LB_LDS = LB_WBYTES + LB_NST * LB_STAGE;   // 144 KiB

__device__ uint4 lb_zero16[4];                       // DMA source of rows beyond the slice

__device__ __forceinline__ uint32_t lb_lds_addr(const void* p) { return (uint32_t)(uintptr_t)(lds_void*)p; }

template <int OFF> __device__ __forceinline__ u32x4 lb_rd128(uint32_t addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int OFF> __device__ __forceinline__ uint2 lb_rd_tr(uint32_t addr) {
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  u32x2 t;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t) : "v"(addr), "n"(OFF));
  uint2 v; v.x = t.x; v.y = t.y;
  return v;
}
// rows r .. r+3 and r+4 .. r+7 of one 16-column unit: the 8 contraction elements of a lane
__device__ __forceinline__ u32x4 lb_frag_tr(uint32_t addr) {
  const uint2 lo = lb_rd_tr<0>(addr), hi = lb_rd_tr<4 * LB_ROWB>(addr);
  u32x4 r; r.x = lo.x; r.y = lo.y; r.z = hi.x; r.w = hi.y;
  return r;
}
#define LB_LGKM0() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

__device__ __forceinline__ void lb_mma(f32x4& acc, const u32x4& a, const u32x4& b) {
  union { u32x4 u; bf16x8 v; } ua, ub;
  ua.u = a; ub.u = b;
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.v, ub.v, acc, 0, 0, 0);
}

template <bool DG>
__global__ __launch_bounds__(512) void linbwd_sq_kernel(const sodt_linbwd_args g, float* __restrict__ partial, float* __restrict__ bpartial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lbase = lb_lds_addr(dsm);

  const int split = xcd_remap(blockIdx.x, gridDim.x);
  const long rows_per = (((g.M + g.splits - 1) / g.splits) + LB_ROWS - 1) / LB_ROWS * LB_ROWS;
  const long mbeg = (long)split * rows_per;
  const long mend = (mbeg + rows_per < g.M) ? (mbeg + rows_per) : g.M;
  if (mbeg >= mend) return;                   // dead slice: no partial tile (the reduction reads the live ones only)
  const int nrows = (int)(mend - mbeg);
  const int nsteps = (nrows + LB_ROWS - 1) / LB_ROWS;

  // ---- resident wT image: row r (output column of dX), 16-byte chunk c at r * 384 + ((c ^ f(r)) << 4)
  //      (4,608 chunks = 9 per thread, all nine loads in flight before the first LDS write)
  {
    uint4 wv[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int id = tid + 512 * e, r = id / 24, c = id - r * 24;
      wv[e] = *(const uint4*)((const bf16*)g.wT + (long)r * g.ldw + 8 * c);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int id = tid + 512 * e, r = id / 24, c = id - r * 24;
      const int f = ((r >> 1) & 1) | (((r >> 3) & 3) << 1);
      *(uint4*)(dsm + r * LB_ROWB + ((c ^ f) << 4)) = wv[e];
    }
  }
  __syncthreads();                            // (no DMA in flight yet: a plain barrier)

  // ---- DMA descriptors: an image is 768 chunks = 12 wave-instructions; waves 0-3 bring dY, waves 4-7 X, three instructions each.
  //      chunk id = 64 j + lane -> row id / 24, chunk id % 24; the source column carries the swizzle.  Named scalars only (arrays
  //      indexed through a lambda end up in scratch, whose reloads drain the DMA queue).
  const unsigned char* zero = (const unsigned char*)lb_zero16;
  const bool ximg = wid >= 4;
  const int jb = 3 * (wid & 3);
  const long ld_src = ximg ? g.ldx : g.ldy;
  const unsigned char* src0 = (const unsigned char*)(ximg ? g.X : g.dY);
  auto chunk_row = [&](int e) { return (64 * (jb + e) + lane) / 24; };
  auto chunk_col = [&](int e) {
    const int id = 64 * (jb + e) + lane;
    const int r2 = id / 24, c2 = id - r2 * 24;
    const int sw2 = ((r2 >> 1) & 1) | (((r2 >> 3) & 1) << 1);
    return ((((c2 >> 1) ^ sw2) << 1) | (c2 & 1)) << 3;
  };
  const int drow0 = chunk_row(0), drow1 = chunk_row(1), drow2 = chunk_row(2);
  const unsigned char* cur0 = src0 + (((mbeg + drow0) * ld_src + chunk_col(0)) << 1);
  const unsigned char* cur1 = src0 + (((mbeg + drow1) * ld_src + chunk_col(1)) << 1);
  const unsigned char* cur2 = src0 + (((mbeg + drow2) * ld_src + chunk_col(2)) << 1);
  const long dstep = (long)LB_ROWS * ld_src * 2;
  const uint32_t ddst = LB_WBYTES + (ximg ? LB_IMG : 0) + jb * 1024;
  int rel = 0;                                // row base of the next stage to issue, relative to mbeg
  auto issue = [&](int slot) {
    const uint32_t dst = ddst + slot * LB_STAGE;
    const unsigned char* s0 = rel + drow0 < nrows ? cur0 : zero;
    const unsigned char* s1 = rel + drow1 < nrows ? cur1 : zero;
    const unsigned char* s2 = rel + drow2 < nrows ? cur2 : zero;
    __builtin_amdgcn_global_load_lds((glb_void*)s0, (lds_void*)(dsm + dst), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)s1, (lds_void*)(dsm + dst + 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)s2, (lds_void*)(dsm + dst + 2048), 16, 0, 0);
    rel += LB_ROWS;
    cur0 += dstep; cur1 += dstep; cur2 += dstep;
  };

  // ---- dW fragments: lane (fg, q = fr >> 2, p = fr & 3) reads 8 bytes of LDS row 8 fg + q (+4); wave (wr, wc) owns dW rows
  //      n = 48 wr .. + 47 (three 16-column units of the dY image) and columns k = 96 wc .. + 95 (six units of the X image)
  const int q_ = fr >> 2, p_ = fr & 3;
  const int frow = 8 * fg + q_;
  const int swQ = (q_ >> 1) | ((fg & 1) << 1);
  const uint32_t tbase = lbase + LB_WBYTES + frow * LB_ROWB + 8 * p_;
  uint32_t pa[3], qa[6];
#pragma unroll
  for (int i = 0; i < 3; ++i) pa[i] = tbase + (((wr * 3 + i) ^ swQ) << 5);
#pragma unroll
  for (int j = 0; j < 6; ++j) qa[j] = tbase + LB_IMG + (((wc * 6 + j) ^ swQ) << 5);

  // ---- dX fragments (waves 0-5, t = wid): dY rows by ds_read_b128 from the same stage image (lane (fr, fg): row 16 u + fr, n =
  //      32 ks + 8 fg ..), wT rows 32 t + 8 (fr >> 2) + (fr & 3) (+4 for the second tile of the pair)
  const int s2 = ((fr >> 1) & 1) | (((fr >> 3) & 1) << 1);
  const uint32_t yRd0 = lbase + LB_WBYTES + fr * LB_ROWB + (((fg >> 1) ^ s2) << 5) + ((fg & 1) << 4);          // ks even
  const uint32_t yRd1 = lbase + LB_WBYTES + fr * LB_ROWB + (((2 + (fg >> 1)) ^ s2) << 5) + ((fg & 1) << 4);    // ks odd
  const int fW = ((fr >> 1) & 1) | (((fr >> 2) & 3) << 1);
  const int wrow = 32 * (wid < 6 ? wid : 0) + 8 * (fr >> 2) + (fr & 3);
  const uint32_t wRd0 = lbase + wrow * LB_ROWB + ((fg ^ fW) << 4);
  const uint32_t wRd1 = lbase + wrow * LB_ROWB + (((4 + fg) ^ fW) << 4);
  const bool nt_wave = wid < 6;
  const int ocol = 32 * wid + 8 * fg;         // first of this lane's 8 dX columns

  const bool do_bias = g.dbias != nullptr && wc == 0;
  u32x4 ones; ones.x = ones.y = ones.z = ones.w = 0x3F803F80u;

  f32x4 acc[3][6], bacc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 6; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // aux rows of the NEXT stage (DGELU): rows beyond M are clamped - the loads are issued unconditionally, their count is what
  // the waits rely on
  u32x4 pre0, pre1;
  pre0.x = pre0.y = pre0.z = pre0.w = 0u; pre1 = pre0;
  auto aux_ptr = [&](int stage, int u) {
    long m = mbeg + (long)stage * LB_ROWS + 16 * u + fr;
    if (m >= g.M) m = g.M - 1;
    return (const bf16*)g.aux + m * g.ldaux + ocol;
  };

  issue(0);
  if (DG && nt_wave) {
    const bf16* a0 = aux_ptr(0, 0);
    const bf16* a1 = aux_ptr(0, 1);
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pre0) : "v"(a0) : "memory");
    asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pre1) : "v"(a1) : "memory");
  }
  issue(1);
  int slot = 0;
  for (int s = 0; s < nsteps; ++s) {
    // queue, oldest first: .. DMA(s) | stores(s-1) aux(s) DMA(s+1): everything but the fixed-count tail has landed
    if (DG && nt_wave) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const uint32_t so = slot * LB_STAGE;

    if (nt_wave) {
      f32x4 na00 = f32x4{0.f, 0.f, 0.f, 0.f}, na01 = na00, na10 = na00, na11 = na00;
#define LB_NT_RD(KS, YB, WB, T)                                                                       \
      const u32x4 fy0##T = lb_rd128<128 * ((KS) >> 1)>(YB + so);                                      \
      const u32x4 fy1##T = lb_rd128<128 * ((KS) >> 1) + 16 * LB_ROWB>(YB + so);                       \
      const u32x4 fw0##T = lb_rd128<128 * ((KS) >> 1)>(WB);                                           \
      const u32x4 fw1##T = lb_rd128<128 * ((KS) >> 1) + 4 * LB_ROWB>(WB);
#define LB_NT_MM(T)                                                                                   \
      lb_mma(na00, fw0##T, fy0##T); lb_mma(na01, fw1##T, fy0##T);                                     \
      lb_mma(na10, fw0##T, fy1##T); lb_mma(na11, fw1##T, fy1##T);
      {
        LB_NT_RD(0, yRd0, wRd0, a) LB_NT_RD(1, yRd1, wRd1, b)
        LB_LGKM0();
        LB_NT_MM(a) LB_NT_MM(b)
      }
      {
        LB_NT_RD(2, yRd0, wRd0, a) LB_NT_RD(3, yRd1, wRd1, b)
        LB_LGKM0();
        LB_NT_MM(a) LB_NT_MM(b)
      }
      {
        LB_NT_RD(4, yRd0, wRd0, a) LB_NT_RD(5, yRd1, wRd1, b)
        LB_LGKM0();
        LB_NT_MM(a) LB_NT_MM(b)
      }
#undef LB_NT_RD
#undef LB_NT_MM
      // lane (fg, fr): row 16 u + fr of the stage, columns ocol .. ocol + 7 (tile 0: + 0..3, tile 1: + 4..7)
      if (DG) {            // aux(s) has landed once only DMA(s+1) is outstanding; the operands tie the wait to the values
        asm volatile("s_waitcnt vmcnt(3)" : "+v"(pre0), "+v"(pre1) :: "memory");
        __builtin_amdgcn_sched_barrier(0);
      }
      const int r0 = s * LB_ROWS + fr;
      {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { v[r] = na00[r]; v[4 + r] = na01[r]; }
        if (DG) {
          float x[8];
          uint4 pu; pu.x = pre0.x; pu.y = pre0.y; pu.z = pre0.z; pu.w = pre0.w;
          unpack<bf16>(pu, x);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= dgelu_t<bf16>(x[j]);
        }
        if (r0 < nrows) *(uint4*)((bf16*)g.dX + (mbeg + r0) * g.lddx + ocol) = pack<bf16>(v);
      }
      {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { v[r] = na10[r]; v[4 + r] = na11[r]; }
        if (DG) {
          float x[8];
          uint4 pu; pu.x = pre1.x; pu.y = pre1.y; pu.z = pre1.z; pu.w = pre1.w;
          unpack<bf16>(pu, x);
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] *= dgelu_t<bf16>(x[j]);
        }
        if (r0 + 16 < nrows) *(uint4*)((bf16*)g.dX + (mbeg + r0 + 16) * g.lddx + ocol) = pack<bf16>(v);
      }
      if (DG) {
        __builtin_amdgcn_sched_barrier(0);
        const bf16* a0 = aux_ptr(s + 1, 0);
        const bf16* a1 = aux_ptr(s + 1, 1);
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pre0) : "v"(a0) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(pre1) : "v"(a1) : "memory");
      }
    }
    issue(slot == 0 ? LB_NST - 1 : slot - 1);            // stage s + 2 -> slot (s + 2) % 3: last read in iteration s - 1

    {
      u32x4 fp[3], fq[6];
#pragma unroll
      for (int i = 0; i < 3; ++i) fp[i] = lb_frag_tr(pa[i] + so);
#pragma unroll
      for (int j = 0; j < 6; ++j) fq[j] = lb_frag_tr(qa[j] + so);
      LB_LGKM0();
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) lb_mma(acc[i][j], fp[i], fq[j]);
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 3; ++i) lb_mma(bacc[i], fp[i], ones);
      }
    }
    slot = slot == LB_NST - 1 ? 0 : slot + 1;
  }
  // the tail DMAs and the last aux loads must land before the wave goes on (the operands keep the aux registers allocated
  // until then)
  if (DG) asm volatile("s_waitcnt vmcnt(0)" : "+v"(pre0), "+v"(pre1) :: "memory");
  else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);

  // acc[i][j][r]: dW row n = 48 wr + 16 i + 4 fg + r, column k = 96 wc + 16 j + fr
  if (partial) {
    float* part = partial + (long)split * LB_C * LB_C + (wr * 48 + 4 * fg) * LB_C + wc * 96 + fr;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(16 * i + r) * LB_C + 16 * j] = acc[i][j][r];
  } else {
    float* d = g.dW + (long)(wr * 48 + 4 * fg) * g.lddw + wc * 96 + fr;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 6; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(d + (long)(16 * i + r) * g.lddw + 16 * j, acc[i][j][r]);
  }
  if (do_bias && fr == 0) {          // bacc[i][r]: row 4 fg + r <-> n, all columns equal
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = wr * 48 + 16 * i + 4 * fg + r;
        if (bpartial) bpartial[(long)split * LB_C + n] = bacc[i][r];
        else atomicAdd(g.dbias + n, bacc[i][r]);
      }
  }
}

// dW[n][k] += sum over the live slices of partial[s][n][k] (and dbias[n] += sum of bpartial[s][n]): 64 float4 columns per
// workgroup, the slices dealt over its four waves in a fixed order and combined through LDS in a fixed order
// (nrow rows of dW: 192 for the square layer, 576 for the wide one; the bias blocks follow the wblocks tile blocks)
__global__ __launch_bounds__(256) void linbwd_reduce_kernel(const float* __restrict__ partial, float* __restrict__ dW, int lddw, int live,
                                                           const float* __restrict__ bpartial, float* __restrict__ dbias, int wblocks, int nrow) {
  __shared__ float4 red[4][64];
  const bool bias = (int)blockIdx.x >= wblocks;
  const float* src = bias ? bpartial : partial;
  const long slice = bias ? nrow : (long)nrow * LB_C;
  const long n4 = slice / 4;
  const int c = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const long i = (long)(bias ? (int)blockIdx.x - wblocks : (int)blockIdx.x) * 64 + c;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i < n4) {
    const float* p = src + i * 4;
    int s = sg;
    for (; s + 12 < live; s += 16) {
      const float4 v0 = *(const float4*)(p + (long)s * slice), v1 = *(const float4*)(p + (long)(s + 4) * slice);
      const float4 v2 = *(const float4*)(p + (long)(s + 8) * slice), v3 = *(const float4*)(p + (long)(s + 12) * slice);
      a.x += (v0.x + v1.x) + (v2.x + v3.x); a.y += (v0.y + v1.y) + (v2.y + v3.y);
      a.z += (v0.z + v1.z) + (v2.z + v3.z); a.w += (v0.w + v1.w) + (v2.w + v3.w);
    }
    for (; s < live; s += 4) {
      const float4 v = *(const float4*)(p + (long)s * slice);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  red[sg][c] = a;
  __syncthreads();
  if (sg == 0 && i < n4) {
    const float4 b1 = red[1][c], b2 = red[2][c], b3 = red[3][c];
    a.x += b1.x + b2.x + b3.x; a.y += b1.y + b2.y + b3.y; a.z += b1.z + b2.z + b3.z; a.w += b1.w + b2.w + b3.w;
    float* d;
    if (bias) d = dbias + i * 4;
    else { const int n = (int)((i * 4) / LB_C); d = dW + (long)n * lddw + (int)(i * 4 - (long)n * LB_C); }
    float4 o = *(float4*)d;
    o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
    *(float4*)d = o;
  }
}

template <bool DG>
int launch_linbwd(const sodt_linbwd_args* g, float* partial, float* bpartial, hipStream_t st) {
  return sodt_launch<linbwd_sq_kernel<DG>>(dim3((unsigned)g->splits), dim3(512), LB_LDS, st, *g, partial, bpartial);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The wide form: backward of the 192 -> 576 linear layer (attn.qkv), dX[M][192] = dY[M][576] @ W, dW[576][192] += dY^T @ X.
// wT [192][576] (216 KiB) and the dW accumulator (442 KB) do not fit one CU, so K = 192 (the columns of dX, X and dW) is cut into
// three slabs of 64 and THREE sibling workgroups share an M-slice: workgroup (slice, slab j) streams all 576 columns of dY for
// its rows plus X[:, 64 j .. 64 j + 63], keeps wT rows 64 j .. 64 j + 63 resident (72 KiB) and produces dX[:, slab j] (the
// contraction over N is whole: no cross-workgroup sum) and the slice's partial dW[:, slab j].  The siblings are consecutive
// logical ids of xcd_remap, so they run on one XCD at the same time and two of the three dY reads are served by its L2.
//   * Stages of 32 rows: dY image [32][576] (36 KiB) then X-slab image [32][64] (4 KiB), two slots.  Waves 4-7 bring a stage in
//     ten 1 KiB LDS-DMA pieces each (the images are contiguous: piece I lands at I KiB of the slot; pieces 0-35 dY, 36-39 X) and
//     hold nothing else in the vector-memory queue, so the count they wait for at the top of stage s - everything they have in
//     flight, DMA(s) - is exact; DMA(s + 1) goes out right after the barrier, into the slot every wave has just left.
//   * Waves 0-3 (c = wid & 1, u = wid >> 1) form the 16 x 32 block of dX at rows 16 u, slab columns 32 c: 18 contraction steps
//     of 32 (N ascending, the order of gemm_nt3_kernel), fragments read two steps ahead of their MFMAs behind counted lgkmcnt
//     waits; the W rows are permuted as in the square kernel, so a lane stores 16 bytes.  They never wait on vector memory.
//   * All eight waves, as a 4 (n) x 2 (k) grid, add dY^T X into 9 x 2 accumulator tiles each (n units 9 wr .. 9 wr + 8, slab
//     columns 32 wc ..); dbias of the n units 12 j .. 12 j + 11 belongs to slab j (ones-vector MFMA, the units of a wave row
//     alternating between its two waves).
// The swizzles are the square kernel's: every row pitch here (1152 and 128 bytes) is 128 modulo 256 like its 384.
constexpr int LW_N = 576, LW_KS = 64;
constexpr int LW_YROWB = LW_N * 2;                    // 1152 bytes per row of the dY image and of the wT slab
constexpr int LW_XROWB = LW_KS * 2;                   // 128 bytes per row of the X-slab image
constexpr int LW_WBYTES = LW_KS * LW_YROWB;           // 72 KiB
constexpr int LW_YIMG = LB_ROWS * LW_YROWB;           // 36 KiB
constexpr int LW_XIMG = LB_ROWS * LW_XROWB;           // 4 KiB
constexpr int LW_STAGE = LW_YIMG + LW_XIMG;           // 40 KiB
constexpr int LW_NST = 2;
constexpr int LW_LDS = LW_WBYTES + LW_NST * LW_STAGE; // 152 KiB
constexpr int LW_NDMA = 10;                           // DMA pieces per loader wave and stage
constexpr int LW_YPIECES = LW_YIMG / 1024;            // 36

template <int ROWB> __device__ __forceinline__ u32x4 lw_frag_tr(uint32_t addr) {
  const uint2 lo = lb_rd_tr<0>(addr), hi = lb_rd_tr<4 * ROWB>(addr);
  u32x4 r; r.x = lo.x; r.y = lo.y; r.z = hi.x; r.w = hi.y;
  return r;
}
#define LW_LGKM(N) do { asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

__global__ __launch_bounds__(512) void linbwd_wide_kernel(const sodt_linbwd_args g, float* __restrict__ partial, float* __restrict__ bpartial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wid >> 1, wc = wid & 1;
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lbase = lb_lds_addr(dsm);

  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = lid / 3, slab = lid - 3 * split;
  const long rows_per = (((g.M + g.splits - 1) / g.splits) + LB_ROWS - 1) / LB_ROWS * LB_ROWS;
  const long mbeg = (long)split * rows_per;
  const long mend = (mbeg + rows_per < g.M) ? (mbeg + rows_per) : g.M;
  if (mbeg >= mend) return;                   // dead slice
  const int nrows = (int)(mend - mbeg);
  const int nsteps = (nrows + LB_ROWS - 1) / LB_ROWS;

  // ---- resident wT slab: rows 64 slab .. + 63 (output columns of dX), 72 chunks of 16 bytes each, chunk c of row r at
  //      r * 1152 + ((c ^ f(r)) << 4) (4,608 chunks = 9 per thread)
  {
    uint4 wv[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int id = tid + 512 * e, r = id / 72, c = id - r * 72;
      wv[e] = *(const uint4*)((const bf16*)g.wT + (long)(LW_KS * slab + r) * g.ldw + 8 * c);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int id = tid + 512 * e, r = id / 72, c = id - r * 72;
      const int f = ((r >> 1) & 1) | (((r >> 3) & 3) << 1);
      *(uint4*)(dsm + r * LW_YROWB + ((c ^ f) << 4)) = wv[e];
    }
  }
  __syncthreads();                            // (no DMA in flight yet: a plain barrier)

  // ---- DMA descriptors of the loader waves 4-7: piece I = 10 (wid - 4) + e, chunk id = 64 I + lane (dY: row id / 72; X: row
  //      (id - 2304) / 8); the source column carries the swizzle of the 32-byte unit
  const unsigned char* zero = (const unsigned char*)lb_zero16;
  const bool loader = wid >= 4;
  const int piece0 = LW_NDMA * (wid & 3);
  const long ystep = (long)LB_ROWS * g.ldy * 2, xstep = (long)LB_ROWS * g.ldx * 2;
  const unsigned char* cur[LW_NDMA];
  int drow[LW_NDMA];
#pragma unroll
  for (int e = 0; e < LW_NDMA; ++e) {
    const int I = piece0 + e;
    const bool isx = I >= LW_YPIECES;
    const int idy = 64 * I + lane, idx = idy - 64 * LW_YPIECES;
    const int r2 = isx ? (idx >> 3) : idy / 72;
    const int c2 = isx ? (idx & 7) : idy - r2 * 72;
    const int sw2 = ((r2 >> 1) & 1) | (((r2 >> 3) & 1) << 1);
    const int col = ((((c2 >> 1) ^ sw2) << 1) | (c2 & 1)) << 3;
    drow[e] = r2;
    cur[e] = isx ? (const unsigned char*)((const bf16*)g.X + (mbeg + r2) * g.ldx + LW_KS * slab + col)
                 : (const unsigned char*)((const bf16*)g.dY + (mbeg + r2) * g.ldy + col);
  }

  // ---- dW fragments: lane (fg, q = fr >> 2, p = fr & 3) reads 8 bytes of LDS row 8 fg + q (+4); wave (wr, wc) owns dW rows
  //      n = 144 wr .. + 143 (nine 16-column units of the dY image) and slab columns 32 wc .. + 31 (two units of the X image)
  const int q_ = fr >> 2, p_ = fr & 3;
  const int frow = 8 * fg + q_;
  const int swQ = (q_ >> 1) | ((fg & 1) << 1);
  uint32_t pa[9], qa[2];
#pragma unroll
  for (int i = 0; i < 9; ++i) pa[i] = lbase + LW_WBYTES + frow * LW_YROWB + 8 * p_ + (((wr * 9 + i) ^ swQ) << 5);
#pragma unroll
  for (int j = 0; j < 2; ++j) qa[j] = lbase + LW_WBYTES + LW_YIMG + frow * LW_XROWB + 8 * p_ + (((wc * 2 + j) ^ swQ) << 5);

  // ---- dX fragments (waves 0-3): dY rows by ds_read_b128 (lane (fr, fg): row 16 u + fr, n = 32 ks + 8 fg ..), wT slab rows
  //      32 c + 8 (fr >> 2) + (fr & 3) (+4 for the second tile of the pair)
  const bool nt_wave = wid < 4;
  const int xc = wid & 1, xu = (wid >> 1) & 1;
  const int s2 = ((fr >> 1) & 1) | (((fr >> 3) & 1) << 1);
  const uint32_t yrow = lbase + LW_WBYTES + (16 * xu + fr) * LW_YROWB + ((fg & 1) << 4);
  const uint32_t yRd0 = yrow + (((fg >> 1) ^ s2) << 5);                // ks even
  const uint32_t yRd1 = yrow + (((2 + (fg >> 1)) ^ s2) << 5);          // ks odd
  const int fW = ((fr >> 1) & 1) | (((fr >> 2) & 3) << 1);
  const int wrow = 32 * xc + 8 * (fr >> 2) + (fr & 3);
  const uint32_t wRd0 = lbase + wrow * LW_YROWB + ((fg ^ fW) << 4);
  const uint32_t wRd1 = lbase + wrow * LW_YROWB + (((4 + fg) ^ fW) << 4);
  const int ocol = LW_KS * slab + 32 * xc + 8 * fg;          // first of this lane's 8 dX columns

  // dbias: n unit U belongs to slab U / 12; inside wave row wr the units alternate between wc = 0 (i even) and wc = 1 (i odd)
  const bool do_bias = g.dbias != nullptr;
  u32x4 ones; ones.x = ones.y = ones.z = ones.w = 0x3F803F80u;

  f32x4 acc[9][2], bacc[5];
#pragma unroll
  for (int i = 0; i < 9; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 5; ++i) bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (loader) {
    const uint32_t dst = LW_WBYTES + piece0 * 1024;
#pragma unroll
    for (int e = 0; e < LW_NDMA; ++e) {
      const unsigned char* s = drow[e] < nrows ? cur[e] : zero;
      __builtin_amdgcn_global_load_lds((glb_void*)s, (lds_void*)(dsm + dst + e * 1024), 16, 0, 0);
      cur[e] += (piece0 + e >= LW_YPIECES) ? xstep : ystep;
    }
  }
  int slot = 0;
  for (int s = 0; s < nsteps; ++s) {
    // loader waves: DMA(s) is all they have in flight; the other waves have only dX stores there and wait for nothing
    if (loader) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const uint32_t so = slot * LW_STAGE;

    if (loader) {
      if (s + 1 < nsteps) {                    // stage s + 1 -> the other slot: last read in iteration s - 1
        const uint32_t dst = LW_WBYTES + (slot ^ 1) * LW_STAGE + piece0 * 1024;
        const int rel = (s + 1) * LB_ROWS;
        if (rel + LB_ROWS <= nrows) {
#pragma unroll
          for (int e = 0; e < LW_NDMA; ++e) {
            __builtin_amdgcn_global_load_lds((glb_void*)cur[e], (lds_void*)(dsm + dst + e * 1024), 16, 0, 0);
            cur[e] += (piece0 + e >= LW_YPIECES) ? xstep : ystep;
          }
        } else {
#pragma unroll
          for (int e = 0; e < LW_NDMA; ++e) {
            const unsigned char* sp = rel + drow[e] < nrows ? cur[e] : zero;
            __builtin_amdgcn_global_load_lds((glb_void*)sp, (lds_void*)(dsm + dst + e * 1024), 16, 0, 0);
            cur[e] += (piece0 + e >= LW_YPIECES) ? xstep : ystep;
          }
        }
      }
    } else {
      f32x4 na0 = f32x4{0.f, 0.f, 0.f, 0.f}, na1 = na0;
      u32x4 fyA0, fyB0, fw0A0, fw1A0, fw0B0, fw1B0, fyA1, fyB1, fw0A1, fw1A1, fw0B1, fw1B1;
      // group G = contraction steps 2 G (A) and 2 G + 1 (B); buffer T
#define LW_NT_RD(G, T)                                                                                \
      fyA##T = lb_rd128<128 * (G)>(yRd0 + so); fyB##T = lb_rd128<128 * (G)>(yRd1 + so);                \
      fw0A##T = lb_rd128<128 * (G)>(wRd0); fw1A##T = lb_rd128<128 * (G) + 4 * LW_YROWB>(wRd0);         \
      fw0B##T = lb_rd128<128 * (G)>(wRd1); fw1B##T = lb_rd128<128 * (G) + 4 * LW_YROWB>(wRd1);
#define LW_NT_MM(T)                                                                                   \
      lb_mma(na0, fw0A##T, fyA##T); lb_mma(na1, fw1A##T, fyA##T);                                     \
      lb_mma(na0, fw0B##T, fyB##T); lb_mma(na1, fw1B##T, fyB##T);
      LW_NT_RD(0, 0)
      LW_NT_RD(1, 1) LW_LGKM(6); LW_NT_MM(0)
      LW_NT_RD(2, 0) LW_LGKM(6); LW_NT_MM(1)
      LW_NT_RD(3, 1) LW_LGKM(6); LW_NT_MM(0)
      LW_NT_RD(4, 0) LW_LGKM(6); LW_NT_MM(1)
      LW_NT_RD(5, 1) LW_LGKM(6); LW_NT_MM(0)
      LW_NT_RD(6, 0) LW_LGKM(6); LW_NT_MM(1)
      LW_NT_RD(7, 1) LW_LGKM(6); LW_NT_MM(0)
      LW_NT_RD(8, 0) LW_LGKM(6); LW_NT_MM(1)
      LW_LGKM(0); LW_NT_MM(0)
#undef LW_NT_RD
#undef LW_NT_MM
      // lane (fg, fr): row 16 u + fr of the stage, columns ocol .. ocol + 7 (tile 0: + 0..3, tile 1: + 4..7)
      const int r0 = s * LB_ROWS + 16 * xu + fr;
      float v[8];
#pragma unroll
      for (int r = 0; r < 4; ++r) { v[r] = na0[r]; v[4 + r] = na1[r]; }
      if (r0 < nrows) *(uint4*)((bf16*)g.dX + (mbeg + r0) * g.lddx + ocol) = pack<bf16>(v);
    }

    {
      u32x4 fp[9], fq[2];
#pragma unroll
      for (int i = 0; i < 9; ++i) fp[i] = lw_frag_tr<LW_YROWB>(pa[i] + so);
#pragma unroll
      for (int j = 0; j < 2; ++j) fq[j] = lw_frag_tr<LW_XROWB>(qa[j] + so);
      LB_LGKM0();
#pragma unroll
      for (int i = 0; i < 9; ++i) { lb_mma(acc[i][0], fp[i], fq[0]); lb_mma(acc[i][1], fp[i], fq[1]); }
      if (do_bias) {
        if (wc == 0) {
#pragma unroll
          for (int ii = 0; ii < 5; ++ii)
            if ((wr * 9 + 2 * ii) / 12 == slab) lb_mma(bacc[ii], fp[2 * ii], ones);
        } else {
#pragma unroll
          for (int ii = 0; ii < 4; ++ii)
            if ((wr * 9 + 2 * ii + 1) / 12 == slab) lb_mma(bacc[ii], fp[2 * ii + 1], ones);
        }
      }
    }
    slot ^= 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);

  // acc[i][j][r]: dW row n = 144 wr + 16 i + 4 fg + r, column k = 64 slab + 32 wc + 16 j + fr
  const int kcol = LW_KS * slab + 32 * wc + fr;
  if (partial) {
    float* part = partial + (long)split * LW_N * LB_C + (long)(wr * 144 + 4 * fg) * LB_C + kcol;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[(16 * i + r) * LB_C + 16 * j] = acc[i][j][r];
  } else {
    float* d = g.dW + (long)(wr * 144 + 4 * fg) * g.lddw + kcol;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(d + (long)(16 * i + r) * g.lddw + 16 * j, acc[i][j][r]);
  }
  if (do_bias && fr == 0) {          // bacc[ii][r]: unit i = 2 ii + wc, row 4 fg + r <-> n, all columns equal
#pragma unroll
    for (int ii = 0; ii < 5; ++ii) {
      const int i = 2 * ii + wc;
      if (i < 9 && (wr * 9 + i) / 12 == slab) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int n = wr * 144 + 16 * i + 4 * fg + r;
          if (bpartial) bpartial[(long)split * LW_N + n] = bacc[ii][r];
          else atomicAdd(g.dbias + n, bacc[ii][r]);
        }
      }
    }
  }
}

}  // namespace

extern "C" int sodt_linear_bwd_sq(const sodt_linbwd_args* g, int dtype, sodt_stream_t st) {
  if (!g || dtype != SODT_BF16 || g->N != LB_C || g->K != LB_C || g->M <= 0 || g->splits < 1 || g->splits > 65535) return SODT_EINVAL;
  if (!g->dY || !g->X || !g->wT || !g->dX || !g->dW) return SODT_EINVAL;
  if (g->flags != 0 && g->flags != SODT_EPI_DGELU) return SODT_EINVAL;
  if ((g->ldy % 8) || (g->ldx % 8) || (g->ldw % 8) || (g->lddx % 8) || (g->lddw % 4)) return SODT_EINVAL;
  if (g->ldy < LB_C || g->ldx < LB_C || g->ldw < LB_C || g->lddx < LB_C || g->lddw < LB_C) return SODT_EINVAL;
  if ((((uintptr_t)g->dY) | ((uintptr_t)g->X) | ((uintptr_t)g->wT) | ((uintptr_t)g->dX) | ((uintptr_t)g->dW)) & 15) return SODT_EINVAL;
  if (g->dbias && (((uintptr_t)g->dbias) & 15)) return SODT_EINVAL;
  if (g->flags & SODT_EPI_DGELU) {
    if (!g->aux || (g->ldaux % 8) || g->ldaux < LB_C || (((uintptr_t)g->aux) & 15)) return SODT_EINVAL;
  }
  // scratch protocol of sodt_gemm_tn_args: splits * N * K floats hold the partial dW tiles; when the scratch also has room for
  // splits * N more, the dbias rows go through it too (deterministic), otherwise dbias alone keeps its atomics
  const long tile_floats = (long)g->splits * LB_C * LB_C;
  const bool use_partial = g->partial && g->splits > 1 && tile_floats <= g->partial_floats && (((uintptr_t)g->partial) & 15) == 0;
  float* partial = use_partial ? g->partial : nullptr;
  float* bpartial = (use_partial && g->dbias && tile_floats + (long)g->splits * LB_C <= g->partial_floats) ? g->partial + tile_floats : nullptr;
  const int rc = (g->flags & SODT_EPI_DGELU) ? launch_linbwd<true>(g, partial, bpartial, (hipStream_t)st)
                                             : launch_linbwd<false>(g, partial, bpartial, (hipStream_t)st);
  if (rc || !use_partial) return rc;
  const long rows_per = ((((long)g->M + g->splits - 1) / g->splits) + LB_ROWS - 1) / LB_ROWS * LB_ROWS;
  const int live = (int)(((long)g->M + rows_per - 1) / rows_per);
  const int wblocks = LB_C * LB_C / 4 / 64;
  return sodt_launch<linbwd_reduce_kernel>(dim3(wblocks + (bpartial ? 1 : 0)), dim3(256), 0, (hipStream_t)st, (const float*)partial,
                                           g->dW, g->lddw, live, (const float*)bpartial, g->dbias, wblocks, LB_C);
}

extern "C" int sodt_linear_bwd_wide(const sodt_linbwd_args* g, int dtype, sodt_stream_t st) {
  if (!g || dtype != SODT_BF16 || g->N != LW_N || g->K != LB_C || g->M <= 0 || g->splits < 1 || g->splits > 21845) return SODT_EINVAL;
  if (!g->dY || !g->X || !g->wT || !g->dX || !g->dW || g->flags != 0) return SODT_EINVAL;
  if ((g->ldy % 8) || (g->ldx % 8) || (g->ldw % 8) || (g->lddx % 8) || (g->lddw % 4)) return SODT_EINVAL;
  if (g->ldy < LW_N || g->ldx < LB_C || g->ldw < LW_N || g->lddx < LB_C || g->lddw < LB_C) return SODT_EINVAL;
  if ((((uintptr_t)g->dY) | ((uintptr_t)g->X) | ((uintptr_t)g->wT) | ((uintptr_t)g->dX) | ((uintptr_t)g->dW)) & 15) return SODT_EINVAL;
  if (g->dbias && (((uintptr_t)g->dbias) & 15)) return SODT_EINVAL;
  // the scratch protocol of sodt_linear_bwd_sq with N = 576: splits * N * K floats of partial tiles, then splits * N of dbias rows
  const long tile_floats = (long)g->splits * LW_N * LB_C;
  const bool use_partial = g->partial && g->splits > 1 && tile_floats <= g->partial_floats && (((uintptr_t)g->partial) & 15) == 0;
  float* partial = use_partial ? g->partial : nullptr;
  float* bpartial = (use_partial && g->dbias && tile_floats + (long)g->splits * LW_N <= g->partial_floats) ? g->partial + tile_floats : nullptr;
  // three sibling workgroups per slice, consecutive logical ids
  const int rc = sodt_launch<linbwd_wide_kernel>(dim3(3u * (unsigned)g->splits), dim3(512), LW_LDS, (hipStream_t)st, *g, partial, bpartial);
  if (rc || !use_partial) return rc;
  const long rows_per = ((((long)g->M + g->splits - 1) / g->splits) + LB_ROWS - 1) / LB_ROWS * LB_ROWS;
  const int live = (int)(((long)g->M + rows_per - 1) / rows_per);
  const int wblocks = LW_N * LB_C / 4 / 64;
  return sodt_launch<linbwd_reduce_kernel>(dim3(wblocks + (bpartial ? (LW_N / 4 + 63) / 64 : 0)), dim3(256), 0, (hipStream_t)st,
                                           (const float*)partial, g->dW, g->lddw, live, (const float*)bpartial, g->dbias, wblocks, LW_N);
}
