// Backward of the stage-1 linear MLP (fc1 192 -> 768, GELU, fc2 768 -> 192; bf16) around ONE pass over xn2 and dY:
//     h    = xn2 @ fc1.weight^T + fc1.bias            recomputed, never stored
//     dh   = (dY @ fc2.weight) * gelu'(h)             [M][768] bf16, bit-identical to sodt_gemm_nt's SODT_EPI_BIAS | SODT_EPI_DGELU_RC
//     dW1[768][192] += dh^T @ xn2,   db1[768] += column sums of dh            (f32)
//     dW2[192][768] += dY^T @ GELU(h), db2[192] += column sums of dY          (f32)
// It replaces sodt_gemm_tn (dW2) + sodt_gemm_nt (DGELU_RC) + sodt_gemm_tn (dW1): GELU(h) is no longer written by the forward and
// read back, and dh is read once (by the dxn = dh @ fc1.weight GEMM that stays) instead of twice.
//
// Structure (gfx950).  The hidden dimension is cut into EIGHT slabs of 96 columns and eight sibling workgroups share an M-slice
// (consecutive logical ids of xcd_remap, as linbwd_wide_kernel's three): each streams the slice's xn2 and dY rows - seven of the
// eight reads served by the XCD's L2 - and owns everything of its slab: dh[:, slab], dW1[slab, :], db1[slab], dW2[:, slab].
// No sum crosses workgroups (db2 is slab 0's).
//   * Resident in LDS (72 KiB): fc1.weight rows of the slab [96][192] and the rows of fc2.weight^T of the slab [96][192], both with
//     linbwd_sq_kernel's W swizzle (row pitch 384 bytes).
//   * xn2 and dY rows arrive by LDS-DMA in 32-row stages (12 KiB + 12 KiB, linbwd_sq_kernel's two images and its descriptors),
//     two slots, one stage in flight.
//   * Phase 1 of a stage (waves 0-5; wave (c, u) owns rows 16 u .. + 15, slab columns 32 c .. + 31): h and dA = dY @ W2[:, slab]
//     in the SAME lanes (K = 192 ascending in 32-element steps, operands swapped and the W rows permuted as in linbwd_sq_kernel:
//     a lane ends with 8 consecutive columns of one row), then gelu'(h) - rounded to bf16 where sodt_gemm_nt parks it - and
//     GELU(h) in registers; dh goes to HBM in 16-byte stores, and dh and GELU(h) go to two LDS staging images (bf16, [32][96] at a
//     256-byte pitch, the 32-byte unit XOR-swizzled by row bits 0, 1, 3: a ds_read_b64_tr_b16 touches eight rows per half wave),
//     double-buffered.
//   * Phase 2 (all waves, one stage behind): dW1[slab] += dh^T xn2 on a 2 (n) x 4 (k) wave grid and dW2[:, slab] +=
//     dY^T GELU(h) on a 4 (n) x 2 (k) grid, 3 x 3 accumulator tiles each held across the slice, both operands through
//     ds_read_b64_tr_b16; db1 / db2 by one MFMA per unit against a vector of ones.
//   * One barrier per stage.  Phase 1 is activation-VALU heavy (a logistic GELU and the gelu' polynomial per element) and six
//     waves put two of them on two of the four SIMDs; run back to back with phase 2 behind a second barrier (the first version)
//     the launch took 0.93 ms at M = 524,288, no faster than the three launches.  So phase 2 of stage s - 1 shares the interval
//     of phase 1 of stage s, the two waves of a SIMD taking them in opposite order (see the loop).
//   144 + 144 MFMAs per stage and workgroup, linbwd_sq_kernel's count.
//   * Partial tiles go to the caller's scratch with plain stores and mlpbwd_reduce_kernel adds the live slices in a fixed order
//     (linbwd_reduce_kernel's order; one launch for the two weights and the two biases, dW2's rows being 768 wide).  Without a
//     scratch that fits: f32 atomics.
#include "gemm_epi.h"
#include "launch.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int MB_C = 192, MB_H = 768, MB_SL = 96, MB_NSLAB = MB_H / MB_SL;
constexpr int MB_ROWB = MB_C * 2;                      // 384 bytes per row of the weight slabs and of the streamed images
constexpr int MB_WIMG = MB_SL * MB_ROWB;               // 36 KiB: one weight slab
constexpr int MB_WBYTES = 2 * MB_WIMG;                 // fc1.weight slab, then fc2.weight^T slab
constexpr int MB_ROWS = 32, MB_NST = 2;
constexpr int MB_IMG = MB_ROWS * MB_ROWB;              // 12 KiB per operand and stage
constexpr int MB_STAGE = 2 * MB_IMG;                   // xn2 image, then dY image
constexpr int MB_SROWB = 256;                          // row pitch of the staging images (eight 32-byte units, six used)
constexpr int MB_SIMG = MB_ROWS * MB_SROWB;            // 8 KiB
constexpr int MB_STG = MB_WBYTES + MB_NST * MB_STAGE;  // two staging buffers: dh image, then GELU(h) image, each
constexpr int MB_LDS = MB_STG + 4 * MB_SIMG;           // 152 KiB
constexpr long MB_TILE = (long)MB_H * MB_C;            // floats of one weight-gradient tile (either weight)

struct MlpBwdArgs {
  const bf16* xn; int ldxn;
  const bf16* dY; int ldy;
  const bf16* w1; int ldw1;
  const float* b1;
  const bf16* w2T; int ldw2;
  bf16* dh; int lddh;
  bf16* hact; int ldha;
  float* dW1; int lddw1;
  float* db1;
  float* dW2; int lddw2;
  float* db2;
  long M;
  int splits;
};

__device__ uint4 mb_zero16[4];                         // DMA source of rows beyond the slice

__device__ __forceinline__ uint32_t mb_lds_addr(const void* p) { return (uint32_t)(uintptr_t)(lds_void*)p; }

template <int OFF> __device__ __forceinline__ u32x4 mb_rd128(uint32_t addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
template <int OFF> __device__ __forceinline__ uint2 mb_rd_tr(uint32_t addr) {
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  u32x2 t;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(t) : "v"(addr), "n"(OFF));
  uint2 v; v.x = t.x; v.y = t.y;
  return v;
}
// rows r .. r+3 and r+4 .. r+7 of one 16-column unit: the 8 contraction elements of a lane
template <int ROWB> __device__ __forceinline__ u32x4 mb_frag_tr(uint32_t addr) {
  const uint2 lo = mb_rd_tr<0>(addr), hi = mb_rd_tr<4 * ROWB>(addr);
  u32x4 r; r.x = lo.x; r.y = lo.y; r.z = hi.x; r.w = hi.y;
  return r;
}
// (inline asm: a store the compiler sees would be ordered behind the LDS-DMA in flight with a vmcnt(0))
__device__ __forceinline__ void mb_wr128(uint32_t addr, const uint4& v) {
  u32x4 t; t.x = v.x; t.y = v.y; t.z = v.z; t.w = v.w;
  asm volatile("ds_write_b128 %0, %1" :: "v"(addr), "v"(t) : "memory");
}
#define MB_LGKM0() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

__device__ __forceinline__ void mb_mma(f32x4& acc, const u32x4& a, const u32x4& b) {
  union { u32x4 u; bf16x8 v; } ua, ub;
  ua.u = a; ub.u = b;
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.v, ub.v, acc, 0, 0, 0);
}

__global__ __launch_bounds__(512) void mlp_bwd_kernel(const MlpBwdArgs g, float* __restrict__ partial, float* __restrict__ bpartial) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lbase = mb_lds_addr(dsm);

  const int lid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = lid / MB_NSLAB, slab = lid - MB_NSLAB * split;
  const long rows_per = (((g.M + g.splits - 1) / g.splits) + MB_ROWS - 1) / MB_ROWS * MB_ROWS;
  const long mbeg = (long)split * rows_per;
  const long mend = (mbeg + rows_per < g.M) ? (mbeg + rows_per) : g.M;
  if (mbeg >= mend) return;                   // dead slice: no partial tile (the reduction reads the live ones only)
  const int nrows = (int)(mend - mbeg);
  const int nsteps = (nrows + MB_ROWS - 1) / MB_ROWS;

  // ---- phase-1 geometry (waves 0-5): wave (c, u) forms rows 16 u + fr, slab columns 32 c + 8 fg .. + 7 of h and dA
  const bool p1_wave = wid < 6;
  const int pc = p1_wave ? (wid >> 1) : 0, pu = wid & 1;
  const int ocol = MB_SL * slab + 32 * pc + 8 * fg;          // first of this lane's 8 hidden columns
  // fc1.bias of the lane's columns: loaded AHEAD of the weight slabs, so the wait for those covers it
  const float4 bA = *(const float4*)(g.b1 + ocol), bB = *(const float4*)(g.b1 + ocol + 4);

  // ---- resident weight slabs: image 0 = fc1.weight rows 96 slab .., image 1 = fc2.weight^T rows 96 slab ..; row r, 16-byte
  //      chunk c at r * 384 + ((c ^ f(r)) << 4) (2 x 2,304 chunks = 9 per thread, all nine loads in flight before the first LDS write)
  {
    uint4 wv[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int id = tid + 512 * e, img = id / 2304, rem = id - 2304 * img, r = rem / 24, c = rem - r * 24;
      const bf16* src = img ? g.w2T + (long)(MB_SL * slab + r) * g.ldw2 : g.w1 + (long)(MB_SL * slab + r) * g.ldw1;
      wv[e] = *(const uint4*)(src + 8 * c);
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int id = tid + 512 * e, img = id / 2304, rem = id - 2304 * img, r = rem / 24, c = rem - r * 24;
      const int f = ((r >> 1) & 1) | (((r >> 3) & 3) << 1);
      *(uint4*)(dsm + img * MB_WIMG + r * MB_ROWB + ((c ^ f) << 4)) = wv[e];
    }
  }
  float bias[8] = {bA.x, bA.y, bA.z, bA.w, bB.x, bB.y, bB.z, bB.w};
#pragma unroll
  for (int j = 0; j < 8; ++j) asm volatile("" : "+v"(bias[j]));     // the values are in registers before the first DMA goes out
  __syncthreads();                            // (no DMA in flight yet: a plain barrier)

  // ---- DMA descriptors (linbwd_sq_kernel's): an image is 768 chunks = 12 wave-instructions; waves 0-3 bring xn2, waves 4-7 dY,
  //      three instructions each.  chunk id = 64 j + lane -> row id / 24, chunk id % 24; the source column carries the swizzle.
  const unsigned char* zero = (const unsigned char*)mb_zero16;
  const bool yimg = wid >= 4;
  const int jb = 3 * (wid & 3);
  const long ld_src = yimg ? g.ldy : g.ldxn;
  const unsigned char* src0 = (const unsigned char*)(yimg ? g.dY : g.xn);
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
  const long dstep = (long)MB_ROWS * ld_src * 2;
  const uint32_t ddst = MB_WBYTES + (yimg ? MB_IMG : 0) + jb * 1024;
  int rel = 0;                                // row base of the next stage to issue, relative to mbeg
  auto issue = [&](int slot) {
    const uint32_t dst = ddst + slot * MB_STAGE;
    const unsigned char* s0 = rel + drow0 < nrows ? cur0 : zero;
    const unsigned char* s1 = rel + drow1 < nrows ? cur1 : zero;
    const unsigned char* s2 = rel + drow2 < nrows ? cur2 : zero;
    __builtin_amdgcn_global_load_lds((glb_void*)s0, (lds_void*)(dsm + dst), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)s1, (lds_void*)(dsm + dst + 1024), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((glb_void*)s2, (lds_void*)(dsm + dst + 2048), 16, 0, 0);
    rel += MB_ROWS;
    cur0 += dstep; cur1 += dstep; cur2 += dstep;
  };

  // ---- phase-1 fragments: activation rows by ds_read_b128 (lane (fr, fg): row 16 u + fr, k = 32 ks + 8 fg ..; the dY image sits
  //      MB_IMG behind the xn2 image), weight-slab rows 32 c + 8 (fr >> 2) + (fr & 3) (+4 for the second tile of the pair; the
  //      fc2.weight^T slab sits MB_WIMG behind the fc1.weight slab)
  const int s2 = ((fr >> 1) & 1) | (((fr >> 3) & 1) << 1);
  const uint32_t arow = lbase + MB_WBYTES + (16 * pu + fr) * MB_ROWB + ((fg & 1) << 4);
  const uint32_t aRd0 = arow + (((fg >> 1) ^ s2) << 5);                // ks even
  const uint32_t aRd1 = arow + (((2 + (fg >> 1)) ^ s2) << 5);          // ks odd
  const int fW = ((fr >> 1) & 1) | (((fr >> 2) & 3) << 1);
  const int wrow = 32 * pc + 8 * (fr >> 2) + (fr & 3);
  const uint32_t wRd0 = lbase + wrow * MB_ROWB + ((fg ^ fW) << 4);
  const uint32_t wRd1 = lbase + wrow * MB_ROWB + (((4 + fg) ^ fW) << 4);
  // staging write of the lane's 16 bytes: row 16 u + fr, 16-byte chunk 4 c + fg, the unit swizzled by row bits 0, 1, 3
  const int f3w = (fr & 3) | (((fr >> 3) & 1) << 2);
  const uint32_t stW = lbase + MB_STG + (16 * pu + fr) * MB_SROWB + ((((4 * pc + fg) >> 1) ^ f3w) << 5) + ((fg & 1) << 4);

  // ---- phase-2 fragments: lane (fg, q = fr >> 2, p = fr & 3) reads 8 bytes of LDS row 8 fg + q (+4).
  //      dW1: wave (wr1 = wid >> 2, wc1 = wid & 3) owns slab rows 48 wr1 .. + 47 (three units of the dh staging image) and columns
  //           48 wc1 .. + 47 (three units of the xn2 image)
  //      dW2: wave (wr2 = wid >> 1, wc2 = wid & 1) owns rows 48 wr2 .. + 47 (three units of the dY image) and slab columns
  //           48 wc2 .. + 47 (three units of the GELU(h) staging image)
  const int wr1 = wid >> 2, wc1 = wid & 3, wr2 = wid >> 1, wc2 = wid & 1;
  const int q_ = fr >> 2, p_ = fr & 3;
  const int frow = 8 * fg + q_;
  const int swQ = (q_ >> 1) | ((fg & 1) << 1);
  const int f3r = q_ | ((fg & 1) << 2);
  const uint32_t ibase = lbase + MB_WBYTES + frow * MB_ROWB + 8 * p_;
  const uint32_t sbase = lbase + MB_STG + frow * MB_SROWB + 8 * p_;
  uint32_t pa1[3], qa1[3], pa2[3], qa2[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    pa1[i] = sbase + (((3 * wr1 + i) ^ f3r) << 5);
    qa1[i] = ibase + (((3 * wc1 + i) ^ swQ) << 5);
    pa2[i] = ibase + MB_IMG + (((3 * wr2 + i) ^ swQ) << 5);
    qa2[i] = sbase + MB_SIMG + (((3 * wc2 + i) ^ f3r) << 5);
  }
  // db1 of the slab: waves 0 and 4 (wc1 == 0).  db2 (slab 0 only) on four OTHER waves, one per wr2, so that one accumulator set
  // serves both: waves 1 (wr2 0), 2 (wr2 1), 5 (wr2 2), 6 (wr2 3)
  const bool do_b1 = wc1 == 0, do_b2 = slab == 0 && (wid == 1 || wid == 2 || wid == 5 || wid == 6);
  u32x4 ones; ones.x = ones.y = ones.z = ones.w = 0x3F803F80u;

  f32x4 acc1[3][3], acc2[3][3], bacc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) acc1[i][j] = acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // One barrier per stage: between barrier s and barrier s + 1 a wave runs phase 1 of stage s (waves 0-5) AND phase 2 of stage
  // s - 1 (all waves), whose streamed-image fragments it read in its own previous interval and holds in registers (so two image
  // slots are enough) and whose dh / GELU(h) sit in the other staging buffer.  Waves 0-3 run phase 1 first, waves 4-7 phase 2
  // first: the two waves of a SIMD are then in different phases and one's activation VALU work runs under the other's MFMAs.
  // The dh (and GELU(h)) stores of a stage are issued behind the NEXT barrier, ahead of that interval's DMA: a wave then has
  // nothing younger than the DMA in its vector-memory queue and the wait at the top is exact.
  const bool p2_first = wid >= 4;
  u32x4 hq1[3], hp2[3];                        // xn2 / dY image fragments of the stage whose phase 2 is pending
  uint4 dh_hold = make_uint4(0u, 0u, 0u, 0u), ha_hold = dh_hold;
  int r_hold = nrows;                         // row of the held dh / GELU(h) chunk (nrows: nothing held)

  auto phase1 = [&](const int s, const uint32_t so, const uint32_t st) {
    f32x4 h0 = f32x4{0.f, 0.f, 0.f, 0.f}, h1 = h0, d0 = h0, d1 = h0;
    // group G = contraction steps 2 G (a) and 2 G + 1 (b), K ascending: twelve fragment reads, eight MFMAs
#define MB_P1(G)                                                                                                  \
    {                                                                                                             \
      const u32x4 fxa = mb_rd128<128 * (G)>(aRd0 + so), fxb = mb_rd128<128 * (G)>(aRd1 + so);                      \
      const u32x4 fya = mb_rd128<128 * (G) + MB_IMG>(aRd0 + so), fyb = mb_rd128<128 * (G) + MB_IMG>(aRd1 + so);    \
      const u32x4 w1a0 = mb_rd128<128 * (G)>(wRd0), w1a1 = mb_rd128<128 * (G) + 4 * MB_ROWB>(wRd0);                \
      const u32x4 w1b0 = mb_rd128<128 * (G)>(wRd1), w1b1 = mb_rd128<128 * (G) + 4 * MB_ROWB>(wRd1);                \
      const u32x4 w2a0 = mb_rd128<128 * (G) + MB_WIMG>(wRd0), w2a1 = mb_rd128<128 * (G) + MB_WIMG + 4 * MB_ROWB>(wRd0); \
      const u32x4 w2b0 = mb_rd128<128 * (G) + MB_WIMG>(wRd1), w2b1 = mb_rd128<128 * (G) + MB_WIMG + 4 * MB_ROWB>(wRd1); \
      MB_LGKM0();                                                                                                 \
      mb_mma(h0, w1a0, fxa); mb_mma(h1, w1a1, fxa); mb_mma(d0, w2a0, fya); mb_mma(d1, w2a1, fya);                 \
      mb_mma(h0, w1b0, fxb); mb_mma(h1, w1b1, fxb); mb_mma(d0, w2b0, fyb); mb_mma(d1, w2b1, fyb);                 \
    }
    MB_P1(0) MB_P1(1) MB_P1(2)
#undef MB_P1
    // lane (fg, fr): row 16 u + fr of the stage, hidden columns ocol .. ocol + 7 (tile 0: + 0..3, tile 1: + 4..7)
    float h[8], v[8], a[8], x[8];
#pragma unroll
    for (int r = 0; r < 4; ++r) { h[r] = h0[r]; h[4 + r] = h1[r]; v[r] = d0[r]; v[4 + r] = d1[r]; }
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] += bias[j];
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = gelu_sig(h[j]);
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = dgelu_t<bf16>(h[j]);
    unpack<bf16>(pack<bf16>(h), x);           // gelu'(h) as bf16: sodt_gemm_nt parks it in that form between its K halves
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= x[j];
    dh_hold = pack<bf16>(v);
    ha_hold = pack<bf16>(a);
    mb_wr128(stW + st, dh_hold);
    mb_wr128(stW + st + MB_SIMG, ha_hold);
    r_hold = s * MB_ROWS + 16 * pu + fr;
  };
  auto flush = [&]() {                        // the held chunk of the previous stage goes to HBM
    if (p1_wave && r_hold < nrows) {
      *(uint4*)(g.dh + (mbeg + r_hold) * g.lddh + ocol) = dh_hold;
      if (g.hact) *(uint4*)(g.hact + (mbeg + r_hold) * g.ldha + ocol) = ha_hold;
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto phase2 = [&](const uint32_t st) {
    u32x4 fp1[3], fq2[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      fp1[i] = mb_frag_tr<MB_SROWB>(pa1[i] + st);
      fq2[i] = mb_frag_tr<MB_SROWB>(qa2[i] + st);
    }
    MB_LGKM0();
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) mb_mma(acc1[i][j], fp1[i], hq1[j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) mb_mma(acc2[i][j], hp2[i], fq2[j]);
    if (do_b1) {
#pragma unroll
      for (int i = 0; i < 3; ++i) mb_mma(bacc[i], fp1[i], ones);
    }
    if (do_b2) {
#pragma unroll
      for (int i = 0; i < 3; ++i) mb_mma(bacc[i], hp2[i], ones);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto hold_frags = [&](const uint32_t so) {  // (retired by the lgkmcnt(0) at the top of the next interval at the latest)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      hq1[i] = mb_frag_tr<MB_ROWB>(qa1[i] + so);
      hp2[i] = mb_frag_tr<MB_ROWB>(pa2[i] + so);
    }
  };

  issue(0);
  for (int s = 0; s < nsteps; ++s) {
    // DMA(s) is the youngest thing in the wave's vector-memory queue; its staging writes and held fragments retire with it
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const uint32_t so = (s & 1) * MB_STAGE, st = (s & 1) * (2 * MB_SIMG), stp = st ^ (2 * MB_SIMG);
    flush();
    issue((s + 1) & 1);                        // stage s + 1 -> the other slot: last read in interval s - 1 (rows past the slice: zeros)
    if (p2_first && s > 0) phase2(stp);
    if (p1_wave) phase1(s, so, st);
    if (!p2_first && s > 0) phase2(stp);
    hold_frags(so);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");     // (the tail DMA must land before the LDS is released)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  flush();
  phase2(((nsteps - 1) & 1) * (2 * MB_SIMG));

  // acc1[i][j][r]: dW1 row n = 96 slab + 48 wr1 + 16 i + 4 fg + r, column k = 48 wc1 + 16 j + fr
  // acc2[i][j][r]: dW2 row c = 48 wr2 + 16 i + 4 fg + r, column n = 96 slab + 48 wc2 + 16 j + fr
  const int n1 = MB_SL * slab + 48 * wr1 + 4 * fg, k1 = 48 * wc1 + fr;
  const int c2 = 48 * wr2 + 4 * fg, n2 = MB_SL * slab + 48 * wc2 + fr;
  if (partial) {
    float* p1 = partial + (long)split * MB_TILE + (long)n1 * MB_C + k1;
    float* p2 = partial + ((long)g.splits + split) * MB_TILE + (long)c2 * MB_H + n2;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          p1[(16 * i + r) * MB_C + 16 * j] = acc1[i][j][r];
          p2[(16 * i + r) * MB_H + 16 * j] = acc2[i][j][r];
        }
  } else {
    float* d1 = g.dW1 + (long)n1 * g.lddw1 + k1;
    float* d2 = g.dW2 + (long)c2 * g.lddw2 + n2;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          atomicAdd(d1 + (long)(16 * i + r) * g.lddw1 + 16 * j, acc1[i][j][r]);
          atomicAdd(d2 + (long)(16 * i + r) * g.lddw2 + 16 * j, acc2[i][j][r]);
        }
  }
  if (fr == 0) {                     // bacc[i][r]: row 4 fg + r of unit i, all columns equal
    if (do_b1) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (bpartial) bpartial[(long)split * MB_H + n1 + 16 * i + r] = bacc[i][r];
          else atomicAdd(g.db1 + n1 + 16 * i + r, bacc[i][r]);
        }
    }
    if (do_b2) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (bpartial) bpartial[(long)g.splits * MB_H + (long)split * MB_C + c2 + 16 * i + r] = bacc[i][r];
          else atomicAdd(g.db2 + c2 + 16 * i + r, bacc[i][r]);
        }
    }
  }
}

// dW1, dW2 (and db1, db2) += the sum over the live slices of their partial tiles (rows): 64 float4 columns per workgroup, the
// slices dealt over its four waves in a fixed order and combined through LDS in a fixed order - linbwd_reduce_kernel's order,
// here for four outputs of two row widths in one launch.  Blocks [0, 576) dW1, [576, 1152) dW2, then 3 of db1 and 1 of db2.
constexpr int MB_RBLK = (int)(MB_TILE / 4 / 64);       // 576 blocks per weight

__global__ __launch_bounds__(256) void mlpbwd_reduce_kernel(const float* __restrict__ partial, const float* __restrict__ bpartial,
                                                           int splits, int live, float* __restrict__ dW1, int lddw1,
                                                           float* __restrict__ dW2, int lddw2, float* __restrict__ db1,
                                                           float* __restrict__ db2) {
  __shared__ float4 red[4][64];
  int blk = (int)blockIdx.x;
  const float* src; long slice; int width, ldd; float* dst;
  if (blk < MB_RBLK) { src = partial; slice = MB_TILE; width = MB_C; dst = dW1; ldd = lddw1; }
  else if (blk < 2 * MB_RBLK) { blk -= MB_RBLK; src = partial + (long)splits * MB_TILE; slice = MB_TILE; width = MB_H; dst = dW2; ldd = lddw2; }
  else if (blk < 2 * MB_RBLK + 3) { blk -= 2 * MB_RBLK; src = bpartial; slice = MB_H; width = MB_H; dst = db1; ldd = MB_H; }
  else { blk = 0; src = bpartial + (long)splits * MB_H; slice = MB_C; width = MB_C; dst = db2; ldd = MB_C; }
  const long n4 = slice / 4;
  const int c = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const long i = (long)blk * 64 + c;
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
    const int n = (int)((i * 4) / width);
    float* d = dst + (long)n * ldd + (int)(i * 4 - (long)n * width);
    float4 o = *(float4*)d;
    o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
    *(float4*)d = o;
  }
}

}  // namespace

extern "C" int sodt_mlp_bwd(const void* xn, int ldxn, const void* dY, int ldy, const void* w1, int ldw1, const float* b1,
                            const void* w2T, int ldw2, void* dh, int lddh, void* hact, int ldha, float* dW1, int lddw1, float* db1,
                            float* dW2, int lddw2, float* db2, long M, int C, int splits, float* partial, long partial_floats,
                            int dtype, sodt_stream_t st) {
  if (dtype != SODT_BF16 || C != MB_C || M <= 0 || M > 0x7fffffffL || splits < 1 || splits > 8191) return SODT_EINVAL;
  if (!xn || !dY || !w1 || !b1 || !w2T || !dh || !dW1 || !db1 || !dW2 || !db2) return SODT_EINVAL;
  if ((ldxn % 8) || (ldy % 8) || (ldw1 % 8) || (ldw2 % 8) || (lddh % 8) || (lddw1 % 4) || (lddw2 % 4)) return SODT_EINVAL;
  if (ldxn < MB_C || ldy < MB_C || ldw1 < MB_C || ldw2 < MB_C || lddh < MB_H || lddw1 < MB_C || lddw2 < MB_H) return SODT_EINVAL;
  if ((((uintptr_t)xn) | ((uintptr_t)dY) | ((uintptr_t)w1) | ((uintptr_t)b1) | ((uintptr_t)w2T) | ((uintptr_t)dh) | ((uintptr_t)dW1) |
       ((uintptr_t)db1) | ((uintptr_t)dW2) | ((uintptr_t)db2)) & 15) return SODT_EINVAL;
  if (hact && ((ldha % 8) || ldha < MB_H || (((uintptr_t)hact) & 15))) return SODT_EINVAL;
  // scratch protocol of sodt_linear_bwd_sq for two tiles: splits * 147,456 floats of dW1 partials, as many of dW2 partials; when
  // the scratch also has room for splits * (768 + 192) more, the bias rows go through it too, otherwise they keep their atomics
  const long tile_floats = 2 * (long)splits * MB_TILE;
  const bool use_partial = partial && splits > 1 && tile_floats <= partial_floats && (((uintptr_t)partial) & 15) == 0;
  float* part = use_partial ? partial : nullptr;
  float* bpart = (use_partial && tile_floats + (long)splits * (MB_H + MB_C) <= partial_floats) ? partial + tile_floats : nullptr;
  MlpBwdArgs g;
  g.xn = (const bf16*)xn; g.ldxn = ldxn; g.dY = (const bf16*)dY; g.ldy = ldy; g.w1 = (const bf16*)w1; g.ldw1 = ldw1; g.b1 = b1;
  g.w2T = (const bf16*)w2T; g.ldw2 = ldw2; g.dh = (bf16*)dh; g.lddh = lddh; g.hact = (bf16*)hact; g.ldha = ldha;
  g.dW1 = dW1; g.lddw1 = lddw1; g.db1 = db1; g.dW2 = dW2; g.lddw2 = lddw2; g.db2 = db2; g.M = M; g.splits = splits;
  // eight sibling workgroups per slice, consecutive logical ids
  const int rc = sodt_launch<mlp_bwd_kernel>(dim3((unsigned)(MB_NSLAB * splits)), dim3(512), MB_LDS, (hipStream_t)st, g, part, bpart);
  if (rc || !use_partial) return rc;
  const long rows_per = (((M + splits - 1) / splits) + MB_ROWS - 1) / MB_ROWS * MB_ROWS;
  const int live = (int)((M + rows_per - 1) / rows_per);
  return sodt_launch<mlpbwd_reduce_kernel>(dim3(2 * MB_RBLK + (bpart ? 4 : 0)), dim3(256), 0, (hipStream_t)st, (const float*)part,
                                           (const float*)bpart, splits, live, dW1, lddw1, dW2, lddw2, db1, db2);
}
