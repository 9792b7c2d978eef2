// Fused linear MLP of a Swin block, bf16 (backbone_vit.py:884-890 with the block's residual add of :1128):
//
//     out = resid + fc2( GELU( fc1(xn) ) )          xn, resid, out [M][C];  fc1.weight [4C][C], fc2.weight [C][4C]
//
// ONE launch; the 4C-wide hidden activation never goes to HBM unless the caller asks for it (training: GELU(h) is the operand
// of fc2's weight gradient).  The two-GEMM chain it replaces wrote the hidden tensor once and read it back once in the forward
// alone (805 MB each way per stage-1 block at B=8 @1024^2).
//
// Structure (gfx950, one persistent workgroup of 8 waves per CU):
//   * a workgroup owns a tile of 256 token rows, wave w the rows 32 w .. 32 w + 31; the tile's xn rows sit in LDS for the whole
//     tile (3 K-blocks of [256][64 channels], 96 KB, filled by LDS-DMA, XOR-swizzled on the 16-byte chunk like gemm3.hip's A image;
//     every wave reads only its own rows, so the next tile's rows are requested by the wave itself right after its last fc1 read).
//   * the hidden dimension is walked in 24 slabs of 32 columns.  Per slab: W1 rows [32][192] and W2 columns [192][32] arrive by
//     LDS-DMA in a two-stage ring (12 KB + 12 KB per stage, one raw s_barrier and one counted s_waitcnt vmcnt per slab - the next
//     slab's DMAs and this slab's GELU(h) stores stay in flight across the barrier);
//         h^T (32 x 32 tokens)  = W1slab . xn^T        24 MFMA 16x16x32 per wave, bias b1 as the accumulator's initial value
//         g = GELU(h)                                  in registers; the accumulators of a TRANSPOSED product hold 4 consecutive
//                                                      hidden columns of one token per lane, and with W1's rows fed to the MFMA in the
//                                                      order 8 g + 4 t + r two tiles give a lane 8 consecutive hidden columns: exactly
//                                                      the k-contiguous B operand of the next product (and one 16-byte store of GELU(h))
//         out^T (192 x 32 tokens) += W2slab . g^T      24 MFMA per wave; W2's rows in the same permuted order, so a lane ends with 8
//                                                      consecutive output channels of a token
//   * out^T starts as resid + b2 (the residual rows are loaded at the start of the tile and land under the first slab), and is stored
//     from registers, 16 bytes per lane.
// Fragment reads are inline-asm ds_read_b128 behind counted lgkmcnt waits (hipcc drains vmcnt(0) before any LDS read it can see
// while an LDS-DMA is outstanding).  LDS: 96 KB xn + 2 x 24 KB weights + 3.75 KB biases = 147.75 KB.
//
// Roofline: 16 T C^2 flops over 3 T C 2 B (inference) = 309 GFLOP / 604 MB at stage 1 of B=8 @1024^2: MFMA-bound by AI (512 flop/B);
// with the GELU(h) store (training) 1.41 GB: HBM-priced (0.28 ms at 5 TB/s against 0.12 ms of matrix time).
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int ML_C = 192, ML_H = 768;
constexpr int ML_BM = 256, ML_HS = 32, ML_NSLAB = ML_H / ML_HS;       // 24 slabs
constexpr int ML_XKB = ML_BM * 128;                                    // one K-block of the xn tile: 32 KiB
constexpr int ML_XN = 0;
constexpr int ML_WR = 3 * ML_XKB;                                      // weight ring
constexpr int ML_W1B = 3 * ML_HS * 128;                                // W1 slab: 3 K-blocks x [32 rows][128 B] = 12 KiB
constexpr int ML_W2B = ML_C * 64;                                      // W2 slab: [192 rows][64 B] = 12 KiB
constexpr int ML_WST = ML_W1B + ML_W2B;                                // 24 KiB per stage
constexpr int ML_B1 = ML_WR + 2 * ML_WST;                              // f32 b1[768]
constexpr int ML_B2 = ML_B1 + ML_H * 4;                                // f32 b2[192]
constexpr int ML_LDS = ML_B2 + ML_C * 4;

__device__ uint4 g_mlp_zero[8];                                        // DMA source of the rows beyond M

__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(lds_void*)p; }
template <int OFF> __device__ __forceinline__ u32x4 lds_rd128(uint32_t addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF));
  return v;
}
#define ML_LGKM(N) do { asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define ML_VM(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")

__device__ __forceinline__ f32x4 mma(const u32x4& w, const u32x4& a, const f32x4& c) {
  union { u32x4 u; bf16x8 v; } uw, ua;
  uw.u = w; ua.u = a;
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(uw.v, ua.v, c, 0, 0, 0);
}

// (gelu_sig, the logistic GELU of this kernel, lives in common.h: csrc/mlpbwd.hip recomputes the same activation)
struct MlpArgs {
  const bf16* xn; const bf16* w1; const float* b1; const bf16* w2; const float* b2; const bf16* resid;
  bf16* out; bf16* hact; long M;
};

#ifdef ML_STAMPS     // diagnostic build only (tools/exp/ab_build.sh mlp -DML_STAMPS stamps): shader-cycle sums per wave
__device__ unsigned long long g_mlp_stamps[256 * 8 * 8];
#define ML_T(V) unsigned long long V; do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(V) :: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define ML_ACC(I, A, B) st_sum[I] += (B) - (A)
#else
#define ML_T(V) do {} while (0)
#define ML_ACC(I, A, B) do {} while (0)
#endif

template <bool B> struct BoolC { static constexpr bool value = B; };
template <int I> struct IntC { static constexpr int value = I; };

// SAVE: GELU(h) is also written to hact [M][768] (the training form); RES: a residual operand exists
//
// Schedule of one tile (26 barrier-separated steps k; W1(j) / W2(j) = the slab-j pieces of fc1.weight / fc2.weight):
//     step 0        fc1(0)                                   -> hA                      then out^T = resid + b2
//     step s + 1    fc2(s - 1) | GELU(s) | fc1(s + 1)        s = 0 .. 23 (fc2 from s = 1, fc1 up to s = 22)
//     step 25       fc2(23)                                  then the output stores
// Inside a step the matrix work (fc2 of the PREVIOUS slab, fc1 of the NEXT slab) does not depend on the vector work (GELU of this
// slab): a wave's own stream keeps the matrix pipe and the VALU busy at the same time, and the two waves of a SIMD no longer
// take turns on one pipe (the first version ran fc1 -> GELU -> fc2 per slab with both waves of a SIMD in the same phase: 0.45 ms,
// of which 24 % was exposed GELU - tools/exp ablations, profiles/r05_mlp_ablation.md).  h and g alternate between two register
// sets (A: even slabs, B: odd slabs).  Step k reads ring stage k & 1 (W1(k), W2(k - 2)) and requests W1(k + 1), W2(k - 1) into the
// other stage right after its barrier; every wave issues exactly three DMAs per step (from a zero buffer where a piece does not
// exist), so the counted waits are the same for every wave.
template <bool SAVE, bool RES>
__global__ __launch_bounds__(512) void mlp_fwd_kernel(const MlpArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fi = lane & 15, fg = lane >> 4;
  const uint32_t lbase = lds_addr(dsm);

  for (int i = tid; i < ML_H; i += 512) *(float*)(dsm + ML_B1 + 4 * i) = g.b1[i];
  for (int i = tid; i < ML_C; i += 512) *(float*)(dsm + ML_B2 + 4 * i) = g.b2[i];
  __syncthreads();

  const int ntiles = (int)((g.M + ML_BM - 1) / ML_BM);
  const int G = gridDim.x;
  const int lw = xcd_remap(blockIdx.x, G);
  const int nt_my = lw < ntiles ? (ntiles - lw + G - 1) / G : 0;
  if (nt_my == 0) return;
  const unsigned char* zero = (const unsigned char*)g_mlp_zero + ((lane & 7) << 4);

  // ---- DMA of a tile's xn rows: wave w, piece (kb, q) = rows 32 w + 8 q + (lane >> 3), 128 B of K-block kb per row; the LDS
  //      image is lane-linear, the swizzle (chunk ^ ((row >> 1) & 7)) sits on the SOURCE chunk
  auto issue_xn = [&](int tile) {
    const long m0 = (long)tile * ML_BM;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 32 * wid + 8 * q + (lane >> 3);
      const int cs = (lane & 7) ^ (4 * (q & 1) + ((lane >> 4) & 3));
      const long m = m0 + row;
      const unsigned char* src = m < g.M ? (const unsigned char*)(g.xn + m * ML_C) + (cs << 4) : zero;
      const int kstep = m < g.M ? 128 : 0;
#pragma unroll
      for (int kb = 0; kb < 3; ++kb)
        __builtin_amdgcn_global_load_lds((glb_void*)(src + kb * kstep), (lds_void*)(dsm + ML_XN + kb * ML_XKB + (32 * wid + 8 * q) * 128), 16, 0, 0);
    }
  };
  // ---- the three DMAs of a step into ring stage st: waves 0-3 bring W1(s1) (rows 8 w .. 8 w + 7 of the slab, one 1-KiB piece per
  //      K-block), waves 4-7 bring W2(s2) (three pieces of 16 rows x 64 B); a slab index < 0 = the piece does not exist (zeros)
  const int w1row = 8 * (wid & 3) + (lane >> 3);
  const int w1cs = (lane & 7) ^ (((lane >> 4) & 1) | ((wid & 3) << 1));           // f(row) = ((row >> 1) & 1) | (((row >> 3) & 3) << 1)
  const unsigned char* w1src = (const unsigned char*)(g.w1 + (long)w1row * ML_C) + (w1cs << 4);
  const int w2row = 48 * (wid & 3) + (lane >> 2);                                   // + 16 q
  auto issue_w = [&](int s1, int s2, int st) {
    if (wid < 4) {
      const unsigned char* p = s1 >= 0 ? w1src + (long)s1 * (ML_HS * ML_C * 2) : zero;
      const int kstep = s1 >= 0 ? 128 : 0;
#pragma unroll
      for (int kb = 0; kb < 3; ++kb)
        __builtin_amdgcn_global_load_lds((glb_void*)(p + kb * kstep), (lds_void*)(dsm + ML_WR + st * ML_WST + kb * (ML_HS * 128) + (wid & 3) * 1024), 16, 0, 0);
    } else {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const int row = w2row + 16 * q;
        const int cs = (lane & 3) ^ ((row >> 3) & 2);
        const unsigned char* p = s2 >= 0 ? (const unsigned char*)(g.w2 + (long)row * ML_H + s2 * ML_HS) + (cs << 4) : zero;
        __builtin_amdgcn_global_load_lds((glb_void*)p, (lds_void*)(dsm + ML_WR + st * ML_WST + ML_W1B + (48 * (wid & 3) + 16 * q) * 64), 16, 0, 0);
      }
    }
  };

  // ---- fragment read addresses (lane parts)
  const int fA = (fi >> 1) & 7;
  const int fW = ((fi >> 1) & 1) | (((fi >> 2) & 3) << 1);
  const int prow = 8 * (fi >> 2) + (fi & 3);                                        // permuted weight row of the lane (+ 4 t)
  const uint32_t xb0 = lbase + ML_XN + (32 * wid + fi) * 128 + ((fg ^ fA) << 4);
  const uint32_t xb1 = lbase + ML_XN + (32 * wid + fi) * 128 + (((4 + fg) ^ fA) << 4);
  const uint32_t w1b0 = lbase + ML_WR + prow * 128 + ((fg ^ fW) << 4);
  const uint32_t w1b1 = lbase + ML_WR + prow * 128 + (((4 + fg) ^ fW) << 4);
  const uint32_t w2b = lbase + ML_WR + ML_W1B + prow * 64 + ((fg ^ ((fi >> 2) & 2)) << 4);
  const uint32_t b1a = lbase + ML_B1 + 32 * fg;
  const uint32_t b2a = lbase + ML_B2 + 32 * fg;

  f32x4 out[6][2][2];               // [32-channel group p][tile tt][token tile u]: channel 32 p + 8 fg + 4 tt + r of token 16 u + fi
  f32x4 hA[2][2], hB[2][2];         // h^T of the even / odd slabs: [tile t][token tile u], hidden column 32 s + 8 fg + 4 t + r
  u32x4 gA[2], gB[2];               // GELU(h) of the even / odd slabs, packed: the B operand of fc2, [token tile u]

#ifdef ML_STAMPS
  unsigned long long st_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
  issue_xn(lw);
  issue_w(0, -1, 0);
  for (int ord = 0; ord < nt_my; ++ord) {
    const int tile = lw + ord * G;
    const long m0 = (long)tile * ML_BM;
    const bool has_next = ord + 1 < nt_my;
    const bool partial = m0 + ML_BM > g.M;                 // only the last tile: its stores may be skipped, so waits assume none
    const long tok0 = m0 + 32 * wid + fi;                   // token of u = 0; u = 1: + 16
    const bool ok0 = tok0 < g.M, ok1 = tok0 + 16 < g.M;
    const long tk0 = ok0 ? tok0 : g.M - 1, tk1 = ok1 ? tok0 + 16 : g.M - 1;          // clamped: loads stay in bounds
    // residual rows of the tile (plain loads: hipcc waits for them where out^T is initialised, at the end of step 0)
    uint4 pre[6][2];
    if (RES) {
#pragma unroll
      for (int p = 0; p < 6; ++p) {
        pre[p][0] = *(const uint4*)(g.resid + tk0 * ML_C + 32 * p + 8 * fg);
        pre[p][1] = *(const uint4*)(g.resid + tk1 * ML_C + 32 * p + 8 * fg);
      }
    }
    // GELU(h) rows of this wave: a wave-uniform base (scalar registers) + one 32-bit lane offset
    unsigned char* hbase = SAVE ? (unsigned char*)(g.hact + (m0 + 32 * wid) * ML_H) : nullptr;
    const uint32_t hoff = (uint32_t)(fi * ML_H + 8 * fg) * 2;

    // One step's work.  FC2: out^T += W2(s - 1) . gin;  GELU: gout = GELU(hin) (slab s; stored when SAVE);  FC1: hout = W1(s + 1) . xn^T
    // + b1.  ST = the ring stage read (compile-time).  Fragment reads run one MFMA group ahead of their use (counted lgkmcnt); the
    // GELU of one accumulator pair sits behind each MFMA group of four.
    auto step = [&](auto fc2_c, auto gelu_c, auto fc1_c, auto st_c, const int s, f32x4 (&hin)[2][2], f32x4 (&hout)[2][2],
                    u32x4 (&gin)[2], u32x4 (&gout)[2]) {
      constexpr bool FC2 = decltype(fc2_c)::value, GELU = decltype(gelu_c)::value, FC1 = decltype(fc1_c)::value;
      constexpr int SO = decltype(st_c)::value * ML_WST;
      constexpr int NSLOT = (FC2 ? 6 : 0) + (FC1 ? 6 : 0);
      // GELU of accumulator pair P (u = P >> 2, t = (P >> 1) & 1, registers 2 (P & 1), + 1) -> one dword of gout[u]
      auto pair = [&](auto pc) {
        constexpr int P = decltype(pc)::value, U = P >> 2, T = (P >> 1) & 1, R0 = 2 * (P & 1), WD = 2 * T + (P & 1);
#ifdef ML_ABL_NOGELU          // (timing ablations of tools/exp/ab_build.sh builds only)
        const uint32_t w = pack2bf(hin[T][U][R0], hin[T][U][R0 + 1]);
#else
        const uint32_t w = pack2bf(gelu_sig(hin[T][U][R0]), gelu_sig(hin[T][U][R0 + 1]));
#endif
        if constexpr (WD == 0) gout[U].x = w; else if constexpr (WD == 1) gout[U].y = w; else if constexpr (WD == 2) gout[U].z = w; else gout[U].w = w;
        if constexpr (SAVE && (P & 3) == 3) {
          if (U == 0 ? ok0 : ok1)
            *(uint4*)(hbase + (hoff + (uint32_t)(U * 16 * ML_H * 2 + s * ML_HS * 2))) = make_uint4(gout[U].x, gout[U].y, gout[U].z, gout[U].w);
        }
      };
      // vector work of MFMA-group slot I: 12 slots -> one pair each in the first eight; 6 slots -> two pairs each in the first four
      auto vslot = [&](auto ic) {
        constexpr int I = decltype(ic)::value;
        if constexpr (GELU) {
          if constexpr (NSLOT == 12) { if constexpr (I < 8) pair(IntC<I>{}); }
          else if constexpr (I < 4) { pair(IntC<2 * I>{}); pair(IntC<2 * I + 1>{}); }
        }
      };
      u32x4 a0, a1, c0, c1;                       // fc2 fragments, two sets
      u32x4 wa0, wa1, xa0, xa1, wb0, wb1, xc0, xc1, bb0, bb1;     // fc1 fragments, two sets; b1 of the slab
#define ML_RD2(A0, A1, P) A0 = lds_rd128<(P) * 2048 + SO>(w2b); A1 = lds_rd128<(P) * 2048 + 256 + SO>(w2b);
#define ML_MM2(A0, A1, P)                                                                           \
      out[P][0][0] = mma(A0, gin[0], out[P][0][0]); out[P][0][1] = mma(A0, gin[1], out[P][0][1]);   \
      out[P][1][0] = mma(A1, gin[0], out[P][1][0]); out[P][1][1] = mma(A1, gin[1], out[P][1][1]);
#define ML_RD1(W0, W1, X0, X1, KB, WB, XB, XO)                                                      \
      W0 = lds_rd128<(KB) * 4096 + SO>(WB); W1 = lds_rd128<(KB) * 4096 + 512 + SO>(WB);             \
      X0 = lds_rd128<XO>(XB); X1 = lds_rd128<XO + 2048>(XB);
#define ML_MM1(W0, W1, X0, X1)                                                                      \
      hout[0][0] = mma(W0, X0, hout[0][0]); hout[0][1] = mma(W0, X1, hout[0][1]);                   \
      hout[1][0] = mma(W1, X0, hout[1][0]); hout[1][1] = mma(W1, X1, hout[1][1]);
      // first reads of the fc1 part: b1 of slab s + 1 and the first 32-channel step
#define ML_RD1_FIRST()                                                                              \
      bb0 = lds_rd128<0>(b1a + 128 * (s + 1)); bb1 = lds_rd128<16>(b1a + 128 * (s + 1));            \
      ML_RD1(wa0, wa1, xa0, xa1, 0, w1b0, xb0, 0)
      constexpr int F1 = FC2 ? 6 : 0;             // slot number of the first fc1 group
      if constexpr (FC2) {
        ML_RD2(a0, a1, 0)
        ML_RD2(c0, c1, 1)
        ML_LGKM(2);
        ML_MM2(a0, a1, 0) vslot(IntC<0>{});
        ML_RD2(a0, a1, 2)
        ML_LGKM(2);
        ML_MM2(c0, c1, 1) vslot(IntC<1>{});
        ML_RD2(c0, c1, 3)
        ML_LGKM(2);
        ML_MM2(a0, a1, 2) vslot(IntC<2>{});
        ML_RD2(a0, a1, 4)
        ML_LGKM(2);
        ML_MM2(c0, c1, 3) vslot(IntC<3>{});
        ML_RD2(c0, c1, 5)
        ML_LGKM(2);
        ML_MM2(a0, a1, 4) vslot(IntC<4>{});
        if constexpr (FC1) { ML_RD1_FIRST() ML_LGKM(6); } else { ML_LGKM(0); }
        ML_MM2(c0, c1, 5) vslot(IntC<5>{});
      } else if constexpr (FC1) {
        ML_RD1_FIRST()
      }
      if constexpr (FC1) {
        ML_RD1(wb0, wb1, xc0, xc1, 0, w1b1, xb1, 0)
        ML_LGKM(4);
        {
          f32x4 z0, z1;
          z0[0] = __uint_as_float(bb0.x); z0[1] = __uint_as_float(bb0.y); z0[2] = __uint_as_float(bb0.z); z0[3] = __uint_as_float(bb0.w);
          z1[0] = __uint_as_float(bb1.x); z1[1] = __uint_as_float(bb1.y); z1[2] = __uint_as_float(bb1.z); z1[3] = __uint_as_float(bb1.w);
          hout[0][0] = mma(wa0, xa0, z0); hout[0][1] = mma(wa0, xa1, z0);
          hout[1][0] = mma(wa1, xa0, z1); hout[1][1] = mma(wa1, xa1, z1);
        }
        vslot(IntC<F1 + 0>{});
        ML_RD1(wa0, wa1, xa0, xa1, 1, w1b0, xb0, 32768)
        ML_LGKM(4);
        ML_MM1(wb0, wb1, xc0, xc1) vslot(IntC<F1 + 1>{});
        ML_RD1(wb0, wb1, xc0, xc1, 1, w1b1, xb1, 32768)
        ML_LGKM(4);
        ML_MM1(wa0, wa1, xa0, xa1) vslot(IntC<F1 + 2>{});
        ML_RD1(wa0, wa1, xa0, xa1, 2, w1b0, xb0 + 32768, 32768)
        ML_LGKM(4);
        ML_MM1(wb0, wb1, xc0, xc1) vslot(IntC<F1 + 3>{});
        ML_RD1(wb0, wb1, xc0, xc1, 2, w1b1, xb1 + 32768, 32768)
        ML_LGKM(4);
        ML_MM1(wa0, wa1, xa0, xa1) vslot(IntC<F1 + 4>{});
        ML_LGKM(0);
        ML_MM1(wb0, wb1, xc0, xc1) vslot(IntC<F1 + 5>{});
      }
#undef ML_RD2
#undef ML_MM2
#undef ML_RD1
#undef ML_MM1
#undef ML_RD1_FIRST
    };
    // top of a step: the DMAs requested one step ago have landed for every wave
#define ML_TOP() do { __builtin_amdgcn_s_barrier(); asm volatile("" ::: "memory"); } while (0)
    constexpr BoolC<true> Y{};
    constexpr BoolC<false> N{};

    // ---- step 0: fc1(0).  In flight behind the awaited DMAs: the residual loads; after the first tile also the previous tile's
    //      12 output stores (that tile was complete: only the last tile can be partial)
    if (ord == 0) { if (RES) ML_VM(12); else ML_VM(0); }
    else { if (RES) ML_VM(24); else ML_VM(12); }
    ML_TOP();
    issue_w(1, -1, 1);
    step(N, N, Y, IntC<0>{}, -1, hA, hA, gA, gA);
    // out^T = resid + b2
#pragma unroll
    for (int p = 0; p < 6; ++p) {
      const u32x4 c0 = lds_rd128<0>(b2a + 128 * p), c1 = lds_rd128<16>(b2a + 128 * p);
      ML_LGKM(0);
      const float bz[8] = {__uint_as_float(c0.x), __uint_as_float(c0.y), __uint_as_float(c0.z), __uint_as_float(c0.w),
                           __uint_as_float(c1.x), __uint_as_float(c1.y), __uint_as_float(c1.z), __uint_as_float(c1.w)};
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float x[8];
        if (RES) unpack<bf16>(pre[p][u], x);
        else { for (int j = 0; j < 8; ++j) x[j] = 0.f; }
#pragma unroll
        for (int r = 0; r < 4; ++r) { out[p][0][u][r] = x[r] + bz[r]; out[p][1][u][r] = x[4 + r] + bz[4 + r]; }
      }
    }
    // ---- step 1 (slab 0): GELU(0) | fc1(1)
    ML_VM(0);
    ML_TOP();
    issue_w(2, 0, 0);
    step(N, Y, Y, IntC<1>{}, 0, hA, hB, gA, gA);
    // ---- steps 2 .. 23 (slabs 1 .. 22), two per iteration: the register sets and the ring stage alternate
#pragma unroll 1
    for (int s = 1; s < ML_NSLAB - 2; s += 2) {
      ML_T(t0);
      if (SAVE && !partial) ML_VM(2); else ML_VM(0);
      ML_T(t1);
      ML_TOP();
      ML_T(t2);
      issue_w(s + 2, s, 1);
      ML_T(t3);
      step(Y, Y, Y, IntC<0>{}, s, hB, hA, gA, gB);
      ML_T(t4);
      ML_ACC(0, t0, t1); ML_ACC(1, t1, t2); ML_ACC(2, t2, t3); ML_ACC(3, t3, t4);
      if (SAVE && !partial) ML_VM(2); else ML_VM(0);
      ML_T(t5);
      ML_TOP();
      ML_T(t6);
      issue_w(s + 3 < ML_NSLAB ? s + 3 : -1, s + 1, 0);
      ML_T(t7);
      step(Y, Y, Y, IntC<1>{}, s + 1, hA, hB, gB, gA);
      ML_T(t8);
      ML_ACC(0, t4, t5); ML_ACC(1, t5, t6); ML_ACC(2, t6, t7); ML_ACC(3, t7, t8);
    }
    // the wave's xn rows are dead after fc1(23): request the next tile's
    if (has_next) issue_xn(tile + G);
    // ---- step 24 (slab 23): fc2(22) | GELU(23)
    if (has_next) { if (SAVE) ML_VM(14); else ML_VM(12); }
    else if (SAVE && !partial) ML_VM(2);
    else ML_VM(0);
    ML_TOP();
    issue_w(-1, ML_NSLAB - 1, 1);
    step(Y, Y, N, IntC<0>{}, ML_NSLAB - 1, hB, hB, gA, gB);
    // ---- step 25: fc2(23)
    if (SAVE && !partial) ML_VM(2); else ML_VM(0);
    ML_TOP();
    issue_w(has_next ? 0 : -1, -1, 0);
    step(Y, N, N, IntC<1>{}, ML_NSLAB, hA, hA, gB, gB);
#undef ML_TOP
    // ---- the tile's output rows, from registers: 8 consecutive channels per lane and group
#pragma unroll
    for (int p = 0; p < 6; ++p)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) { v[r] = out[p][0][u][r]; v[4 + r] = out[p][1][u][r]; }
        const long tok = tok0 + 16 * u;
        if (tok < g.M) *(uint4*)(g.out + tok * ML_C + 32 * p + 8 * fg) = pack<bf16>(v);
      }
  }
  ML_VM(0);
#ifdef ML_STAMPS
  if (lane == 0)
    for (int i = 0; i < 8; ++i) g_mlp_stamps[(blockIdx.x * 8 + wid) * 8 + i] = st_sum[i];
#endif
}

template <bool SAVE, bool RES> int launch_mlp(const MlpArgs& a, hipStream_t st) {
  const long ntiles = (a.M + ML_BM - 1) / ML_BM;
  const int grid = (int)(ntiles < 256 ? ntiles : 256);
  return sodt_launch<mlp_fwd_kernel<SAVE, RES>>(dim3(grid), dim3(512), ML_LDS, st, a);
}

}  // namespace

extern "C" int sodt_mlp_fwd(const void* xn, const void* w1, const float* b1, const void* w2, const float* b2, const void* resid,
                            void* out, void* hact, long M, int C, int dtype, sodt_stream_t st_) {
  hipStream_t st = (hipStream_t)st_;
  if (!xn || !w1 || !b1 || !w2 || !b2 || !out || M <= 0 || C <= 0 || (C % 8) != 0) return SODT_EINVAL;
  if (dtype == SODT_F32 || C != ML_C) {
    // the parity path (and widths the fused kernel is not built for): the two-GEMM chain through the caller's hidden buffer
    if (!hact) return SODT_EINVAL;
    const int H4 = 4 * C;
    sodt_gemm_args g1 = {};
    g1.a.nseg = 1; g1.a.spatial = 0; g1.a.Ho = 1; g1.a.Wo = 1;
    g1.a.s[0].p = xn; g1.a.s[0].ld = C; g1.a.s[0].klen = C; g1.a.s[0].mul = 1;
    g1.W = w1; g1.ldw = C; g1.C = hact; g1.ldc = H4; g1.bias = b1;
    g1.M = (int)M; g1.N = H4; g1.K = C; g1.flags = SODT_EPI_BIAS | SODT_EPI_GELU;
    int rc = sodt_gemm_nt(&g1, dtype, st_);
    if (rc != SODT_OK) return rc;
    sodt_gemm_args g2 = {};
    g2.a.nseg = 1; g2.a.spatial = 0; g2.a.Ho = 1; g2.a.Wo = 1;
    g2.a.s[0].p = hact; g2.a.s[0].ld = H4; g2.a.s[0].klen = H4; g2.a.s[0].mul = 1;
    g2.W = w2; g2.ldw = H4; g2.C = out; g2.ldc = C; g2.bias = b2;
    g2.R = resid; g2.ldr = C;
    g2.M = (int)M; g2.N = C; g2.K = H4; g2.flags = SODT_EPI_BIAS | (resid ? SODT_EPI_RESID : 0);
    return sodt_gemm_nt(&g2, dtype, st_);
  }
  if (dtype != SODT_BF16) return SODT_EINVAL;
  if ((((uintptr_t)xn | (uintptr_t)w1 | (uintptr_t)w2 | (uintptr_t)out | (uintptr_t)resid | (uintptr_t)hact) & 15) ||
      (((uintptr_t)b1 | (uintptr_t)b2) & 3))
    return SODT_EINVAL;
  MlpArgs a;
  a.xn = (const bf16*)xn; a.w1 = (const bf16*)w1; a.b1 = b1; a.w2 = (const bf16*)w2; a.b2 = b2; a.resid = (const bf16*)resid;
  a.out = (bf16*)out; a.hact = (bf16*)hact; a.M = M;
  if (hact) return resid ? launch_mlp<true, true>(a, st) : launch_mlp<true, false>(a, st);
  return resid ? launch_mlp<false, true>(a, st) : launch_mlp<false, false>(a, st);
}

#ifdef ML_STAMPS
extern "C" int sodt_debug_mlp_stamps(unsigned long long* host_256x8x8) {
  return hipMemcpyFromSymbol(host_256x8x8, HIP_SYMBOL(g_mlp_stamps), sizeof(unsigned long long) * 256 * 8 * 8) == hipSuccess ? SODT_OK : SODT_ELAUNCH;
}
#endif
