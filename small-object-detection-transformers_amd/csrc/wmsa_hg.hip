// Fused W-MSA / SW-MSA half of a Swin block for gfx950, bf16 throughput path: FOUR WAVES PER WINDOW.
//
//     x_mid = x + Proj( WindowAttention( LN1(x) ) )          backbone_vit.py:1088-1126, :961-992
//     xn2   = LN2(x_mid)                                     backbone_vit.py:1128 (the MLP's input)
//
// Same contract, parameter pack and saved-tensor layouts as wmsa_block.hip (which stays the f32 parity path); what
// changes is the work decomposition.  wmsa_block.hip gives one wave a whole window: a 24 KB LN1 tile per wave caps the
// workgroup at four waves = ONE wave per SIMD with a 512-register budget, so MFMA, softmax VALU and memory phases of a
// window run back to back and a lone wave issues one VALU instruction per 4 cycles.  Here a workgroup is EIGHT waves
// (two per SIMD, <= 256 registers each) working on TWO windows:
//
//   * the four waves of a window share its LN1 tile in LDS ([64][192] bf16, XOR-swizzled 16-byte chunks) and split the
//     HEADS: at step i = 0, 1, 2 wave j owns head 4 i + j end to end (q^T, k^T, v by MFMA from the shared tile, S^T = K Q^T,
//     relative-position bias from the strip-difference table, -100 shift mask, softmax in registers, O^T = V^T P^T) - the
//     operand chaining of wmsa_block.hip unchanged, nothing of a head ever leaves the wave's registers;
//   * token-major phases (LN1 prologue, residual + LN2 epilogue) split the TOKENS: wave j owns rows 16 j .. 16 j + 15;
//   * the output projection splits the OUTPUT CHANNELS: O^T of the 12 heads meets in the (dead) LN1 tile, wave j computes
//     out^T rows 48 j .. 48 j + 47 against it with the same three-fragment k-loop as the QKV phase, and the result goes
//     back through the tile for the token-major epilogue;
//   * weights: the Wq / Wk / Wv fragments of the four heads of a step (72 KB) sit in ONE LDS buffer shared by both
//     windows, refilled by LDS-DMA (global_load_lds_dwordx4) right after the step's QKV phase - the softmax / PV part of
//     the step hides the copy; Wproj (72 KB, natural k order) goes through the same buffer.  Relative-position tables
//     and q/k/v biases of all 12 heads (26 KB) stay resident.
//   * ~9 workgroup barriers per window pair; every global store drains in the background (counted vmcnt).
//
// LDS: 2 x 24 KB tiles + 72 KB weights + 25.5 KB tables + 3.75 KB vectors = 149.25 KB.
#include "wmsa_common.h"
#include "launch.h"

namespace {

constexpr int HG_TILE = 64 * 384;                       // one window's [64][192] bf16 tile
constexpr int HG_WBUF_OFF = 2 * HG_TILE;                // 49152
constexpr int HG_HEADW = 18432;                         // Wq | Wk | Wv fragments of one head (3 x 6 KB) = 3 Wproj strips
constexpr int HG_WBUF = 4 * HG_HEADW;                   // 73728
constexpr int HG_TAB_OFF = HG_WBUF_OFF + HG_WBUF;       // 122880
constexpr int HG_TABH = 1920 + 256;                     // table (4 shifted copies) + q/k/v bias of one head
constexpr int HG_LNV_OFF = HG_TAB_OFF + WHEADS * HG_TABH;   // 148992: bproj | g1 | b1 | g2 | b2 (f32)
constexpr int HG_LDS_INF = HG_LNV_OFF + 5 * WC * 4, HG_LDS_SAVE = HG_LDS_INF;      // 152832 (both forms)
static_assert(HG_LDS_SAVE <= 160 * 1024, "LDS budget");
static_assert(WL<bf16>::STAGE == 24576 && WL<bf16>::BIAS_OFF == HG_HEADW && WL<bf16>::BQKV_OFF == HG_HEADW + 1920, "pack layout");

// STAMP: diagnostic build (sodt_debug_wmsa_hg_stamps): wave 0 of every workgroup sums shader cycles per phase
__device__ long long g_hg_stamps[512][12];     // rows 0..255: wave 0 (window A, older), 256..511: wave 4 (window B, same SIMD)
__device__ __forceinline__ long long hg_now() {
  long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
// census build (tools/valu_census.py, -DSODT_HG_MARK): phase markers in the assembly, no instruction
#ifdef SODT_HG_MARK
#define HG_MARK(name) asm volatile("; HGMARK " name)
#else
#define HG_MARK(name) do {} while (0)
#endif
#define HG_STAMP(i) do { if constexpr (STAMP) { const long long now_ = hg_now(); acc_st[i] += now_ - last_st; last_st = now_; } } while (0)

template <bool SAVE, bool STAMP = false>
__global__ __launch_bounds__(512, 2) void wmsa_hg_kernel(const WArgs a) {
  typedef bf16 T;
  using L = WL<bf16>;
  constexpr int E = 2, KPL = 8, ROWB = 384;
  typedef uint2 k16_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  lds_u8* const sm3 = (lds_u8*)smem;
  const unsigned smem0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), ww = w >> 2, j = w & 3;
  const int t = lane & 15, g = lane >> 4;
  const unsigned tile = (unsigned)(ww * HG_TILE);
  // fragment addressing into the window's tile (see wmsa_block.hip: chunk c of row r sits at c ^ (r & 7))
  const unsigned gx3 = (unsigned)((g ^ (t & 3)) << 4), swb = (unsigned)(((t >> 2) & 1) * 64);
  const unsigned xrow = tile + (unsigned)(t * ROWB) + gx3;
  const unsigned xfE = smem0 + xrow + swb, xfO = smem0 + xrow - swb;
  const unsigned wb16 = smem0 + HG_WBUF_OFF + (unsigned)(j * HG_HEADW) + (unsigned)(lane * 16);
  // bias-table addressing of this lane (wmsa_block.hip): four consecutive entries at one aligned address, strip difference 0
  const int j0 = 7 - (t & 7) + 4 * (g & 1), jv = j0 & 3;
  const int bias_lane_off = (((jv * 15 + (t >> 3) - (g >> 1) + 7) * 16) + (j0 - jv)) * E;

  // ---- weights: LDS-DMA of 72 one-KB pieces, nine per wave.  stage 0..2: Wq|Wk|Wv fragments of heads 4 s .. 4 s + 3,
  // stage 3: Wproj in natural k order (WL::HGW_OFF)
  const int rot = (int)((blockIdx.x >> 3) * 7 + (blockIdx.x & 7) * 3) % 72;     // (blocks b, b + 8, ... share an XCD: distinct rotations)
  // pieces q0 .. q1 - 1 of this wave's nine: the issue of a 1 KB piece stalls the wave for 100+ cycles while the CU's address
  // path works through the burst, so the nine are spread over the VALU work of the phase that hides the copy
  auto dma_part = [&](int stage, int q0, int q1) {
#ifdef SODT_HG_ABLATE_DMA      // timing-only A/B build (tools/exp/ab_build.sh): never defined in the library build
    return;
#endif
    const unsigned char* gsrc = a.wpk + L::HGW_OFF + (size_t)stage * HG_WBUF;     // the stages are one contiguous stream
#pragma unroll
    for (int q = q0; q < q1; ++q) {
      // (the piece order is rotated per workgroup: every CU streams the same 72 KB, and walking it in the same order at the
      //  same time piles the requests of an XCD's 32 CUs onto one L2 channel after the other)
      int p = w + 8 * q + rot;
      p = p >= 72 ? p - 72 : p;
      const unsigned off = (unsigned)p << 10;
      asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                   :: "v"((unsigned)(lane * 16) + off), "s"(gsrc), "s"(smem0 + HG_WBUF_OFF + off) : "memory", "m0");
    }
  };
  auto dma_w = [&](int stage) { dma_part(stage, 0, 9); };
#define HG_VMWAIT(N) asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory")

  dma_w(0);
  // resident: tables + q/k/v bias of the 12 heads, projection bias, LayerNorm vectors
  for (int i = tid; i < WHEADS * (HG_TABH / 16); i += 512) {
    const int h = i / (HG_TABH / 16), c = i % (HG_TABH / 16);
    ((uint4*)(smem + HG_TAB_OFF + h * HG_TABH))[c] = ((const uint4*)(a.wpk + (size_t)h * L::STAGE + L::BIAS_OFF))[c];
  }
  for (int i = tid; i < 5 * WC / 4; i += 512) ((float4*)(smem + HG_LNV_OFF))[i] = ((const float4*)(a.wpk + L::TAIL_OFF))[i];

  const int npairs = (a.nwin + 1) / 2;
  // Token-major phases (LN1 prologue, attention-output save, residual + LN2 epilogue): EIGHT lanes per token row.  Wave j owns
  // tile rows 16 j .. 16 j + 15 as two half-groups hh = 0, 1 of eight rows; lane (r8 = lane >> 3, c8 = lane & 7) holds chunks
  // c8 + 8 i (i = 0..2) of row 16 j + 8 hh + r8.  One global load / store instruction then moves 8 rows x 128 contiguous bytes -
  // whole cache lines (the 8 tokens of a half-group are one window row: consecutive token rows in memory) - instead of round
  // 3's 16 rows x 64 bytes: half the line requests in the CU's address path for the same bytes.  Register index: 3 hh + i.
  auto row_of = [&](int pair, int hh) {
    int item = 2 * pair + ww;
    if (item >= a.nwin) item = a.nwin - 1;
    const int wx_ = item % a.nwx; item /= a.nwx;
    const int wy_ = item % a.nwy; const int b_ = item / a.nwy;
    return (unsigned)wtoken(a, b_, wy_, wx_, 16 * j + 8 * hh + (lane >> 3));
  };
  uint4 xc[6], xnext[6];      // x of this wave's 16 tokens: the current pair's (LN1 input AND residual) and the next pair's
  if ((int)blockIdx.x < npairs) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const unsigned ro = row_of(blockIdx.x, hh) * (unsigned)ROWB + (unsigned)((lane & 7) * 16);
#pragma unroll
      for (int i = 0; i < 3; ++i) xc[3 * hh + i] = *(const uint4*)(a.x + (ro + 128u * i));
    }
  }
  // Per-lane addresses of the token-major phases, the tile hand-overs and the output rows are re-derived from a LAUNDERED lane
  // id where they are used: as loop invariants they would stay live across the head steps - hipcc spills them - while
  // re-deriving costs a few VALU instructions per window pair.
  // LDS: chunk c of tile row r sits at position c ^ (r & 7) (r & 7 = r8 here): lane base + 8 hh rows + 128 i bytes
#define HG_TOKEN_PTRS()                                                                                   \
  int ll_ = lane; LAUNDER(ll_);                                                                           \
  const int r8 = ll_ >> 3, c8 = ll_ & 7;                                                                  \
  lds_u8* const p_t0 = sm3 + tile + (unsigned)((16 * j + r8) * ROWB) + (unsigned)((c8 ^ r8) << 4);       \
  lds_u8* const p_ln = sm3 + HG_LNV_OFF + c8 * KPL * 4;                                                   \
  const unsigned myrow0 = (unsigned)wtoken(a, b, wy, wx, 16 * j + r8);                                    \
  const unsigned myrow1 = (unsigned)wtoken(a, b, wy, wx, 16 * j + 8 + r8);                                \
  const unsigned myoff0 = myrow0 * (unsigned)ROWB + (unsigned)(c8 * 16);                                  \
  const unsigned myoff1 = myrow1 * (unsigned)ROWB + (unsigned)(c8 * 16)
#define HG_TPTR(hh, i) (p_t0 + (hh) * 8 * ROWB + 128 * (i))
#define HG_GOFF(hh, i) (((hh) ? myoff1 : myoff0) + 128u * (i))
  // bias tables of this wave's heads 4 step + j: one base per lane, the step is an immediate offset
  const unsigned tbl = smem0 + HG_TAB_OFF + (unsigned)(j * HG_TABH);
  const unsigned bb3 = tbl + (unsigned)bias_lane_off - (unsigned)(3 * 2 * 16 * E);
  const unsigned sbg = tbl + 1920u + (unsigned)(16 * g), sbt = tbl + 1920u + (unsigned)(4 * t);
  __syncthreads();
  long long acc_st[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, last_st = 0;
  if constexpr (STAMP) last_st = hg_now();

  for (int it = blockIdx.x; it < npairs; it += gridDim.x) {
    HG_MARK("pair-setup");
    int item = 2 * it + ww;
    const bool valid = item < a.nwin;
    if (!valid) item = a.nwin - 1;
    int tq = item;
    const int wx = tq % a.nwx; tq /= a.nwx;
    const int wy = tq % a.nwy; const int b = tq / a.nwy;
    const bool msk = a.shift > 0 && (wy == a.nwy - 1 || wx == a.nwx - 1);
    const unsigned whoff = (unsigned)item * WHEADS;
    unsigned diffm[4] = {0u, 0u, 0u, 0u};
    if (msk) {
      int kr[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) kr[i] = wrid(a, wy, wx, 16 * (i >> 2) + 4 * g + (i & 3));
#pragma unroll
      for (int ms = 0; ms < 4; ++ms) {
        const int qr = wrid(a, wy, wx, 16 * ms + t);
#pragma unroll
        for (int i = 0; i < 16; ++i) diffm[ms] |= (qr != kr[i] ? 1u : 0u) << i;
      }
    }

    // ================= prologue: LN1 of this wave's 16 tokens -> tile rows 16 j .. 16 j + 15
    HG_MARK("LN1");
    {
      HG_TOKEN_PTRS();
      // x is unpacked once and the statistics are taken in one pass (sum and sum of squares; f32, 192 values of O(1..10): the
      // cancellation in E[x^2] - mean^2 is ~1e-6 relative, far inside bf16's tolerance): 2 VALU slots per element for the
      // statistics and 2 FMAs for the normalisation instead of round 3's three passes
      // x is unpacked once and the statistics are taken in one pass (sum and sum of squares; f32, 192 values of O(1..10): the
      // cancellation in E[x^2] - mean^2 is ~1e-6 relative, far inside bf16's tolerance): 2 VALU slots per element for the
      // statistics and 2 FMAs for the normalisation instead of round 3's three passes
      float f[6][KPL];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          unpack<T>(xc[3 * hh + i], f[3 * hh + i]);
#pragma unroll
          for (int k = 0; k < KPL; ++k) { s += f[3 * hh + i][k]; q = fmaf(f[3 * hh + i][k], f[3 * hh + i][k], q); }
        }
        s = group8_sum(s);
        q = group8_sum(q);
        const float mu = s * (1.0f / WC);
        const float rstd = rsqrtf(fmaxf(q * (1.0f / WC) - mu * mu, 0.f) + 1e-5f);
        const float nmr = -mu * rstd;
        if (SAVE && valid && c8 == 0) *(float2*)((unsigned char*)a.st1 + (hh ? myrow1 : myrow0) * 8u) = make_float2(mu, rstd);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int k = 0; k < KPL; ++k) f[3 * hh + i][k] = fmaf(f[3 * hh + i][k], rstd, nmr);
      }
      wave_sync();                                       // this wave's epilogue reads of the same rows are done
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        float ga[KPL], be[KPL];
#pragma unroll
        for (int k = 0; k < KPL; k += 4) {
          *(f32x4*)(ga + k) = *(const __attribute__((address_space(3))) f32x4*)(p_ln + (WC + 64 * i + k) * 4);
          *(f32x4*)(be + k) = *(const __attribute__((address_space(3))) f32x4*)(p_ln + (2 * WC + 64 * i + k) * 4);
        }
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
#pragma unroll
          for (int k = 0; k < KPL; ++k) f[3 * hh + i][k] = fmaf(f[3 * hh + i][k], ga[k], be[k]);
          const uint4 y = pack<T>(f[3 * hh + i]);
          *(__attribute__((address_space(3))) u32x4_*)HG_TPTR(hh, i) = u32x4_{y.x, y.y, y.z, y.w};
          if (SAVE && valid) *(uint4*)(a.xn1 + HG_GOFF(hh, i)) = y;
        }
      }
    }
    // W(0) was requested before the previous pair's epilogue stores (or at kernel start): everything older than the
    // youngest stores has landed.  The stores themselves stay in flight.
    HG_STAMP(0);
    // The count is the number of store INSTRUCTIONS this wave has issued since that request, all of them under `valid` and none
    // under a lane-dependent branch that could skip the instruction (the c8 == 0 statistics stores keep 8 lanes active):
    //   inference: x_mid 6 + xn2 6 of the previous pair                                                           = 12
    //   training:  LN2 statistics 2 + x_mid 6 + xn2 6 of the previous pair, LN1 statistics 2 + xn1 6 of this pair = 22
    // A smaller number than the stores really in flight only waits longer; a larger one would let QKV read a half-landed weight
    // buffer - tests/test_wmsa_block_gpu.py runs geometries with several pairs per workgroup (and a clamped tail: that wave
    // issued fewer stores and waits for everything) in both forms against the float64 reference.
    if (!SAVE) HG_VMWAIT(12);
    else if (valid) HG_VMWAIT(22);
    else HG_VMWAIT(0);
    __syncthreads();                                     // B1: tiles complete, W(0) visible
    HG_STAMP(1);

    k16_t poall[3][4];
    static_for<0, 3>([&](auto i_) {
      constexpr int step = decltype(i_)::value;
      const int h = 4 * step + j;
      constexpr int TBO = step * 4 * HG_TABH;            // table / bias of head 4 step + j relative to the lane bases
      typedef typename KR<T>::type kreg_t;
      // ---- q^T, k^T (channel rows, token columns) and v (token rows, channel columns) of head h
      HG_MARK("QKV");
      u32x4_ bqr = lds_rd128a<TBO + 192>(sbg), bkr = lds_rd128a<TBO + 64>(sbg);      // (+192: the q bias x hd^-1/2 x log2 e)
      unsigned bvr = lds_rd32a<TBO + 128>(sbt);
      // fragments are single-buffered: the reads of k-step kk + 1 are issued right after the MFMAs of k-step kk (which
      // have taken their operands) and land while those execute; the SIMD's second wave fills what is left of the gap
      u32x4_ wf[3], xf[4];
      auto issue_k = [&](auto kk_) {
        constexpr int kk = decltype(kk_)::value;
        wf[0] = lds_rd128a<0 + kk * 1024>(wb16);
        wf[1] = lds_rd128a<6144 + kk * 1024>(wb16);
        wf[2] = lds_rd128a<12288 + kk * 1024>(wb16);
        static_for<0, 4>([&](auto ms_) {
          constexpr int ms = decltype(ms_)::value;
          xf[ms] = lds_rd128a<ms * 16 * ROWB + 64 * kk>((kk & 1) ? xfO : xfE);
        });
      };
      issue_k(std::integral_constant<int, 0>{});
      k16_t pqs[4], pkk[4], pv[4];
      f32x4 qT[4], kT[4], vv[4];
      static_for<0, 6>([&](auto kk_) {
        constexpr int kk = decltype(kk_)::value;
        LDS_WAIT(0);
        LDS_DEP(wf[0]); LDS_DEP(wf[1]); LDS_DEP(wf[2]);
        LDS_DEP(xf[0]); LDS_DEP(xf[1]); LDS_DEP(xf[2]); LDS_DEP(xf[3]);
        if constexpr (kk == 0) {
          LDS_DEP(bqr); LDS_DEP(bkr); LDS_DEP(bvr);
          const f32x4 bqv = KR<float>::f4(bqr), bkv = KR<float>::f4(bkr);
          const float bvs = __uint_as_float(bvr);
#pragma unroll
          for (int ms = 0; ms < 4; ++ms) { qT[ms] = bqv; kT[ms] = bkv; vv[ms] = f32x4{bvs, bvs, bvs, bvs}; }
        }
        const uint4 wq = u4(wf[0]), wk = u4(wf[1]), wv = u4(wf[2]);
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          const uint4 x4 = u4(xf[ms]);
          mma16<T>(qT[ms], wq, x4);
          mma16<T>(kT[ms], wk, x4);
          mma16<T>(vv[ms], x4, wv);
        }
        if constexpr (kk + 1 < 6) issue_k(std::integral_constant<int, kk + 1>{});
      });
      HG_MARK("QKV-post");
      // the head's bias-table entries (7 x 4 per lane): requested now, used after the hand-over barrier
      kreg_t biar[7];
      static_for<0, 7>([&](auto d_) { constexpr int d = decltype(d_)::value; biar[d] = KR<T>::template rd<TBO + d * 2 * 16 * E>(bb3); });
      // hd^-1/2 x log2 e is folded into the packed Wq / q bias (sodt_wmsa_pack): q^T leaves the MFMAs scaled and S^T ready for exp2
#pragma unroll
      for (int ms = 0; ms < 4; ++ms) {
        pqs[ms] = pk16<T>(qT[ms]);
        pkk[ms] = pk16<T>(kT[ms]); pv[ms] = pk16<T>(vv[ms]);
      }
      HG_STAMP(2);
      __syncthreads();                                   // B2/4/6: everyone is done with the weight buffer (step 2: and the LN1 tile)
      HG_STAMP(3);
      dma_part(step + 1, 0, 3);                          // next heads' weights / Wproj land under the softmax (pieces 3..8: inside it)
      // (training: nothing of q / k / v is saved - the backward, sodt_wmsa_block_bwd, recomputes them from xn1)

      HG_STAMP(4);
      // Softmax of S^T (already in log2 units: bias x log2 e is the accumulator's initial value).  FAST form: no row maximum -
      // softmax is shift invariant and f32 / bf16 carry exp2(s) for |s| < 100 (|score| < 69 nats) without over- or underflow -
      // and the row sums come out of the matrix pipe (an all-ones A operand against the packed P^T the PV product consumes:
      // every accumulator row holds the sum of its query column), so a strip costs 16 v_exp + 8 v_cvt_pk instead of ~100 VALU
      // slots.  A row whose sum leaves [1e-30, 1e30] (or is NaN) sends the WAVE through the EXACT form below (row maximum
      // subtracted, VALU sums: round 3's body) - wave-uniform, no barrier inside; tests force it with large logits.
      auto body = [&](auto MSK_, auto EXACT_) -> bool {
        constexpr bool MSK = decltype(MSK_)::value, EXACT = decltype(EXACT_)::value;
        if constexpr (EXACT) HG_MARK("softmax-exact(cold)"); else if constexpr (MSK) HG_MARK("softmax+PV masked"); else HG_MARK("softmax+PV");
        // ---- S^T = K Q^T: row = key 16 ks + 4 g + r, column = query 16 ms + t; the bias is the accumulator's initial value
        f32x4 bia[7];
        if constexpr (!EXACT) LDS_WAIT(0);
#pragma unroll
        for (int d = 0; d < 7; ++d) { if constexpr (!EXACT) LDS_DEP(biar[d]); bia[d] = KR<T>::f4(biar[d]); }
        k16_t pp[4][4];                                  // P^T strips, packed: [ks][ms]
        float inv[4];
        float lsel = 0.f;
        bool bad = false;
        const uint4 ones = make_uint4(0x3F803F80u, 0x3F803F80u, 0x3F803F80u, 0x3F803F80u);
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          f32x4 s[4];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) { s[ks] = bia[ms - ks + 3]; mmak16(s[ks], pkk[ks], pqs[ms]); }
          if constexpr (MSK) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if ((diffm[ms] >> (4 * ks + r)) & 1u) s[ks][r] += -100.0f * WMSA_LOG2E;
          }
          float sum, lsev;
          if constexpr (EXACT) {
            float mx = -1e30f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
              for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[ks][r]);
            mx = rows_max(mx);
            f32x4 sum4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
              s[ks] = f32x4{__builtin_amdgcn_exp2f(s[ks][0] - mx), __builtin_amdgcn_exp2f(s[ks][1] - mx),
                            __builtin_amdgcn_exp2f(s[ks][2] - mx), __builtin_amdgcn_exp2f(s[ks][3] - mx)};
              sum4 += s[ks];
              pp[ks][ms] = pk16<T>(s[ks]);
            }
            sum = rows_sum((sum4[0] + sum4[1]) + (sum4[2] + sum4[3]));
            lsev = mx * (1.0f / WMSA_LOG2E) + __logf(sum);
          } else {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
              s[ks] = f32x4{__builtin_amdgcn_exp2f(s[ks][0]), __builtin_amdgcn_exp2f(s[ks][1]),
                            __builtin_amdgcn_exp2f(s[ks][2]), __builtin_amdgcn_exp2f(s[ks][3])};
              pp[ks][ms] = pk16<T>(s[ks]);
            }
            f32x4 sa = mma16z<bf16>(ones, make_uint4(pp[0][ms].x, pp[0][ms].y, pp[1][ms].x, pp[1][ms].y));
            mma16<bf16>(sa, ones, make_uint4(pp[2][ms].x, pp[2][ms].y, pp[3][ms].x, pp[3][ms].y));
            sum = sa[0];
            bad |= !(sum > 1e-30f && sum < 1e30f);
            lsev = __logf(sum);
            if (ms < 3) dma_part(step + 1, 3 + 2 * ms, 5 + 2 * ms);       // (issued once: the exact form runs after the fast one)
          }
          inv[ms] = __builtin_amdgcn_rcpf(sum);
          if (SAVE) lsel = g == ms ? lsev : lsel;          // every row group holds the query's sum: group g keeps strip g
        }
        // log-sum-exp of the head's 64 queries: ONE 256-byte store (lane (g, t) <-> query 16 g + t) instead of four 64-byte ones
        if (SAVE && valid) (a.lsew + (size_t)(whoff + h) * 64)[lane] = lsel;
        // ---- O^T = V^T P^T: row = channel 4 g + r, column = query
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kp = 0; kp < 2; ++kp)
            mma16<bf16>(o, make_uint4(pv[2 * kp].x, pv[2 * kp].y, pv[2 * kp + 1].x, pv[2 * kp + 1].y),
                        make_uint4(pp[2 * kp][ms].x, pp[2 * kp][ms].y, pp[2 * kp + 1][ms].x, pp[2 * kp + 1][ms].y));
          o *= inv[ms];
          poall[step][ms] = pk16<T>(o);
        }
        return bad;
      };
      {
        const bool bad = msk ? body(std::true_type{}, std::false_type{}) : body(std::false_type{}, std::false_type{});
        if (__builtin_expect(__ballot(bad) != 0ull, 0)) {
          if (msk) body(std::true_type{}, std::true_type{}); else body(std::false_type{}, std::true_type{});
        }
      }
      HG_STAMP(5);

      HG_MARK("step-end");
      if constexpr (step < 2) {
        HG_VMWAIT(0);                                    // this wave's pieces of the next weights have landed
        __syncthreads();                                 // B3/5
        HG_STAMP(6);
      }
    });

    HG_MARK("O->tile");
    // ================= O^T of this wave's three heads -> the (dead) LN1 tile, now the attention-output tile [64][192]
    // (every wave passed B6 after its last QKV phase: nobody reads LN1 rows any more)
    {
      // head 4 step + j, channels 4 g .. 4 g + 3 of token (ms, t): chunk 2 h + (g >> 1) = 8 step + (2 j + (g >> 1)), stored
      // at chunk ^ (t & 7): the step is a +128-byte immediate
      int ll_ = lane; LAUNDER(ll_);
      const int tl = ll_ & 15, gl = ll_ >> 4;
      lds_u8* const p_ao = sm3 + tile + tl * ROWB + (((2 * j + (gl >> 1)) ^ (tl & 7)) << 4) + 8 * (gl & 1);
#pragma unroll
      for (int step = 0; step < 3; ++step)
#pragma unroll
        for (int ms = 0; ms < 4; ++ms)
          *(__attribute__((address_space(3))) u32x2_*)(p_ao + ms * 16 * ROWB + 128 * step) = u32x2_{poall[step][ms].x, poall[step][ms].y};
    }
    HG_VMWAIT(0);                                        // Wproj has landed
    __syncthreads();                                     // B7: attention-output tiles complete, Wproj visible
    HG_STAMP(7);

    // x rows of the next pair: requested here, ahead of the projection (1.7 - 2.4 K cycles of matrix work cover a good part of
    // the HBM round trip; round 3 requested them next to the W(0) copy after the projection and then sat in the staging phase
    // for ~9 K cycles) and ahead of this phase's stores
    const bool more = it + (int)gridDim.x < npairs;
    {
      const int nx = it + (int)gridDim.x < npairs ? it + (int)gridDim.x : it;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const unsigned ro = row_of(nx, hh) * (unsigned)ROWB + (unsigned)((lane & 7) * 16);
#pragma unroll
        for (int i = 0; i < 3; ++i) xnext[3 * hh + i] = *(const uint4*)(a.x + (ro + 128u * i));
      }
    }
    if (SAVE && valid) {                                 // attention output, natural token order (operand of the dWproj GEMM)
      HG_TOKEN_PTRS();
#pragma unroll
      for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int i = 0; i < 3; ++i)
          *(uint4*)(a.ao + HG_GOFF(hh, i)) = u4((u32x4_)*(const __attribute__((address_space(3))) u32x4_*)HG_TPTR(hh, i));
    }
    HG_MARK("projection");
    // ================= output projection: out^T rows 48 j .. 48 j + 47 (three 16-row strips) x 64 tokens, K = 192
    f32x4 oT[3][4];
    {
      u32x4_ wf[3], xf[4];
      auto issue_k = [&](auto kk_) {
        constexpr int kk = decltype(kk_)::value;
        wf[0] = lds_rd128a<0 + kk * 1024>(wb16);
        wf[1] = lds_rd128a<6144 + kk * 1024>(wb16);
        wf[2] = lds_rd128a<12288 + kk * 1024>(wb16);
        static_for<0, 4>([&](auto ms_) {
          constexpr int ms = decltype(ms_)::value;
          xf[ms] = lds_rd128a<ms * 16 * ROWB + 64 * kk>((kk & 1) ? xfO : xfE);
        });
      };
      // projection bias of this lane's channels 16 (3 j + nl) + 4 g .. + 3: the accumulators' initial value
      int llp = lane; LAUNDER(llp);
      const unsigned pbb = smem0 + HG_LNV_OFF + (unsigned)((48 * j + 4 * (llp >> 4)) * 4);
      u32x4_ pbr[3];
      pbr[0] = lds_rd128a<0>(pbb); pbr[1] = lds_rd128a<64>(pbb); pbr[2] = lds_rd128a<128>(pbb);
      issue_k(std::integral_constant<int, 0>{});
      static_for<0, 6>([&](auto kk_) {
        constexpr int kk = decltype(kk_)::value;
        LDS_WAIT(0);
        LDS_DEP(wf[0]); LDS_DEP(wf[1]); LDS_DEP(wf[2]);
        LDS_DEP(xf[0]); LDS_DEP(xf[1]); LDS_DEP(xf[2]); LDS_DEP(xf[3]);
        if constexpr (kk == 0) {
          LDS_DEP(pbr[0]); LDS_DEP(pbr[1]); LDS_DEP(pbr[2]);
#pragma unroll
          for (int nl = 0; nl < 3; ++nl)
#pragma unroll
            for (int ms = 0; ms < 4; ++ms) oT[nl][ms] = KR<float>::f4(pbr[nl]);
        }
#pragma unroll
        for (int nl = 0; nl < 3; ++nl) {
          const uint4 wa = u4(wf[nl]);
#pragma unroll
          for (int ms = 0; ms < 4; ++ms) mma16<T>(oT[nl][ms], wa, u4(xf[ms]));
        }
        if constexpr (kk + 1 < 6) issue_k(std::integral_constant<int, kk + 1>{});
      });
    }
    HG_STAMP(8);
    __syncthreads();                                     // B8: everyone is done with the attention-output tile and Wproj
    HG_STAMP(9);

    HG_MARK("staging");
    // the first weights of the next pair: requested before the output stores (a load queued behind a store waits for the
    // store's acknowledgement), consumed by the next prologue
    // out^T (+ bias) -> tile, run dtype: the rounding a separate projection launch applies to its output
    {
      int ll_ = lane; LAUNDER(ll_);
      const int tl = ll_ & 15, gl = ll_ >> 4;
      lds_u8* const p_t = sm3 + tile + tl * ROWB + 8 * (gl & 1);
#pragma unroll
      for (int nl = 0; nl < 3; ++nl) {
        if (more) dma_part(0, 3 * nl, 3 * nl + 3);
        const int cw = 2 * (3 * j + nl) + (gl >> 1);
        lds_u8* const p_o = p_t + ((cw ^ (tl & 7)) << 4);
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          const k16_t v = pk16<T>(oT[nl][ms]);
          *(__attribute__((address_space(3))) u32x2_*)(p_o + ms * 16 * ROWB) = u32x2_{v.x, v.y};
        }
      }
    }
    __syncthreads();                                     // B9: output tiles complete
    HG_STAMP(10);

    // ================= epilogue: x_mid = x + (out + bproj), xn2 = LN2(x_mid) for this wave's 16 tokens
    HG_MARK("epilogue");
    {
      HG_TOKEN_PTRS();
      float v[6][KPL];
      uint4 xmp[6];                                      // x_mid in bf16: what is stored, and what LN2 normalises
      float mu2[2], rs2[2];
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          float f[KPL], o[KPL];
          unpack<T>(xc[3 * hh + i], f);                  // residual: the x this wave loaded for LN1, still in registers
          unpack<T>(u4((u32x4_)*(const __attribute__((address_space(3))) u32x4_*)HG_TPTR(hh, i)), o);
          // x_mid is stored in bf16: LN2 normalises the ROUNDED value, as a separate LayerNorm launch reading x_mid would
#pragma unroll
          for (int k = 0; k < KPL; ++k) f[k] += o[k];
          xmp[3 * hh + i] = pack<T>(f);
          unpack<T>(xmp[3 * hh + i], v[3 * hh + i]);
#pragma unroll
          for (int k = 0; k < KPL; ++k) { s += v[3 * hh + i][k]; q = fmaf(v[3 * hh + i][k], v[3 * hh + i][k], q); }
        }
        s = group8_sum(s);
        q = group8_sum(q);
        mu2[hh] = s * (1.0f / WC);
        rs2[hh] = rsqrtf(fmaxf(q * (1.0f / WC) - mu2[hh] * mu2[hh], 0.f) + 1e-5f);
      }
#ifdef SODT_HG_ABLATE_STORES   // timing-only A/B build (tools/exp/ab_build.sh): never defined in the library build
      if (false) {
#else
      if (valid) {
#endif
        if (SAVE && c8 == 0) {
          *(float2*)((unsigned char*)a.st2 + myrow0 * 8u) = make_float2(mu2[0], rs2[0]);
          *(float2*)((unsigned char*)a.st2 + myrow1 * 8u) = make_float2(mu2[1], rs2[1]);
        }
#pragma unroll
        for (int hh = 0; hh < 2; ++hh)
#pragma unroll
          for (int i = 0; i < 3; ++i) *(uint4*)(a.xm + HG_GOFF(hh, i)) = xmp[3 * hh + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          float ga[KPL], be[KPL];
#pragma unroll
          for (int k = 0; k < KPL; k += 4) {
            *(f32x4*)(ga + k) = *(const __attribute__((address_space(3))) f32x4*)(p_ln + (3 * WC + 64 * i + k) * 4);
            *(f32x4*)(be + k) = *(const __attribute__((address_space(3))) f32x4*)(p_ln + (4 * WC + 64 * i + k) * 4);
          }
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) {
            const float nmr = -mu2[hh] * rs2[hh];
#pragma unroll
            for (int k = 0; k < KPL; ++k) v[3 * hh + i][k] = fmaf(fmaf(v[3 * hh + i][k], rs2[hh], nmr), ga[k], be[k]);
            *(uint4*)(a.xn2 + HG_GOFF(hh, i)) = pack<T>(v[3 * hh + i]);
          }
        }
      } else {
        HG_VMWAIT(0);                                    // (no stores were issued: the counted wait of the next prologue must not run short)
      }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) xc[i] = xnext[i];
    HG_STAMP(11);
  }
  HG_MARK("exit");
  HG_VMWAIT(0);
  if constexpr (STAMP) {
    if ((tid == 0 || tid == 256) && blockIdx.x < 256)
      for (int i = 0; i < 12; ++i) g_hg_stamps[blockIdx.x + (tid ? 256 : 0)][i] = acc_st[i];
  }
}

bool g_hg_stamp_enable = false;

template <bool SAVE, bool STAMP = false>
int hg_launch(const WArgs& a, hipStream_t st) {
  constexpr int LDS = SAVE ? HG_LDS_SAVE : HG_LDS_INF;
  const int npairs = (a.nwin + 1) / 2;
  const int grid = npairs < 256 ? npairs : 256;          // one workgroup per CU, persistent over the window pairs
  return sodt_launch<wmsa_hg_kernel<SAVE, STAMP>>(dim3(grid), dim3(512), LDS, st, a);
}

}  // namespace

int wmsa_hg_launch(const WArgs& a, bool save, hipStream_t st) {
  if (g_hg_stamp_enable) return save ? hg_launch<true, true>(a, st) : hg_launch<false, true>(a, st);
  return save ? hg_launch<true>(a, st) : hg_launch<false>(a, st);
}

/* diagnostic hook (tools/mb_wmsa.py --hg-stamps): enable != 0 makes the following bf16 launches run the instrumented build; out
 * (host, 512 x 12 long long, nullable: rows 0..255 wave 0, 256..511 wave 4) receives the per-phase shader-cycle sums of wave 0 of each workgroup of the last such
 * launch: [LN1, B1 wait, QKV, B2/4/6 wait, dma issue + saves, softmax + PV, B3/5 wait, O^T -> tile + B7, projection, B8 wait,
 * residual loads + staging + B9, epilogue] */
extern "C" int sodt_debug_wmsa_hg_stamps(long long* out, int enable) {
  g_hg_stamp_enable = enable != 0;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hg_stamps), sizeof(long long) * 512 * 12) != hipSuccess) return SODT_ELAUNCH;
  return SODT_OK;
}
