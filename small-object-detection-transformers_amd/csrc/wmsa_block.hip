// Fused W-MSA / SW-MSA half of a Swin block for gfx950: one launch computes
//
//     x_mid = x + Proj( WindowAttention( LN1(x) ) )          backbone_vit.py:1088-1126, :961-992
//     xn2   = LN2(x_mid)                                     backbone_vit.py:1128 (the MLP's input)
//
// for C = 192 (12 heads x 16), 8x8 windows, shift 0 or s (stage 1 of model.yaml: backbone_vit.py:117-133).  The input
// is read once and x_mid / xn2 are written once; LayerNorm, the QKV projection, q k^T, relative-position bias, the
// -100 shift mask, softmax, p v, the output projection, bias, residual and the second LayerNorm never touch HBM.
// roll / window_partition / window_unpartition / roll back (:1094-1124, :619-672) are index arithmetic on the global
// loads and stores.  Training additionally writes what the hand-written backward needs (LN1 output, LN statistics,
// q / k / v, log-sum-exp, attention output): see "saved tensors" below.
//
// Work decomposition (wave64, one workgroup per CU, persistent over windows):
//   * ONE WAVE OWNS ONE WINDOW (64 tokens) end to end, so the whole chain is wave-local: no workgroup barrier orders
//     any data flow inside a window.  A workgroup is NWV such waves (4 for bf16, 2 for f32).
//   * The weights (Wqkv 221 KB + Wproj 74 KB in bf16: more than the 160 KB of LDS) are streamed per HEAD: stage h =
//     {Wq_h, Wk_h, Wv_h (48 x 192), Wproj[:, h] (192 x 16), the head's relative-position bias table, its q/k/v
//     bias} = 26 KB, double-buffered in LDS and shared by the NWV windows, i.e. every weight byte crosses
//     L2 -> LDS once per 256 token rows.  The only workgroup barrier is the stage hand-over, once per head.
//     Stages are copied global -> registers -> LDS by all threads while the previous head computes (plain loads:
//     the compiler's own vmcnt bookkeeping keeps them in flight; side-output stores issued later do not delay them).
//   * LN1(x) of the wave's window stays in LDS ([64][192], XOR-swizzled 16-byte chunks: every fragment read is
//     conflict-free) and is the B operand of q^T = Wq xn^T, k^T = Wk xn^T and the A operand of v = xn Wv^T.
//   * Operand chaining without LDS: the 16x16 accumulator of a TRANSPOSED product holds four consecutive channels
//     of one token per lane, which is exactly the k16 operand layout (lane (g, t): k = 4 g + j) of the next MFMA:
//         q^T, k^T accumulators        -> A / B operands of S^T = K Q^T            (v_mfma_f32_16x16x16_bf16)
//         v accumulators (4 tokens of one channel per lane) and P^T = softmax(S^T) -> A / B operands of O^T = V^T P^T
//         O^T accumulators             -> B operand of out^T += Wproj[:, h] O^T    (accumulated over the 12 heads in
//                                         48 accumulator tiles = 192 VGPRs; one wave per SIMD, 512-register budget)
//     The softmax of a query is 16 in-lane values + two cross-group shuffles; 1 / sum is an in-lane scalar of O^T.
//   * Relative-position bias: for 8x8 windows the table entry of (query, key) depends on the 16-token strips only
//     through their difference, so a lane needs 7 x 4 values per head; the stage carries the head's table x log2 e in
//     four 0..3-element-shifted copies so that each group of four is ONE aligned LDS read.
//   * Epilogue: out^T + bias goes through the wave's (now dead) LN1 tile in f32, is read back token-major together
//     with x (coalesced 16-byte chunks), LN2 is computed in registers, x_mid and xn2 leave as 16-byte stores.
//
// Saved tensors (training; all written with full-line coalesced stores from registers, v through a 2 KB patch):
//   xn1 [M][C], ao [M][C] natural token order (operands of the dWqkv / dWproj GEMMs), st1 / st2 [M][2] f32,
//   qkvw [window][head][q|k|v][64 tokens][16]  and  lsew [window][head][64]  in WINDOW-MAJOR order (window =
//   (b * nwy + wy) * nwx + wx after the cyclic shift, token = window-local row-major): the layout the attention
//   backward stages into LDS anyway (sodt_window_attn_bwd_wm), 6 KB contiguous per (window, head).
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"
#include <type_traits>
#include <cstdlib>

#include "wmsa_common.h"

namespace {

// STAMP: diagnostic build (sodt_debug_wmsa_stamps): wave 0 of every workgroup sums shader cycles per phase
__device__ long long g_wmsa_stamps[256][8];
__device__ __forceinline__ long long stamp_now() {
  long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
#define STAMP_TO(i) do { if constexpr (STAMP) { const long long now_ = stamp_now(); acc_st[i] += now_ - last_st; last_st = now_; } } while (0)

template <typename T, int NWV, int NST, bool SAVE, bool STAMP = false>
__global__ __launch_bounds__(NWV * 64, 1) void wmsa_block_kernel(const WArgs a) {
  using L = WL<T>;
  constexpr int E = L::E, KPL = L::KPL, NT = NWV * 64;
  constexpr int NCHK = L::STAGE / 16;                    // 16-byte chunks per stage
  constexpr int NPF = (NCHK + NT - 1) / NT;              // per thread: 7 (bf16, 256 threads) / 26 (f32, 128 threads)
  typedef typename K16<T>::type k16_t;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // smem: LN1 tiles [NWV][64][ROWB] | stages [NST][STAGE] | v patches [NWV][64][16] | proj bias + LayerNorm vectors

  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), t = lane & 15, g = lane >> 4;
  // LDS byte offsets as  per-lane base (one VGPR) + compile-time immediate.  LN1 tile: chunk c = 4 k + g of token row
  // r = 16 ms + t sits at chunk c ^ (r & 7) = 4 (k ^ b) + (g ^ (t & 3)), b = bit 2 of t: even k moves by +64 b bytes,
  // odd k by -64 b, so two bases serve every (ms, k).
  constexpr unsigned SST0 = NWV * L::XNB, SVP0 = SST0 + NST * L::STAGE, SLN0 = SVP0 + NWV * L::VPB;   // SLN0: bproj | g1 | b1 | g2 | b2 (f32)
  const unsigned xnb = (unsigned)(w * L::XNB);
  const unsigned gx3 = (unsigned)((g ^ (t & 3)) << 4);
  const unsigned xrow = xnb + (unsigned)(t * L::ROWB) + gx3, swb = (unsigned)(((t >> 2) & 1) * 64);
  const unsigned smem0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) void*)smem;      // LDS address of the arena
  const unsigned xfE = smem0 + xrow + swb, xfO = smem0 + xrow - swb;
#define XN_ADDR(ms, k) ((((k) & 1) ? xfO : xfE) - smem0 + (unsigned)((ms) * 16 * L::ROWB + 64 * (k)))
  // the same tile as the epilogue's f32 staging area [tokens][192] f32: chunk c4 of row r at c4 ^ (r & 3)
  const unsigned strow = xnb + (unsigned)(t * WC * 4) + gx3;
  const unsigned l16 = (unsigned)(lane * 16), lk16 = (unsigned)(lane * L::K16B);
  const unsigned vpw = SVP0 + (unsigned)(w * L::VPB) + (unsigned)((4 * g * WHD + t) * E);   // + (16 ms + r) * WHD * E
  const unsigned vpr = SVP0 + (unsigned)(w * L::VPB) + l16;
  constexpr bool save = SAVE;          // training build: the save-for-backward outputs (their registers and address math exist only here)
  // proj bias and the two LayerNorms' weight / bias: global -> LDS once per workgroup; lanes read them at
  // lnb + (channel offset of their chunk) with immediates
  for (int i = tid; i < 5 * WC / 4; i += NT) ((float4*)(smem + SLN0))[i] = ((const float4*)(a.wpk + L::TAIL_OFF))[i];
  const unsigned lnb = SLN0 + (unsigned)(g * KPL * 4);    // this lane's first channel inside a 4-chunk group
  const float scale2 = 0.25f * WMSA_LOG2E;               // hd^-1/2 x log2 e
  // compiler-visible LDS accesses go through POINTER bases + constant byte offsets (inbounds pointer arithmetic folds into
  // the DS offset field; `unsigned` sums may wrap, so hipcc materialised - and spilled - one address VGPR per access)
  typedef __attribute__((address_space(3))) unsigned char lds_u8;
  lds_u8* const sm3 = (lds_u8*)smem;
  lds_u8* p_vpw = sm3 + vpw;
  lds_u8* p_vpr = sm3 + vpr;
  // ---- stage copy.  Double-buffered (bf16): LDS-DMA (global_load_lds_dwordx4: no registers, no ds_write), 1 KB per wave
  // instruction, issued right after the hand-over barrier for the NEXT head and waited for (vmcnt) just before the next
  // barrier.  The DMA is inline asm: hipcc does not know a VMEM operation is writing LDS, so it neither waits vmcnt(0)
  // in front of the LDS accesses it can see nor reorders them (memory clobber).  Single-buffered (f32 parity path): a
  // plain copy loop between two barriers.
  static_assert(NST == 1 || NPF == 6, "six 4 KB slices per stage");
#define PF_ISSUE(BUF, STG)                                                              \
  if constexpr (NST == 2) {                                                             \
    const unsigned char* gsrc_ = a.wpk + (unsigned)((STG) * L::STAGE);                  \
    const unsigned ldst_ = smem0 + SST0 + (unsigned)((BUF) * L::STAGE) + (unsigned)(w * 1024); \
    const unsigned voff_ = (unsigned)(tid * 16);                                        \
    _Pragma("unroll") for (int i_ = 0; i_ < NPF; ++i_) {                                \
      if (i_ < NPF - 1 || tid + (NPF - 1) * NT < NCHK)                                  \
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"   \
                     :: "v"(voff_), "s"(gsrc_ + i_ * NT * 16), "s"(ldst_ + (unsigned)(i_ * NT * 16)) : "memory", "m0"); \
    }                                                                                   \
  }
#define PF_WAIT() do { if constexpr (NST == 2) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); } while (0)
  // The stage DMA of head h + 1 is issued at the top of head h, BEFORE that head's save-for-backward stores (q, k: 8, v: 2,
  // lse: 4, attention output: 4 VMEM instructions per wave).  VMEM operations retire in issue order, so "at most
  // NSAVE_KEEP outstanding" means the DMA has landed while the youngest stores stay in flight across the hand-over
  // barrier instead of being waited for (~2K cycles per head).  NSAVE_KEEP is two below the 18 issued: a wait that
  // keeps FEWER operations than were issued after the DMA only over-waits.
  constexpr int NSAVE_KEEP = 16;
  static_assert(8 + L::VPB / 1024 + 4 + 4 >= NSAVE_KEEP + 2 || !SAVE || NST == 1, "stores per head");
#define PF_WAIT_KEEP_STORES(COND) do { if constexpr (NST == 2) {                        \
    if (SAVE && (COND)) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");               \
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); } } while (0)
#define PF_COPY(STG)                                                                    \
  if constexpr (NST == 1) {                                                             \
    const uint4* src_ = (const uint4*)(a.wpk + (unsigned)((STG) * L::STAGE));           \
    uint4* dst_ = (uint4*)(smem + SST0);                                                \
    for (int idx_ = tid; idx_ < NCHK; idx_ += NT) dst_[idx_] = src_[idx_];              \
  }
  PF_ISSUE(0, 0)
  PF_COPY(0)
  int sidx = 0;
  long long acc_st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, last_st = 0;
  if constexpr (STAMP) last_st = stamp_now();

  // bias-table addressing of this lane (see the header): four consecutive entries r = 0..3 at one aligned address
  const int j0 = 7 - (t & 7) + 4 * (g & 1), jv = j0 & 3;
  const int bias_lane_off = L::BIAS_OFF + (((jv * 15 + (t >> 3) - (g >> 1) + 7) * 16) + (j0 - jv)) * E;   // strip difference 0

  const int nquads = (a.nwin + NWV - 1) / NWV;
  // token rows of window-quad `q` for this lane (clamped for the tail): byte offsets of its four token strips
  auto strip_offsets = [&](int q, unsigned* ro, int t, int g) {      // t, g: the caller's (laundered) lane coordinates
    int it_ = q * NWV + w;
    if (it_ >= a.nwin) it_ = a.nwin - 1;
    const int wx_ = it_ % a.nwx; it_ /= a.nwx;
    const int wy_ = it_ % a.nwy; const int b_ = it_ / a.nwy;
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) ro[ms] = (unsigned)wtoken(a, b_, wy_, wx_, 16 * ms + t) * (unsigned)L::ROWB + (unsigned)(g * 16);
  };
  // x of the NEXT window is requested before the current window's output stores (loads and stores retire in issue
  // order per wave: a load behind a store waits for the store's acknowledgement) and lands during the epilogue
  uint4 xc[4][L::CHL];
  if (NST == 2 && (int)blockIdx.x < nquads) {
    unsigned ro[4];
    strip_offsets(blockIdx.x, ro, t, g);
#pragma unroll
    for (int ms = 0; ms < 4; ++ms)
#pragma unroll
      for (int i = 0; i < L::CHL; ++i) xc[ms][i] = *(const uint4*)(a.x + (ro[ms] + 64u * i));
  }
  __syncthreads();                                       // LayerNorm vectors are in LDS
  for (int it = blockIdx.x; it < nquads; it += gridDim.x) {
    int item = it * NWV + w;
    const bool valid = item < a.nwin;
    if (!valid) item = a.nwin - 1;
    int tq = item;
    const int wx = tq % a.nwx; tq /= a.nwx;
    const int wy = tq % a.nwy; const int b = tq / a.nwy;
    const bool msk = a.shift > 0 && (wy == a.nwy - 1 || wx == a.nwx - 1);
    const unsigned whoff = (unsigned)item * WHEADS;       // (window, head 0) index of the window-major tensors
    // bit (4 ks + r) of diffm[ms]: query (ms, t) and key (ks, 4 g + r) lie in different mask regions
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

    // ================= prologue: LN1 of the window -> LDS tile (and xn1 / st1 when saving)
    // Prologue and epilogue re-derive their per-lane addresses from a LAUNDERED lane id: values that stayed live across
    // the head loop would be spilled there and reloaded here through scratch - a VMEM round trip queued behind stores.
    {
      int lane_p = (int)(threadIdx.x & 63);
      LAUNDER(lane_p);
      const int tp = lane_p & 15, gp = lane_p >> 4;
      unsigned prow[4], poff[4];
#pragma unroll
      for (int ms = 0; ms < 4; ++ms) {
        prow[ms] = (unsigned)wtoken(a, b, wy, wx, 16 * ms + tp);
        poff[ms] = prow[ms] * (unsigned)L::ROWB + (unsigned)(gp * 16);
      }
      lds_u8* q_ln = sm3 + SLN0 + gp * KPL * 4;
      const unsigned prow0 = (unsigned)(w * L::XNB + tp * L::ROWB + ((gp ^ (tp & 3)) << 4)), psw = (unsigned)(((tp >> 2) & 1) * 64);
      lds_u8* q_xE = sm3 + prow0 + psw;
      lds_u8* q_xO = sm3 + prow0 - psw;
      if constexpr (NST == 1) {   // parity build: no cross-window prefetch
#pragma unroll
        for (int ms = 0; ms < 4; ++ms)
#pragma unroll
          for (int i = 0; i < L::CHL; ++i) xc[ms][i] = *(const uint4*)(a.x + (poff[ms] + 64u * i));
      }
      float mean[4], rstd[4];
#pragma unroll
      for (int ms = 0; ms < 4; ++ms) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < L::CHL; ++i) {
          float f[KPL];
          unpack<T>(xc[ms][i], f);
#pragma unroll
          for (int j = 0; j < KPL; ++j) s += f[j];
        }
        s = rows_sum(s);
        const float mu = s * (1.0f / WC);
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < L::CHL; ++i) {
          float f[KPL];
          unpack<T>(xc[ms][i], f);
#pragma unroll
          for (int j = 0; j < KPL; ++j) { const float d = f[j] - mu; q = fmaf(d, d, q); }
        }
        q = rows_sum(q);
        mean[ms] = mu;
        rstd[ms] = rsqrtf(q * (1.0f / WC) + 1e-5f);
        if (save && valid && gp == 0) *(float2*)((unsigned char*)a.st1 + prow[ms] * 8u) = make_float2(mu, rstd[ms]);
      }
      wave_sync();                                       // the previous window's epilogue is done with the tile
#pragma unroll
      for (int i = 0; i < L::CHL; ++i) {
        float ga[KPL], be[KPL];
#pragma unroll
        for (int j = 0; j < KPL; j += 4) {
          *(f32x4*)(ga + j) = *(const __attribute__((address_space(3))) f32x4*)(q_ln + (WC + 4 * i * KPL + j) * 4);
          *(f32x4*)(be + j) = *(const __attribute__((address_space(3))) f32x4*)(q_ln + (2 * WC + 4 * i * KPL + j) * 4);
        }
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          float f[KPL];
          unpack<T>(xc[ms][i], f);
#pragma unroll
          for (int j = 0; j < KPL; ++j) f[j] = fmaf((f[j] - mean[ms]) * rstd[ms], ga[j], be[j]);
          const uint4 y = pack<T>(f);
          *(__attribute__((address_space(3))) u32x4_*)(((i & 1) ? q_xO : q_xE) + (ms * 16 * L::ROWB + 64 * i)) = u32x4_{y.x, y.y, y.z, y.w};
          if (save && valid) *(uint4*)(a.xn1 + (poff[ms] + 64u * i)) = y;
        }
      }
      wave_sync();
    }

    STAMP_TO(6);
    // ================= the 12 heads
    // O^T of every head stays packed in registers (one k16 operand per token strip): the output projection contracts
    // over all 192 channels after the loop with full-depth MFMAs, and the head loop runs without the 192 out^T accumulators
    k16_t poall[WHEADS][4];

    for (int h = 0; h < WHEADS; ++h) {
      const int buf = NST == 2 ? (sidx & 1) : 0;
      STAMP_TO(5);
      PF_WAIT_KEEP_STORES(valid && h > 0);               // this wave's slices of stage `buf` have landed
      __syncthreads();                                   // stage `buf` is complete; everyone has left the other buffer
      STAMP_TO(0);
      const unsigned sbo = SST0 + (unsigned)(buf * L::STAGE);      // this head's stage
      const unsigned wb16 = smem0 + sbo + l16;
      const unsigned bb3 = smem0 + sbo + (unsigned)bias_lane_off - (unsigned)(3 * 2 * 16 * E);       // strip difference -3
      const unsigned sbg = smem0 + sbo + (unsigned)(16 * g), sbt = smem0 + sbo + (unsigned)(4 * t);
      PF_ISSUE(buf ^ 1, h + 1)                           // (stage 12 = first projection stage follows head 11)

      auto body = [&](auto MSK_) {
        constexpr bool MSK = decltype(MSK_)::value;
        // ---- q^T, k^T (channel rows, token columns) and v (token rows, channel columns) of this head.
        // LDS issue order: q/k/v bias (3) + table entries (7), fragments of k-step 0 (7), then per k-step the fragments of
        // the next one (7) BEFORE the 12 MFMAs of the current step.
        typedef typename KR<T>::type kreg_t;
        u32x4_ bqr = lds_rd128a<L::BQKV_OFF>(sbg), bkr = lds_rd128a<L::BQKV_OFF + 64>(sbg);
        unsigned bvr = lds_rd32a<L::BQKV_OFF + 128>(sbt);
        kreg_t biar[7];
        static_for<0, 7>([&](auto d_) { constexpr int d = decltype(d_)::value; biar[d] = KR<T>::template rd<d * 2 * 16 * E>(bb3); });
        u32x4_ wf[2][3], xf[2][4];
        auto issue_k = [&](auto kk_) {
          constexpr int kk = decltype(kk_)::value, bsel = kk & 1;
          wf[bsel][0] = lds_rd128a<L::WQ_OFF + kk * 1024>(wb16);
          wf[bsel][1] = lds_rd128a<L::WK_OFF + kk * 1024>(wb16);
          wf[bsel][2] = lds_rd128a<L::WV_OFF + kk * 1024>(wb16);
          static_for<0, 4>([&](auto ms_) {
            constexpr int ms = decltype(ms_)::value;
            xf[bsel][ms] = lds_rd128a<ms * 16 * L::ROWB + 64 * kk>((kk & 1) ? xfO : xfE);
          });
        };
        issue_k(std::integral_constant<int, 0>{});
        k16_t pq[4], pkk[4], pv[4];
        f32x4 qT[4], kT[4], vv[4];
        static_for<0, L::KSTEPS>([&](auto kk_) {
          constexpr int kk = decltype(kk_)::value, bsel = kk & 1;
          if constexpr (kk + 1 < L::KSTEPS) {
            issue_k(std::integral_constant<int, kk + 1>{});
            LDS_WAIT(7);
          } else {
            LDS_WAIT(0);
          }
          LDS_DEP(wf[bsel][0]); LDS_DEP(wf[bsel][1]); LDS_DEP(wf[bsel][2]);
          LDS_DEP(xf[bsel][0]); LDS_DEP(xf[bsel][1]); LDS_DEP(xf[bsel][2]); LDS_DEP(xf[bsel][3]);
          if constexpr (kk == 0) {
            LDS_DEP(bqr); LDS_DEP(bkr); LDS_DEP(bvr);
            const f32x4 bqv = KR<float>::f4(bqr), bkv = KR<float>::f4(bkr);
            const float bvs = __uint_as_float(bvr);
#pragma unroll
            for (int ms = 0; ms < 4; ++ms) { qT[ms] = bqv; kT[ms] = bkv; vv[ms] = f32x4{bvs, bvs, bvs, bvs}; }
          }
          const uint4 wq = u4(wf[bsel][0]), wk = u4(wf[bsel][1]), wv = u4(wf[bsel][2]);
#pragma unroll
          for (int ms = 0; ms < 4; ++ms) {
            const uint4 x4 = u4(xf[bsel][ms]);
            mma16<T>(qT[ms], wq, x4);
            mma16<T>(kT[ms], wk, x4);
            mma16<T>(vv[ms], x4, wv);
          }
        });
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          pq[ms] = pk16<T>(qT[ms]); pkk[ms] = pk16<T>(kT[ms]); pv[ms] = pk16<T>(vv[ms]);
          if constexpr (SAVE) {     // v -> [token][16] patch (the accumulator holds four tokens of ONE channel per lane)
#pragma unroll
            for (int r = 0; r < 4; ++r)
              *(__attribute__((address_space(3))) T*)(p_vpw + (16 * ms + r) * WHD * E) = from_f<T>(vv[ms][r]);
          }
        }
        STAMP_TO(1);
        if (save && valid) {
          unsigned char* qb = a.qkvw + (size_t)(whoff + h) * (3 * 64 * WHD * E);     // uniform
          int lane_s = (int)(threadIdx.x & 63);        // re-derived per head: a hoisted 64-bit address per store would live across the loop
          LAUNDER(lane_s);
          const unsigned lo = (unsigned)((lane_s & 15) * (WHD * E) + (lane_s >> 4) * L::K16B);
#pragma unroll
          for (int ms = 0; ms < 4; ++ms) {
            *(k16_t*)(qb + (lo + (unsigned)(16 * ms * WHD * E))) = pq[ms];
            *(k16_t*)(qb + (lo + (unsigned)(64 * WHD * E + 16 * ms * WHD * E))) = pkk[ms];
          }
          wave_sync();
#pragma unroll
          for (int i = 0; i < L::VPB / 1024; ++i)
            *(uint4*)(qb + (unsigned)(2 * 64 * WHD * E + (i * 64 + lane) * 16)) = u4((u32x4_)*(const __attribute__((address_space(3))) u32x4_*)(p_vpr + i * 1024));
          wave_sync();
        }
        STAMP_TO(2);
        // ---- S^T = K Q^T: row = key 16 ks + 4 g + r, column = query 16 ms + t; softmax per query
        f32x4 bia[7];
#pragma unroll
        for (int d = 0; d < 7; ++d) { LDS_DEP(biar[d]); bia[d] = KR<T>::f4(biar[d]); }     // older than every fragment read: landed
        k16_t pp[4][4];                                  // P^T strips, packed: [ks][ms]
        float inv[4];
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          f32x4 s[4];
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) { s[ks] = f32x4{0.f, 0.f, 0.f, 0.f}; mmak16(s[ks], pkk[ks], pq[ms]); }
          float mx = -1e30f;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float v = fmaf(s[ks][r], scale2, bia[ms - ks + 3][r]);
              if constexpr (MSK) { if ((diffm[ms] >> (4 * ks + r)) & 1u) v += -100.0f * WMSA_LOG2E; }
              s[ks][r] = v;
              mx = fmaxf(mx, v);
            }
          mx = rows_max(mx);
          float sum = 0.f;
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float p = __builtin_amdgcn_exp2f(s[ks][r] - mx); s[ks][r] = p; sum += p; }
            pp[ks][ms] = pk16<T>(s[ks]);
          }
          sum = rows_sum(sum);
          inv[ms] = __builtin_amdgcn_rcpf(sum);
          if (save && valid && g == 0)
            (a.lsew + (size_t)(whoff + h) * 64)[16 * ms + t] = mx * (1.0f / WMSA_LOG2E) + __logf(sum);
        }
        STAMP_TO(3);
        // ---- O^T = V^T P^T: row = channel 4 g + r, column = query
        k16_t po[4];
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
          if constexpr (std::is_same<T, bf16>::value) {
#pragma unroll
            for (int kp = 0; kp < 2; ++kp)
              mma16<bf16>(o, make_uint4(pv[2 * kp].x, pv[2 * kp].y, pv[2 * kp + 1].x, pv[2 * kp + 1].y),
                          make_uint4(pp[2 * kp][ms].x, pp[2 * kp][ms].y, pp[2 * kp + 1][ms].x, pp[2 * kp + 1][ms].y));
          } else {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) mmak16(o, pv[ks], pp[ks][ms]);
          }
          o *= inv[ms];
          po[ms] = pk16<T>(o);
          if (save && valid) {
            // token offset re-derived per head from a laundered lane id: four hoisted 64-bit store addresses (or their
            // spilled 32-bit sources) would otherwise live across the whole head loop
            int lane_o = (int)(threadIdx.x & 63);
            LAUNDER(lane_o);
            const unsigned ao_off = (unsigned)wtoken(a, b, wy, wx, 16 * ms + (lane_o & 15)) * (unsigned)L::ROWB + (unsigned)((lane_o >> 4) * L::K16B);
            *(k16_t*)(a.ao + (size_t)(WHD * h * E) + ao_off) = po[ms];
          }
        }
        // park O^T of head h (a uniform switch: a register array cannot be indexed by the loop counter)
        static_for<0, WHEADS>([&](auto hh_) {
          constexpr int hh = decltype(hh_)::value;
          if (h == hh) {
#pragma unroll
            for (int ms = 0; ms < 4; ++ms) poall[hh][ms] = po[ms];
          }
        });
      };
      if (msk) body(std::true_type{}); else body(std::false_type{});
      STAMP_TO(4);

      if (NST == 1) __syncthreads();                     // single buffer: everyone is done reading before it is refilled
      PF_COPY(h + 1)
      ++sidx;
    }

    // ================= output projection: out^T = Wproj O^T, three stages of four 16-channel strips
    f32x4 outT[WHEADS][4];                               // out^T: [n strip][token strip], row = channel 16 n + 4 g + r, column = token t
    static_for<0, 3>([&](auto ps_) {
      constexpr int ps = decltype(ps_)::value;
      const int buf = NST == 2 ? (sidx & 1) : 0;
      STAMP_TO(4);
      PF_WAIT_KEEP_STORES(valid && ps == 0);             // (stage 12 was requested at the top of head 11)
      __syncthreads();
      STAMP_TO(0);
      const unsigned pb16 = smem0 + SST0 + (unsigned)(buf * L::STAGE) + l16;
      PF_ISSUE(buf ^ 1, (ps == 2 ? 0 : WHEADS + 1 + ps))  // after the last projection stage: head 0 of the next window group
      u32x4_ af[2];
      af[0] = lds_rd128a<0>(pb16);
      static_for<0, 4 * L::KP>([&](auto i_) {
        constexpr int i = decltype(i_)::value, nl = i / L::KP, kp = i % L::KP, n = 4 * ps + nl;
        if constexpr (i + 1 < 4 * L::KP) {
          af[(i + 1) & 1] = lds_rd128a<(i + 1) * 1024>(pb16);
          LDS_WAIT(1);
        } else {
          LDS_WAIT(0);
        }
        LDS_DEP(af[i & 1]);
        const uint4 wa = u4(af[i & 1]);
#pragma unroll
        for (int ms = 0; ms < 4; ++ms) {
          uint4 ob;
          if constexpr (std::is_same<T, bf16>::value)
            ob = make_uint4(poall[2 * kp][ms].x, poall[2 * kp][ms].y, poall[2 * kp + 1][ms].x, poall[2 * kp + 1][ms].y);
          else
            ob = poall[kp][ms];
          if constexpr (kp == 0) outT[n][ms] = mma16z<T>(wa, ob); else mma16<T>(outT[n][ms], wa, ob);
        }
      });
      if (NST == 1) __syncthreads();
      PF_COPY((ps == 2 ? 0 : WHEADS + 1 + ps))
      ++sidx;
    });

    STAMP_TO(5);
    // ================= epilogue: x_mid = x + (out + bproj), xn2 = LN2(x_mid)
    // out^T + bias is staged through the wave's (dead) LN1 tile in the run dtype - for bf16 that is the rounding a separate
    // projection launch (or torch autocast: F.linear returns bf16, then shortcut + x) applies to its output - which drains all
    // 192 accumulator registers at once.  Load / store order: VMEM operations of a wave retire in issue order, so every load
    // of the epilogue - the residual x, and the x of the NEXT window - is issued before the first store; a load queued
    // behind a store would wait for the store's acknowledgement from memory.  Per-lane addresses are re-derived from a
    // laundered lane id (see the prologue).
    int lane_e = (int)(threadIdx.x & 63);
    LAUNDER(lane_e);
    const int te = lane_e & 15, ge = lane_e >> 4;
    unsigned erow[4], eoff[4];
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      erow[ms] = (unsigned)wtoken(a, b, wy, wx, 16 * ms + te);
      eoff[ms] = erow[ms] * (unsigned)L::ROWB + (unsigned)(ge * 16);
    }
    uint4 xr[4][L::CHL];
#pragma unroll
    for (int ms = 0; ms < 4; ++ms)
#pragma unroll
      for (int i = 0; i < L::CHL; ++i) xr[ms][i] = *(const uint4*)(a.x + (eoff[ms] + 64u * i));
    lds_u8* e_ln = sm3 + SLN0 + ge * KPL * 4;
    lds_u8* e_bp = sm3 + SLN0 + ge * 16;
    lds_u8* e_row = sm3 + w * L::XNB + te * L::ROWB;     // token 16 ms + te of the tile: + ms * 16 * ROWB
    wave_sync();                                         // the heads are done reading the tile
#pragma unroll
    for (int n = 0; n < WHEADS; ++n) {
      const f32x4 bp = *(const __attribute__((address_space(3))) f32x4*)(e_bp + 64 * n);
      // channels 16 n + 4 ge .. + 3: byte (16 n + 4 ge) E of the row = chunk cw, sub-offset sb; stored at chunk cw ^ (te & 7)
      const int cb = (16 * n + 4 * ge) * E, cw = cb >> 4, sb = cb & 15;
      lds_u8* dst = e_row + (((cw ^ (te & 7)) << 4) + sb);
#pragma unroll
      for (int ms = 0; ms < 4; ++ms)
        *(__attribute__((address_space(3))) typename KR<T>::type*)(dst + ms * 16 * L::ROWB) = KR<T>::reg(pk16<T>(outT[n][ms] + bp));
    }
    if constexpr (NST == 2) {     // next window's x (unconditional, clamped: the old xc dies in the prologue, not across the heads)
      __builtin_amdgcn_sched_barrier(0);
      unsigned ro[4];
      strip_offsets(it + (int)gridDim.x < nquads ? it + (int)gridDim.x : it, ro, te, ge);
#pragma unroll
      for (int ms = 0; ms < 4; ++ms)
#pragma unroll
        for (int i = 0; i < L::CHL; ++i) xc[ms][i] = *(const uint4*)(a.x + (ro[ms] + 64u * i));
      __builtin_amdgcn_sched_barrier(0);
    }
    wave_sync();
    const unsigned esw = (unsigned)(((te >> 2) & 1) * 64);
    lds_u8* e_rE = e_row + ((ge ^ (te & 3)) << 4) + esw;   // chunk 4 i + ge of the row: even i at +64 b, odd i at -64 b (see XN_ADDR)
    lds_u8* e_rO = e_row + ((ge ^ (te & 3)) << 4) - esw;
#pragma unroll
    for (int ms = 0; ms < 4; ++ms) {
      float v[L::CHL][KPL];
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < L::CHL; ++i) {
        float f[KPL], o[KPL];
        unpack<T>(xr[ms][i], f);
        unpack<T>(u4((u32x4_)*(const __attribute__((address_space(3))) u32x4_*)(((i & 1) ? e_rO : e_rE) + (ms * 16 * L::ROWB + 64 * i))), o);
        // x_mid is stored in T: LN2 normalises the ROUNDED value, exactly as a separate LayerNorm launch reading x_mid would
        // (and as the LayerNorm backward, which re-reads x_mid, assumes)
#pragma unroll
        for (int j = 0; j < KPL; ++j) { v[i][j] = to_f(from_f<T>(f[j] + o[j])); s += v[i][j]; }
      }
      s = rows_sum(s);
      const float mu = s * (1.0f / WC);
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < L::CHL; ++i)
#pragma unroll
        for (int j = 0; j < KPL; ++j) { const float d = v[i][j] - mu; q = fmaf(d, d, q); }
      q = rows_sum(q);
      const float rs = rsqrtf(q * (1.0f / WC) + 1e-5f);
      if (valid) {
        if (save && ge == 0) *(float2*)((unsigned char*)a.st2 + erow[ms] * 8u) = make_float2(mu, rs);
#pragma unroll
        for (int i = 0; i < L::CHL; ++i) {
          const uint4 xmv = pack<T>(v[i]);
          *(uint4*)(a.xm + (eoff[ms] + 64u * i)) = xmv;
          float f[KPL], ga[KPL], be[KPL];
#pragma unroll
          for (int j = 0; j < KPL; j += 4) {
            *(f32x4*)(ga + j) = *(const __attribute__((address_space(3))) f32x4*)(e_ln + (3 * WC + 4 * i * KPL + j) * 4);
            *(f32x4*)(be + j) = *(const __attribute__((address_space(3))) f32x4*)(e_ln + (4 * WC + 4 * i * KPL + j) * 4);
          }
#pragma unroll
          for (int j = 0; j < KPL; ++j) f[j] = fmaf((v[i][j] - mu) * rs, ga[j], be[j]);
          *(uint4*)(a.xn2 + (eoff[ms] + 64u * i)) = pack<T>(f);
        }
      }
    }
    STAMP_TO(7);
  }
  if constexpr (STAMP) {
    if (tid == 0 && blockIdx.x < 256)
      for (int i = 0; i < 8; ++i) g_wmsa_stamps[blockIdx.x][i] = acc_st[i];
  }
}

// ---- parameter packing: raw f32 parameters of one block -> the stage-ordered buffer above
template <typename T>
__global__ __launch_bounds__(256) void wmsa_pack_kernel(const float* __restrict__ qkv_w, const float* __restrict__ qkv_b,
                                                       const float* __restrict__ proj_w, const float* __restrict__ proj_b,
                                                       const float* __restrict__ table, const float* __restrict__ n1w,
                                                       const float* __restrict__ n1b, const float* __restrict__ n2w,
                                                       const float* __restrict__ n2b, unsigned char* __restrict__ wpk) {
  using L = WL<T>;
  constexpr int KPL = L::KPL, KU = L::KU;
  const int h = blockIdx.x, tid = threadIdx.x;
  if (h == WHEADS) {
    float* tl = (float*)(wpk + L::TAIL_OFF);
    for (int i = tid; i < WC; i += 256) {
      tl[i] = proj_b[i]; tl[WC + i] = n1w[i]; tl[2 * WC + i] = n1b[i]; tl[3 * WC + i] = n2w[i]; tl[4 * WC + i] = n2b[i];
    }
    return;
  }
  if (h > WHEADS + 3) {
    if constexpr (L::PROJ2_BYTES > 0) {
      T* dst = (T*)(wpk + L::PROJ2_OFF);
      for (int e = tid + 256 * (h - WHEADS - 4); e < WHEADS * L::KP * 64 * KPL; e += 256 * 4) {
        const int frag = e / (64 * KPL), l = (e / KPL) % 64, j = e % KPL;
        const int n = frag / L::KP, kp = frag % L::KP;
        dst[e] = from_f<T>(proj_w[(long)(16 * n + (l & 15)) * WC + KU * kp + KPL * (l >> 4) + j]);
      }
    }
    return;
  }
  if (h > WHEADS) {
    // projection stage ps: strips n = 4 ps .. 4 ps + 3, fragment (n, kp): lane (g, t) = row 16 n + t, KPL consecutive k
    // slots; bf16: slots j < 4 <-> channel 32 kp + 4 g + j (head 2 kp), j >= 4 <-> 32 kp + 16 + 4 g + (j - 4) (head 2 kp + 1),
    // the order in which two k16 O^T operands concatenate; f32: channel 16 kp + 4 g + j
    const int ps = h - WHEADS - 1;
    T* dst = (T*)(wpk + (long)(WHEADS + ps) * L::STAGE);
    for (int e = tid; e < 4 * L::KP * 64 * KPL; e += 256) {
      const int frag = e / (64 * KPL), l = (e / KPL) % 64, j = e % KPL;
      const int nl = frag / L::KP, kp = frag % L::KP, n = 4 * ps + nl;
      const int ch = KPL == 8 ? 32 * kp + 16 * (j >> 2) + 4 * (l >> 4) + (j & 3) : 16 * kp + 4 * (l >> 4) + j;
      dst[e] = from_f<T>(proj_w[(long)(16 * n + (l & 15)) * WC + ch]);
    }
    return;
  }
  unsigned char* sb = wpk + (long)h * L::STAGE;
  // Wq_h / Wk_h / Wv_h in fragment order: [k-step][lane][KPL], lane (g, t) = row 16 h + t, columns KU kk + KPL g + j
  for (int sect = 0; sect < 3; ++sect) {
    T* dst = (T*)(sb + sect * L::WFRAG);
    for (int e = tid; e < L::KSTEPS * 64 * KPL; e += 256) {
      const int kk = e / (64 * KPL), l = (e / KPL) % 64, j = e % KPL;
      const float wv_ = qkv_w[(long)(sect * WC + WHD * h + (l & 15)) * WC + KU * kk + KPL * (l >> 4) + j];
      dst[e] = from_f<T>(wv_);
      if constexpr (L::HGW_BYTES > 0)      // the same fragments in the contiguous stream of wmsa_hg.hip; there Wq (and the q bias
        //                                    copy below) carry hd^-1/2 x log2 e, so S^T leaves the MFMA ready for exp2
        ((T*)(wpk + L::HGW_OFF + (long)h * 3 * L::WFRAG + sect * L::WFRAG))[e] = from_f<T>(sect == 0 ? wv_ * (0.25f * WMSA_LOG2E) : wv_);
    }
  }
  // relative-position bias of this head x log2 e: copy v, row dyi, position i holds table[dyi][14 - (i + v)]
  {
    T* dst = (T*)(sb + L::BIAS_OFF);
    for (int e = tid; e < 4 * 15 * 16; e += 256) {
      const int v = e / 240, dyi = (e / 16) % 15, i = e % 16, jj = i + v;
      dst[e] = from_f<T>(jj <= 14 ? table[(dyi * 15 + (14 - jj)) * WHEADS + h] * WMSA_LOG2E : 0.f);
    }
  }
  float* bq = (float*)(sb + L::BQKV_OFF);
  // [48..63]: the q bias x hd^-1/2 x log2 e (wmsa_hg.hip's scaled q)
  for (int i = tid; i < 64; i += 256)
    bq[i] = i < 48 ? qkv_b[(i / 16) * WC + WHD * h + (i % 16)] : qkv_b[WHD * h + (i - 48)] * (0.25f * WMSA_LOG2E);
}

bool g_wmsa_stamp_enable = false;

template <typename T, int NWV, int NST, bool SAVE, bool STAMP = false>
int launch_block(const WArgs& a, hipStream_t st) {
  using L = WL<T>;
  constexpr int LDS = NWV * L::XNB + NST * L::STAGE + NWV * L::VPB + 5 * WC * 4;
  static_assert(LDS <= 160 * 1024, "LDS budget");
  const int nquads = (a.nwin + NWV - 1) / NWV;
  const int grid = nquads < 256 ? nquads : 256;          // one workgroup per CU, persistent over the window groups
  return sodt_launch<wmsa_block_kernel<T, NWV, NST, SAVE, STAMP>>(dim3(grid), dim3(NWV * 64), LDS, st, a);
}

bool wmsa_shape_ok(int B, int H, int W, int C, int heads, int ws, int shift) {
  return B > 0 && C == WC && heads == WHEADS && ws == WWS && H > 0 && W > 0 && H % WWS == 0 && W % WWS == 0 &&
         shift >= 0 && shift < WWS && (long)B * H * W < (1L << 31) / (WC * 4);
}

}  // namespace

extern "C" long sodt_wmsa_pack_bytes(int C, int heads, int ws, int dtype) {
  if (C != WC || heads != WHEADS || ws != WWS) return 0;
  return dtype == SODT_BF16 ? WL<bf16>::PACK_BYTES : (dtype == SODT_F32 ? WL<float>::PACK_BYTES : 0);
}

extern "C" int sodt_wmsa_pack(const float* qkv_w, const float* qkv_b, const float* proj_w, const float* proj_b,
                              const float* rpb_table, const float* n1_w, const float* n1_b, const float* n2_w,
                              const float* n2_b, void* wpk, int C, int heads, int ws, int dtype, sodt_stream_t st_) {
  if (!qkv_w || !qkv_b || !proj_w || !proj_b || !rpb_table || !n1_w || !n1_b || !n2_w || !n2_b || !wpk) return SODT_EINVAL;
  if (C != WC || heads != WHEADS || ws != WWS) return SODT_EINVAL;
  hipStream_t st = (hipStream_t)st_;
  if (dtype == SODT_BF16)
    return sodt_launch<wmsa_pack_kernel<bf16>>(dim3(WHEADS + 8), dim3(256), 0, st, qkv_w, qkv_b, proj_w, proj_b, rpb_table,
                                               n1_w, n1_b, n2_w, n2_b, (unsigned char*)wpk);
  if (dtype == SODT_F32)
    return sodt_launch<wmsa_pack_kernel<float>>(dim3(WHEADS + 8), dim3(256), 0, st, qkv_w, qkv_b, proj_w, proj_b, rpb_table,
                                                n1_w, n1_b, n2_w, n2_b, (unsigned char*)wpk);
  return SODT_EINVAL;
}

extern "C" int sodt_wmsa_block_fwd(const void* x, const void* wpk, void* xm, void* xn2, float* st1, float* st2,
                                   void* xn1, void* qkvw, float* lsew, void* ao,
                                   int B, int H, int W, int C, int heads, int ws, int shift, int dtype, sodt_stream_t st_) {
  if (!x || !wpk || !xm || !xn2 || !wmsa_shape_ok(B, H, W, C, heads, ws, shift)) return SODT_EINVAL;
  const bool save = xn1 != nullptr;
  if (save && (!lsew || !ao || !st1 || !st2)) return SODT_EINVAL;
  // q / k / v are saved by the f32 parity kernel only: the bf16 backward (sodt_wmsa_block_bwd) recomputes them from xn1
  if (save && ((dtype == SODT_F32) != (qkvw != nullptr))) return SODT_EINVAL;
  WArgs a;
  a.x = (const unsigned char*)x; a.wpk = (const unsigned char*)wpk;
  a.xm = (unsigned char*)xm; a.xn2 = (unsigned char*)xn2; a.st1 = st1; a.st2 = st2;
  a.xn1 = (unsigned char*)xn1; a.qkvw = (unsigned char*)qkvw; a.lsew = lsew; a.ao = (unsigned char*)ao;
  a.B = B; a.H = H; a.W = W; a.shift = shift; a.nwy = H / WWS; a.nwx = W / WWS; a.nwin = B * a.nwy * a.nwx;
  hipStream_t st = (hipStream_t)st_;
  if (dtype == SODT_BF16) {
    // throughput path: four waves per window (wmsa_hg.hip).  The one-wave-per-window bf16 build below only runs as the
    // instrumented diagnostic build armed through sodt_debug_wmsa_stamps (an explicit API call, no environment switch).
    if (!g_wmsa_stamp_enable) return wmsa_hg_launch(a, save, st);
    // instrumented build: inference form only (its training form would write q / k / v).  A training call while the stamps are armed
    // must not silently run the inference form - xn1, ao, the statistics and lsew would stay unwritten for the backward
    if (save) return SODT_EINVAL;
    return launch_block<bf16, 4, 2, false, true>(a, st);
  }
  if (dtype == SODT_F32) return save ? launch_block<float, 2, 1, true>(a, st) : launch_block<float, 2, 1, false>(a, st);
  return SODT_EINVAL;
}

/* diagnostic hook (tools/mb_wmsa.py --stamps): enable != 0 makes the following bf16 launches run the instrumented
 * build; out (host, 256 x 8 long long, nullable) receives the per-phase shader-cycle sums of wave 0 of each
 * workgroup of the last such launch: [barrier wait, QKV, pack/save, S+softmax, PV+proj, stage store, prologue, epilogue] */
extern "C" int sodt_debug_wmsa_stamps(long long* out, int enable) {
  g_wmsa_stamp_enable = enable != 0;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wmsa_stamps), sizeof(long long) * 256 * 8) != hipSuccess) return SODT_ELAUNCH;
  return SODT_OK;
}
