// The Detect level (a 1x1 convolution K -> na * no on the stride-4 map, the model's widest row count) in one pass each way (bf16):
//     forward   pred[b][a][p][o] = X[b * HW + p][:] . W[a * no + o][:] + bias[a * no + o]         f32, Detect.forward's layout
//     backward  dZ[m][n] = bf16(dpred[b][a][p][o])   (round-to-nearest-even, what sodt_detect_unpermute stores)
//               dX[M][K]  = dZ @ W                    bf16
//               dW[N][K] += dZ^T @ X                  f32
//               dbias[N] += column sums of dZ         f32
// The launches these replace (sodt_gemm_nt with SODT_EPI_DETECT; sodt_detect_unpermute + sodt_gemm_tn + sodt_gemm_nt) are
// priced by bytes: here X is read once, pred / dpred cross HBM once in their native layout and the [M][48] bf16 copy of dpred
// never exists.
//
// Structure (csrc/linbwd.hip's): one 512-thread workgroup per M-slice, the slice walked in 32-row stages.
//   * X rows arrive by LDS-DMA, three stages deep, two in flight; one raw barrier per stage behind a counted vmcnt.  The image is
//     kept in FRAGMENT order: 16-byte chunk (row 16 u + fr, columns 32 ks + 8 fg ..) sits at chunk index (2 ks + u) * 64 + 16 fg + fr,
//     so the MFMA operand of a wave is 64 consecutive chunks (ds_read_b128, no bank conflict, no swizzle to undo) and one DMA
//     instruction fills exactly one operand.
//   * The weight (48 x K bf16 at most, rows >= na * no zero) is small enough for the registers of the waves that use it, where it
//     stays for the life of the workgroup: nothing is re-read per stage, from LDS or elsewhere.
//   * forward: waves 0-5 own the 2 x 3 output tiles of a stage (K ascending in 32-element MFMAs into one accumulator, bias added
//     in f32: sodt_gemm_nt's products and order).  The tile goes to an LDS staging buffer laid out [anchor][row][o] - per anchor
//     that IS the contiguous run of 32 * no floats the stage owns in pred - and leaves from there in aligned 16-byte chunks, one
//     stage late (two staging buffers, still one barrier per stage).  A stage that crosses an image boundary splits its runs there.
//   * backward: the dpred runs are fetched two stages ahead into registers with a fixed number of loads per thread (the waits
//     stay counted), rounded, and written to two small LDS images: [m][n] in fragment order for dX, [n][m] for dW.  Waves
//     w < K / 32 compute dX columns 32 w .. 32 w + 31 with the weight rows permuted inside the group so that a lane ends with 8
//     consecutive columns of one row (linbwd's store); every wave adds dZ^T X into its 16-column dW tiles (X through
//     ds_read_b64_tr_b16), wave 0 also dbias against a vector of ones.  Each slice's partial goes to the caller's scratch with
//     plain stores and detect_bwd_reduce_kernel adds the live slices in a fixed order: deterministic, no float atomics.
#include "common.h"
#include "launch.h"

namespace {

typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int DT_ROWS = 32, DT_NST = 3, DT_NP = 48;
constexpr int FW_NST = 6;                            // the forward's X stages in LDS: five in flight (8 KiB each at K = 128)
constexpr int DT_OUTB = DT_ROWS * DT_NP * 4;         // forward staging buffer: 6 KiB
constexpr int DT_D1B = DT_ROWS * 64 * 2;             // dZ [m][n], n padded to 64: 4 KiB
constexpr int DT_D2B = DT_NP * DT_ROWS * 2;          // dZ [n][m]: 3 KiB

__device__ uint4 dt_zero16[4];                       // DMA source of rows beyond the slice

__device__ __forceinline__ uint32_t dt_lds_addr(const void* p) { return (uint32_t)(uintptr_t)(lds_void*)p; }
__device__ __forceinline__ u32x4 dt_rd128(uint32_t addr) {
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ float dt_rd32(uint32_t addr) {
  float v;
  asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr));
  return v;
}
__device__ __forceinline__ void dt_wr32(uint32_t addr, float v) { asm volatile("ds_write_b32 %0, %1" :: "v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ void dt_wr16(uint32_t addr, uint32_t v) { asm volatile("ds_write_b16 %0, %1" :: "v"(addr), "v"(v) : "memory"); }
// rows r .. r+3 and r+4 .. r+7 of one 16-column unit (the +4 rows sit 64 bytes on in the fragment-ordered image)
__device__ __forceinline__ u32x4 dt_frag_tr(uint32_t addr) {
  typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
  u32x2 lo, hi;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(lo) : "v"(addr));
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:64" : "=v"(hi) : "v"(addr));
  u32x4 r; r.x = lo.x; r.y = lo.y; r.z = hi.x; r.w = hi.y;
  return r;
}
#define DT_LGKM0() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)

__device__ __forceinline__ void dt_mma(f32x4& acc, const u32x4& a, const u32x4& b) {
  union { u32x4 u; bf16x8 v; } ua, ub;
  ua.u = a; ub.u = b;
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ua.v, ub.v, acc, 0, 0, 0);
}

struct DtSlice { long mbeg; int nrows, nsteps; };
__device__ __forceinline__ DtSlice dt_slice(long M, int splits, int split) {
  const long rows_per = (((M + splits - 1) / splits) + DT_ROWS - 1) / DT_ROWS * DT_ROWS;
  DtSlice s;
  s.mbeg = (long)split * rows_per;
  const long mend = (s.mbeg + rows_per < M) ? (s.mbeg + rows_per) : M;
  s.nrows = mend > s.mbeg ? (int)(mend - s.mbeg) : 0;
  s.nsteps = (s.nrows + DT_ROWS - 1) / DT_ROWS;
  return s;
}

// The X image of one stage is 2 KS wave-instructions of DMA (instruction j: k-step j >> 1, row half j & 1); wave w issues j = w
// and j = w + 8 where they exist, so a wave has nd = 0, 1 or 2 of them per stage.
#define DT_DMA_SETUP()                                                                                                    \
  const unsigned char* zero = (const unsigned char*)dt_zero16;                                                            \
  const int j0 = wid, j1 = wid + 8;                                                                                       \
  const bool have0 = j0 < 2 * KS, have1 = j1 < 2 * KS;                                                                    \
  const int nd = (have0 ? 1 : 0) + (have1 ? 1 : 0);                                                                       \
  const int drow0 = 16 * (j0 & 1) + fr, drow1 = 16 * (j1 & 1) + fr;                                                       \
  const unsigned char* cur0 = (const unsigned char*)g.X + (((sl.mbeg + drow0) * g.ldx + 32 * (j0 >> 1) + 8 * fg) << 1);   \
  const unsigned char* cur1 = (const unsigned char*)g.X + (((sl.mbeg + drow1) * g.ldx + 32 * (j1 >> 1) + 8 * fg) << 1);   \
  const long dstep = (long)DT_ROWS * g.ldx * 2;                                                                           \
  int rel = 0;                                                                                                            \
  auto issue = [&](int slot) {                                                                                            \
    if (have0) {                                                                                                          \
      const unsigned char* s0 = rel + drow0 < sl.nrows ? cur0 : zero;                                                     \
      __builtin_amdgcn_global_load_lds((glb_void*)s0, (lds_void*)(dsm + slot * IMG + j0 * 1024), 16, 0, 0);               \
    }                                                                                                                     \
    if (have1) {                                                                                                          \
      const unsigned char* s1 = rel + drow1 < sl.nrows ? cur1 : zero;                                                     \
      __builtin_amdgcn_global_load_lds((glb_void*)s1, (lds_void*)(dsm + slot * IMG + j1 * 1024), 16, 0, 0);               \
    }                                                                                                                     \
    rel += DT_ROWS;                                                                                                       \
    cur0 += dstep; cur1 += dstep;                                                                                         \
  }

// everything but the newest `EXTRA + nd` vector-memory operations of this wave has completed, and its LDS writes have landed
#define DT_WAIT(EXTRA)                                                                                                    \
  do {                                                                                                                    \
    if (nd == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"((EXTRA) + 2) : "memory");                           \
    else if (nd == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"((EXTRA) + 1) : "memory");                      \
    else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(EXTRA) : "memory");                                         \
  } while (0)

// ------------------------------------------------------------------------------------------------------------------ forward
template <int KS>
__global__ __launch_bounds__(512) void detect_fwd_kernel(const sodt_detect_args g, const int splits) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  constexpr int IMG = 2048 * KS;
  constexpr int OOFF = FW_NST * IMG;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lbase = dt_lds_addr(dsm);
  const int na = g.na, no = g.no, N = na * no, HW = g.HW;
  const long M = (long)g.B * HW;
  const DtSlice sl = dt_slice(M, splits, xcd_remap(blockIdx.x, gridDim.x));
  if (sl.nrows <= 0) return;

  // ---- this wave's output tile: rows 16 u .. + 15 of the stage, columns 16 nt .. + 15; lane (fr, fg) holds column n = 16 nt + fr
  const bool cw = wid < 6;
  const int u = wid >= 3 ? 1 : 0, nt = wid - 3 * u;
  const int n = 16 * nt + fr;
  const bool n_ok = cw && n < N;
  u32x4 wf[KS];
  float bv = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (n_ok) v = *(const uint4*)((const bf16*)g.W + (long)n * g.ldw + 32 * ks + 8 * fg);
    wf[ks].x = v.x; wf[ks].y = v.y; wf[ks].z = v.z; wf[ks].w = v.w;
  }
  if (n_ok && g.bias) bv = g.bias[n];
  // the loads above are consumed here, before the first DMA: no compiler-placed wait is left for the loop
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" :: "v"(wf[ks]));
  asm volatile("" :: "v"(bv));
  const int an = n_ok ? n / no : 0, on = n_ok ? n - an * no : 0;
  const uint32_t owr = lbase + OOFF + 4 * (an * (DT_ROWS * no) + (16 * u + 4 * fg) * no + on);    // + r * no * 4 for accumulator r
  const uint32_t xrd = lbase + ((u * 64 + lane) << 4);                                             // + ks * 2048

  // ---- DMA: waves 0-3 issue instructions j = wid + 4 e (k-step j >> 1 = (wid >> 1) + 2 e, row half j & 1 = wid & 1) and store
  //      nothing, so their memory queue holds DMAs only and the counted wait is exact; waves 4-7 store pred and wait for no DMA
  const unsigned char* zero = (const unsigned char*)dt_zero16;
  const bool dmaw = wid < 4;
  const int nd = dmaw ? (2 * KS - wid + 3) / 4 : 0;
  const int drow = 16 * (wid & 1) + fr;
  const unsigned char* cur = (const unsigned char*)g.X + (((sl.mbeg + drow) * g.ldx + 32 * (wid >> 1) + 8 * fg) << 1);
  const long dstep = (long)DT_ROWS * g.ldx * 2;
  int rel = 0;
  auto issue = [&](int slot) {
    if (dmaw) {
      const bool ok = rel + drow < sl.nrows;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (wid + 4 * e < 2 * KS) {
          const unsigned char* s_ = ok ? cur + 128 * e : zero;
          __builtin_amdgcn_global_load_lds((glb_void*)s_, (lds_void*)(dsm + slot * IMG + (wid + 4 * e) * 1024), 16, 0, 0);
        }
      }
    }
    rel += DT_ROWS;
    cur += dstep;
  };
  // all but the newest FW_NST - 2 stages of this wave's DMAs have landed, and its LDS writes too
#define FW_WAIT()                                                                                                         \
  do {                                                                                                                    \
    if (nd == 4) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(4 * (FW_NST - 2)) : "memory");                      \
    else if (nd == 3) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(3 * (FW_NST - 2)) : "memory");                 \
    else if (nd == 2) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(2 * (FW_NST - 2)) : "memory");                 \
    else if (nd == 1) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" :: "n"(FW_NST - 2) : "memory");                       \
    else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                               \
  } while (0)

  // ---- pred cursor of the next stage to store: image sb, pixel sp
  long sb = sl.mbeg / HW;
  int sp = (int)(sl.mbeg - sb * HW);
  auto store_stage = [&](int st) {
    const int rows = sl.nrows - st * DT_ROWS < DT_ROWS ? sl.nrows - st * DT_ROWS : DT_ROWS;
    const uint32_t obase = lbase + OOFF + (st & 1) * DT_OUTB;
    int r_lo = 0;
    while (r_lo < rows) {
      const int len = rows - r_lo < HW - sp ? rows - r_lo : HW - sp;
      const int cnt = len * no;
      for (int a = wid - 4; a >= 0 && a < na; a += 4) {
        const long G0 = (((long)sb * na + a) * HW + sp) * no;
        const int mis = (int)(G0 & 3);
        float* gp0 = g.pred + (G0 - mis);
        const uint32_t l0 = obase + 4 * (a * (DT_ROWS * no) + r_lo * no);
        const int nch = (mis + cnt + 3) >> 2;
        for (int c = lane; c < nch; c += 64) {
          const int e0 = 4 * c - mis;
          float v[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            int e = e0 + q;
            e = e < 0 ? 0 : (e >= cnt ? cnt - 1 : e);
            v[q] = dt_rd32(l0 + 4 * e);
          }
          asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) :: "memory");
          __builtin_amdgcn_sched_barrier(0);
          float* gp = gp0 + 4 * c;
          if (e0 >= 0 && e0 + 3 < cnt) {      // (written as one instruction: the compiler otherwise folds it into the ragged path's pieces)
            const f32x4 v4 = f32x4{v[0], v[1], v[2], v[3]};
            asm volatile("global_store_dwordx4 %0, %1, off" :: "v"(gp), "v"(v4) : "memory");
          } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (e0 + q >= 0 && e0 + q < cnt) gp[q] = v[q];
          }
        }
      }
      r_lo += len;
      sp += len;
      if (sp >= HW) { sp = 0; ++sb; }
    }
  };

#pragma unroll
  for (int i = 0; i < FW_NST - 1; ++i) issue(i);
  int slot = 0;
  for (int s = 0; s < sl.nsteps; ++s) {
    // queue of a DMA wave, oldest first: DMA(s) | DMA(s+1) .. DMA(s + FW_NST - 2)
    FW_WAIT();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (s > 0) store_stage(s - 1);
    __builtin_amdgcn_sched_barrier(0);
    issue(slot == 0 ? FW_NST - 1 : slot - 1);            // stage s + FW_NST - 1 -> the slot last read in iteration s - 1
    if (cw) {
      u32x4 xa[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) xa[ks] = dt_rd128(xrd + slot * IMG + ks * 2048);
      DT_LGKM0();
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) dt_mma(acc, xa[ks], wf[ks]);
      if (n_ok) {
        const uint32_t o = owr + (s & 1) * DT_OUTB;
#pragma unroll
        for (int r = 0; r < 4; ++r) dt_wr32(o + 4 * r * no, acc[r] + bv);
      }
    }
    slot = slot == FW_NST - 1 ? 0 : slot + 1;
  }
#undef FW_WAIT
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  store_stage(sl.nsteps - 1);
}

// ----------------------------------------------------------------------------------------------------------------- backward
// one of a thread's three dpred elements: (a, r, o) fixed for the life of the workgroup, the image / pixel cursor moves on by
// 32 rows with every load
struct DtElem {
  bool act;          // the element exists (j < 32 * N)
  int r;             // stage row
  long ao;           // a * HW * no + o
  uint32_t d1, d2;   // byte offsets in the two dZ images
  long m;            // absolute row of the next load
  long b; int p;     // m = b * HW + p
};

template <int KS>
__global__ __launch_bounds__(512) void detect_bwd_kernel(const sodt_detect_args g, const int splits, float* __restrict__ partial,
                                                         const int do_dx, const int do_w) {
  extern __shared__ __attribute__((aligned(16))) unsigned char dsm[];
  constexpr int IMG = 2048 * KS, K = 32 * KS;
  constexpr int D1OFF = DT_NST * IMG, D2OFF = D1OFF + 2 * DT_D1B, LDS_END = D2OFF + 2 * DT_D2B;
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fr = lane & 15, fg = lane >> 4;
  const uint32_t lbase = dt_lds_addr(dsm);
  const int na = g.na, no = g.no, N = na * no, HW = g.HW;
  const long M = (long)g.B * HW;
  const int split = xcd_remap(blockIdx.x, gridDim.x);
  const DtSlice sl = dt_slice(M, splits, split);
  if (sl.nrows <= 0) return;                  // dead slice: no partial (the reduction reads the live ones only)

  // ---- the dZ images start as zeros: columns >= N are never written, so they stay the zero padding of both products
  for (int i = tid; i < (LDS_END - D1OFF) / 16; i += 512) *(uint4*)(dsm + D1OFF + 16 * i) = make_uint4(0, 0, 0, 0);

  // ---- dX operand (waves w < KS): W^T rows k = 32 w + 8 (fr >> 2) + (fr & 3) (+ 4 for the second tile), n = 32 nk + 8 fg ..
  const bool dxw = do_dx && wid < KS;
  u32x4 wa[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int nk = 0; nk < 2; ++nk) {
      uint32_t h[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        // (every load is issued, at a clamped address, and masked afterwards: 32 independent loads, not 32 round trips)
        const int n = 32 * nk + 8 * fg + j, k = 32 * wid + 8 * (fr >> 2) + (fr & 3) + 4 * t;
        const bool ok = dxw && n < N;
        const uint32_t w = *((const unsigned short*)g.W + (ok ? (long)n * g.ldw + k : 0L));
        h[j] = ok ? w : 0u;
      }
      wa[t][nk].x = h[0] | (h[1] << 16); wa[t][nk].y = h[2] | (h[3] << 16);
      wa[t][nk].z = h[4] | (h[5] << 16); wa[t][nk].w = h[6] | (h[7] << 16);
    }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int nk = 0; nk < 2; ++nk) asm volatile("" :: "v"(wa[t][nk]));      // consumed before the first DMA (see the forward)
  __syncthreads();                            // (no DMA in flight yet: a plain barrier)

  DT_DMA_SETUP();

  // ---- dpred elements j = tid + 512 e: anchor a = j / (32 no), row r, output o - consecutive threads walk one anchor's run
  const float* dp = g.pred;
  DtElem E0, E1, E2;
  auto elem_init = [&](DtElem& E, int e) {
    const int j = tid + 512 * e;
    E.act = j < DT_ROWS * N;
    const int a = E.act ? j / (DT_ROWS * no) : 0;
    const int rem = E.act ? j - a * (DT_ROWS * no) : 0;
    E.r = rem / no;
    const int o = rem - E.r * no, n = a * no + o;
    E.ao = (long)a * HW * no + o;
    E.d1 = ((((n >> 5) * 2 + (E.r >> 4)) * 64 + ((n >> 3) & 3) * 16 + (E.r & 15)) << 4) + ((n & 7) << 1);
    E.d2 = ((((n >> 4) * 64) + (E.r >> 3) * 16 + (n & 15)) << 4) + ((E.r & 7) << 1);
    E.m = sl.mbeg + E.r;
    E.b = E.m / HW;
    E.p = (int)(E.m - E.b * HW);
  };
  elem_init(E0, 0); elem_init(E1, 1); elem_init(E2, 2);
  // one load per element and stage, issued whether or not the element is live (the waits count them): a dead one reads dpred[0]
  auto elem_ptr = [&](DtElem& E) {
    const float* q = (E.act && E.m < M) ? dp + ((E.b * na * HW + E.p) * no + E.ao) : dp;
    E.m += DT_ROWS;
    E.p += DT_ROWS;
    while (E.p >= HW) { E.p -= HW; ++E.b; }
    return q;
  };
#define DT_LOAD3(P0, P1, P2)                                                                       \
  do {                                                                                             \
    const float* q0 = elem_ptr(E0); const float* q1 = elem_ptr(E1); const float* q2 = elem_ptr(E2); \
    asm volatile("global_load_dword %0, %1, off" : "=v"(P0) : "v"(q0) : "memory");                 \
    asm volatile("global_load_dword %0, %1, off" : "=v"(P1) : "v"(q1) : "memory");                 \
    asm volatile("global_load_dword %0, %1, off" : "=v"(P2) : "v"(q2) : "memory");                 \
  } while (0)
  // round to bf16 (nearest even, sodt_detect_unpermute's conversion) and write both images of stage `st`; rows beyond the slice
  // become zeros by selection, so nothing read past the operand can reach a product
  auto put = [&](const DtElem& E, float v, int st) {
    if (!E.act) return;
    const bool live = st * DT_ROWS + E.r < sl.nrows;
    const uint32_t bits = live ? (pack2bf(v, 0.f) & 0xffffu) : 0u;
    dt_wr16(lbase + D1OFF + (st & 1) * DT_D1B + E.d1, bits);
    dt_wr16(lbase + D2OFF + (st & 1) * DT_D2B + E.d2, bits);
  };
#define DT_PUT3(P0, P1, P2, ST) do { put(E0, P0, ST); put(E1, P1, ST); put(E2, P2, ST); } while (0)

  // ---- dW: this wave's 16-column tiles kt = wid and wid + 8 of X (where they exist), all three 16-row tiles of dZ^T
  const bool kt0 = do_w && wid < 2 * KS, kt1 = do_w && wid + 8 < 2 * KS;
  const int q_ = fr >> 2, p_ = fr & 3;
  auto xtr_addr = [&](int kt) {               // lane (fg, q, p): row 8 fg + q, columns 16 kt + 4 p .. + 3 of the X image
    const int row = 8 * fg + q_, c = 2 * kt + (p_ >> 1);
    return lbase + (((((c >> 2) * 2 + (row >> 4)) * 64 + (c & 3) * 16 + (row & 15)) << 4) + ((p_ & 1) << 3));
  };
  const uint32_t xt0 = xtr_addr(wid), xt1 = xtr_addr(wid + 8);
  const uint32_t zt = lbase + D2OFF + (lane << 4);                           // + i * 1024: dZ^T rows n = 16 i + fr, m = 8 fg ..
  const uint32_t zx = lbase + D1OFF + (lane << 4);                           // + (2 nk + u) * 1024: dZ rows m = 16 u + fr, n = 32 nk + 8 fg ..
  const bool do_bias = do_w && wid == 0 && g.dbias != nullptr;
  u32x4 ones; ones.x = ones.y = ones.z = ones.w = 0x3F803F80u;
  f32x4 acc[2][3], bacc[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) { acc[0][i] = acc[1][i] = bacc[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const int ocol = 32 * wid + 8 * fg;         // first of this lane's 8 dX columns

  // ---- prologue.  Queue afterwards, oldest first: B(1) X(0) A(2) X(1)
  float pa0 = 0.f, pa1 = 0.f, pa2 = 0.f, pb0 = 0.f, pb1 = 0.f, pb2 = 0.f;     // sets A (even stages) and B (odd stages)
  DT_LOAD3(pa0, pa1, pa2);
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(pa0), "+v"(pa1), "+v"(pa2) :: "memory");
  __builtin_amdgcn_sched_barrier(0);
  DT_PUT3(pa0, pa1, pa2, 0);
  __builtin_amdgcn_sched_barrier(0);
  DT_LOAD3(pb0, pb1, pb2);
  issue(0);
  DT_LOAD3(pa0, pa1, pa2);
  issue(1);

  int slot = 0;
  // one stage; (Q0, Q1, Q2) is the register set that holds stage s + 1 and is refilled with stage s + 3
#define DT_STAGE(S, Q0, Q1, Q2)                                                                                           \
  do {                                                                                                                    \
    /* queue: set(s+1) X(s) | stores(s-1) set(s+2) X(s+1): all but the three loads and the newest DMA have landed */      \
    DT_WAIT(3);                                                                                                           \
    asm volatile("" : "+v"(Q0), "+v"(Q1), "+v"(Q2) :: "memory");                                                          \
    __builtin_amdgcn_s_barrier();                                                                                         \
    asm volatile("" ::: "memory");                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    DT_PUT3(Q0, Q1, Q2, (S) + 1);                                                                                         \
    const uint32_t db = ((S) & 1);                                                                                        \
    if (dxw) {                                                                                                            \
      const u32x4 z00 = dt_rd128(zx + db * DT_D1B), z01 = dt_rd128(zx + db * DT_D1B + 2048);                              \
      const u32x4 z10 = dt_rd128(zx + db * DT_D1B + 1024), z11 = dt_rd128(zx + db * DT_D1B + 3072);                       \
      DT_LGKM0();                                                                                                         \
      f32x4 d00 = f32x4{0.f, 0.f, 0.f, 0.f}, d01 = d00, d10 = d00, d11 = d00;      /* d[u][tile] */                        \
      dt_mma(d00, wa[0][0], z00); dt_mma(d01, wa[1][0], z00); dt_mma(d10, wa[0][0], z10); dt_mma(d11, wa[1][0], z10);     \
      dt_mma(d00, wa[0][1], z01); dt_mma(d01, wa[1][1], z01); dt_mma(d10, wa[0][1], z11); dt_mma(d11, wa[1][1], z11);     \
      const int r0 = (S) * DT_ROWS + fr;                                                                                  \
      float v[8];                                                                                                         \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) { v[r] = d00[r]; v[4 + r] = d01[r]; }                                 \
      if (r0 < sl.nrows) *(uint4*)((bf16*)g.dX + (sl.mbeg + r0) * g.lddx + ocol) = pack<bf16>(v);                         \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) { v[r] = d10[r]; v[4 + r] = d11[r]; }                                 \
      if (r0 + 16 < sl.nrows) *(uint4*)((bf16*)g.dX + (sl.mbeg + r0 + 16) * g.lddx + ocol) = pack<bf16>(v);               \
    }                                                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                    \
    DT_LOAD3(Q0, Q1, Q2);                                                                                                 \
    issue(slot == 0 ? DT_NST - 1 : slot - 1);            /* stage s + 2 -> slot (s + 2) % 3: last read in iteration s - 1 */ \
    if (kt0) {                                                                                                            \
      const uint32_t so = slot * IMG;                                                                                     \
      u32x4 fz[3], fx0, fx1;                                                                                              \
      _Pragma("unroll") for (int i = 0; i < 3; ++i) fz[i] = dt_rd128(zt + db * DT_D2B + i * 1024);                        \
      fx0 = dt_frag_tr(xt0 + so);                                                                                         \
      fx1 = fx0;                                                                                                          \
      if (kt1) fx1 = dt_frag_tr(xt1 + so);                                                                                \
      DT_LGKM0();                                                                                                         \
      _Pragma("unroll") for (int i = 0; i < 3; ++i) dt_mma(acc[0][i], fz[i], fx0);                                        \
      if (kt1) { _Pragma("unroll") for (int i = 0; i < 3; ++i) dt_mma(acc[1][i], fz[i], fx1); }                           \
      if (do_bias) { _Pragma("unroll") for (int i = 0; i < 3; ++i) dt_mma(bacc[i], fz[i], ones); }                        \
    }                                                                                                                     \
    slot = slot == DT_NST - 1 ? 0 : slot + 1;                                                                             \
  } while (0)

  for (int s = 0; s < sl.nsteps; s += 2) {
    DT_STAGE(s, pb0, pb1, pb2);
    if (s + 1 < sl.nsteps) DT_STAGE(s + 1, pa0, pa1, pa2);
  }
  // the tail DMAs and the last loads must land before the wave goes on (the operands keep the registers allocated until then)
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(pa0), "+v"(pa1), "+v"(pa2), "+v"(pb0), "+v"(pb1), "+v"(pb2) :: "memory");
  __builtin_amdgcn_sched_barrier(0);

  // acc[t][i][r]: dW row n = 16 i + 4 fg + r, column k = 16 (wid + 8 t) + fr; the slice's tile is [48][K], its dbias row follows
  if (do_w) {
    float* part = partial + (long)split * (DT_NP * K + DT_NP);
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (t == 0 ? kt0 : kt1) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) part[(16 * i + 4 * fg + r) * K + 16 * (wid + 8 * t) + fr] = acc[t][i][r];
      }
    }
    if (do_bias && fr == 0) {
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) part[DT_NP * K + 16 * i + 4 * fg + r] = bacc[i][r];
    }
  }
#undef DT_STAGE
#undef DT_PUT3
#undef DT_LOAD3
}

// dW[n][k] += sum over the live slices of partial[s][n][k], dbias[n] += sum of partial[s][48 K + n]: 32 elements per workgroup,
// the slices dealt over eight thread groups in a fixed order and combined through LDS in a fixed order
__global__ __launch_bounds__(256) void detect_bwd_reduce_kernel(const float* __restrict__ partial, int live, float* __restrict__ dW, int lddw,
                                                               float* __restrict__ dbias, int N, int K) {
  __shared__ float red[8][32];
  const int c = threadIdx.x & 31, sg = threadIdx.x >> 5;
  const int nw = N * K, total = nw + (dbias ? N : 0);
  const int i = blockIdx.x * 32 + c;
  const long slice = (long)DT_NP * K + DT_NP;
  float a = 0.f;
  if (i < total) {
    const float* p = partial + (i < nw ? i : DT_NP * K + (i - nw));
    int s = sg;
    for (; s + 24 < live; s += 32) {
      const float v0 = p[(long)s * slice], v1 = p[(long)(s + 8) * slice], v2 = p[(long)(s + 16) * slice], v3 = p[(long)(s + 24) * slice];
      a += (v0 + v1) + (v2 + v3);
    }
    for (; s < live; s += 8) a += p[(long)s * slice];
  }
  red[sg][c] = a;
  __syncthreads();
  if (sg == 0 && i < total) {
#pragma unroll
    for (int q = 1; q < 8; ++q) a += red[q][c];
    if (i < nw) { const int n = i / K; dW[(long)n * lddw + (i - n * K)] += a; }
    else dbias[i - nw] += a;
  }
}

template <int KS> int launch_fwd(const sodt_detect_args* g, hipStream_t st) {
  return sodt_launch<detect_fwd_kernel<KS>>(dim3((unsigned)g->splits), dim3(512), FW_NST * 2048 * KS + 2 * DT_OUTB, st, *g, g->splits);
}
template <int KS> int launch_bwd(const sodt_detect_args* g, int do_dx, int do_w, hipStream_t st) {
  return sodt_launch<detect_bwd_kernel<KS>>(dim3((unsigned)g->splits), dim3(512), DT_NST * 2048 * KS + 2 * DT_D1B + 2 * DT_D2B, st, *g,
                                            g->splits, g->partial, do_dx, do_w);
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// what both entries ask of the record (include/sodt_hip.h)
bool detect_common_ok(const sodt_detect_args* g, int dtype) {
  if (!g || dtype != SODT_BF16) return false;
  if (g->B <= 0 || g->HW <= 0 || g->na <= 0 || g->no <= 0 || g->na * g->no > DT_NP) return false;
  if ((long)g->B * g->HW > 0x7fffffffL) return false;
  if (g->K < 32 || g->K > 256 || (g->K % 32)) return false;
  if (g->splits < 1 || g->splits > 65535) return false;
  if (!g->X || !g->W || !g->pred || !aligned16(g->X) || !aligned16(g->W) || !aligned16(g->pred)) return false;
  if ((g->ldx % 8) || (g->ldw % 8) || g->ldx < g->K || g->ldw < g->K) return false;
  return true;
}

}  // namespace

extern "C" int sodt_detect_fwd(const sodt_detect_args* g, int dtype, sodt_stream_t st) {
  if (!detect_common_ok(g, dtype)) return SODT_EINVAL;
  if (g->bias && !aligned16(g->bias)) return SODT_EINVAL;
  switch (g->K / 32) {
    case 1: return launch_fwd<1>(g, (hipStream_t)st);
    case 2: return launch_fwd<2>(g, (hipStream_t)st);
    case 3: return launch_fwd<3>(g, (hipStream_t)st);
    case 4: return launch_fwd<4>(g, (hipStream_t)st);
    case 5: return launch_fwd<5>(g, (hipStream_t)st);
    case 6: return launch_fwd<6>(g, (hipStream_t)st);
    case 7: return launch_fwd<7>(g, (hipStream_t)st);
    default: return launch_fwd<8>(g, (hipStream_t)st);
  }
}

extern "C" int sodt_detect_bwd(const sodt_detect_args* g, int dtype, sodt_stream_t st) {
  if (!detect_common_ok(g, dtype)) return SODT_EINVAL;
  if (g->flags & ~(SODT_DETECT_NO_WGRAD | SODT_DETECT_NO_DX)) return SODT_EINVAL;
  const int do_w = !(g->flags & SODT_DETECT_NO_WGRAD), do_dx = !(g->flags & SODT_DETECT_NO_DX);
  if (!do_w && !do_dx) return SODT_EINVAL;
  if (do_dx && (!g->dX || !aligned16(g->dX) || (g->lddx % 8) || g->lddx < g->K)) return SODT_EINVAL;
  const int N = g->na * g->no;
  int live = 0;
  if (do_w) {
    if (!g->dW || !aligned16(g->dW) || (g->lddw % 4) || g->lddw < g->K) return SODT_EINVAL;
    if (g->dbias && !aligned16(g->dbias)) return SODT_EINVAL;
    // every slice leaves a [48][K] tile and a 48-float dbias row in the scratch: without room for them the entry refuses
    if (!g->partial || !aligned16(g->partial) || (long)g->splits * (DT_NP * g->K + DT_NP) > g->partial_floats) return SODT_EINVAL;
    const long M = (long)g->B * g->HW;
    const long rows_per = (((M + g->splits - 1) / g->splits) + DT_ROWS - 1) / DT_ROWS * DT_ROWS;
    live = (int)((M + rows_per - 1) / rows_per);
  }
  int rc;
  switch (g->K / 32) {
    case 1: rc = launch_bwd<1>(g, do_dx, do_w, (hipStream_t)st); break;
    case 2: rc = launch_bwd<2>(g, do_dx, do_w, (hipStream_t)st); break;
    case 3: rc = launch_bwd<3>(g, do_dx, do_w, (hipStream_t)st); break;
    case 4: rc = launch_bwd<4>(g, do_dx, do_w, (hipStream_t)st); break;
    case 5: rc = launch_bwd<5>(g, do_dx, do_w, (hipStream_t)st); break;
    case 6: rc = launch_bwd<6>(g, do_dx, do_w, (hipStream_t)st); break;
    case 7: rc = launch_bwd<7>(g, do_dx, do_w, (hipStream_t)st); break;
    default: rc = launch_bwd<8>(g, do_dx, do_w, (hipStream_t)st); break;
  }
  if (rc || !do_w) return rc;
  const int total = N * g->K + (g->dbias ? N : 0);
  return sodt_launch<detect_bwd_reduce_kernel>(dim3((unsigned)((total + 31) / 32)), dim3(256), 0, (hipStream_t)st, (const float*)g->partial, live,
                                               g->dW, g->lddw, g->dbias, N, g->K);
}
