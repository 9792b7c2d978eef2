// non_max_suppression of general.py:425-512 for a whole batch in one launch sequence, with no host read: the batched
// sibling of nms.hip (which stays as it is, one image per call).  Same candidate key, same f32 operations in the same
// order for every `>` the reference evaluates (obj > conf, obj*cls > conf, IoU > thr); this file is compiled with
// -ffp-contract=off (build.py SOURCE_FLAGS), so no multiply-add is fused and the kept candidate ids are the oracle's.
//
// Pipeline (all on the caller's stream, the same launches for every B and every count):
//   nmsb_candidates : one thread per decoded row of every image (grid.y = image); the autolabelling rows of
//                     general.py:451-458 are virtual rows N + k read from `labels` (obj = 1, one-hot class), never
//                     materialised.  A wave counts its candidates, takes ONE slot range from the image's device counter
//                     and writes key = (~score_bits << 32) | (row * nc + class) into the image's fixed-capacity segment.
//   nmsb_hist<1>, nmsb_hist<2>, nmsb_select : images with more than 30000 candidates keep only the keys that can be
//                     among the 30000 smallest (a two-level histogram of the key's top 24 bits finds the cut)
//   rocprim segmented radix sort of the B segments [b * cap, b * cap + selected[b]), end offsets read on the device
//                     (one workgroup per segment, no size partitioning: that path of rocPRIM copies counts to the host)
//   nmsb_gather     : [x1 y1 x2 y2 score cls] and the class-offset box of the first min(count, 30000) sorted keys
//   nmsb_greedy     : one workgroup per image walks the sorted boxes 64 at a time: every box of the chunk against the
//                     <= 300 kept boxes held in LDS and against the later boxes of its chunk (16 waves share both), then
//                     one wave resolves the chunk in order in registers and appends the survivors.  Stops at 300 kept:
//                     torchvision.ops.nms followed by i[:max_det], with 300 n IoU tests at most and no IoU matrix.
//   nmsb_merge      : one wave per kept detection, grid (300, B): merge-NMS and the redundancy filter where the image's
//                     count before truncation is in (1, 3000) (general.py:499-505), a plain copy elsewhere
//   nmsb_pack       : per-image counts -> (B+1) offsets, rows and candidate ids packed image after image
#include <climits>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int MAX_NMS = 30000;     // general.py:438
constexpr int MAX_DET = 300;       // general.py:437
constexpr float MAX_WH = 4096.f;   // general.py:436
constexpr int MERGE_BELOW = 3000;  // general.py:499
constexpr int MAX_B = 4096;        // offsets of nmsb_pack live in LDS
constexpr int CHUNK = 64, PARTS = 16, GREEDY_TPB = CHUNK * PARTS;

__device__ __forceinline__ uint64_t make_key(float score, uint32_t id) {
  return ((uint64_t)(~__float_as_uint(score)) << 32) | id;   // score > 0 here, so its bit pattern is monotonic
}

__device__ __forceinline__ bool iou_gt(const float4 a, const float4 b, float thr) {
  const float aa = (a.z - a.x) * (a.w - a.y), ab = (b.z - b.x) * (b.w - b.y);
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = w * h;
  return inter / (aa + ab - inter) > thr;
}

// The decoded rows of the batch: z (B, N, 5+nc) followed, per image, by the nlab[b] <= lab_cap autolabelling rows.
struct row_src {
  const float* z; const float* labels; const int* nlab;
  int N, nc, lab_cap;
};

// Row i of image b as [cx cy w h obj] and its class scores: `cls` points at them, or is null for an autolabelling row
// whose scores are 1 at class `hot` and 0 elsewhere (no class at all if the label's class is not in [0, nc)).
struct row_view {
  float x, y, w, h, obj;
  const float* cls; int hot;
  __device__ __forceinline__ float cls_at(int j) const { return cls ? cls[j] : (j == hot ? 1.f : 0.f); }
};

__device__ __forceinline__ row_view load_row(const row_src& S, int b, int i) {
  row_view v;
  if (i < S.N) {
    const float* r = S.z + ((long)b * S.N + i) * (S.nc + 5);
    v.x = r[0]; v.y = r[1]; v.w = r[2]; v.h = r[3]; v.obj = r[4]; v.cls = r + 5; v.hot = -1;
  } else {
    const float* l = S.labels + ((long)b * S.lab_cap + (i - S.N)) * 5;
    const float c = l[0];
    v.x = l[1]; v.y = l[2]; v.w = l[3]; v.h = l[4]; v.obj = 1.f; v.cls = nullptr;
    v.hot = (c > -1.f && c < (float)S.nc) ? (int)c : -1;      // l[:, 0].long() truncates towards zero
  }
  return v;
}

__global__ __launch_bounds__(256) void nmsb_candidates_kernel(row_src S, int rows, float conf, int multi,
                                                             const unsigned char* __restrict__ allow,
                                                             uint64_t* __restrict__ keys, long cap, int* __restrict__ count) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63;
  const int nrows = S.N + (S.nlab ? min(max(S.nlab[b], 0), S.lab_cap) : 0);
  const bool live = i < rows && i < nrows;
  row_view v;
  int c = 0, bj = 0;
  float best = 0.f;
  if (live) {
    v = load_row(S, b, i);
    if (v.obj > conf || i >= S.N) {            // autolabelling rows join after the objectness cut (general.py:446,451)
      if (multi) {
        for (int j = 0; j < S.nc; ++j) c += (v.cls_at(j) * v.obj > conf && (!allow || allow[j])) ? 1 : 0;
      } else {
        best = v.cls_at(0) * v.obj;
        for (int j = 1; j < S.nc; ++j) {
          const float s = v.cls_at(j) * v.obj;
          if (s > best) { best = s; bj = j; }
        }
        c = (best > conf && (!allow || allow[bj])) ? 1 : 0;
      }
    }
  }
  int incl = c;                                 // inclusive prefix sum over the wave: one atomic per wave, not per candidate
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  int base = 0;
  if (lane == 63 && incl > 0) base = atomicAdd(count + b, incl);
  base = __shfl(base, 63);
  if (c == 0) return;
  long slot = base + incl - c;
  uint64_t* kb = keys + (long)b * cap;
  if (multi) {
    for (int j = 0; j < S.nc; ++j) {
      const float s = v.cls_at(j) * v.obj;
      if (s > conf && (!allow || allow[j])) {
        if (slot < cap) kb[slot] = make_key(s, (uint32_t)(i * S.nc + j));
        ++slot;
      }
    }
  } else if (slot < cap) {
    kb[slot] = make_key(best, (uint32_t)(i * S.nc + bj));
  }
}

// ---- the 30000 cut before the sort -----------------------------------------------------------------------------------
// Only the 30000 smallest keys of an image can survive the sort (general.py:489-490), and a segment is sorted by ONE
// workgroup, so an image with more candidates first drops the keys that cannot be among them: a two-level histogram
// of the key's top 24 bits (12 + 12; sign, exponent and 15 mantissa bits of the inverted score) gives the prefix P of the
// 30000th smallest key, and every key whose prefix is <= P is kept - all 30000 smallest and the few that share the last
// prefix.  Which keys sit in front after the sort, and their order, is unchanged.  Images at or below 30000 keep all.
constexpr int HBINS = 4096;

// The first bin at which the running sum of hist[0 .. HBINS) reaches `need` (HBINS - 1 if it never does) and the sum of the
// bins below it.  Called by all 256 threads of a workgroup; s_part: 258 ints of LDS.
__device__ int find_bin(const int* __restrict__ hist, int need, int& below, int* s_part) {
  const int tid = threadIdx.x;
  int loc = 0;
  for (int q = 0; q < 16; ++q) loc += hist[tid * 16 + q];
  s_part[tid] = loc;
  __syncthreads();
  if (tid == 0) {
    int run = 0, t = 0;
    for (; t < 255; ++t) {
      if (run + s_part[t] >= need) break;
      run += s_part[t];
    }
    s_part[256] = t; s_part[257] = run;
  }
  __syncthreads();
  const int t = s_part[256];
  int run = s_part[257], bin = t * 16;
  for (int q = 0; q < 15; ++q) {
    const int h = hist[t * 16 + q];
    if (run + h >= need) break;
    run += h; ++bin;
  }
  below = run;
  __syncthreads();
  return bin;
}

// hist: (B, 2, HBINS) int32, zeroed by the entry point.  LEVEL 1 counts key bits 63..52 of every candidate, LEVEL 2 bits
// 51..40 of the candidates inside the level-1 bin that holds the 30000th key.
template <int LEVEL>
__global__ __launch_bounds__(256) void nmsb_hist_kernel(const uint64_t* __restrict__ keys, long cap, const int* __restrict__ count,
                                                       int* __restrict__ hist) {
  __shared__ int s_h[HBINS];
  __shared__ int s_part[258];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = (int)min((long)max(count[b], 0), cap);
  if (n <= MAX_NMS) return;
  int* h1 = hist + (long)b * 2 * HBINS;
  int* h2 = h1 + HBINS;
  int t1 = 0;
  if (LEVEL == 2) { int below; t1 = find_bin(h1, MAX_NMS, below, s_part); }
  for (int q = tid; q < HBINS; q += 256) s_h[q] = 0;
  __syncthreads();
  const uint64_t* kb = keys + (long)b * cap;
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
    const uint32_t hi = (uint32_t)(kb[i] >> 32);
    if (LEVEL == 1) atomicAdd(&s_h[hi >> 20], 1);
    else if ((int)(hi >> 20) == t1) atomicAdd(&s_h[(hi >> 8) & (HBINS - 1)], 1);
  }
  __syncthreads();
  int* out = LEVEL == 1 ? h1 : h2;
  for (int q = tid; q < HBINS; q += 256)
    if (s_h[q]) atomicAdd(out + q, s_h[q]);
}

__global__ __launch_bounds__(256) void nmsb_select_kernel(const uint64_t* __restrict__ keys, long cap, const int* __restrict__ count,
                                                         const int* __restrict__ hist, uint64_t* __restrict__ sel,
                                                         int* __restrict__ nsel) {
  __shared__ int s_part[258];
  const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  const int n = (int)min((long)max(count[b], 0), cap);
  uint32_t prefix = 0xffffffu;
  if (n > MAX_NMS) {
    const int* h1 = hist + (long)b * 2 * HBINS;
    int below1, below2;
    const int t1 = find_bin(h1, MAX_NMS, below1, s_part);
    const int t2 = find_bin(h1 + HBINS, MAX_NMS - below1, below2, s_part);
    prefix = ((uint32_t)t1 << 12) | (uint32_t)t2;
  }
  // Count first, take ONE slot range per workgroup, then write: an atomic per wave and step (6144 returning adds on one
  // address per image at cap = 393,216) made this kernel 1.45 ms of a 2.4 ms call.  The second read of the workgroup's
  // 32 KB of keys comes from cache.
  __shared__ int s_wave[4], s_base;
  const uint64_t* kb = keys + (long)b * cap;
  uint64_t* sb = sel + (long)b * cap;
  int c = 0;
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) c += (uint32_t)(kb[i] >> 40) <= prefix ? 1 : 0;
  int incl = c;
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(incl, d);
    if (lane >= d) incl += up;
  }
  if (lane == 63) s_wave[tid >> 6] = incl;
  __syncthreads();
  if (tid == 0) {
    const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
    s_base = total ? atomicAdd(nsel + b, total) : 0;
  }
  __syncthreads();
  long slot = s_base + incl - c;
  for (int w = 0; w < (tid >> 6); ++w) slot += s_wave[w];
  for (int i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
    const uint64_t k = kb[i];
    if ((uint32_t)(k >> 40) <= prefix) {
      if (slot < cap) sb[slot] = k;
      ++slot;
    }
  }
}

__global__ __launch_bounds__(256) void nmsb_gather_kernel(row_src S, const uint64_t* __restrict__ sorted, long cap,
                                                         const int* __restrict__ count, int nmax, int agnostic,
                                                         float* __restrict__ det, float4* __restrict__ boxes) {
  const int b = blockIdx.y, s = blockIdx.x * 256 + threadIdx.x;
  if (s >= min(count[b], nmax)) return;
  const uint32_t id = (uint32_t)(sorted[(long)b * cap + s] & 0xffffffffu);
  const int i = id / S.nc, j = id - i * S.nc;
  const row_view v = load_row(S, b, i);
  const float hw = v.w / 2, hh = v.h / 2;
  const float x1 = v.x - hw, y1 = v.y - hh, x2 = v.x + hw, y2 = v.y + hh;
  float* d = det + ((long)b * nmax + s) * 6;
  d[0] = x1; d[1] = y1; d[2] = x2; d[3] = y2; d[4] = v.cls_at(j) * v.obj; d[5] = (float)j;
  const float c = agnostic ? 0.f : (float)j * MAX_WH;
  boxes[(long)b * nmax + s] = make_float4(x1 + c, y1 + c, x2 + c, y2 + c);
}

// Greedy suppression of image blockIdx.x.  Thread (cand = tid & 63, part = tid >> 6) tests box `cand` of the chunk against
// the kept boxes part, part + 16, ... and against the chunk's boxes t > cand, t = part, part + 16, ...; wave 0 ORs the 16
// partial results and resolves the chunk in order exactly as the diagonal step of nms.hip's nms_reduce_kernel does.
__global__ __launch_bounds__(GREEDY_TPB) void nmsb_greedy_kernel(const float4* __restrict__ boxes, const int* __restrict__ count,
                                                                int nmax, float thr, int* __restrict__ keep,
                                                                int* __restrict__ nkeep) {
  __shared__ float4 s_kept[MAX_DET];
  __shared__ float4 s_cb[2][CHUNK];
  __shared__ uint64_t s_diag[PARTS][CHUNK];
  __shared__ unsigned char s_sup[PARTS][CHUNK];
  __shared__ int s_nk;
  const int b = blockIdx.x, tid = threadIdx.x, cand = tid & (CHUNK - 1), part = tid / CHUNK;
  const int n = min(max(count[b], 0), nmax);
  const float4* bx = boxes + (long)b * nmax;
  // Loads past n are clamped into the image's nmax slots: whatever they read belongs to a dead candidate (c0 + tid >= n).
  if (tid == 0) s_nk = 0;
  if (tid < CHUNK) s_cb[0][tid] = bx[min(tid, nmax - 1)];
  __syncthreads();
  int buf = 0;
  for (int c0 = 0; c0 < n; c0 += CHUNK, buf ^= 1) {
    float4 nxt = make_float4(0.f, 0.f, 0.f, 0.f);                 // the next chunk travels while this one is tested
    if (part == 0) nxt = bx[min(c0 + CHUNK + cand, nmax - 1)];
    const float4 my = s_cb[buf][cand];
    const int nk = s_nk;
    bool sup = false;
    for (int q = part; q < nk; q += PARTS) sup |= iou_gt(s_kept[q], my, thr);
    uint64_t bits = 0;
    for (int t = part; t < CHUNK; t += PARTS)
      if (t > cand && iou_gt(my, s_cb[buf][t], thr)) bits |= 1ull << t;
    s_sup[part][cand] = sup ? 1 : 0;
    s_diag[part][cand] = bits;
    __syncthreads();
    if (tid < CHUNK) {
      bool dead = c0 + tid >= n;
      uint64_t diag = 0;
      for (int p = 0; p < PARTS; ++p) { dead |= s_sup[p][tid] != 0; diag |= s_diag[p][tid]; }
      uint64_t rem = __ballot(dead), kept = 0;
      for (int r = 0; r < CHUNK; ++r) {
        const uint64_t d = __shfl(diag, r);
        if (!((rem >> r) & 1)) { kept |= 1ull << r; rem |= d; }
      }
      const int slot = nk + __popcll(kept & ((1ull << tid) - 1));
      if (((kept >> tid) & 1) && slot < MAX_DET) {
        s_kept[slot] = my;
        keep[b * MAX_DET + slot] = c0 + tid;
      }
      if (tid == 0) s_nk = min(MAX_DET, nk + __popcll(kept));
      s_cb[buf ^ 1][tid] = nxt;
    }
    __syncthreads();
    if (s_nk >= MAX_DET) break;
  }
  if (tid == 0) nkeep[b] = s_nk;
}

// general.py:500-506: boxes(i) = sum_j w_ij * box_j / sum_j w_ij, w_ij = [IoU(i, j) > thr] * score_j; redundant: > 1 member
__global__ __launch_bounds__(64) void nmsb_merge_kernel(const float* __restrict__ det, const float4* __restrict__ boxes,
                                                       const int* __restrict__ count, int nmax, const int* __restrict__ keep,
                                                       const int* __restrict__ nkeep, float thr, float* __restrict__ rows,
                                                       int* __restrict__ valid) {
  const int k = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (k >= nkeep[b]) return;
  const int total = count[b], n = min(total, nmax);
  const float* dt = det + (long)b * nmax * 6;
  const float4* bx = boxes + (long)b * nmax;
  const int i = keep[b * MAX_DET + k];
  float* o = rows + ((long)b * MAX_DET + k) * 6;
  const float* di = dt + (long)i * 6;
  if (!(total > 1 && total < MERGE_BELOW)) {   // general.py:499 tests the count before the 30000 cut
    if (lane < 6) o[lane] = di[lane];
    if (lane == 0) valid[b * MAX_DET + k] = 1;
    return;
  }
  const float4 a = bx[i];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, ws = 0.f; int cnt = 0;
  for (int j = lane; j < n; j += 64) {
    if (iou_gt(a, bx[j], thr)) {
      const float* dj = dt + (long)j * 6;
      const float w = dj[4];
      s0 += w * dj[0]; s1 += w * dj[1]; s2 += w * dj[2]; s3 += w * dj[3]; ws += w; ++cnt;
    }
  }
  s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); s3 = wave_sum(s3); ws = wave_sum(ws);
  cnt += __shfl_xor(cnt, 1); cnt += __shfl_xor(cnt, 2); cnt += __shfl_xor(cnt, 4);
  cnt += __shfl_xor(cnt, 8); cnt += __shfl_xor(cnt, 16); cnt += __shfl_xor(cnt, 32);
  if (lane == 0) {
    o[0] = s0 / ws; o[1] = s1 / ws; o[2] = s2 / ws; o[3] = s3 / ws; o[4] = di[4]; o[5] = di[5];
    valid[b * MAX_DET + k] = cnt > 1;
  }
}

// One workgroup: per-image survivor counts (a wave per image), their exclusive scan in LDS, then the packed copy.  The
// rows past out_off[B] were zeroed by the entry point before this kernel.
__global__ __launch_bounds__(1024) void nmsb_pack_kernel(const float* __restrict__ rows, const int* __restrict__ valid,
                                                        const int* __restrict__ keep, const int* __restrict__ nkeep,
                                                        const uint64_t* __restrict__ sorted, long cap, int B,
                                                        float* __restrict__ out_rows, int* __restrict__ out_index,
                                                        int* __restrict__ out_off) {
  __shared__ int s_off[MAX_B + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int b = wave; b < B; b += 16) {
    const int nk = min(nkeep[b], MAX_DET);
    int cnt = 0;
    for (int k0 = 0; k0 < nk; k0 += 64) {
      const int k = k0 + lane;
      cnt += __popcll(__ballot(k < nk && valid[b * MAX_DET + k]));
    }
    if (lane == 0) s_off[b + 1] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    s_off[0] = 0;
    for (int b = 0; b < B; ++b) s_off[b + 1] += s_off[b];
  }
  __syncthreads();
  for (int b = tid; b <= B; b += 1024) out_off[b] = s_off[b];
  for (int b = wave; b < B; b += 16) {
    const int nk = min(nkeep[b], MAX_DET);
    int base = s_off[b];
    for (int k0 = 0; k0 < nk; k0 += 64) {
      const int k = k0 + lane;
      const bool v = k < nk && valid[b * MAX_DET + k];
      const uint64_t m = __ballot(v);
      const int pos = base + __popcll(m & ((1ull << lane) - 1));
      if (v) {
        const float* r = rows + ((long)b * MAX_DET + k) * 6;
        for (int c = 0; c < 6; ++c) out_rows[(long)pos * 6 + c] = r[c];
        out_index[pos] = (int)(sorted[(long)b * cap + keep[b * MAX_DET + k]] & 0xffffffffu);
      }
      base += __popcll(m);
    }
  }
}

// Radix sort with one workgroup per segment.  The warp-sort configuration is disabled on purpose: with it rocPRIM sorts
// segments by size first and copies the class counts to the host, which is a synchronisation and a data-dependent launch list.
using sort_config = rocprim::segmented_radix_sort_config<8, rocprim::kernel_config<256, 16>, rocprim::DisabledWarpSortConfig>;

// Segment b is [b * cap, b * cap + count[b]): rocPRIM wants one iterator type for both ends, so the begin offsets are
// this functor with a null count.
struct seg_offset {
  const int* count; unsigned cap;
  __host__ __device__ unsigned operator()(unsigned b) const {
    if (!count) return b * cap;
    const int c = count[b];
    return b * cap + (c < 0 ? 0u : ((unsigned)c < cap ? (unsigned)c : cap));
  }
};

// count: the device counters (null for the size query, which evaluates no offset)
hipError_t sort_segments(void* tmp, size_t& tmp_bytes, rocprim::double_buffer<uint64_t>& keys, unsigned B, unsigned cap,
                         const int* count, hipStream_t stream) {
  const auto first = rocprim::make_counting_iterator(0u);
  return rocprim::segmented_radix_sort_keys<sort_config>(tmp, tmp_bytes, keys, B * cap, B,
                                                         rocprim::make_transform_iterator(first, seg_offset{nullptr, cap}),
                                                         rocprim::make_transform_iterator(first, seg_offset{count, cap}), 0, 64,
                                                         stream);
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct ws_layout {
  size_t count, nsel, hist, zero_bytes, keys_a, keys_b, sort_tmp, sort_tmp_bytes, det, boxes, keep, nkeep, rows, valid, total;
  long cap; int nmax;
};

// Every size follows from B, rows = N + lab_cap, nc and multi_label: cap = rows * (multi_label and nc > 1 ? nc : 1)
// candidates per image at most, of which min(cap, 30000) survive the sort.
int layout(int B, long rows, int nc, int multi, ws_layout& L) {
  if (B <= 0 || B > MAX_B || rows <= 0 || nc <= 0 || rows * nc > (long)INT_MAX) return SODT_EINVAL;
  const long cap = rows * (multi && nc > 1 ? nc : 1);
  if ((long)B * cap > (long)INT_MAX) return SODT_EINVAL;
  const int nmax = (int)(cap < MAX_NMS ? cap : MAX_NMS);
  size_t tb = 0;
  // The size query touches no key, but it must see two non-null buffers: with a null one rocPRIM budgets a third key array
  // of its own inside the temporary storage.
  uint64_t* const unused = reinterpret_cast<uint64_t*>(sizeof(uint64_t));
  rocprim::double_buffer<uint64_t> none(unused, unused);
  if (sort_segments(nullptr, tb, none, (unsigned)B, (unsigned)cap, nullptr, nullptr) != hipSuccess) return SODT_ELAUNCH;
  size_t o = 0;
  L.cap = cap; L.nmax = nmax;
  L.count = o; o += align256((size_t)B * 4);                 // count | nsel | hist: one region, zeroed by one memset
  L.nsel = o; o += align256((size_t)B * 4);
  L.hist = o; o += align256((size_t)B * 2 * HBINS * 4);
  L.zero_bytes = o - L.count;
  L.keys_a = o; o += align256((size_t)B * cap * 8);
  L.keys_b = o; o += align256((size_t)B * cap * 8);
  L.sort_tmp = o; L.sort_tmp_bytes = tb; o += align256(tb);
  L.det = o; o += align256((size_t)B * nmax * 24);
  L.boxes = o; o += align256((size_t)B * nmax * 16);
  L.keep = o; o += align256((size_t)B * MAX_DET * 4);
  L.nkeep = o; o += align256((size_t)B * 4);
  L.rows = o; o += align256((size_t)B * MAX_DET * 24);
  L.valid = o; o += align256((size_t)B * MAX_DET * 4);
  L.total = o;
  return SODT_OK;
}

}  // namespace

extern "C" int sodt_nms_batch_workspace_bytes(int B, long rows, int nc, int multi_label, size_t* bytes) {
  ws_layout L;
  if (!bytes || layout(B, rows, nc, multi_label, L) != SODT_OK) return SODT_EINVAL;
  *bytes = L.total;
  return SODT_OK;
}

extern "C" int sodt_nms_batch(const float* z, int B, int N, int nc, const float* labels, const int* nlab, int lab_cap,
                              float conf_thres, float iou_thres, int multi_label, const unsigned char* class_allow,
                              int agnostic, void* ws, size_t ws_bytes, float* out_rows, int* out_index, int* out_off,
                              hipStream_t stream) {
  ws_layout L;
  if (!z || !ws || !out_rows || !out_index || !out_off || N <= 0 || lab_cap < 0) return SODT_EINVAL;
  if ((lab_cap > 0) != (labels != nullptr) || (labels != nullptr) != (nlab != nullptr)) return SODT_EINVAL;
  if (((uintptr_t)ws & 15) != 0) return SODT_EINVAL;
  const int multi = multi_label && nc > 1;
  if (layout(B, (long)N + lab_cap, nc, multi, L) != SODT_OK || ws_bytes < L.total) return SODT_EINVAL;
  const int rows = N + lab_cap;
  char* base = (char*)ws;
  int* count = (int*)(base + L.count);
  int* nsel = (int*)(base + L.nsel);
  int* hist = (int*)(base + L.hist);
  uint64_t* keys_a = (uint64_t*)(base + L.keys_a);
  uint64_t* keys_b = (uint64_t*)(base + L.keys_b);
  float* det = (float*)(base + L.det);
  float4* boxes = (float4*)(base + L.boxes);
  int* keep = (int*)(base + L.keep);
  int* nkeep = (int*)(base + L.nkeep);
  float* rws = (float*)(base + L.rows);
  int* valid = (int*)(base + L.valid);
  const row_src S{z, labels, nlab, N, nc, lab_cap};
  if (hipMemsetAsync(count, 0, L.zero_bytes, stream) != hipSuccess) return SODT_ELAUNCH;
  if (hipMemsetAsync(out_rows, 0, (size_t)B * MAX_DET * 24, stream) != hipSuccess) return SODT_ELAUNCH;
  if (hipMemsetAsync(out_index, 0, (size_t)B * MAX_DET * 4, stream) != hipSuccess) return SODT_ELAUNCH;
  if (int err = sodt_launch<nmsb_candidates_kernel>(dim3((rows + 255) / 256, B), dim3(256), 0, stream, S, rows, conf_thres, multi,
                                                    class_allow, keys_a, L.cap, count)) return err;
  const dim3 sweep((unsigned)((L.cap + 4095) / 4096 < 128 ? (L.cap + 4095) / 4096 : 128), B);   // 16 keys per thread at least
  if (int err = sodt_launch<nmsb_hist_kernel<1>>(sweep, dim3(256), 0, stream, keys_a, L.cap, count, hist)) return err;
  if (int err = sodt_launch<nmsb_hist_kernel<2>>(sweep, dim3(256), 0, stream, keys_a, L.cap, count, hist)) return err;
  if (int err = sodt_launch<nmsb_select_kernel>(sweep, dim3(256), 0, stream, keys_a, L.cap, count, hist, keys_b, nsel)) return err;
  rocprim::double_buffer<uint64_t> keys(keys_b, keys_a);       // the candidates themselves are not needed any more
  size_t tb = L.sort_tmp_bytes;
  if (sort_segments(base + L.sort_tmp, tb, keys, (unsigned)B, (unsigned)L.cap, nsel, stream) != hipSuccess) return SODT_ELAUNCH;
  const uint64_t* sorted = keys.current();
  if (int err = sodt_launch<nmsb_gather_kernel>(dim3((L.nmax + 255) / 256, B), dim3(256), 0, stream, S, sorted, L.cap, count, L.nmax,
                                                agnostic, det, boxes)) return err;
  if (int err = sodt_launch<nmsb_greedy_kernel>(dim3(B), dim3(GREEDY_TPB), 0, stream, boxes, count, L.nmax, iou_thres, keep, nkeep))
    return err;
  if (int err = sodt_launch<nmsb_merge_kernel>(dim3(MAX_DET, B), dim3(64), 0, stream, det, boxes, count, L.nmax, keep, nkeep,
                                               iou_thres, rws, valid)) return err;
  return sodt_launch<nmsb_pack_kernel>(dim3(1), dim3(1024), 0, stream, rws, valid, keep, nkeep, sorted, L.cap, B, out_rows,
                                       out_index, out_off);
}
