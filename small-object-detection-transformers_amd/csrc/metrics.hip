// Validation statistics on the GPU: the per-image true-positive matching of test.py:155-240 and ap_per_class /
// compute_ap of basics/utils/metrics.py:18-106.
//
// Bit-exactness: scale_coords / xywh2xyxy / box_iou are evaluated with the reference's f32 operations in its order
// (build.py compiles this file with -ffp-contract=off: the pragma below alone does not stop the backend from fusing
// under the global -ffp-contract=fast; true divisions), so `correct` is identical to the reference's.  The AP side runs
// in f64 with numpy's operation order (np.interp's bracket rule, np.trapz's pairwise sum, the sequential class mean).
//
// sodt_eval_match (one launch sequence per batch):
//   match_keys    : one thread per target; key = image index (B for rows of no image in the batch)
//   rocprim radix sort of (key, row) pairs - stable, so each image's targets keep the reference's row order (ti)
//   match_offsets : per-image [toff[b], toff[b+1]) by lower_bound on the sorted keys
//   match_image   : one workgroup per image: scale the image's targets, then one thread per prediction takes the
//                   best same-class target (lowest index on ties, like torch's CPU max(1)) and claims it with
//                   atomicMin(row); a prediction is a true positive iff it is the lowest row that claimed its target.
//   The last step is the reference's greedy walk (test.py:226-237) without the walk: a prediction's best target never
//   depends on what earlier predictions took, and a taken target is only skipped, so within a class the target goes to
//   the first prediction in NMS row order whose best target it is.  Targets of different classes never compete, so one
//   claim array serves every class at once.
//
// sodt_ap_per_class:
//   ap_hist       : n_l / n_p per class, composite sort key (class << 32 | descending-confidence bits)
//   rocprim radix sort of (key, row) pairs: class segments, descending confidence, ties in input row order
//   ap_classes    : segment starts, the unique target classes in ascending order (np.unique), nt (np.bincount)
//   ap_scan       : one workgroup per class: chunked block scans of the 10 TP columns (forward) and of the
//                   precision envelope (backward, compute_ap's reversed np.maximum.accumulate)
//   ap_curves     : one workgroup per class: r / p at the 1000 points of np.linspace(0, 1, 1000) and the 10 APs
//   ap_finalize   : f1, the first argmax of f1.mean(0), p / r / f1 at that index
//
// sodt_confusion_update (ConfusionMatrix.process_batch, metrics.py:117-155, for a whole batch):
//   match_keys / radix sort / match_offsets as above, then
//   confusion_image : one workgroup per image over IoU tiles in LDS.  The reference's two "sort by IoU, np.unique"
//                   passes are two argmax reductions: per detection over its labels, then per label over the
//                   detections that kept it.  Each is an atomicMax on a (IoU bits, ~index) word, so equal IoUs go to
//                   the lower label, then the lower detection (the reference's argsort leaves them unordered).  The
//                   counts go through an LDS histogram into an integer matrix: the result does not depend on the order
//                   of images or of workgroups.
#pragma clang fp contract(off)
#include <climits>
#include <rocprim/block/block_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int NIOU = 10;            // torch.linspace(0.5, 0.95, 10) (test.py:100)
constexpr int NPX = 1000;           // px = np.linspace(0, 1, 1000) (metrics.py:40)
constexpr int NAP = 101;            // x = np.linspace(0, 1, 101) (metrics.py:97)
constexpr int MAX_CLASSES = 4096;   // per-class curves are (nc, 1000) f64 in the workspace
constexpr long MAX_ROWS = 1L << 27; // predictions / targets per call (the (n, 10) f64 envelope stays < 11 GB)
constexpr int TPB = 256;
constexpr int IPT = 4;              // items per thread of one chunk of the block scans

struct Thr { float v[NIOU]; };

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

inline unsigned bits_for(unsigned long v) {   // bits to hold the values 0..v
  unsigned b = 1;
  while ((1ul << b) <= v) ++b;
  return b;
}

// ---------------------------------------------------------------------------------------------------------------
// matching

// torch's clamp_(lo, hi) (general.py:348-352): min(max(v, lo), hi), NaN kept
__device__ __forceinline__ float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// scale_coords (general.py:323-336) with ratio_pad = ((gain, _), (padw, padh)): f32 subtract, true divide, clip
__device__ __forceinline__ float4 scale_box(float x1, float y1, float x2, float y2, const float* g) {
  const float h0 = g[0], w0 = g[1], gain = g[2], pw = g[3], ph = g[4];
  x1 = (x1 - pw) / gain; y1 = (y1 - ph) / gain; x2 = (x2 - pw) / gain; y2 = (y2 - ph) / gain;
  return make_float4(clampf(x1, 0.f, w0), clampf(y1, 0.f, h0), clampf(x2, 0.f, w0), clampf(y2, 0.f, h0));
}

// box_iou (general.py:392-414) for one pair: inter / ((area1 + area2) - inter)
__device__ __forceinline__ float box_iou1(const float4 a, const float4 b) {
  const float a1 = (a.z - a.x) * (a.w - a.y), a2 = (b.z - b.x) * (b.w - b.y);
  const float w = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
  const float h = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
  const float inter = w * h;
  return inter / ((a1 + a2) - inter);
}

__global__ __launch_bounds__(256) void match_keys_kernel(const float* __restrict__ tg, int nt, int B,
                                                        uint32_t* __restrict__ keys, uint32_t* __restrict__ rows) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nt) return;
  const float im = tg[(long)t * 6];
  keys[t] = (im >= 0.f && im < (float)B && im == floorf(im)) ? (uint32_t)im : (uint32_t)B;   // targets[:, 0] == si
  rows[t] = (uint32_t)t;
}

__global__ __launch_bounds__(256) void match_offsets_kernel(const uint32_t* __restrict__ keys, int nt, int B,
                                                           int* __restrict__ toff) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b > B) return;
  int lo = 0, hi = nt;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < (uint32_t)b) lo = mid + 1; else hi = mid;
  }
  toff[b] = lo;
}

__global__ __launch_bounds__(TPB) void match_image_kernel(const float* __restrict__ det, const int* __restrict__ det_off,
                                                         int n_det, int B, const float* __restrict__ tg, int nt,
                                                         const uint32_t* __restrict__ trow, const int* __restrict__ toff,
                                                         const float* __restrict__ geom, Thr thr,
                                                         float4* __restrict__ tbox, float* __restrict__ tcls_g,
                                                         int* __restrict__ claim, int* __restrict__ best_t,
                                                         float* __restrict__ best_iou, unsigned char* __restrict__ correct,
                                                         float* __restrict__ tcls_out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* g = geom + (long)b * 5;
  const int t0 = toff[b], t1 = toff[b + 1];
  // targets of this image: xywh2xyxy (general.py:269-276) then scale_coords (test.py:218-219)
  for (int t = t0 + tid; t < t1; t += TPB) {
    const float* r = tg + (long)trow[t] * 6;
    const float x = r[2], y = r[3], w = r[4], h = r[5];
    tbox[t] = scale_box(x - w / 2, y - h / 2, x + w / 2, y + h / 2, g);
    tcls_g[t] = r[1];
    tcls_out[t] = r[1];
    claim[t] = INT_MAX;
  }
  if (b == 0)   // rows of no image in the batch: never matched, marked as padding (-1) in the target-class output
    for (int t = toff[B] + tid; t < nt; t += TPB) tcls_out[t] = -1.f;
  __syncthreads();
  const int d0 = min(max(det_off[b], 0), n_det), d1 = min(max(det_off[b + 1], d0), n_det);
  for (int p = d0 + tid; p < d1; p += TPB) {
    const float* r = det + (long)p * 6;
    const float4 pb = scale_box(r[0], r[1], r[2], r[3], g);   // test.py:170
    const float pc = r[5];
    int bt = -1; float bi = 0.f;
    for (int t = t0; t < t1; ++t) {   // ti in row order; the first maximum wins (NaN counts as the maximum, as in torch)
      if (tcls_g[t] != pc) continue;
      const float v = box_iou1(pb, tbox[t]);
      if (bt < 0 || v > bi || (v != v && bi == bi)) { bt = t; bi = v; }
    }
    if (bt >= 0 && bi > thr.v[0]) atomicMin(&claim[bt], p);   // test.py:229 (ious > iouv[0])
    else bt = -1;
    best_t[p] = bt; best_iou[p] = bi;
  }
  __syncthreads();
  // test.py:230-237.  The reference also stops a class's walk once len(detected) == nl; by then every target of the
  // image is in `detected`, so every later candidate of the class is in detected_set and would be skipped anyway: the
  // break never changes `correct`, and it has no counterpart here.
  for (int p = d0 + tid; p < d1; p += TPB) {
    const int bt = best_t[p];
    const bool tp = bt >= 0 && claim[bt] == p;
    const float bi = best_iou[p];
    unsigned char* o = correct + (long)p * NIOU;
#pragma unroll
    for (int k = 0; k < NIOU; ++k) o[k] = tp && bi > thr.v[k];   // ious[j] > iouv, strict
  }
}

struct match_layout {
  size_t keys_in, keys_out, rows_in, rows_out, sort_tmp, sort_tmp_bytes, toff, tbox, tcls, claim, best_t, best_iou, total;
};

int match_layout_of(int B, long n_det, long nt, match_layout& L) {
  if (B <= 0 || n_det < 0 || nt < 0 || n_det > MAX_ROWS || nt > MAX_ROWS) return SODT_EINVAL;
  size_t tb = 0;
  if (nt > 0 && rocprim::radix_sort_pairs<rocprim::default_config, const uint32_t*, uint32_t*, const uint32_t*, uint32_t*>(
                    nullptr, tb, nullptr, nullptr, nullptr, nullptr, (size_t)nt, 0, bits_for((unsigned long)B)) != hipSuccess)
    return SODT_ELAUNCH;
  size_t o = 0;
  L.keys_in = o; o += align256((size_t)nt * 4);
  L.keys_out = o; o += align256((size_t)nt * 4);
  L.rows_in = o; o += align256((size_t)nt * 4);
  L.rows_out = o; o += align256((size_t)nt * 4);
  L.sort_tmp = o; L.sort_tmp_bytes = tb; o += align256(tb);
  L.toff = o; o += align256((size_t)(B + 1) * 4);
  L.tbox = o; o += align256((size_t)nt * 16);
  L.tcls = o; o += align256((size_t)nt * 4);
  L.claim = o; o += align256((size_t)nt * 4);
  L.best_t = o; o += align256((size_t)n_det * 4);
  L.best_iou = o; o += align256((size_t)n_det * 4);
  L.total = o;
  return SODT_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// ap_per_class

struct Cnt10 { int c[NIOU]; };
struct Dbl10 { double v[NIOU]; };
struct AddCnt10 {
  __device__ Cnt10 operator()(const Cnt10& a, const Cnt10& b) const {
    Cnt10 r;
#pragma unroll
    for (int j = 0; j < NIOU; ++j) r.c[j] = a.c[j] + b.c[j];
    return r;
  }
};
struct MaxDbl10 {
  __device__ Dbl10 operator()(const Dbl10& a, const Dbl10& b) const {
    Dbl10 r;
#pragma unroll
    for (int j = 0; j < NIOU; ++j) r.v[j] = a.v[j] > b.v[j] ? a.v[j] : b.v[j];
    return r;
  }
};
struct Int2 { int a, b; };
struct AddInt2 {
  __device__ Int2 operator()(const Int2& x, const Int2& y) const { return Int2{x.a + y.a, x.b + y.b}; }
};

// class c is an integral value in [0, nc); everything else returns -1
__device__ __forceinline__ int class_id(float c, int nc) {
  return (c >= 0.f && c < (float)nc && c == floorf(c)) ? (int)c : -1;
}

// ascending key order == descending confidence (the float bits made monotonic, then inverted)
__device__ __forceinline__ uint32_t desc_conf_bits(float c) {
  const uint32_t u = __float_as_uint(c);
  const uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

__global__ __launch_bounds__(256) void ap_hist_kernel(const unsigned char* __restrict__ tp, const float* __restrict__ conf,
                                                     const float* __restrict__ pred_cls, int n,
                                                     const float* __restrict__ target_cls, int nt, int nc,
                                                     uint64_t* __restrict__ keys, uint32_t* __restrict__ rows,
                                                     int* __restrict__ n_l, int* __restrict__ n_p, int* __restrict__ info) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < nt) {
    const float c = target_cls[i];
    if (!(c < 0.f)) {   // negative target classes are padding rows (sodt_eval_match's rows of no image)
      const int ci = class_id(c, nc);
      if (ci >= 0) atomicAdd(&n_l[ci], 1); else atomicAdd(&info[1], 1);
    }
  }
  if (i < n) {
    int ci = class_id(pred_cls[i], nc);
    if (ci >= 0) atomicAdd(&n_p[ci], 1); else ci = nc;   // a class no target can have: sorted last, never read
    keys[i] = ((uint64_t)ci << 32) | desc_conf_bits(conf[i]);
    rows[i] = (uint32_t)i;
    const unsigned char* r = tp + (long)i * NIOU;
    int any = 0;
#pragma unroll
    for (int j = 0; j < NIOU; ++j) any |= r[j];
    if (any) atomicAdd(&info[2], 1);
  }
}

// one workgroup: segment starts (exclusive scan of n_p), ascending unique target classes (np.unique), nt
__global__ __launch_bounds__(TPB) void ap_classes_kernel(const int* __restrict__ n_l, const int* __restrict__ n_p, int nc,
                                                        int* __restrict__ seg, int* __restrict__ ci_of,
                                                        int* __restrict__ classes, int* __restrict__ nt_count,
                                                        int* __restrict__ info) {
  using Scan = rocprim::block_scan<Int2, TPB>;
  __shared__ typename Scan::storage_type st;
  Int2 carry{0, 0};
  for (int c0 = 0; c0 < nc; c0 += TPB) {
    const int c = c0 + threadIdx.x;
    const Int2 v = c < nc ? Int2{n_p[c], n_l[c] > 0} : Int2{0, 0};
    Int2 incl, tot;
    Scan().inclusive_scan(v, incl, tot, st, AddInt2());
    if (c < nc) {
      seg[c] = carry.a + incl.a - v.a;
      const int u = carry.b + incl.b - v.b;
      ci_of[c] = v.b ? u : -1;
      if (v.b) classes[u] = c;
      nt_count[c] = n_l[c];
    }
    carry = AddInt2()(carry, tot);
    __syncthreads();
  }
  if (threadIdx.x == 0) { seg[nc] = carry.a; info[0] = carry.b; }
}

// one workgroup per class: tpc = tp.cumsum(0) per column (metrics.py:53-54) and the precision envelope of compute_ap
// (metrics.py:91-94), both as chunked block scans of 10-column vectors; also gathers the sorted confidences.
__global__ __launch_bounds__(TPB) void ap_scan_kernel(const unsigned char* __restrict__ tp, const float* __restrict__ conf,
                                                     const uint32_t* __restrict__ order, const int* __restrict__ seg,
                                                     const int* __restrict__ n_l, int* __restrict__ tpc,
                                                     double* __restrict__ env, float* __restrict__ conf_s) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const long s0 = seg[c];
  const int np = seg[c + 1] - seg[c];
  if (n_l[c] == 0 || np == 0) return;
  using ScanC = rocprim::block_scan<Cnt10, TPB>;
  using ScanD = rocprim::block_scan<Dbl10, TPB>;
  __shared__ union { typename ScanC::storage_type c; typename ScanD::storage_type d; } st;
  constexpr int CHUNK = TPB * IPT;

  Cnt10 carry;
#pragma unroll
  for (int j = 0; j < NIOU; ++j) carry.c[j] = 0;
  for (int base = 0; base < np; base += CHUNK) {
    Cnt10 run, loc[IPT];
#pragma unroll
    for (int j = 0; j < NIOU; ++j) run.c[j] = 0;
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
      const int i = base + tid * IPT + q;
      if (i < np) {
        const uint32_t row = order[s0 + i];
        const unsigned char* r = tp + (long)row * NIOU;
#pragma unroll
        for (int j = 0; j < NIOU; ++j) run.c[j] += r[j] != 0;
        conf_s[s0 + i] = conf[row];
      }
      loc[q] = run;
    }
    Cnt10 incl, tot;
    ScanC().inclusive_scan(run, incl, tot, st.c, AddCnt10());
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
      const int i = base + tid * IPT + q;
      if (i < np) {
        int* o = tpc + (s0 + i) * NIOU;
#pragma unroll
        for (int j = 0; j < NIOU; ++j) o[j] = carry.c[j] + (incl.c[j] - run.c[j]) + loc[q].c[j];
      }
    }
    carry = AddCnt10()(carry, tot);
    __syncthreads();
  }
  __syncthreads();   // tpc written by other threads is read below

  // env[i][j] = max(precision[i..np-1][j], 0): the reversed running maximum of [1, precision, 0] without its sentinels
  Dbl10 dcarry;
#pragma unroll
  for (int j = 0; j < NIOU; ++j) dcarry.v[j] = 0.0;
  for (int top = np; top > 0; top -= CHUNK) {
    Dbl10 run, loc[IPT];
#pragma unroll
    for (int j = 0; j < NIOU; ++j) run.v[j] = 0.0;
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
      const int i = top - 1 - (tid * IPT + q);
      if (i >= 0) {
        const int* t = tpc + (s0 + i) * NIOU;
#pragma unroll
        for (int j = 0; j < NIOU; ++j) {
          const double pr = (double)t[j] / (double)(i + 1);   // tpc / (tpc + fpc), fpc = (1 - tp).cumsum(0)
          run.v[j] = pr > run.v[j] ? pr : run.v[j];
        }
      }
      loc[q] = run;
    }
    Dbl10 excl, tot;
    ScanD().exclusive_scan(run, excl, dcarry, tot, st.d, MaxDbl10());
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
      const int i = top - 1 - (tid * IPT + q);
      if (i >= 0) {
        const Dbl10 e = MaxDbl10()(excl, loc[q]);
        double* o = env + (s0 + i) * NIOU;
#pragma unroll
        for (int j = 0; j < NIOU; ++j) o[j] = e.v[j];
      }
    }
    dcarry = MaxDbl10()(dcarry, tot);
    __syncthreads();
  }
}

// np.interp (numpy/_core/src/multiarray/compiled_base.c, arr_interp) for one x over a non-decreasing xp: j is the
// largest index with xp[j] <= x (binary_search_with_guess), so a run of repeated xp values resolves to its last entry.
template <class XP, class FP>
__device__ double np_interp(double x, long len, XP xp, FP fp, double left, double right) {
  if (x > xp(len - 1)) return right;
  if (x < xp(0)) return left;
  long lo = 0, hi = len;
  while (lo < hi) {
    const long mid = lo + ((hi - lo) >> 1);
    if (x >= xp(mid)) lo = mid + 1; else hi = mid;
  }
  const long j = lo - 1;
  if (j == len - 1 || xp(j) == x) return fp(j);
  const double slope = (fp(j + 1) - fp(j)) / (xp(j + 1) - xp(j));
  double r = slope * (x - xp(j)) + fp(j);
  if (r != r) {
    r = slope * (x - xp(j + 1)) + fp(j + 1);
    if (r != r && fp(j) == fp(j + 1)) r = fp(j);
  }
  return r;
}

__device__ __forceinline__ double px_at(int k) { return k == NPX - 1 ? 1.0 : (double)k * (1.0 / (NPX - 1)); }
__device__ __forceinline__ double ax_at(int k) { return k == NAP - 1 ? 1.0 : (double)k * (1.0 / (NAP - 1)); }

// numpy's pairwise sum (8 accumulators) of n <= 128 doubles, plus the reduction's identity 0
__device__ double np_sum_small(const double* a, int n) {
  double res;
  int i;
  if (n < 8) {
    res = 0.0;
    for (i = 0; i < n; ++i) res += a[i];
    return 0.0 + res;
  }
  double r[8];
  for (int k = 0; k < 8; ++k) r[k] = a[k];
  for (i = 8; i < n - (n % 8); i += 8)
    for (int k = 0; k < 8; ++k) r[k] += a[i + k];
  res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return 0.0 + res;
}

// one workgroup per class: r[ci], p[ci] at px (metrics.py:57-62) and ap[ci, 0..9] (compute_ap, metrics.py:84-99)
__global__ __launch_bounds__(TPB) void ap_curves_kernel(const int* __restrict__ seg, const int* __restrict__ n_l,
                                                       const int* __restrict__ ci_of, const int* __restrict__ tpc,
                                                       const double* __restrict__ env, const float* __restrict__ conf_s,
                                                       double* __restrict__ pcurve, double* __restrict__ rcurve,
                                                       double* __restrict__ ap) {
  const int c = blockIdx.x, tid = threadIdx.x;
  const int ci = ci_of[c];
  if (ci < 0) return;
  const long s0 = seg[c];
  const long np = seg[c + 1] - seg[c];
  double* pr = pcurve + (long)ci * NPX;
  double* rr = rcurve + (long)ci * NPX;
  if (np == 0) {   // metrics.py:50-51: the row stays zero
    for (int k = tid; k < NPX; k += TPB) { pr[k] = 0.0; rr[k] = 0.0; }
    if (tid < NIOU) ap[(long)ci * NIOU + tid] = 0.0;
    return;
  }
  const double nl = (double)n_l[c] + 1e-16;
  const int* t = tpc + s0 * NIOU;
  const double* e = env + s0 * NIOU;
  const float* cf = conf_s + s0;
  auto xp = [=](long i) { return -(double)cf[i]; };
  auto rec0 = [=](long i) { return (double)t[i * NIOU] / nl; };
  auto pre0 = [=](long i) { return (double)t[i * NIOU] / (double)(i + 1); };
  for (int k = tid; k < NPX; k += TPB) {
    const double x = -px_at(k);
    rr[k] = np_interp(x, np, xp, rec0, 0.0, rec0(np - 1));
    pr[k] = np_interp(x, np, xp, pre0, 1.0, pre0(np - 1));
  }
  __shared__ double y[NIOU][NAP];
  __shared__ double term[NIOU][NAP - 1];
  for (int q = tid; q < NIOU * NAP; q += TPB) {
    const int j = q / NAP, k = q - j * NAP;
    const double rlast = (double)t[(np - 1) * NIOU + j] / nl;
    // mrec = [0, recall, recall[-1] + 0.01], mpre = envelope of [1, precision, 0]
    auto mrec = [=](long i) { return i == 0 ? 0.0 : (i == np + 1 ? rlast + 0.01 : (double)t[(i - 1) * NIOU + j] / nl); };
    auto mpre = [=](long i) { return i == 0 ? 1.0 : (i == np + 1 ? 0.0 : e[(i - 1) * NIOU + j]); };
    y[j][k] = np_interp(ax_at(k), np + 2, mrec, mpre, 1.0, 0.0);
  }
  __syncthreads();
  for (int q = tid; q < NIOU * (NAP - 1); q += TPB) {   // np.trapz: (d * (y[1:] + y[:-1])) / 2.0
    const int j = q / (NAP - 1), k = q - j * (NAP - 1);
    term[j][k] = ((ax_at(k + 1) - ax_at(k)) * (y[j][k + 1] + y[j][k])) / 2.0;
  }
  __syncthreads();
  if (tid < NIOU) ap[(long)ci * NIOU + tid] = np_sum_small(term[tid], NAP - 1);
}

__device__ __forceinline__ double f1_of(double p, double r) { return ((2.0 * p) * r) / ((p + r) + 1e-16); }

// f1 = 2pr / (p + r + 1e-16); i = f1.mean(0).argmax() (the first maximum); p, r, f1 at i (metrics.py:66-75)
__global__ __launch_bounds__(1024) void ap_finalize_kernel(const double* __restrict__ pcurve, const double* __restrict__ rcurve,
                                                          int* __restrict__ info, double* __restrict__ p,
                                                          double* __restrict__ r, double* __restrict__ f1) {
  __shared__ double sv[1024];
  __shared__ int si[1024];
  const int tid = threadIdx.x, nu = info[0];
  if (nu == 0) { if (tid == 0) info[3] = 0; return; }
  double m = -1.0;
  if (tid < NPX) {
    double s = 0.0;
    for (int ci = 0; ci < nu; ++ci) s += f1_of(pcurve[(long)ci * NPX + tid], rcurve[(long)ci * NPX + tid]);
    m = s / (double)nu;
  }
  sv[tid] = m; si[tid] = tid;
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if (tid < w) {
      const double a = sv[tid], b = sv[tid + w];
      if (b > a || (b == a && si[tid + w] < si[tid])) { sv[tid] = b; si[tid] = si[tid + w]; }
    }
    __syncthreads();
  }
  const int k = si[0];
  for (int ci = tid; ci < nu; ci += 1024) {
    const double pp = pcurve[(long)ci * NPX + k], rr = rcurve[(long)ci * NPX + k];
    p[ci] = pp; r[ci] = rr; f1[ci] = f1_of(pp, rr);
  }
  if (tid == 0) info[3] = k;
}

struct ap_layout {
  size_t keys_in, keys_out, rows_in, rows_out, sort_tmp, sort_tmp_bytes, n_l, n_p, seg, ci_of, tpc, env, conf_s, pcurve,
      rcurve, total;
};

int ap_layout_of(long n, long nt, int nc, ap_layout& L) {
  if (n < 0 || nt < 0 || n > MAX_ROWS || nt > MAX_ROWS || nc <= 0 || nc > MAX_CLASSES) return SODT_EINVAL;
  size_t tb = 0;
  if (n > 0 && rocprim::radix_sort_pairs<rocprim::default_config, const uint64_t*, uint64_t*, const uint32_t*, uint32_t*>(
                   nullptr, tb, nullptr, nullptr, nullptr, nullptr, (size_t)n, 0, 32 + bits_for((unsigned long)nc)) != hipSuccess)
    return SODT_ELAUNCH;
  size_t o = 0;
  L.keys_in = o; o += align256((size_t)n * 8);
  L.keys_out = o; o += align256((size_t)n * 8);
  L.rows_in = o; o += align256((size_t)n * 4);
  L.rows_out = o; o += align256((size_t)n * 4);
  L.sort_tmp = o; L.sort_tmp_bytes = tb; o += align256(tb);
  L.n_l = o; o += align256((size_t)(nc + 1) * 4);
  L.n_p = o; o += align256((size_t)(nc + 1) * 4);
  L.seg = o; o += align256((size_t)(nc + 1) * 4);
  L.ci_of = o; o += align256((size_t)nc * 4);
  L.tpc = o; o += align256((size_t)n * NIOU * 4);
  L.env = o; o += align256((size_t)n * NIOU * 8);
  L.conf_s = o; o += align256((size_t)n * 4);
  L.pcurve = o; o += align256((size_t)nc * NPX * 8);
  L.rcurve = o; o += align256((size_t)nc * NPX * 8);
  L.total = o;
  return SODT_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// confusion matrix

constexpr int CF_LT = 64;       // labels of one LDS tile: one per lane of a wave
constexpr int CF_DT = 256;      // detections of one LDS tile
constexpr int CF_HIST = 8192;   // a matrix of up to this many cells (nc <= 89) is counted in LDS first

// the float bits made monotonic: a < b  <=>  asc_bits(a) < asc_bits(b) for non-NaN a, b
__device__ __forceinline__ uint32_t asc_bits(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// A candidate pair as one word for atomicMax: the higher IoU wins, then the lower index of the other side.  Never 0.
__device__ __forceinline__ unsigned long long pair_key(uint32_t iou_bits, int other) {
  return ((unsigned long long)iou_bits << 32) | (0xFFFFFFFFu - (uint32_t)other);
}
__device__ __forceinline__ int key_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }
// keys are written by atomics at L2; read them there too
__device__ __forceinline__ unsigned long long key_load(const unsigned long long* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per image.  IoU tiles of CF_DT detections x CF_LT labels: lane l of every wave holds label l of the
// tile in registers, the waves stride over the tile's detections (a wave-uniform LDS read).
//   1. column reduction: dkey[p] = max over the image's labels of pair_key(iou, label), iou > iou_thres
//   2. row reduction over the survivors: lkey[t] = max over detections whose best label is t of pair_key(iou, p)
//   3. labels: matched -> [gc, dc], else [nc, gc]
//   4. if any label matched: kept detections that are not their label's winner -> [dc, nc]
__global__ __launch_bounds__(TPB) void confusion_image_kernel(
    const float* __restrict__ det, const int* __restrict__ det_off, int n_det, const float* __restrict__ tg,
    const uint32_t* __restrict__ trow, const int* __restrict__ toff, const float* __restrict__ geom, int nc, float conf,
    float iou_thres, float4* __restrict__ tbox, unsigned long long* __restrict__ dkey, unsigned long long* __restrict__ lkey,
    unsigned long long* __restrict__ matrix, int* __restrict__ info) {
  __shared__ float4 s_det[CF_DT];
  __shared__ float4 s_lab[CF_LT];
  __shared__ unsigned char s_keep[CF_DT];
  __shared__ int s_hist[CF_HIST];
  __shared__ int s_any;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n1 = nc + 1, cells = n1 * n1;
  const bool hist = cells <= CF_HIST;
  const float* g = geom ? geom + (long)b * 5 : nullptr;
  const int t0 = toff[b], t1 = toff[b + 1];
  const int d0 = min(max(det_off[b], 0), n_det), d1 = min(max(det_off[b + 1], d0), n_det);
  auto count = [&](int r, int c) {   // a class outside [0, nc) arrives as -1: reported in info, never written
    if (r < 0 || c < 0) return;
    if (hist) atomicAdd(&s_hist[r * n1 + c], 1);
    else atomicAdd(&matrix[(long)r * n1 + c], 1ull);
  };

  if (hist) for (int i = tid; i < cells; i += TPB) s_hist[i] = 0;
  if (tid == 0) s_any = 0;
  for (int t = t0 + tid; t < t1; t += TPB) {
    const float* r = tg + (long)trow[t] * 6;
    // with geometry: xywh2xyxy then scale_coords, as match_image_kernel; without: the row holds x1 y1 x2 y2 as they are
    tbox[t] = g ? scale_box(r[2] - r[4] / 2, r[3] - r[5] / 2, r[2] + r[4] / 2, r[3] + r[5] / 2, g)
                : make_float4(r[2], r[3], r[4], r[5]);
    lkey[t] = 0;
  }
  for (int p = d0 + tid; p < d1; p += TPB) dkey[p] = 0;

  for (int dt = d0; dt < d1; dt += CF_DT) {
    const int nd = min(CF_DT, d1 - dt);
    __syncthreads();   // the previous tile has been consumed; the first time: tbox / dkey / lkey are written
    if (tid < nd) {
      const float* r = det + (long)(dt + tid) * 6;
      s_det[tid] = g ? scale_box(r[0], r[1], r[2], r[3], g) : make_float4(r[0], r[1], r[2], r[3]);
      s_keep[tid] = r[4] > conf;   // metrics.py:127, strict
    }
    for (int lt = t0; lt < t1; lt += CF_LT) {
      const int nl = min(CF_LT, t1 - lt);
      __syncthreads();
      if (tid < nl) s_lab[tid] = tbox[lt + tid];
      __syncthreads();
      const int l = tid & (CF_LT - 1);
      if (l < nl) {
        const float4 lb = s_lab[l];
        for (int d = tid / CF_LT; d < nd; d += TPB / CF_LT) {
          if (!s_keep[d]) continue;
          const float v = box_iou1(lb, s_det[d]);   // box_iou(labels, detections), metrics.py:130
          if (v > iou_thres) atomicMax(&dkey[dt + d], pair_key(asc_bits(v), lt + l));
        }
      }
    }
  }
  __syncthreads();
  for (int p = d0 + tid; p < d1; p += TPB) {
    const unsigned long long k = key_load(&dkey[p]);
    if (k) atomicMax(&lkey[key_index(k)], pair_key((uint32_t)(k >> 32), p));
  }
  __syncthreads();
  for (int t = t0 + tid; t < t1; t += TPB) {
    const int gc = class_id(tg[(long)trow[t] * 6 + 1], nc);
    if (gc < 0) atomicAdd(&info[0], 1);
    const unsigned long long k = key_load(&lkey[t]);
    if (k) {
      s_any = 1;
      count(gc, class_id(det[(long)key_index(k) * 6 + 5], nc));   // metrics.py:148
    } else {
      count(nc, gc);                                              // metrics.py:150
    }
  }
  __syncthreads();
  const bool any = s_any != 0;   // metrics.py:152, `if n:`
  for (int p = d0 + tid; p < d1; p += TPB) {
    const float* r = det + (long)p * 6;
    if (!(r[4] > conf)) continue;
    const int dc = class_id(r[5], nc);
    if (dc < 0) atomicAdd(&info[1], 1);
    const unsigned long long k = key_load(&dkey[p]);
    const bool won = k && key_index(key_load(&lkey[key_index(k)])) == p;
    if (any && !won) count(dc, nc);                               // metrics.py:155
  }
  if (!hist) return;
  __syncthreads();
  for (int i = tid; i < cells; i += TPB) {
    const int v = s_hist[i];
    if (v) atomicAdd(&matrix[i], (unsigned long long)v);
  }
}

struct confusion_layout { size_t keys_in, keys_out, rows_in, rows_out, sort_tmp, sort_tmp_bytes, toff, tbox, dkey, lkey, total; };

int confusion_layout_of(int B, long n_det, long nt, confusion_layout& L) {
  if (B <= 0 || n_det < 0 || nt < 0 || n_det > MAX_ROWS || nt > MAX_ROWS) return SODT_EINVAL;
  size_t tb = 0;
  if (nt > 0 && rocprim::radix_sort_pairs<rocprim::default_config, const uint32_t*, uint32_t*, const uint32_t*, uint32_t*>(
                    nullptr, tb, nullptr, nullptr, nullptr, nullptr, (size_t)nt, 0, bits_for((unsigned long)B)) != hipSuccess)
    return SODT_ELAUNCH;
  size_t o = 0;
  L.keys_in = o; o += align256((size_t)nt * 4);
  L.keys_out = o; o += align256((size_t)nt * 4);
  L.rows_in = o; o += align256((size_t)nt * 4);
  L.rows_out = o; o += align256((size_t)nt * 4);
  L.sort_tmp = o; L.sort_tmp_bytes = tb; o += align256(tb);
  L.toff = o; o += align256((size_t)(B + 1) * 4);
  L.tbox = o; o += align256((size_t)nt * 16);
  L.dkey = o; o += align256((size_t)n_det * 8);
  L.lkey = o; o += align256((size_t)nt * 8);
  L.total = o;
  return SODT_OK;
}

}  // namespace

extern "C" int sodt_eval_match_workspace_bytes(int B, long n_det, long nt, size_t* bytes) {
  match_layout L;
  if (!bytes || match_layout_of(B, n_det, nt, L) != SODT_OK) return SODT_EINVAL;
  *bytes = L.total;
  return SODT_OK;
}

extern "C" int sodt_eval_match(const float* det, const int* det_off, int B, long n_det, const float* targets, long nt,
                               const float* geom, const float* iouv, void* ws, size_t ws_bytes, unsigned char* correct,
                               float* tcls_out, hipStream_t stream) {
  match_layout L;
  if (!det_off || !geom || !iouv || !ws || (n_det > 0 && (!det || !correct)) || (nt > 0 && (!targets || !tcls_out)))
    return SODT_EINVAL;
  if (match_layout_of(B, n_det, nt, L) != SODT_OK || ws_bytes < L.total) return SODT_EINVAL;
  Thr thr;
  for (int k = 0; k < NIOU; ++k) thr.v[k] = iouv[k];   // host array
  char* base = (char*)ws;
  uint32_t* keys_in = (uint32_t*)(base + L.keys_in);
  uint32_t* keys_out = (uint32_t*)(base + L.keys_out);
  uint32_t* rows_in = (uint32_t*)(base + L.rows_in);
  uint32_t* rows_out = (uint32_t*)(base + L.rows_out);
  int* toff = (int*)(base + L.toff);
  const int ntt = (int)nt;
  if (ntt > 0) {
    if (int err = sodt_launch<match_keys_kernel>(dim3((ntt + 255) / 256), dim3(256), 0, stream, targets, ntt, B, keys_in, rows_in)) return err;
    size_t tb = L.sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(base + L.sort_tmp, tb, (const uint32_t*)keys_in, keys_out, (const uint32_t*)rows_in,
                                  rows_out, (size_t)ntt, 0, bits_for((unsigned long)B), stream) != hipSuccess)
      return SODT_ELAUNCH;
  }
  if (int err = sodt_launch<match_offsets_kernel>(dim3((B + 1 + 255) / 256), dim3(256), 0, stream, keys_out, ntt, B, toff)) return err;
  return sodt_launch<match_image_kernel>(B, TPB, 0, stream, det, det_off, (int)n_det, B, targets, ntt, rows_out, toff, geom, thr,
                                            (float4*)(base + L.tbox), (float*)(base + L.tcls), (int*)(base + L.claim),
                                            (int*)(base + L.best_t), (float*)(base + L.best_iou), correct, tcls_out);
}

extern "C" int sodt_ap_per_class_workspace_bytes(long n, long nt, int nc, size_t* bytes) {
  ap_layout L;
  if (!bytes || ap_layout_of(n, nt, nc, L) != SODT_OK) return SODT_EINVAL;
  *bytes = L.total;
  return SODT_OK;
}

extern "C" int sodt_ap_per_class(const unsigned char* tp, const float* conf, const float* pred_cls, long n,
                                 const float* target_cls, long nt, int nc, void* ws, size_t ws_bytes, double* p, double* r,
                                 double* f1, double* ap, int* classes, int* nt_count, int* info, hipStream_t stream) {
  ap_layout L;
  if (!ws || !p || !r || !f1 || !ap || !classes || !nt_count || !info || (n > 0 && (!tp || !conf || !pred_cls)) ||
      (nt > 0 && !target_cls))
    return SODT_EINVAL;
  if (ap_layout_of(n, nt, nc, L) != SODT_OK || ws_bytes < L.total) return SODT_EINVAL;
  char* base = (char*)ws;
  uint64_t* keys_in = (uint64_t*)(base + L.keys_in);
  uint64_t* keys_out = (uint64_t*)(base + L.keys_out);
  uint32_t* rows_in = (uint32_t*)(base + L.rows_in);
  uint32_t* rows_out = (uint32_t*)(base + L.rows_out);
  int* n_l = (int*)(base + L.n_l);
  int* n_p = (int*)(base + L.n_p);
  int* seg = (int*)(base + L.seg);
  int* ci_of = (int*)(base + L.ci_of);
  int* tpc = (int*)(base + L.tpc);
  double* env = (double*)(base + L.env);
  float* conf_s = (float*)(base + L.conf_s);
  double* pc = (double*)(base + L.pcurve);
  double* rc = (double*)(base + L.rcurve);
  // n_l, n_p and seg are adjacent: one clear covers the counters
  if (hipMemsetAsync(n_l, 0, L.seg - L.n_l, stream) != hipSuccess) return SODT_ELAUNCH;
  if (hipMemsetAsync(info, 0, 4 * sizeof(int), stream) != hipSuccess) return SODT_ELAUNCH;
  const long m = n > nt ? n : nt;
  if (m > 0)
    if (int err = sodt_launch<ap_hist_kernel>(dim3((int)((m + 255) / 256)), dim3(256), 0, stream, tp, conf, pred_cls, (int)n, target_cls, (int)nt, nc,
                                                              keys_in, rows_in, n_l, n_p, info)) return err;
  if (n > 0) {
    size_t tb = L.sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(base + L.sort_tmp, tb, (const uint64_t*)keys_in, keys_out, (const uint32_t*)rows_in,
                                  rows_out, (size_t)n, 0, 32 + bits_for((unsigned long)nc), stream) != hipSuccess)
      return SODT_ELAUNCH;
  }
  if (int err = sodt_launch<ap_classes_kernel>(dim3(1), TPB, 0, stream, n_l, n_p, nc, seg, ci_of, classes, nt_count, info)) return err;
  if (n > 0) { if (int err = sodt_launch<ap_scan_kernel>(nc, TPB, 0, stream, tp, conf, rows_out, seg, n_l, tpc, env, conf_s)) return err; }
  if (int err = sodt_launch<ap_curves_kernel>(nc, TPB, 0, stream, seg, n_l, ci_of, tpc, env, conf_s, pc, rc, ap)) return err;
  return sodt_launch<ap_finalize_kernel>(dim3(1), dim3(1024), 0, stream, pc, rc, info, p, r, f1);
}

extern "C" int sodt_confusion_update_workspace_bytes(int B, long n_det, long nt, size_t* bytes) {
  confusion_layout L;
  if (!bytes || confusion_layout_of(B, n_det, nt, L) != SODT_OK) return SODT_EINVAL;
  *bytes = L.total;
  return SODT_OK;
}

extern "C" int sodt_confusion_update(const float* det, const int* det_off, int B, long n_det, const float* targets, long nt,
                                     const float* geom, int nc, float conf, float iou_thres, void* ws, size_t ws_bytes,
                                     long long* matrix, int* info, hipStream_t stream) {
  confusion_layout L;
  if (!det_off || !ws || !matrix || !info || (n_det > 0 && !det) || (nt > 0 && !targets) || nc <= 0 || nc > MAX_CLASSES)
    return SODT_EINVAL;
  if (confusion_layout_of(B, n_det, nt, L) != SODT_OK || ws_bytes < L.total) return SODT_EINVAL;
  char* base = (char*)ws;
  uint32_t* keys_in = (uint32_t*)(base + L.keys_in);
  uint32_t* keys_out = (uint32_t*)(base + L.keys_out);
  uint32_t* rows_in = (uint32_t*)(base + L.rows_in);
  uint32_t* rows_out = (uint32_t*)(base + L.rows_out);
  int* toff = (int*)(base + L.toff);
  const int ntt = (int)nt;
  if (ntt > 0) {   // group the targets by image exactly as sodt_eval_match does: a stable sort keeps each image's row order
    if (int err = sodt_launch<match_keys_kernel>(dim3((ntt + 255) / 256), dim3(256), 0, stream, targets, ntt, B, keys_in, rows_in)) return err;
    size_t tb = L.sort_tmp_bytes;
    if (rocprim::radix_sort_pairs(base + L.sort_tmp, tb, (const uint32_t*)keys_in, keys_out, (const uint32_t*)rows_in,
                                  rows_out, (size_t)ntt, 0, bits_for((unsigned long)B), stream) != hipSuccess)
      return SODT_ELAUNCH;
  }
  if (int err = sodt_launch<match_offsets_kernel>(dim3((B + 1 + 255) / 256), dim3(256), 0, stream, keys_out, ntt, B, toff)) return err;
  return sodt_launch<confusion_image_kernel>(B, TPB, 0, stream, det, det_off, (int)n_det, targets, rows_out, toff, geom, nc, conf, iou_thres,
                                                (float4*)(base + L.tbox), (unsigned long long*)(base + L.dkey),
                                                (unsigned long long*)(base + L.lkey), (unsigned long long*)matrix, info);
}
