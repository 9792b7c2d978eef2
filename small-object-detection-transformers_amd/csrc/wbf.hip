// Weighted boxes fusion on the GPU: weighted_boxes of general.py:515-563 (the alternative to non_max_suppression at
// test.py:152-153) and the weighted_boxes_fusion it calls (ensemble_boxes/ensemble_boxes_wbf.py:150-225), for a whole
// batch of images per call.
//
// The clustering is sequential by definition - the fused box a candidate is compared with depends on every earlier
// decision - so the arithmetic of each decision is the reference's own: f32 coordinate accumulators updated through
// f64 (numpy's `f32 += f64` runs the f64 loop and rounds the result), the score sum in f64, the fused coordinate
// (float)((double)acc / sum), the IoU of the f32 boxes in f64.  This file is compiled with -ffp-contract=off.
//
// Pipeline (all on the caller's stream, no host read):
//   wbf_candidates : one thread per decoded row of the batch; compacts the passing rows of each image
//   three stable rocprim radix sorts: by source row (ties of the next one), by descending weighted score, by
//                    (image, label) -> every (image, label) segment is contiguous and in the reference's walk order
//   wbf_gather     : sorted copies of box / weighted score / weight / model
//   wbf_cluster    : one workgroup per (image, label) segment; per candidate all lanes scan the clusters formed so
//                    far, a block-wide argmax picks the match (IoU strictly above the threshold, the lowest cluster
//                    on equal IoUs), lane 0 appends or updates.  Clusters live at [segment start + creation index].
//   two stable radix sorts of the clusters: by descending score, then by image; wbf_output writes each image's rows
//   wbf_member     : (debug) the output row of the cluster each input candidate went into
#pragma clang fp contract(off)
#include <rocprim/device/device_radix_sort.hpp>
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int MAX_MODELS = 32;
constexpr int MAX_B = 65535;
constexpr uint64_t NO_KEY = ~0ull;

struct wbf_weights {
  double w[MAX_MODELS];
  double wsum;     // numpy's weights.sum()
  int n;
};

// numpy's float64 add.reduce over a contiguous array of n <= 128 elements: 0 + pairwise block (8 partial sums above 7)
__host__ __device__ inline double np_sum(const double* a, int n) {
  double res = 0.;
  if (n < 8) {
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
  for (int q = 0; q < 8; ++q) r[q] = a[q];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int q = 0; q < 8; ++q) r[q] += a[i + q];
  double s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) s += a[i];
  return res + s;
}

// ascending key order == descending value
__device__ __forceinline__ uint64_t desc_key(double v) {
  uint64_t b = (uint64_t)__double_as_longlong(v);
  b = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return ~b;
}

// general.py:523-544 for every row of the batch
__global__ __launch_bounds__(256) void wbf_candidates_kernel(const float* __restrict__ z, int N, int nc, float conf, float S,
                                                            float4* __restrict__ boxes, float* __restrict__ scores,
                                                            int* __restrict__ labels, int* __restrict__ src,
                                                            int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= N) return;
  const float* r = z + ((long)b * N + i) * (nc + 5);
  const float obj = r[4];
  if (!(obj > conf)) return;
  float best = r[5] * obj; int bj = 0;
  for (int j = 1; j < nc; ++j) {
    const float s = r[5 + j] * obj;
    if (s > best) { best = s; bj = j; }
  }
  if (!(best > conf)) return;
  const float cx = r[0] / S, cy = r[1] / S, w = r[2] / S, h = r[3] / S;
  const float hw = w / 2, hh = h / 2;
  const int slot = atomicAdd(&counts[b], 1);          // < N: at most one candidate per row
  const long o = (long)b * N + slot;
  boxes[o] = make_float4(cx - hw, cy - hh, cx + hw, cy + hh);
  scores[o] = best; labels[o] = bj; src[o] = i;
}

struct wbf_in {
  const float* scores; const int* labels; const int* model; const int* counts;
  long cap; float skip_thr; int n_models;
};

__device__ __forceinline__ bool wbf_valid(const wbf_in& in, uint32_t idx, int& b) {
  b = (int)(idx / in.cap);
  const long i = idx - (long)b * in.cap;
  if (i >= in.counts[b]) return false;
  if (in.scores[idx] < in.skip_thr) return false;      // ensemble_boxes_wbf.py:47 (equality stays in)
  if (in.model) { const int m = in.model[idx]; if (m < 0 || m >= in.n_models) return false; }
  return true;
}

__global__ __launch_bounds__(256) void wbf_key_src_kernel(const int* __restrict__ src, long P, uint32_t* __restrict__ key,
                                                         uint32_t* __restrict__ val) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  if (key) key[p] = (uint32_t)src[p];
  val[p] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void wbf_key_score_kernel(wbf_in in, wbf_weights W, const uint32_t* __restrict__ val, long P,
                                                           uint64_t* __restrict__ key) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const uint32_t idx = val[p];
  int b;
  uint64_t k = NO_KEY;
  if (wbf_valid(in, idx, b)) {
    const int m = in.model ? in.model[idx] : 0;
    double w = W.w[0];
#pragma unroll
    for (int q = 1; q < MAX_MODELS; ++q) w = (m == q) ? W.w[q] : w;
    k = desc_key((double)in.scores[idx] * w);          // ensemble_boxes_wbf.py:92
  }
  key[p] = k;
}

__global__ __launch_bounds__(256) void wbf_key_seg_kernel(wbf_in in, const uint32_t* __restrict__ val, long P,
                                                         uint64_t* __restrict__ key) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const uint32_t idx = val[p];
  int b;
  key[p] = wbf_valid(in, idx, b) ? (((uint64_t)b << 32) | (uint32_t)in.labels[idx]) : NO_KEY;
}

__global__ __launch_bounds__(256) void wbf_gather_kernel(wbf_in in, wbf_weights W, const float4* __restrict__ boxes,
                                                        const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm,
                                                        long P, float4* __restrict__ sbox, double* __restrict__ ss,
                                                        double* __restrict__ sw, int* __restrict__ smodel) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P || skey[p] == NO_KEY) return;
  const uint32_t idx = perm[p];
  const int m = in.model ? in.model[idx] : 0;
  double w = W.w[0];
#pragma unroll
  for (int q = 1; q < MAX_MODELS; ++q) w = (m == q) ? W.w[q] : w;
  sbox[p] = boxes[idx];
  ss[p] = (double)in.scores[idx] * w;
  sw[p] = w;
  smodel[p] = m;
}

// bb_intersection_over_union (ensemble_boxes_wbf.py:11-28) of two f32 boxes, in f64
__device__ __forceinline__ double wbf_iou(const float4 A, const float4 B) {
  const double xA = fmax((double)A.x, (double)B.x), yA = fmax((double)A.y, (double)B.y);
  const double xB = fmin((double)A.z, (double)B.z), yB = fmin((double)A.w, (double)B.w);
  const double inter = fmax(0., xB - xA) * fmax(0., yB - yA);
  if (inter == 0.) return 0.;
  const double aa = ((double)A.z - (double)A.x) * ((double)A.w - (double)A.y);
  const double ab = ((double)B.z - (double)B.x) * ((double)B.w - (double)B.y);
  return inter / (aa + ab - inter);
}

struct wbf_clusters {
  float4* box;       // the box later candidates are compared with: the first member, or the fused box
  float4* acc;       // f32 running sums of score * coordinate (get_weighted_box's box[4:])
  double* sum;       // sum of member scores
  double* wsum;      // sum of member weights
  double* smax;      // greatest member score
  double* score;     // final confidence
  int* n;            // members; 0 = no cluster in this slot
  uint32_t* mask;    // models present
};

__device__ __forceinline__ long wbf_lower_bound(const uint64_t* __restrict__ k, long P, uint64_t v) {
  long lo = 0, hi = P;
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (k[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ensemble_boxes_wbf.py:196-218 for one cluster.  A cluster of one member is the reference's float64 row, a fused
// cluster its float32 row: the products of a float32 score with an int stay float32 there, everything else is float64.
__device__ __forceinline__ double wbf_confidence(const wbf_weights& W, int conf_type, int overflow, int n, double sum,
                                                 double smax, double wsum, uint32_t mask) {
  const bool fused = n > 1;
  double uniq[MAX_MODELS], absent[MAX_MODELS];
  int nu = 0, na = 0;
  if (conf_type >= 2) {
#pragma unroll
    for (int m = 0; m < MAX_MODELS; ++m) {
      if (m < W.n) {
        if ((mask >> m) & 1) uniq[nu++] = W.w[m]; else absent[na++] = W.w[m];
      }
    }
  }
  if (!fused) {
    const double s = sum, dn = 1.0;
    if (conf_type == 2) return s * dn / wsum * np_sum(uniq, nu) / W.wsum;
    if (conf_type == 3) return s * dn / (wsum + np_sum(absent, na));
    if (!overflow) return (dn < W.wsum) ? s * dn / W.wsum : s * W.wsum / W.wsum;
    return s * dn / W.wsum;
  }
  const float s = conf_type == 1 ? (float)smax : (float)(sum / (double)n);     // get_weighted_box :123-128
  const float wf = (float)wsum;                                                 // :129
  const float sn = s * (float)n;
  if (conf_type == 2) {
    const float t = sn / wf;
    return (double)(float)((double)t * np_sum(uniq, nu) / W.wsum);
  }
  if (conf_type == 3) return (double)(float)((double)sn / ((double)wf + np_sum(absent, na)));
  if (!overflow && !((double)n < W.wsum)) return (double)(float)((double)s * W.wsum / W.wsum);
  return (double)(float)((double)sn / W.wsum);
}

template <int T>
__global__ __launch_bounds__(T) void wbf_cluster_kernel(const uint64_t* __restrict__ skey, long P, const float4* __restrict__ sbox,
                                                       const double* __restrict__ ss, const double* __restrict__ sw,
                                                       const int* __restrict__ smodel, wbf_weights W, double thr, int conf_type,
                                                       int overflow, wbf_clusters cl, int* __restrict__ assign,
                                                       int* __restrict__ out_counts) {
  constexpr int NW = T / 64;
  __shared__ double s_v[NW];
  __shared__ int s_i[NW];
  const int tid = threadIdx.x, b = blockIdx.y, g = blockIdx.x, G = gridDim.x;
  long s = wbf_lower_bound(skey, P, (uint64_t)b << 32);
  for (int seg = 0; s < P; ++seg) {
    const uint64_t key = skey[s];
    if ((int)(key >> 32) != b || key == NO_KEY) break;
    const long e = wbf_lower_bound(skey, P, key + 1);
    if (seg % G == g) {
      int ncl = 0;
      for (long j = s; j < e; ++j) {
        const float4 c = sbox[j];
        double best = thr; int bi = -1;                 // find_matching_box :135-147
        for (int k = tid; k < ncl; k += T) {
          const double v = wbf_iou(cl.box[s + k], c);
          if (v > best) { best = v; bi = k; }
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          const double ov = __shfl_xor(best, d, 64);
          const int oi = __shfl_xor(bi, d, 64);
          if (ov > best || (ov == best && (unsigned)oi < (unsigned)bi)) { best = ov; bi = oi; }
        }
        if (NW > 1) {
          if ((tid & 63) == 0) { s_v[tid >> 6] = best; s_i[tid >> 6] = bi; }
          __syncthreads();
          best = s_v[0]; bi = s_i[0];
#pragma unroll
          for (int q = 1; q < NW; ++q) {
            const double ov = s_v[q]; const int oi = s_i[q];
            if (ov > best || (ov == best && (unsigned)oi < (unsigned)bi)) { best = ov; bi = oi; }
          }
        }
        if (tid == 0) {
          const double sc = ss[j], w = sw[j];
          const int m = smodel[j];
          if (bi >= 0) {                                 // get_weighted_box :105-132 as a running sum
            const long q = s + bi;
            float4 a = cl.acc[q];
            const double sum = cl.sum[q] + sc;
            a.x = (float)((double)a.x + sc * (double)c.x);
            a.y = (float)((double)a.y + sc * (double)c.y);
            a.z = (float)((double)a.z + sc * (double)c.z);
            a.w = (float)((double)a.w + sc * (double)c.w);
            cl.acc[q] = a; cl.sum[q] = sum;
            cl.wsum[q] += w; cl.smax[q] = fmax(cl.smax[q], sc);
            cl.n[q] += 1; cl.mask[q] |= 1u << m;
            cl.box[q] = make_float4((float)((double)a.x / sum), (float)((double)a.y / sum), (float)((double)a.z / sum),
                                    (float)((double)a.w / sum));
            assign[j] = (int)q;
          } else {
            const long q = s + ncl;
            cl.box[q] = c;
            cl.acc[q] = make_float4((float)(sc * (double)c.x), (float)(sc * (double)c.y), (float)(sc * (double)c.z),
                                    (float)(sc * (double)c.w));
            cl.sum[q] = sc; cl.wsum[q] = w; cl.smax[q] = sc; cl.n[q] = 1; cl.mask[q] = 1u << m;
            assign[j] = (int)q;
          }
        }
        if (bi < 0) ++ncl;
        __syncthreads();
      }
      for (int k = tid; k < ncl; k += T) {
        const long q = s + k;
        cl.score[q] = wbf_confidence(W, conf_type, overflow, cl.n[q], cl.sum[q], cl.smax[q], cl.wsum[q], cl.mask[q]);
      }
      if (tid == 0) atomicAdd(&out_counts[b], ncl);
    }
    s = e;
  }
}

__global__ __launch_bounds__(256) void wbf_okey_score_kernel(wbf_clusters cl, long P, uint64_t* __restrict__ key,
                                                            uint32_t* __restrict__ val) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  key[p] = cl.n[p] > 0 ? desc_key(cl.score[p]) : NO_KEY;
  val[p] = (uint32_t)p;
}

__global__ __launch_bounds__(256) void wbf_okey_image_kernel(wbf_clusters cl, const uint64_t* __restrict__ skey,
                                                            const uint32_t* __restrict__ val, long P, uint32_t* __restrict__ key) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= P) return;
  const uint32_t p = val[r];
  key[r] = cl.n[p] > 0 ? (uint32_t)(skey[p] >> 32) : 0xffffffffu;
}

__global__ __launch_bounds__(256) void wbf_output_kernel(wbf_clusters cl, const uint64_t* __restrict__ skey,
                                                        const uint32_t* __restrict__ operm,
                                                        const uint32_t* __restrict__ okey, long P, long cap,
                                                        float4* __restrict__ out_boxes,
                                                        float* __restrict__ out_scores, int* __restrict__ out_labels,
                                                        int* __restrict__ rank) {
  const long r = (long)blockIdx.x * 256 + threadIdx.x;
  if (r >= P) return;
  const uint32_t p = operm[r];
  if (cl.n[p] <= 0) return;
  const uint64_t key = skey[p];
  const int b = (int)(key >> 32);
  long lo = 0, hi = r;                                   // first rank of image b in the sorted image keys
  while (lo < hi) {
    const long mid = (lo + hi) >> 1;
    if (okey[mid] < (uint32_t)b) lo = mid + 1; else hi = mid;
  }
  const long local = r - lo;                             // < clusters of image b <= cap
  const long o = (long)b * cap + local;
  out_boxes[o] = cl.box[p];
  out_scores[o] = (float)cl.score[p];
  out_labels[o] = (int)(uint32_t)key;
  rank[p] = (int)local;
}

__global__ __launch_bounds__(256) void wbf_member_kernel(const uint64_t* __restrict__ skey, const uint32_t* __restrict__ perm,
                                                        const int* __restrict__ assign, const int* __restrict__ rank, long P,
                                                        int* __restrict__ member) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  member[perm[p]] = skey[p] == NO_KEY ? -1 : rank[assign[p]];
}

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct ws_layout {
  size_t k64a, k64b, skey, v32a, v32b, perm, k32a, k32b, sort_tmp, sort_tmp_bytes;
  size_t sbox, ss, sw, smodel, box, acc, sum, wsum, smax, score, n, mask, assign, rank, total;
};

int layout(int B, long cap, ws_layout& L) {
  if (B <= 0 || B > MAX_B || cap <= 0 || (long)B * cap > (1L << 30)) return SODT_EINVAL;
  const size_t P = (size_t)B * cap;
  size_t t64 = 0, t32 = 0;
  if (rocprim::radix_sort_pairs<rocprim::default_config, const uint64_t*, uint64_t*, const uint32_t*, uint32_t*>(
          nullptr, t64, nullptr, nullptr, nullptr, nullptr, P, 0, 64, 0) != hipSuccess) return SODT_ELAUNCH;
  if (rocprim::radix_sort_pairs<rocprim::default_config, const uint32_t*, uint32_t*, const uint32_t*, uint32_t*>(
          nullptr, t32, nullptr, nullptr, nullptr, nullptr, P, 0, 32, 0) != hipSuccess) return SODT_ELAUNCH;
  size_t o = 0;
  auto take = [&](size_t& f, size_t bytes) { f = o; o += align256(bytes); };
  take(L.k64a, P * 8); take(L.k64b, P * 8); take(L.skey, P * 8);
  take(L.v32a, P * 4); take(L.v32b, P * 4); take(L.perm, P * 4);
  take(L.k32a, P * 4); take(L.k32b, P * 4);
  L.sort_tmp_bytes = t64 > t32 ? t64 : t32;
  take(L.sort_tmp, L.sort_tmp_bytes);
  take(L.sbox, P * 16); take(L.ss, P * 8); take(L.sw, P * 8); take(L.smodel, P * 4);
  take(L.box, P * 16); take(L.acc, P * 16); take(L.sum, P * 8); take(L.wsum, P * 8); take(L.smax, P * 8);
  take(L.score, P * 8); take(L.n, P * 4); take(L.mask, P * 4); take(L.assign, P * 4); take(L.rank, P * 4);
  L.total = o;
  return SODT_OK;
}

inline bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

}  // namespace

extern "C" int sodt_wbf_candidates(const float* z, int B, int N, int nc, float conf_thres, float image_size, float* boxes,
                                   float* scores, int* labels, int* src, int* counts, hipStream_t stream) {
  if (!z || !boxes || !scores || !labels || !src || !counts || B <= 0 || B > MAX_B || N <= 0 || nc <= 0 ||
      (long)B * N > (1L << 30) || misaligned(boxes, 16))
    return SODT_EINVAL;
  if (hipMemsetAsync(counts, 0, sizeof(int) * B, stream) != hipSuccess) return SODT_ELAUNCH;
  return sodt_launch<wbf_candidates_kernel>(dim3((N + 255) / 256, B), dim3(256), 0, stream, z, N, nc, conf_thres, image_size, (float4*)boxes, scores,
                                                                     labels, src, counts);
}

extern "C" int sodt_wbf_fuse_workspace_bytes(int B, long cap, size_t* bytes) {
  ws_layout L;
  if (!bytes || layout(B, cap, L) != SODT_OK) return SODT_EINVAL;
  *bytes = L.total;
  return SODT_OK;
}

extern "C" int sodt_wbf_fuse(const float* boxes, const float* scores, const int* labels, const int* model, const int* src,
                             const int* counts, int B, long cap, const double* weights, int n_models, double iou_thr,
                             float skip_box_thr, int conf_type, int allows_overflow, int scan_lanes, void* ws, size_t ws_bytes,
                             float* out_boxes, float* out_scores, int* out_labels, int* out_counts, int* member,
                             hipStream_t stream) {
  ws_layout L;
  if (!boxes || !scores || !labels || !counts || !weights || !ws || !out_boxes || !out_scores || !out_labels || !out_counts)
    return SODT_EINVAL;
  if (n_models < 1 || n_models > MAX_MODELS || conf_type < 0 || conf_type > 3) return SODT_EINVAL;
  if (scan_lanes != 0 && scan_lanes != 64 && scan_lanes != 256) return SODT_EINVAL;
  if (misaligned(boxes, 16) || misaligned(out_boxes, 16) || misaligned(ws, 256)) return SODT_EINVAL;
  if (layout(B, cap, L) != SODT_OK || ws_bytes < L.total) return SODT_EINVAL;
  const long P = (long)B * cap;
  wbf_weights W;
  for (int m = 0; m < MAX_MODELS; ++m) W.w[m] = m < n_models ? weights[m] : 0.;
  W.n = n_models;
  W.wsum = np_sum(weights, n_models);
  char* base = (char*)ws;
  uint64_t *k64a = (uint64_t*)(base + L.k64a), *k64b = (uint64_t*)(base + L.k64b), *skey = (uint64_t*)(base + L.skey);
  uint32_t *v32a = (uint32_t*)(base + L.v32a), *v32b = (uint32_t*)(base + L.v32b), *perm = (uint32_t*)(base + L.perm);
  uint32_t *k32a = (uint32_t*)(base + L.k32a), *k32b = (uint32_t*)(base + L.k32b);
  void* tmp = base + L.sort_tmp;
  size_t tb = L.sort_tmp_bytes;
  float4* sbox = (float4*)(base + L.sbox);
  double *ss = (double*)(base + L.ss), *sw = (double*)(base + L.sw);
  int* smodel = (int*)(base + L.smodel);
  wbf_clusters cl;
  cl.box = (float4*)(base + L.box); cl.acc = (float4*)(base + L.acc); cl.sum = (double*)(base + L.sum);
  cl.wsum = (double*)(base + L.wsum); cl.smax = (double*)(base + L.smax); cl.score = (double*)(base + L.score);
  cl.n = (int*)(base + L.n); cl.mask = (uint32_t*)(base + L.mask);
  int *assign = (int*)(base + L.assign), *rank = (int*)(base + L.rank);
  const wbf_in in{scores, labels, model, counts, cap, skip_box_thr, n_models};
  const unsigned nb = (unsigned)((P + 255) / 256);

  if (hipMemsetAsync(cl.n, 0, (size_t)P * 4, stream) != hipSuccess) return SODT_ELAUNCH;
  if (hipMemsetAsync(out_counts, 0, sizeof(int) * B, stream) != hipSuccess) return SODT_ELAUNCH;
  // order: label, then descending weighted score, then ascending source index (three stable passes, last key first)
  const uint32_t* order = v32a;
  if (src) {
    if (int err = sodt_launch<wbf_key_src_kernel>(nb, dim3(256), 0, stream, src, P, k32a, v32a)) return err;
    if (rocprim::radix_sort_pairs(tmp, tb, (const uint32_t*)k32a, k32b, (const uint32_t*)v32a, v32b, (size_t)P, 0, 32, stream) !=
        hipSuccess) return SODT_ELAUNCH;
    order = v32b;
  } else {
    if (int err = sodt_launch<wbf_key_src_kernel>(nb, dim3(256), 0, stream, nullptr, P, nullptr, v32a)) return err;
  }
  uint32_t* order2 = order == v32a ? v32b : v32a;
  if (int err = sodt_launch<wbf_key_score_kernel>(nb, dim3(256), 0, stream, in, W, order, P, k64a)) return err;
  tb = L.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(tmp, tb, (const uint64_t*)k64a, k64b, order, order2, (size_t)P, 0, 64, stream) != hipSuccess)
    return SODT_ELAUNCH;
  if (int err = sodt_launch<wbf_key_seg_kernel>(nb, dim3(256), 0, stream, in, order2, P, k64a)) return err;
  tb = L.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(tmp, tb, (const uint64_t*)k64a, skey, (const uint32_t*)order2, perm, (size_t)P, 0, 64, stream) !=
      hipSuccess) return SODT_ELAUNCH;
  if (int err = sodt_launch<wbf_gather_kernel>(nb, dim3(256), 0, stream, in, W, (const float4*)boxes, skey, perm, P, sbox, ss, sw, smodel)) return err;

  const dim3 grid((unsigned)(cap < 64 ? cap : 64), (unsigned)B);
  if (int err = scan_lanes == 256
          ? sodt_launch<wbf_cluster_kernel<256>>(grid, dim3(256), 0, stream, skey, P, sbox, ss, sw, smodel, W, iou_thr, conf_type, allows_overflow, cl,
                                                 assign, out_counts)
          : sodt_launch<wbf_cluster_kernel<64>>(grid, dim3(64), 0, stream, skey, P, sbox, ss, sw, smodel, W, iou_thr, conf_type, allows_overflow, cl,
                                                assign, out_counts)) return err;

  // output order: image, then descending score, then label, then creation order (the slot order)
  if (int err = sodt_launch<wbf_okey_score_kernel>(nb, dim3(256), 0, stream, cl, P, k64a, v32a)) return err;
  tb = L.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(tmp, tb, (const uint64_t*)k64a, k64b, (const uint32_t*)v32a, v32b, (size_t)P, 0, 64, stream) !=
      hipSuccess) return SODT_ELAUNCH;
  if (int err = sodt_launch<wbf_okey_image_kernel>(nb, dim3(256), 0, stream, cl, skey, v32b, P, k32a)) return err;
  tb = L.sort_tmp_bytes;
  if (rocprim::radix_sort_pairs(tmp, tb, (const uint32_t*)k32a, k32b, (const uint32_t*)v32b, v32a, (size_t)P, 0, 32, stream) !=
      hipSuccess) return SODT_ELAUNCH;
  if (int err = sodt_launch<wbf_output_kernel>(nb, dim3(256), 0, stream, cl, skey, v32a, k32b, P, cap, (float4*)out_boxes, out_scores, out_labels, rank)) return err;
  return member ? sodt_launch<wbf_member_kernel>(nb, dim3(256), 0, stream, skey, perm, assign, rank, P, member) : SODT_OK;
}
