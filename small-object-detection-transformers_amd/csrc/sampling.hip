// Train.py's --image-weights on the device (Train.py:335-341, basics/utils/general.py:220-244): the per-image class
// counts, the image weights and the weighted draw of random.choices.
//
// Nothing here is near a roofline (a few MB at the COCO size); what matters is that every result is a function of the
// inputs alone:
//   * the counts are integer atomics - exact, whatever the order;
//   * an image weight is ONE f64 accumulator that walks the classes in ascending order, product first, then the add (this
//     file is compiled with -ffp-contract=off); the rows of the count matrix come in through LDS as whole runs;
//   * the cumulative weights are a three-phase scan whose association order depends on n alone (include/sodt_hip.h
//     states it term by term), with no floating-point atomic anywhere;
//   * a draw is one IEEE multiply and Python's bisect_right over cum[0 .. n-2].
// No block waits on another block, no cooperative launch, no host read inside an entry.
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int NT = 256;                  // threads of every kernel here
constexpr int COUNT_BLOCKS = 1024;       // grid cap of class_counts_kernel: one thread per label up to NT * COUNT_BLOCKS labels
constexpr int HIST = 1024;               // classes whose totals class_counts_kernel gathers per block in LDS
constexpr int CT = 32;                  // classes per LDS tile of image_weights_kernel
constexpr int ITEMS = SODT_CHOICES_BLOCK / NT;      // consecutive weights per thread of the block scan
constexpr int MAX_N = 1 << 24;           // images / draws
constexpr int MAX_NC = 1 << 16;
static_assert(ITEMS * NT == SODT_CHOICES_BLOCK && NT == 256, "the scan order of the header is written for 256 x 4");

// ------------------------------------------------------------------------------------------------ sodt_class_counts
__global__ __launch_bounds__(NT) void class_counts_kernel(const int* __restrict__ cls, const int* __restrict__ img, const long M,
                                                          const int n_img, const int nc, int* __restrict__ counts,
                                                          unsigned long long* __restrict__ class_total,
                                                          int* __restrict__ status) {
  // Every label of the data set lands on one of nc addresses of class_total: up to HIST classes the block counts them in LDS
  // first and adds its nc sums once (866,643 labels on 80 classes: 852 us with one global atomic per label, see
  // profiles/r16_image_weights.md).  `in_lds` is uniform over the grid, so the barriers are too.
  __shared__ unsigned s_total[HIST];
  const bool in_lds = nc <= HIST;
  if (in_lds) {
    for (int c = threadIdx.x; c < nc; c += NT) s_total[c] = 0u;
    __syncthreads();
  }
  int bad = 0;
  for (long m = (long)blockIdx.x * NT + threadIdx.x; m < M; m += (long)gridDim.x * NT) {
    const int c = cls[m], i = img[m];
    const int b = ((c < 0 || c >= nc) ? SODT_SAMPLING_BAD_CLASS : 0) | ((i < 0 || i >= n_img) ? SODT_SAMPLING_BAD_IMAGE : 0);
    if (b) { bad |= b; continue; }
    atomicAdd(&counts[(long)i * nc + c], 1);
    if (in_lds) atomicAdd(&s_total[c], 1u);
    else atomicAdd(&class_total[c], 1ull);
  }
  if (in_lds) {
    __syncthreads();
    for (int c = threadIdx.x; c < nc; c += NT)
      if (const unsigned v = s_total[c]) atomicAdd(&class_total[c], (unsigned long long)v);
  }
  if (bad) atomicOr(status, bad);
}

// ------------------------------------------------------------------------------------------------ sodt_image_weights
// One thread per image, NT images per block.  The block's rows are contiguous in memory; a tile of CT classes of all of
// them is read as runs of CT ints (the whole block of memory when nc <= CT) and parked in LDS with a row stride of
// CT + 1 words, which keeps the 32 lanes of a half wave on 32 banks when each walks its own row.
__global__ __launch_bounds__(NT) void image_weights_kernel(const int* __restrict__ counts, const double* __restrict__ cw,
                                                           const int n_img, const int nc, double* __restrict__ iw) {
  __shared__ int s_cnt[NT * (CT + 1)];
  __shared__ double s_cw[CT];
  const int tid = threadIdx.x;
  const long i0 = (long)blockIdx.x * NT;
  const int rows = (int)((n_img - i0) < NT ? (n_img - i0) : NT);
  double acc = 0.0;
  for (int c0 = 0; c0 < nc; c0 += CT) {
    const int w = (nc - c0) < CT ? (nc - c0) : CT;
    __syncthreads();                                   // the previous tile has been consumed
    if (tid < w) s_cw[tid] = cw[c0 + tid];
    for (int e = tid; e < rows * w; e += NT) {
      const int r = e / w, c = e - r * w;
      s_cnt[r * (CT + 1) + c] = counts[(i0 + r) * nc + c0 + c];
    }
    __syncthreads();
    if (tid < rows)
      for (int c = 0; c < w; ++c) acc += s_cw[c] * (double)s_cnt[tid * (CT + 1) + c];
  }
  if (tid < rows) iw[i0 + tid] = acc;
}

// ------------------------------------------------------------------------------------------------ sodt_weighted_choices
// Exclusive prefix of `total` (this thread's sum) over the NT threads of the block, in the header's order: Hillis-Steele
// over the 64 lanes of a wave with offsets 1, 2, .. 32, the four wave totals added left to right, then
// prefix = wave_prefix + lane_prefix (absent terms are +0.0).  *block_total = ((W0 + W1) + W2) + W3 in every thread.
__device__ __forceinline__ double block_exclusive(double total, double* block_total) {
  __shared__ double s_wave[NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double inc = total;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double up = __shfl_up(inc, o);
    if (lane >= o) inc = inc + up;
  }
  double lane_prefix = __shfl_up(inc, 1);
  if (lane == 0) lane_prefix = 0.0;
  __syncthreads();                                     // s_wave may still be read from an earlier call
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  double run = 0.0, wave_prefix = 0.0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    if (w == wave) wave_prefix = run;
    run = (w == 0) ? s_wave[0] : run + s_wave[w];
  }
  *block_total = run;
  return wave_prefix + lane_prefix;
}

// phase 1: block b scans iw[b * W .. b * W + W); loc = the block-local inclusive prefix, totals[b] = the block's sum
__global__ __launch_bounds__(NT) void scan_blocks_kernel(const double* __restrict__ iw, const int n, double* __restrict__ loc,
                                                         double* __restrict__ totals) {
  const long e0 = (long)blockIdx.x * SODT_CHOICES_BLOCK + (long)threadIdx.x * ITEMS;
  double s[ITEMS];
  double run = 0.0;
#pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    const double a = (e0 + j < n) ? iw[e0 + j] : 0.0;
    run = (j == 0) ? a : run + a;
    s[j] = run;
  }
  double bt;
  const double pre = block_exclusive(run, &bt);
#pragma unroll
  for (int j = 0; j < ITEMS; ++j)
    if (e0 + j < n) loc[e0 + j] = pre + s[j];
  if (threadIdx.x == 0) totals[blockIdx.x] = bt;
}

// phase 2, ONE block: offs[b] = the exclusive prefix of totals[0 .. nb); thread t owns the `per` consecutive totals from t * per
__global__ __launch_bounds__(NT) void scan_totals_kernel(const double* __restrict__ totals, const int nb, const int per,
                                                         double* __restrict__ offs) {
  const int b0 = threadIdx.x * per;
  double run = 0.0;
  for (int j = 0; j < per; ++j) {
    const double a = (b0 + j < nb) ? totals[b0 + j] : 0.0;
    run = (j == 0) ? a : run + a;
  }
  double bt;
  const double pre = block_exclusive(run, &bt);
  // the inclusive prefix of block b is pre + (the serial sum up to b); the offset of block b + 1 is that value
  if (threadIdx.x == 0) offs[0] = 0.0;
  run = 0.0;
  for (int j = 0; j < per; ++j) {
    if (b0 + j >= nb) break;
    run = (j == 0) ? totals[b0 + j] : run + totals[b0 + j];
    if (b0 + j + 1 < nb) offs[b0 + j + 1] = pre + run;
  }
}

// phase 3: cum[e] = offs[e / W] + loc[e], in place
__global__ __launch_bounds__(NT) void scan_add_kernel(double* __restrict__ cum, const int n, const double* __restrict__ offs) {
  const long e0 = (long)blockIdx.x * SODT_CHOICES_BLOCK + (long)threadIdx.x * ITEMS;
  const double off = offs[blockIdx.x];
#pragma unroll
  for (int j = 0; j < ITEMS; ++j)
    if (e0 + j < n) cum[e0 + j] = off + cum[e0 + j];
}

// one thread per draw: random.choices' `bisect(cum_weights, random() * total, 0, n - 1)`
__global__ __launch_bounds__(NT) void draw_kernel(const double* __restrict__ cum, const int n, const double* __restrict__ u,
                                                  const int k, int* __restrict__ idx, int* __restrict__ status) {
  const int j = blockIdx.x * NT + threadIdx.x;
  const double total = cum[n - 1];
  const int bad = !(total > 0.0) && total == total ? SODT_SAMPLING_ZERO_TOTAL       // total <= 0; a NaN is "not finite"
                  : !(fabs(total) <= 1.7976931348623157e308) ? SODT_SAMPLING_NONFINITE_TOTAL : 0;
  if (bad && j == 0) atomicOr(status, bad);
  if (j >= k) return;
  if (bad) { idx[j] = -1; return; }
  const double x = u[j] * total;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x < cum[mid]) hi = mid; else lo = mid + 1;
  }
  idx[j] = lo;
}

inline int blocks_of(long n) { return (int)((n + SODT_CHOICES_BLOCK - 1) / SODT_CHOICES_BLOCK); }

}  // namespace

extern "C" int sodt_class_counts(const int* cls, const int* img, long M, int n_img, int nc, int* counts, long long* class_total,
                                 int* status, sodt_stream_t st) {
  if (M < 0 || M > 0x7fffffffL || n_img < 1 || n_img > MAX_N || nc < 1 || nc > MAX_NC) return SODT_EINVAL;
  if (!counts || !class_total || !status || (M > 0 && (!cls || !img))) return SODT_EINVAL;
  if (((uintptr_t)cls & 3) || ((uintptr_t)img & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)class_total & 7) ||
      ((uintptr_t)status & 3))
    return SODT_EINVAL;
  if (M == 0) return SODT_OK;
  long blocks = (M + NT - 1) / NT;
  if (blocks > COUNT_BLOCKS) blocks = COUNT_BLOCKS;
  return sodt_launch<class_counts_kernel>(dim3((unsigned)blocks), dim3(NT), 0, (hipStream_t)st, cls, img, M, n_img, nc, counts,
                                          (unsigned long long*)class_total, status);
}

extern "C" int sodt_image_weights(const int* counts, const double* cw, int n_img, int nc, double* iw, sodt_stream_t st) {
  if (n_img < 1 || n_img > MAX_N || nc < 1 || nc > MAX_NC || !counts || !cw || !iw) return SODT_EINVAL;
  if (((uintptr_t)counts & 3) || ((uintptr_t)cw & 7) || ((uintptr_t)iw & 7)) return SODT_EINVAL;
  return sodt_launch<image_weights_kernel>(dim3((unsigned)((n_img + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)st, counts, cw,
                                           n_img, nc, iw);
}

extern "C" int sodt_weighted_choices_workspace_bytes(int n, int k, size_t* bytes) {
  if (!bytes || n < 1 || n > MAX_N || k < 0 || k > MAX_N) return SODT_EINVAL;
  *bytes = (2 * sizeof(double) * (size_t)blocks_of(n) + 15) & ~(size_t)15;      // block totals, then block offsets
  return SODT_OK;
}

extern "C" int sodt_weighted_choices(const double* iw, int n, const double* u, int k, int* idx, double* cum, int* status, void* ws,
                                     size_t ws_bytes, sodt_stream_t st) {
  size_t need;
  if (sodt_weighted_choices_workspace_bytes(n, k, &need) != SODT_OK) return SODT_EINVAL;
  if (!iw || !cum || !status || !ws || (k > 0 && (!u || !idx))) return SODT_EINVAL;
  if (((uintptr_t)iw & 7) || ((uintptr_t)u & 7) || ((uintptr_t)idx & 3) || ((uintptr_t)cum & 7) || ((uintptr_t)status & 3) ||
      ((uintptr_t)ws & 15) || ws_bytes < need)
    return SODT_EINVAL;
  hipStream_t s = (hipStream_t)st;
  const int nb = blocks_of(n);
  double* totals = (double*)ws;
  double* offs = totals + nb;
  if (int err = sodt_launch<scan_blocks_kernel>(dim3(nb), dim3(NT), 0, s, iw, n, cum, totals)) return err;
  if (int err = sodt_launch<scan_totals_kernel>(dim3(1), dim3(NT), 0, s, (const double*)totals, nb, (nb + NT - 1) / NT, offs))
    return err;
  if (int err = sodt_launch<scan_add_kernel>(dim3(nb), dim3(NT), 0, s, cum, n, (const double*)offs)) return err;
  return sodt_launch<draw_kernel>(dim3((unsigned)((k > 0 ? k : 1) + NT - 1) / NT), dim3(NT), 0, s, (const double*)cum, n, u, k, idx,
                                  status);
}
