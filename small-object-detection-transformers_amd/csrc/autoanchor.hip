// Autoanchor (basics/utils/autoanchor.py) on the device: the ratio metric of check_anchors / kmean_anchors, the
// mutate-and-evaluate evolution and the Lloyd iterations of scipy.cluster.vq.kmeans.
//
// The data are tiny per element (one float2 per label, at most 32 anchors); what matters is that the arithmetic is the
// reference's and that every reduction is deterministic:
//   * per label r = wh / k, x = min over the two axes of min(r, 1 / r), best = max over the anchors of x, all in f32 with
//     IEEE division (this file is compiled with -ffp-contract=off and without any fast-math flag); thresholds are compared
//     in f32 and strictly, as torch compares a float32 tensor with a Python float;
//   * sums are f64 and counts int64: per thread over its labels in index order, over the wave by shuffles, over the block
//     through LDS, then ONE partial per block in the workspace.  The block that draws the last ticket adds the partials
//     in block-index order, so equal inputs give equal bits on every call (no floating-point atomic anywhere);
//   * no block waits on another block, no cooperative launch, no host read inside an entry.
// Anchor sets live in LDS; each thread keeps its label in registers and walks the set.
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

constexpr int MAX_ANCH = 32;      // anchors per set
constexpr int MAX_BLOCKS = 128;   // blocks per anchor set / restart: the ordered tail adds at most this many partials
constexpr int NT = 256;           // threads of the metric kernels

__device__ __forceinline__ float ratio_metric(float w, float h, float kx, float ky) {      // autoanchor.py:34-35, :81-82
  const float rw = w / kx, rh = h / ky;
  return fminf(fminf(rw, 1.0f / rw), fminf(rh, 1.0f / rh));
}

__device__ __forceinline__ double wave_sum_d(double v) {          // fixed order; valid in lane 0
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

union Slot { double d; long long i; };

// blocks of one anchor set / restart for N labels handled `per` to a block and trip
inline unsigned blocks_for(long N, int per) {
  long b = (N + per - 1) / per;
  if (b > MAX_BLOCKS) b = MAX_BLOCKS;
  return (unsigned)(b < 1 ? 1 : b);
}

// ------------------------------------------------------------------------------------------------ sodt_anchor_stats
// grid (bx, S).  out[s][6] = sum(best), sum(best [best > thr]), count(best > thr), count(x > thr), sum(x), sum(x [x > thr])
__global__ __launch_bounds__(NT) void anchor_stats_kernel(const float2* __restrict__ wh, const long N,
                                                          const float* __restrict__ sets, const int n, const float thr,
                                                          unsigned* __restrict__ ticket, Slot* __restrict__ part,
                                                          double* __restrict__ out) {
  __shared__ float s_k[2 * MAX_ANCH];
  __shared__ Slot s_red[6][NT / 64];
  __shared__ Slot s_part[MAX_BLOCKS * 6];
  __shared__ int s_last;
  const int s = blockIdx.y, tid = threadIdx.x;
  if (tid < 2 * n) s_k[tid] = sets[(long)s * 2 * n + tid];
  __syncthreads();
  double sb = 0.0, sbt = 0.0, sx = 0.0, sxt = 0.0;
  long long cb = 0, cx = 0;
  for (long i = (long)blockIdx.x * NT + tid; i < N; i += (long)gridDim.x * NT) {
    const float2 p = wh[i];
    float best = 0.f;
    for (int a = 0; a < n; ++a) {
      const float x = ratio_metric(p.x, p.y, s_k[2 * a], s_k[2 * a + 1]);
      best = a == 0 ? x : fmaxf(best, x);
      sx += (double)x;
      if (x > thr) { sxt += (double)x; ++cx; }
    }
    sb += (double)best;
    if (best > thr) { sbt += (double)best; ++cb; }
  }
  sb = wave_sum_d(sb); sbt = wave_sum_d(sbt); sx = wave_sum_d(sx); sxt = wave_sum_d(sxt);
  cb = wave_sum_ll(cb); cx = wave_sum_ll(cx);
  if ((tid & 63) == 0) {
    const int w = tid >> 6;
    s_red[0][w].d = sb; s_red[1][w].d = sbt; s_red[2][w].i = cb; s_red[3][w].i = cx; s_red[4][w].d = sx; s_red[5][w].d = sxt;
  }
  __syncthreads();
  const unsigned bx = gridDim.x;
  Slot* mine = part + ((size_t)s * bx + blockIdx.x) * 6;
  if (tid < 6) {
    Slot v;
    if (tid == 2 || tid == 3) v.i = (s_red[tid][0].i + s_red[tid][1].i) + (s_red[tid][2].i + s_red[tid][3].i);
    else v.d = (s_red[tid][0].d + s_red[tid][1].d) + (s_red[tid][2].d + s_red[tid][3].d);
    __hip_atomic_store(&mine[tid].i, v.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (tid == 0) {
    // the partial is published before the ticket is drawn (release); the block that draws the last one sees all (acquire)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    s_last = __hip_atomic_fetch_add(&ticket[s], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == bx - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const Slot* all = part + (size_t)s * bx * 6;
  for (unsigned i = tid; i < bx * 6; i += NT) s_part[i].i = __hip_atomic_load(&all[i].i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (tid < 6) {                                                   // block-index order
    double r;
    if (tid == 2 || tid == 3) {
      long long c = 0;
      for (unsigned b = 0; b < bx; ++b) c += s_part[b * 6 + tid].i;
      r = (double)c;
    } else {
      r = 0.0;
      for (unsigned b = 0; b < bx; ++b) r += s_part[b * 6 + tid].d;
    }
    out[(long)s * 6 + tid] = r;
  }
  if (tid == 0) __hip_atomic_store(&ticket[s], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ----------------------------------------------------------------------------------------------- sodt_anchor_evolve
// One generation (autoanchor.py:150-153): kg = max(k * v, 2.0) in f64, the fitness of float32(kg) over all labels,
// and the last block accepts it when fg > f.  Generations are separate launches: stream order lies between them.
__global__ __launch_bounds__(NT) void anchor_evolve_kernel(const float2* __restrict__ wh, const long N, const float thr,
                                                           const int n, double* k, double* f, const double* __restrict__ v,
                                                           unsigned* __restrict__ ticket, double* __restrict__ part,
                                                           int* __restrict__ accepted) {
  __shared__ double s_kg[2 * MAX_ANCH];
  __shared__ float s_k[2 * MAX_ANCH];
  __shared__ double s_red[NT / 64];
  __shared__ double s_part[MAX_BLOCKS];
  __shared__ int s_flag;
  const int tid = threadIdx.x;
  if (tid < 2 * n) {
    const double kg = fmax(k[tid] * v[tid], 2.0);
    s_kg[tid] = kg;
    s_k[tid] = (float)kg;
  }
  __syncthreads();
  double sbt = 0.0;
  for (long i = (long)blockIdx.x * NT + tid; i < N; i += (long)gridDim.x * NT) {
    const float2 p = wh[i];
    float best = ratio_metric(p.x, p.y, s_k[0], s_k[1]);
    for (int a = 1; a < n; ++a) best = fmaxf(best, ratio_metric(p.x, p.y, s_k[2 * a], s_k[2 * a + 1]));
    if (best > thr) sbt += (double)best;
  }
  sbt = wave_sum_d(sbt);
  if ((tid & 63) == 0) s_red[tid >> 6] = sbt;
  __syncthreads();
  const unsigned bx = gridDim.x;
  if (tid == 0) {
    const double tot = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
    __hip_atomic_store(&part[blockIdx.x], tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    s_flag = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == bx - 1;
  }
  __syncthreads();
  if (!s_flag) return;                                             // every other block has read k by now
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  for (unsigned i = tid; i < bx; i += NT) s_part[i] = __hip_atomic_load(&part[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (unsigned b = 0; b < bx; ++b) tot += s_part[b];            // block-index order
    const double fg = tot / (double)N;
    const int acc = fg > *f;
    if (acc) *f = fg;
    if (accepted) *accepted = acc;
    s_flag = acc;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (s_flag && tid < 2 * n) k[tid] = s_kg[tid];
}

// ------------------------------------------------------------------------------------------------ sodt_kmeans_lloyd
// One Lloyd iteration of scipy.cluster.vq.kmeans for R restarts: grid (bx, R), one wave per block.  Each lane owns the
// accumulators of its labels in LDS (acc[quantity][lane]: no two lanes share a word, so no atomics and a fixed order),
// the wave reduces them by shuffles, and the block of a restart that draws the last ticket adds the partials in block
// order, moves the centres, marks empty ones dead and takes the stop decision.
__global__ __launch_bounds__(64) void kmeans_lloyd_kernel(const double2* __restrict__ obs, const long N, double* books,
                                                          int* alive, double* prev, int* done, const int n,
                                                          const double thresh, unsigned* __restrict__ ticket,
                                                          double* __restrict__ part) {
  extern __shared__ double s_acc[];                                // [3 * n][64]
  __shared__ double s_c[2 * MAX_ANCH];
  __shared__ int s_alive[MAX_ANCH];
  __shared__ int s_last;
  const int r = blockIdx.y, lane = threadIdx.x;
  if (done[r]) return;                       // only the last block of r writes done[r], after every block of r has read it
  double* book = books + (long)r * 2 * n;
  if (lane < 2 * n) s_c[lane] = book[lane];
  if (lane < n) s_alive[lane] = alive[(long)r * n + lane];
  for (int q = 0; q < 3 * n; ++q) s_acc[q * 64 + lane] = 0.0;
  __syncthreads();
  double sd = 0.0;
  for (long i = (long)blockIdx.x * 64 + lane; i < N; i += (long)gridDim.x * 64) {
    const double2 p = obs[i];
    double low = INFINITY;
    int code = -1;
    for (int c = 0; c < n; ++c) {
      if (!s_alive[c]) continue;
      const double dx = s_c[2 * c] - p.x, dy = s_c[2 * c + 1] - p.y;
      const double d2 = dx * dx + dy * dy;                         // uncontracted: ties fall as in scipy
      if (d2 < low) { low = d2; code = c; }                        // strict: the lowest live index wins a tie
    }
    if (code >= 0) {
      sd += sqrt(low);
      s_acc[(3 * code) * 64 + lane] += p.x;
      s_acc[(3 * code + 1) * 64 + lane] += p.y;
      s_acc[(3 * code + 2) * 64 + lane] += 1.0;
    }
  }
  const unsigned bx = gridDim.x;
  const int Q = 3 * n + 1;
  double* mine = part + ((size_t)r * bx + blockIdx.x) * Q;
  for (int q = 0; q < Q; ++q) {
    const double t = wave_sum_d(q < 3 * n ? s_acc[q * 64 + lane] : sd);
    if (lane == 0) __hip_atomic_store(&mine[q], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (lane == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    s_last = __hip_atomic_fetch_add(&ticket[r], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == bx - 1;
  }
  __syncthreads();
  if (!s_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const double* all = part + (size_t)r * bx * Q;
  __syncthreads();                                                 // s_acc is reused for the totals
  for (int q = lane; q < Q; q += 64) {
    double t = 0.0;
    for (unsigned b = 0; b < bx; ++b)                              // block-index order
      t += __hip_atomic_load(&all[(size_t)b * Q + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_acc[q] = t;
  }
  __syncthreads();
  if (lane < n && s_alive[lane]) {
    const double cnt = s_acc[3 * lane + 2];
    if (cnt > 0.0) {
      book[2 * lane] = s_acc[3 * lane] / cnt;
      book[2 * lane + 1] = s_acc[3 * lane + 1] / cnt;
    } else {
      alive[(long)r * n + lane] = 0;                               // a centre without members takes no further part
    }
  }
  if (lane == 0) {
    const double cur = s_acc[3 * n] / (double)N;
    const double diff = fabs(prev[r] - cur);
    prev[r] = cur;
    if (diff <= thresh) done[r] = 1;
    __hip_atomic_store(&ticket[r], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

inline size_t tickets_bytes(int count) { return (((size_t)count * sizeof(unsigned)) + 15) & ~(size_t)15; }

}  // namespace

extern "C" int sodt_anchor_stats_workspace_bytes(long N, int S, size_t* bytes) {
  if (!bytes || N < 0 || S < 1 || S > 65535) return SODT_EINVAL;
  *bytes = tickets_bytes(S) + sizeof(Slot) * 6 * (size_t)blocks_for(N, NT) * (size_t)S;
  return SODT_OK;
}

extern "C" int sodt_anchor_stats(const float* wh, long N, const float* sets, int S, int n, float thr, void* ws,
                                 size_t ws_bytes, double* out, sodt_stream_t st) {
  size_t need;
  if (sodt_anchor_stats_workspace_bytes(N, S, &need) != SODT_OK) return SODT_EINVAL;
  if (n < 1 || n > MAX_ANCH || !sets || !out || !ws || (N > 0 && !wh) || thr != thr) return SODT_EINVAL;
  if (((uintptr_t)wh & 7) || ((uintptr_t)sets & 3) || ((uintptr_t)out & 7) || ((uintptr_t)ws & 15) || ws_bytes < need)
    return SODT_EINVAL;
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(ws, 0, tickets_bytes(S), s) != hipSuccess) return SODT_ELAUNCH;
  unsigned* ticket = (unsigned*)ws;
  Slot* part = (Slot*)((char*)ws + tickets_bytes(S));
  return sodt_launch<anchor_stats_kernel>(dim3(blocks_for(N, NT), S), dim3(NT), 0, s, (const float2*)wh, N, sets, n, thr,
                     ticket, part, out);
}

extern "C" int sodt_anchor_evolve_workspace_bytes(long N, size_t* bytes) {
  if (!bytes || N < 0) return SODT_EINVAL;
  *bytes = 16 + sizeof(double) * (size_t)blocks_for(N, NT);
  return SODT_OK;
}

extern "C" int sodt_anchor_evolve(const float* wh, long N, float thr, double* k, int n, double* f, const double* v, int G,
                                  int* accepted, void* ws, size_t ws_bytes, sodt_stream_t st) {
  size_t need;
  if (sodt_anchor_evolve_workspace_bytes(N, &need) != SODT_OK) return SODT_EINVAL;
  if (n < 1 || n > MAX_ANCH || G < 0 || N < 1 || !wh || !k || !f || !ws || (G > 0 && !v) || thr != thr) return SODT_EINVAL;
  if (((uintptr_t)wh & 7) || ((uintptr_t)k & 7) || ((uintptr_t)f & 7) || ((uintptr_t)v & 7) || ((uintptr_t)accepted & 3) ||
      ((uintptr_t)ws & 15) || ws_bytes < need)
    return SODT_EINVAL;
  if (G == 0) return SODT_OK;
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(ws, 0, 16, s) != hipSuccess) return SODT_ELAUNCH;
  unsigned* ticket = (unsigned*)ws;
  double* part = (double*)((char*)ws + 16);
  const dim3 grid(blocks_for(N, NT));
  for (int g = 0; g < G; ++g)
    if (int err = sodt_launch<anchor_evolve_kernel>(grid, dim3(NT), 0, s, (const float2*)wh, N, thr, n, k, f, v + (size_t)g * 2 * n,
                                                   ticket, part, accepted ? accepted + g : (int*)nullptr)) return err;
  return SODT_OK;
}

extern "C" int sodt_kmeans_lloyd_workspace_bytes(long N, int R, int n, size_t* bytes) {
  if (!bytes || N < 1 || R < 1 || R > 65535 || n < 1 || n > MAX_ANCH) return SODT_EINVAL;
  *bytes = tickets_bytes(R) + sizeof(double) * (size_t)(3 * n + 1) * (size_t)blocks_for(N, 64) * (size_t)R;
  return SODT_OK;
}

extern "C" int sodt_kmeans_lloyd(const double* obs, long N, double* books, int* alive, double* prev, int* done, int R, int n,
                                 double thresh, int iters, void* ws, size_t ws_bytes, sodt_stream_t st) {
  size_t need;
  if (sodt_kmeans_lloyd_workspace_bytes(N, R, n, &need) != SODT_OK) return SODT_EINVAL;
  if (!obs || !books || !alive || !prev || !done || !ws || iters < 0 || thresh != thresh) return SODT_EINVAL;
  if (((uintptr_t)obs & 15) || ((uintptr_t)books & 7) || ((uintptr_t)alive & 3) || ((uintptr_t)prev & 7) ||
      ((uintptr_t)done & 3) || ((uintptr_t)ws & 15) || ws_bytes < need)
    return SODT_EINVAL;
  if (iters == 0) return SODT_OK;
  hipStream_t s = (hipStream_t)st;
  if (hipMemsetAsync(ws, 0, tickets_bytes(R), s) != hipSuccess) return SODT_ELAUNCH;
  unsigned* ticket = (unsigned*)ws;
  double* part = (double*)((char*)ws + tickets_bytes(R));
  const dim3 grid(blocks_for(N, 64), R);
  const size_t lds = sizeof(double) * 3 * (size_t)n * 64;           // at most 48 KiB (n = 32)
  for (int it = 0; it < iters; ++it)
    if (int err = sodt_launch<kmeans_lloyd_kernel>(grid, dim3(64), (int)lds, s, (const double2*)obs, N, books, alive, prev, done, n,
                                                  thresh, ticket, part)) return err;
  return SODT_OK;
}
