// Sharpness-aware minimisation around the fused optimizer step (basics/utils/sam.py): the reference's SAM.first_step loops
// over the 273 parameter views with one norm, one clone and one add_ per tensor, and second_step re-points p.data at the
// clones.  Over the engine's flat f32 buffers (the layout and the chunk -> group map of csrc/optim.hip: 4-element chunks,
// at most 4 groups, 255 = not owned and never written) the same is three streaming kernels:
//
//   sam_norm_kernel      sumsq = sum over owned elements of (w * g)^2 in f64, w = |p| for an adaptive group, else 1
//                        (sam.py:49-59); the last block, found by a ticket, finalises the 64-byte record of include/sodt_hip.h:
//                        norm = sqrt(sumsq) * |inv_scale|, found, inv = found ? 0 : 1 / (norm + 1e-12)
//   sam_perturb_kernel   old_p = p;  p += (adaptive ? p*p : 1) * g * inv_scale * (rho[group] * inv);  p_cast = (run dtype) p
//                        (sam.py:19-25); inv, inv_scale and found are read from the record, so nothing returns to the host
//   sam_restore_kernel   p = old_p   (sam.py:34)
//
// inv_scale is what sodt_grad_stats forms (GradScaler's double reciprocal of the device scale, rounded to f32, times the host
// grad_scale): the gradient enters as stored and the division by the norm of the same gradient makes the direction scale-free.
// A gradient that is not finite leaves p bit for bit as it is (inv = 0 would still give 0 * inf = NaN, so the kernel does not
// form e_w at all then); old_p and the mirror are written all the same, and the restore that follows is then a plain copy.
//
// Bytes per owned element: norm 4 read (8 adaptive); perturb 8 read + 8 + 2 written; restore 4 read + 4 written.
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

// the record as the kernels see it (64 bytes; the header documents the layout, callers pass a double*)
struct SamRec {
  double acc_sumsq; unsigned acc_found, ticket;
  double sumsq, norm, inv;
  float found, inv_scale; int reserved[4];
};
static_assert(sizeof(SamRec) == 64, "the SAM record is 64 bytes");

struct SamHyp { float rho[4]; unsigned adaptive; };      // adaptive: bit i = group i

// grad_stats_kernel's shape (csrc/optim.hip): four chunks in flight per thread, f64 partial sums reduced by shuffles and LDS, one
// returning atomic add and one ticket per block, no per-block fence.  ADAPT = false never touches p.
template <bool ADAPT>
__global__ __launch_bounds__(256) void sam_norm_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                      const unsigned char* __restrict__ group, long nchunk, const SamHyp h,
                                                      const float* __restrict__ scale_p, float grad_scale, SamRec* rec) {
  double ss = 0.0;
  unsigned bad = 0;
  const long stride = (long)gridDim.x * 256;
  for (long c0 = (long)blockIdx.x * 256 + threadIdx.x; c0 < nchunk; c0 += 4 * stride) {
    int gi[4];
    float4 gv[4], pv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long c = c0 + u * stride;
      const bool in = c < nchunk;
      gi[u] = in ? (group ? (int)group[c] : 0) : 255;
      gv[u] = in ? ((const float4*)g)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (ADAPT) pv[u] = in ? ((const float4*)p)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (gi[u] < 4) {
        const float ga[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
        float wa[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (ADAPT) {
          if ((h.adaptive >> gi[u]) & 1u) { wa[0] = fabsf(pv[u].x); wa[1] = fabsf(pv[u].y); wa[2] = fabsf(pv[u].z); wa[3] = fabsf(pv[u].w); }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bad |= ((__float_as_uint(ga[j]) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
          const double t = ADAPT ? (double)wa[j] * (double)ga[j] : (double)ga[j];
          ss = fma(t, t, ss);
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { ss += __shfl_down(ss, o); bad |= __shfl_down(bad, o); }
  __shared__ double s_ss[4];
  __shared__ unsigned s_bad[4];
  if ((threadIdx.x & 63) == 0) { s_ss[threadIdx.x >> 6] = ss; s_bad[threadIdx.x >> 6] = bad; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  ss = (s_ss[0] + s_ss[1]) + (s_ss[2] + s_ss[3]);
  bad = s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3];
  // as in grad_stats_kernel: the ticket's increment depends on what the block's atomics return, so they are performed first
  unsigned inc = 1u;
  const double prev = unsafeAtomicAdd(&rec->acc_sumsq, ss);
  asm volatile("" : "+v"(inc) : "v"(prev));
  if (bad) {
    const unsigned pf = atomicOr(&rec->acc_found, 1u);
    asm volatile("" : "+v"(inc) : "v"(pf));
  }
  if (atomicAdd(&rec->ticket, inc) != gridDim.x - 1) return;
  const double sumsq = unsafeAtomicAdd(&rec->acc_sumsq, 0.0);
  bool found = atomicOr(&rec->acc_found, 0u) != 0;
  const float inv_scale = scale_p ? (float)(1.0 / (double)*scale_p) : 1.f;      // GradScaler: scale.double().reciprocal().float()
  const double mul = (double)inv_scale * (double)grad_scale;
  const double norm = sqrt(sumsq) * fabs(mul);
  if (!(norm <= 1.7976931348623157e308)) found = true;       // (an adaptive |p| * g beyond f64, or a scale that is not finite)
  rec->sumsq = sumsq;
  rec->norm = norm;
  rec->inv = found ? 0.0 : 1.0 / (norm + 1e-12);
  rec->found = found ? 1.f : 0.f;
  rec->inv_scale = (float)mul;
}

template <typename TC>
__global__ __launch_bounds__(256) void sam_perturb_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ old_p, TC* __restrict__ pc,
                                                         const unsigned char* __restrict__ group, long nchunk, const SamHyp h,
                                                         const SamRec* __restrict__ rec) {
  const bool live = rec->found == 0.f;
  const float gscale = rec->inv_scale;
  const double inv = rec->inv;
  float k[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) k[i] = (float)((double)h.rho[i] * inv);
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (long)gridDim.x * 256) {
    const int gi = group ? (int)group[c] : 0;
    if (gi >= 4) continue;            // not owned: p, old_p and the mirror keep what they hold
    float4 pv = ((const float4*)p)[c];
    ((float4*)old_p)[c] = pv;
    if (live) {
      const float4 gv = ((const float4*)g)[c];
      const float kg = gi == 0 ? k[0] : gi == 1 ? k[1] : gi == 2 ? k[2] : k[3];
      float pa[4] = {pv.x, pv.y, pv.z, pv.w};
      const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
      const bool ad = ((h.adaptive >> gi) & 1u) != 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = (ad ? pa[j] * pa[j] * ga[j] : ga[j]) * gscale;
        pa[j] = fmaf(e, kg, pa[j]);
      }
      pv = make_float4(pa[0], pa[1], pa[2], pa[3]);
      ((float4*)p)[c] = pv;
    }
    if (pc) {
      if constexpr (sizeof(TC) == 2) ((uint2*)pc)[c] = make_uint2(pack2bf(pv.x, pv.y), pack2bf(pv.z, pv.w));
      else ((float4*)pc)[c] = pv;
    }
  }
}

__global__ __launch_bounds__(256) void sam_restore_kernel(float* __restrict__ p, const float* __restrict__ old_p,
                                                         const unsigned char* __restrict__ group, long nchunk) {
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (long)gridDim.x * 256) {
    const int gi = group ? (int)group[c] : 0;
    if (gi < 4) ((float4*)p)[c] = ((const float4*)old_p)[c];
  }
}

// the per-group hyper-parameters of a call; false: a rho that is negative or NaN (rho null: the norm entry has none).
// The slots from ngroups up get rho 0 and no adaptive flag: a map byte in [ngroups, 4) names no group of the call, so its chunk
// is not moved (it still counts as owned: old_p and the mirror are written, and the restore copies the same values back).
bool sam_hyp(SamHyp& h, int ngroups, const float* rho, const int* adaptive, bool& any_adaptive) {
  h.adaptive = 0;
  for (int i = 0; i < 4; ++i) {
    h.rho[i] = (rho && i < ngroups) ? rho[i] : 0.f;
    if (!(h.rho[i] >= 0.f)) return false;
    if (i < ngroups && adaptive[i]) h.adaptive |= 1u << i;
  }
  any_adaptive = h.adaptive != 0;
  return true;
}

long stream_blocks(long nchunk) {
  const long nb = (nchunk + 255) / 256;
  return nb > 8192 ? 8192 : nb;
}

}  // namespace

extern "C" int sodt_sam_norm(const float* p, const float* g, const unsigned char* group_of_chunk, long n_elems, int ngroups,
                             const int* adaptive, const float* scale, float grad_scale, double* rec, sodt_stream_t st) {
  if (!g || !rec || !adaptive || n_elems <= 0 || (n_elems & 3) || ngroups < 1 || ngroups > 4) return SODT_EINVAL;
  if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)rec) & 15) || ((uintptr_t)scale & 3)) return SODT_EINVAL;
  if (!(grad_scale == grad_scale)) return SODT_EINVAL;
  SamHyp h;
  bool any;
  if (!sam_hyp(h, ngroups, nullptr, adaptive, any) || (any && !p)) return SODT_EINVAL;
  const long nchunk = n_elems >> 2;
  long nb = (nchunk + 1023) / 1024;       // four chunks per thread and trip; one atomic add and one ticket per block
  if (nb > 1024) nb = 1024;
  hipStream_t s = (hipStream_t)st;
  // the three words the blocks share (acc_sumsq, acc_found, ticket: the record's first 16 bytes) start every call at zero
  if (hipMemsetAsync(rec, 0, 16, s) != hipSuccess) return SODT_ELAUNCH;
  if (any)
    return sodt_launch<sam_norm_kernel<true>>(dim3((unsigned)nb), dim3(256), 0, s, p, g, group_of_chunk, nchunk, h, scale,
                                              grad_scale, (SamRec*)rec);
  return sodt_launch<sam_norm_kernel<false>>(dim3((unsigned)nb), dim3(256), 0, s, (const float*)nullptr, g, group_of_chunk,
                                             nchunk, h, scale, grad_scale, (SamRec*)rec);
}

extern "C" int sodt_sam_perturb(float* p, const float* g, float* old_p, void* p_cast, int cast_dtype,
                                const unsigned char* group_of_chunk, long n_elems, int ngroups, const float* rho,
                                const int* adaptive, const double* rec, sodt_stream_t st) {
  if (!p || !g || !old_p || !rec || !rho || !adaptive || n_elems <= 0 || (n_elems & 3) || ngroups < 1 || ngroups > 4)
    return SODT_EINVAL;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)old_p | (uintptr_t)p_cast | (uintptr_t)rec) & 15) return SODT_EINVAL;
  const bool bf = p_cast && cast_dtype == SODT_BF16;
  if (!bf && p_cast && cast_dtype != SODT_F32) return SODT_EINVAL;
  SamHyp h;
  bool any;
  if (!sam_hyp(h, ngroups, rho, adaptive, any)) return SODT_EINVAL;
  const long nchunk = n_elems >> 2;
  const long nb = stream_blocks(nchunk);
  hipStream_t s = (hipStream_t)st;
  if (bf)
    return sodt_launch<sam_perturb_kernel<bf16>>(dim3((unsigned)nb), dim3(256), 0, s, p, g, old_p, (bf16*)p_cast, group_of_chunk,
                                                 nchunk, h, (const SamRec*)rec);
  return sodt_launch<sam_perturb_kernel<float>>(dim3((unsigned)nb), dim3(256), 0, s, p, g, old_p, (float*)p_cast, group_of_chunk,
                                                nchunk, h, (const SamRec*)rec);
}

extern "C" int sodt_sam_restore(float* p, const float* old_p, const unsigned char* group_of_chunk, long n_elems,
                                sodt_stream_t st) {
  if (!p || !old_p || n_elems <= 0 || (n_elems & 3) || (((uintptr_t)p | (uintptr_t)old_p) & 15)) return SODT_EINVAL;
  const long nchunk = n_elems >> 2;
  return sodt_launch<sam_restore_kernel>(dim3((unsigned)stream_blocks(nchunk)), dim3(256), 0, (hipStream_t)st, p, old_p,
                                         group_of_chunk, nchunk);
}
