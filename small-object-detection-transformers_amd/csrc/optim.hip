// Fused optimizer step for the training loop around the hot path: one streaming pass
// over the engine's flat f32 buffers does what the reference spreads over
//   torch.optim.SGD(momentum, nesterov=True) with the two weight-decay groups of basics/optimizer.py:35-49
//     (Train.py:145-150, :448-450: scaler.step(optimizer)),
//   ModelEMA.update  (basics/utils/torch_utils.py:291-301: a Python loop over 273 state_dict tensors), and
//   the cast of the updated f32 masters to the run dtype the GEMM kernels read
// into a single launch: p, g, momentum and EMA are read once and written once, 16 bytes per lane.
//
//   d   = g * grad_scale + wd[group] * p              (torch.optim.SGD: weight decay added to the gradient)
//   m'  = momentum[group] * m + d                     (dampening 0; the first step's "buf = d" is m = 0)
//   u   = nesterov ? d + momentum[group] * m' : m'
//   p'  = p - lr[group] * u
//   e'  = e * ema_decay + (1 - ema_decay) * p'        (skipped when ema == NULL)
//   p16 = (run dtype) p'                              (skipped when p_cast == NULL)
//
// Parameters are padded to multiples of four elements in the flat layout (engine.py), so a 16-byte chunk belongs to one
// parameter and `group_of_chunk` (one byte per chunk) selects its hyper-parameter group.  A byte below 4 is trained - with slot
// 0's hyper-parameters when it is not below ngroups, the launchers fill the unused table slots from slot 0 - and every other
// byte is what 255 is, here and in grad_stats_kernel alike (tests/test_optim_kernels_gpu.py pins both).  HBM-bound: 4 x 4 B
// read + 3 x 4 B + 2 B written per element.
//
// adam_ema_kernel is the sibling for Train.py's --adam (Train.py:147-148: optim.Adam(pg0, lr, betas=(momentum, 0.999)))
// and for AdamW (basics/optimizer.py:11-33): torch.optim.Adam / AdamW with amsgrad=False, maximize=False, step count t,
// same layout, same group map, same EMA and cast tail, one launch.
//
//   coupled:    d = g * grad_scale + wd[group] * p         p0 = p
//   decoupled:  d = g * grad_scale                         p0 = p * (1 - lr[group] * wd[group])
//   m'  = b1 * m + (1 - b1) * d                            (evaluated as torch's lerp does: m + (1 - b1) * (d - m))
//   v'  = b2 * v + (1 - b2) * d * d
//   p'  = p0 - (lr / bc1) * m' / (sqrt(v') / sqrt_bc2 + eps)       bc1 = 1 - b1^t, sqrt_bc2 = sqrt(1 - b2^t)
//
// Everything that depends only on the group (1 - b1, 1 - b2, lr / bc1, sqrt_bc2, 1 - lr * wd) is formed on the host in
// double from the double hyper-parameters, as torch forms them from Python floats, and reaches the kernel as floats:
// 1 - float(0.999) is 1.3e-5 away from float(1 - 0.999), which would show in the first steps' v' / bc2.
// 5 x 4 B read (p, g, m, v, e) + 4 x 4 B + 2 B written per element.
//
// The control path (torch.amp.GradScaler of Train.py:285, :445-450; a skipped step when a gradient is not finite; global-norm
// clipping, torch.nn.utils.clip_grad_norm_) keeps every decision on the device.  grad_stats_kernel makes one pass over the
// owned gradient (4 B read per element) and its last block, found by a ticket, finalises a sodt_step_ctl record
// (include/sodt_hip.h): found_inf, the f64 sum of squares, the clip coefficient, inv_scale_eff = grad_scale / scale *
// clip_coef, the skip flag and the applied-step counter.  The CTL = true instantiations of the two step kernels read
// inv_scale_eff, skip and (Adam) the step count t from that record where the CTL = false ones read host scalars; a skipped
// step leaves p, m (v) alone and still runs the EMA and the cast on the unchanged p.  Adam's lr / (1 - b1^t) and
// sqrt(1 - b2^t) are then formed in the kernel, in double from the double hyper-parameters (the reason is the one above),
// once per thread: lane l of each group of eight forms one of the eight values and the wave shares them.
#include "common.h"
#include "launch.h"
#include "../../include/sodt_hip.h"

namespace {

struct OptHyp { float lr[4], momentum[4], wd[4]; float grad_scale, ema_decay; int nesterov; };

template <typename TC, bool CTL>
__global__ __launch_bounds__(256) void sgd_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                     float* __restrict__ e, TC* __restrict__ pc,
                                                     const unsigned char* __restrict__ group, long nchunk, const OptHyp h,
                                                     const sodt_step_ctl* __restrict__ ctl) {
  float gscale = 1.f;
  bool live = true;
  if constexpr (CTL) { gscale = ctl->inv_scale_eff; live = ctl->skip == 0; }
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (long)gridDim.x * 256) {
    const int gi = group ? (int)group[c] : 0;
    const float lr = h.lr[gi & 3], mu = h.momentum[gi & 3], wd = h.wd[gi & 3];
    float4 pv = ((const float4*)p)[c];
    if (gi < 4 && live) {       // 255 marks padding / frozen parameters: cast only (as does a skipped step, CTL)
      const float4 gv = ((const float4*)g)[c];
      float4 mv = ((const float4*)m)[c];
      float pa[4] = {pv.x, pv.y, pv.z, pv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = fmaf(wd, pa[j], ga[j] * (CTL ? gscale : h.grad_scale));
        ma[j] = fmaf(mu, ma[j], d);
        const float u = h.nesterov ? fmaf(mu, ma[j], d) : ma[j];
        pa[j] = fmaf(-lr, u, pa[j]);
      }
      pv = make_float4(pa[0], pa[1], pa[2], pa[3]);
      ((float4*)p)[c] = pv;
      ((float4*)m)[c] = make_float4(ma[0], ma[1], ma[2], ma[3]);
    }
    if (e) {
      float4 ev = ((const float4*)e)[c];
      const float a = h.ema_decay, b1 = 1.0f - h.ema_decay;
      ev.x = fmaf(ev.x, a, b1 * pv.x); ev.y = fmaf(ev.y, a, b1 * pv.y); ev.z = fmaf(ev.z, a, b1 * pv.z); ev.w = fmaf(ev.w, a, b1 * pv.w);
      ((float4*)e)[c] = ev;
    }
    if (pc) {
      if constexpr (sizeof(TC) == 2) ((uint2*)pc)[c] = make_uint2(pack2bf(pv.x, pv.y), pack2bf(pv.z, pv.w));
      else ((float4*)pc)[c] = pv;
    }
  }
}

struct AdamHyp { float step_size[4], omb1[4], b2[4], omb2[4], sqrt_bc2[4], eps[4], wd[4], decay_mul[4]; float grad_scale, ema_decay; };

// what the CTL = true Adam kernel needs beyond AdamHyp: the record and the doubles the bias corrections are formed from
struct AdamCtl { const sodt_step_ctl* rec; double lr[4], b1[4], b2[4]; };

__device__ __forceinline__ double ipow(double b, long t) {      // b^t, t >= 1, by squaring (wave-uniform trip count)
  double r = 1.0;
  for (; t > 0; t >>= 1, b *= b)
    if (t & 1) r *= b;
  return r;
}

template <typename TC, bool CTL>
__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                      float* __restrict__ v, float* __restrict__ e, TC* __restrict__ pc,
                                                      const unsigned char* __restrict__ group, long nchunk, const AdamHyp h,
                                                      const AdamCtl ca) {
  float gscale = 1.f;
  bool live = true;
  float step_size[4] = {0.f, 0.f, 0.f, 0.f}, sqrt_bc2[4] = {1.f, 1.f, 1.f, 1.f};      // (CTL only; else h.step_size, h.sqrt_bc2)
  if constexpr (CTL) {
    gscale = ca.rec->inv_scale_eff;
    live = ca.rec->skip == 0;
    long t = ca.rec->step;
    if (t < 1) t = 1;                 // (only a skipped step can see 0; nothing then reads these)
    const int l = threadIdx.x & 7, k = l & 3;
    const double lrk = k == 0 ? ca.lr[0] : k == 1 ? ca.lr[1] : k == 2 ? ca.lr[2] : ca.lr[3];
    const double b1k = k == 0 ? ca.b1[0] : k == 1 ? ca.b1[1] : k == 2 ? ca.b1[2] : ca.b1[3];
    const double b2k = k == 0 ? ca.b2[0] : k == 1 ? ca.b2[1] : k == 2 ? ca.b2[2] : ca.b2[3];
    const double bc = 1.0 - ipow(l < 4 ? b1k : b2k, t);
    const float mine = l < 4 ? (float)(lrk / bc) : (float)sqrt(bc);      // lanes 0..3: lr / bc1[k], lanes 4..7: sqrt(bc2[k])
    const int base = (threadIdx.x & 63) & ~7;
#pragma unroll
    for (int i = 0; i < 4; ++i) { step_size[i] = __shfl(mine, base + i); sqrt_bc2[i] = __shfl(mine, base + 4 + i); }
  }
  for (long c = (long)blockIdx.x * 256 + threadIdx.x; c < nchunk; c += (long)gridDim.x * 256) {
    const int gi = group ? (int)group[c] : 0;
    const int k = gi & 3;
    float4 pv = ((const float4*)p)[c];
    if (gi < 4 && live) {       // 255 marks padding / frozen parameters: cast only (as does a skipped step, CTL)
      const float4 gv = ((const float4*)g)[c];
      const float4 mv = ((const float4*)m)[c], vv = ((const float4*)v)[c];
      float pa[4] = {pv.x, pv.y, pv.z, pv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w},
            va[4] = {vv.x, vv.y, vv.z, vv.w};
      const float step = CTL ? step_size[k] : h.step_size[k], omb1 = h.omb1[k], b2 = h.b2[k], omb2 = h.omb2[k],
                  sbc2 = CTL ? sqrt_bc2[k] : h.sqrt_bc2[k], eps = h.eps[k],
                  wd = h.wd[k], dm = h.decay_mul[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float d = fmaf(wd, pa[j], ga[j] * (CTL ? gscale : h.grad_scale));           // wd is 0 in the decoupled form, dm is 1 in the coupled one
        ma[j] = fmaf(omb1, d - ma[j], ma[j]);
        va[j] = fmaf(omb2 * d, d, va[j] * b2);
        const float denom = sqrtf(va[j]) / sbc2 + eps;
        pa[j] = fmaf(-step, ma[j] / denom, pa[j] * dm);
      }
      pv = make_float4(pa[0], pa[1], pa[2], pa[3]);
      ((float4*)p)[c] = pv;
      ((float4*)m)[c] = make_float4(ma[0], ma[1], ma[2], ma[3]);
      ((float4*)v)[c] = make_float4(va[0], va[1], va[2], va[3]);
    }
    if (e) {
      float4 ev = ((const float4*)e)[c];
      const float a = h.ema_decay, b1 = 1.0f - h.ema_decay;
      ev.x = fmaf(ev.x, a, b1 * pv.x); ev.y = fmaf(ev.y, a, b1 * pv.y); ev.z = fmaf(ev.z, a, b1 * pv.z); ev.w = fmaf(ev.w, a, b1 * pv.w);
      ((float4*)e)[c] = ev;
    }
    if (pc) {
      if constexpr (sizeof(TC) == 2) ((uint2*)pc)[c] = make_uint2(pack2bf(pv.x, pv.y), pack2bf(pv.z, pv.w));
      else ((float4*)pc)[c] = pv;
    }
  }
}

// One pass over the owned gradient: per-thread f64 sum of squares and a not-finite flag (exponent all ones), reduced over the
// wave by shuffles and over the block through LDS; one f64 atomic add and one ticket per block (at most 1024 blocks: the
// same-address atomics serialise).  The block that draws the last
// ticket reads the totals back with atomics (every word blocks share is only ever touched by device-scope atomics) and
// finalises the record with ordinary stores; the step kernel that follows is a later launch on the same stream.
__global__ __launch_bounds__(256) void grad_stats_kernel(const float* __restrict__ g, const unsigned char* __restrict__ group,
                                                        long nchunk, const float* __restrict__ scale_p,
                                                        const float* __restrict__ found_in, float grad_scale, float max_norm,
                                                        int skip_nonfinite, sodt_step_ctl* ctl) {
  double ss = 0.0;
  unsigned bad = 0;
  // four chunks per thread and trip, their group bytes and gradients loaded before any is used: the loads depend on the bounds
  // only (an unowned chunk's gradient is read, inside the buffer, and then ignored), so eight of them are in flight per thread
  const long stride = (long)gridDim.x * 256;
  for (long c0 = (long)blockIdx.x * 256 + threadIdx.x; c0 < nchunk; c0 += 4 * stride) {
    int gi[4];
    float4 gv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long c = c0 + u * stride;
      const bool in = c < nchunk;
      gi[u] = in ? (group ? (int)group[c] : 0) : 255;
      gv[u] = in ? ((const float4*)g)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (gi[u] < 4) {
        const float ga[4] = {gv[u].x, gv[u].y, gv[u].z, gv[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bad |= ((__float_as_uint(ga[j]) & 0x7f800000u) == 0x7f800000u) ? 1u : 0u;
          ss = fma((double)ga[j], (double)ga[j], ss);
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
  // The block's contributions must have been performed before its ticket is drawn.  They are returning atomics and the
  // ticket's increment is made to depend on what they return, so the wave waits for them first; no block stores anything
  // another block reads in this launch, so no cache write-back (a release fence per block) is needed.
  unsigned inc = 1u;
  const double prev = unsafeAtomicAdd(&ctl->acc_sumsq, ss);
  asm volatile("" : "+v"(inc) : "v"(prev));
  if (bad) {
    const unsigned pf = atomicOr(&ctl->acc_found, 1u);
    asm volatile("" : "+v"(inc) : "v"(pf));
  }
  if (atomicAdd(&ctl->ticket, inc) != gridDim.x - 1) return;
  const double sumsq = unsafeAtomicAdd(&ctl->acc_sumsq, 0.0);
  bool found = atomicOr(&ctl->acc_found, 0u) != 0;
  if (found_in && *found_in != 0.f) found = true;
  // torch.amp.GradScaler's unscale: inv_scale = scale.double().reciprocal().float()
  const float inv_scale = scale_p ? (float)(1.0 / (double)*scale_p) : 1.f;
  const double mul = (double)inv_scale * (double)grad_scale;
  const double norm = sqrt(sumsq) * fabs(mul);                // the norm of the gradient the update sees, before clipping
  double coef = 1.0;
  if (max_norm > 0.f) {                                       // clip_grad_norm_: max_norm / (norm + 1e-6), clamped to 1
    coef = (double)max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  const int skip = (found && skip_nonfinite) ? 1 : 0;
  ctl->sumsq = sumsq;
  ctl->grad_norm = norm;
  if (!skip) ctl->step = ctl->step + 1;
  ctl->found_inf = found ? 1.f : 0.f;
  ctl->inv_scale_eff = (float)(mul * coef);
  ctl->clip_coef = (float)coef;
  ctl->skip = skip;
}

}  // namespace

static bool flat_args_bad(const void* p, const void* g, const void* s0, const void* s1, const void* ema, const void* p_cast,
                          long n_elems, int ngroups) {
  if (!p || !g || !s0 || !s1 || n_elems <= 0 || (n_elems & 3) || ngroups < 1 || ngroups > 4) return true;
  return (((uintptr_t)p | (uintptr_t)g | (uintptr_t)s0 | (uintptr_t)s1 | (uintptr_t)ema | (uintptr_t)p_cast) & 15) != 0;
}

static int sgd_launch(float* p, const float* g, float* mom, float* ema, void* p_cast, int cast_dtype,
                      const unsigned char* group_of_chunk, long n_elems, int ngroups, const float* lr, const float* momentum,
                      const float* weight_decay, int nesterov, float grad_scale, const sodt_step_ctl* ctl, float ema_decay,
                      sodt_stream_t st) {
  if (flat_args_bad(p, g, mom, mom, ema, p_cast, n_elems, ngroups) || !lr || !momentum || !weight_decay) return SODT_EINVAL;
  OptHyp h;
  for (int i = 0; i < 4; ++i) {
    const int j = i < ngroups ? i : 0;
    h.lr[i] = lr[j]; h.momentum[i] = momentum[j]; h.wd[i] = weight_decay[j];
  }
  h.grad_scale = grad_scale; h.ema_decay = ema_decay; h.nesterov = nesterov;
  const long nchunk = n_elems >> 2;
  long nb = (nchunk + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipStream_t s = (hipStream_t)st;
  const bool bf = p_cast && cast_dtype == SODT_BF16;
  if (!bf && p_cast && cast_dtype != SODT_F32) return SODT_EINVAL;
#define SODT_SGD_LAUNCH(TC, CTL) \
  sodt_launch<sgd_ema_kernel<TC, CTL>>(dim3((unsigned)nb), dim3(256), 0, s, p, g, mom, ema, (TC*)p_cast, group_of_chunk, nchunk, h, ctl)
  if (ctl) return bf ? SODT_SGD_LAUNCH(bf16, true) : SODT_SGD_LAUNCH(float, true);
  return bf ? SODT_SGD_LAUNCH(bf16, false) : SODT_SGD_LAUNCH(float, false);
#undef SODT_SGD_LAUNCH
}

extern "C" int sodt_sgd_ema_step(float* p, const float* g, float* mom, float* ema, void* p_cast, int cast_dtype,
                                 const unsigned char* group_of_chunk, long n_elems, int ngroups, const float* lr,
                                 const float* momentum, const float* weight_decay, int nesterov, float grad_scale,
                                 float ema_decay, sodt_stream_t st) {
  return sgd_launch(p, g, mom, ema, p_cast, cast_dtype, group_of_chunk, n_elems, ngroups, lr, momentum, weight_decay, nesterov,
                    grad_scale, nullptr, ema_decay, st);
}

extern "C" int sodt_sgd_ema_step_ctl(float* p, const float* g, float* mom, float* ema, void* p_cast, int cast_dtype,
                                     const unsigned char* group_of_chunk, long n_elems, int ngroups, const float* lr,
                                     const float* momentum, const float* weight_decay, int nesterov, const sodt_step_ctl* ctl,
                                     float ema_decay, sodt_stream_t st) {
  if (!ctl || ((uintptr_t)ctl & 15)) return SODT_EINVAL;
  return sgd_launch(p, g, mom, ema, p_cast, cast_dtype, group_of_chunk, n_elems, ngroups, lr, momentum, weight_decay, nesterov,
                    1.f, ctl, ema_decay, st);
}

static int adam_launch(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, void* p_cast, int cast_dtype,
                       const unsigned char* group_of_chunk, long n_elems, int ngroups, const double* lr, const double* beta1,
                       const double* beta2, const double* eps, const double* weight_decay, int decoupled, long step,
                       float grad_scale, const sodt_step_ctl* ctl, float ema_decay, sodt_stream_t st) {
  if (flat_args_bad(p, g, exp_avg, exp_avg_sq, ema, p_cast, n_elems, ngroups) || !lr || !beta1 || !beta2 || !eps ||
      !weight_decay || step < 1)
    return SODT_EINVAL;
  AdamHyp h;
  AdamCtl ca;
  ca.rec = ctl;
  for (int i = 0; i < 4; ++i) {
    const int j = i < ngroups ? i : 0;
    if (!(eps[j] > 0.0) || !(beta1[j] >= 0.0 && beta1[j] < 1.0) || !(beta2[j] >= 0.0 && beta2[j] < 1.0)) return SODT_EINVAL;
    const double bc1 = 1.0 - pow(beta1[j], (double)step), bc2 = 1.0 - pow(beta2[j], (double)step);
    h.step_size[i] = (float)(lr[j] / bc1);
    h.omb1[i] = (float)(1.0 - beta1[j]);
    h.b2[i] = (float)beta2[j]; h.omb2[i] = (float)(1.0 - beta2[j]);
    h.sqrt_bc2[i] = (float)sqrt(bc2);
    h.eps[i] = (float)eps[j];
    h.wd[i] = decoupled ? 0.f : (float)weight_decay[j];
    h.decay_mul[i] = decoupled ? (float)(1.0 - lr[j] * weight_decay[j]) : 1.f;
    ca.lr[i] = lr[j]; ca.b1[i] = beta1[j]; ca.b2[i] = beta2[j];        // (CTL: step_size and sqrt_bc2 are formed in the kernel)
  }
  h.grad_scale = grad_scale; h.ema_decay = ema_decay;
  const long nchunk = n_elems >> 2;
  long nb = (nchunk + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipStream_t s = (hipStream_t)st;
  const bool bf = p_cast && cast_dtype == SODT_BF16;
  if (!bf && p_cast && cast_dtype != SODT_F32) return SODT_EINVAL;
#define SODT_ADAM_LAUNCH(TC, CTL)                                                                                            \
  sodt_launch<adam_ema_kernel<TC, CTL>>(dim3((unsigned)nb), dim3(256), 0, s, p, g, exp_avg, exp_avg_sq, ema, (TC*)p_cast, \
                     group_of_chunk, nchunk, h, ca)
  if (ctl) return bf ? SODT_ADAM_LAUNCH(bf16, true) : SODT_ADAM_LAUNCH(float, true);
  return bf ? SODT_ADAM_LAUNCH(bf16, false) : SODT_ADAM_LAUNCH(float, false);
#undef SODT_ADAM_LAUNCH
}

extern "C" int sodt_adam_ema_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, void* p_cast,
                                  int cast_dtype, const unsigned char* group_of_chunk, long n_elems, int ngroups,
                                  const double* lr, const double* beta1, const double* beta2, const double* eps,
                                  const double* weight_decay, int decoupled, long step, float grad_scale, float ema_decay,
                                  sodt_stream_t st) {
  return adam_launch(p, g, exp_avg, exp_avg_sq, ema, p_cast, cast_dtype, group_of_chunk, n_elems, ngroups, lr, beta1, beta2, eps,
                     weight_decay, decoupled, step, grad_scale, nullptr, ema_decay, st);
}

extern "C" int sodt_adam_ema_step_ctl(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* ema, void* p_cast,
                                      int cast_dtype, const unsigned char* group_of_chunk, long n_elems, int ngroups,
                                      const double* lr, const double* beta1, const double* beta2, const double* eps,
                                      const double* weight_decay, int decoupled, const sodt_step_ctl* ctl, float ema_decay,
                                      sodt_stream_t st) {
  if (!ctl || ((uintptr_t)ctl & 15)) return SODT_EINVAL;
  return adam_launch(p, g, exp_avg, exp_avg_sq, ema, p_cast, cast_dtype, group_of_chunk, n_elems, ngroups, lr, beta1, beta2, eps,
                     weight_decay, decoupled, 1, 1.f, ctl, ema_decay, st);
}

extern "C" int sodt_grad_stats(const float* g, const unsigned char* group_of_chunk, long n_elems, const float* scale,
                               const float* found_inf_in, float grad_scale, float max_norm, int skip_nonfinite,
                               sodt_step_ctl* ctl, sodt_stream_t st) {
  if (!g || !ctl || n_elems <= 0 || (n_elems & 3)) return SODT_EINVAL;
  if ((((uintptr_t)g | (uintptr_t)ctl) & 15) || (((uintptr_t)scale | (uintptr_t)found_inf_in) & 3)) return SODT_EINVAL;
  if (!(grad_scale == grad_scale) || !(max_norm == max_norm)) return SODT_EINVAL;
  const long nchunk = n_elems >> 2;
  long nb = (nchunk + 1023) / 1024;       // four chunks per thread and trip; one atomic add and one ticket per block
  if (nb > 1024) nb = 1024;
  hipStream_t s = (hipStream_t)st;
  // the three words the blocks share (acc_sumsq, acc_found, ticket: the record's first 16 bytes) start every call at zero
  if (hipMemsetAsync(ctl, 0, 16, s) != hipSuccess) return SODT_ELAUNCH;
  return sodt_launch<grad_stats_kernel>(dim3((unsigned)nb), dim3(256), 0, s, g, group_of_chunk, nchunk, scale, found_inf_in,
                     grad_scale, max_norm, skip_nonfinite, ctl);
}
