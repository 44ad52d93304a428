// Fused TF-formulation Adam + EMA over a flat f32 parameter range, and per-segment sum of squares
// (gradient norms / global-norm clipping).  Reference: tf.train.AdamOptimizer as called at
// SURFGAN_3D/optimization.py:16,28; tf.train.ExponentialMovingAverage via ExtendedEMA.py:56-59;
// tf.norm / tf.clip_by_global_norm at optimization.py:66-71.  One pass: 5 reads + 4 writes of 4 B/param.
//
// Non-finite step guard (not in the reference; off by default, optimization.StepGraph): an all-finite test over a network's
// flat gradient (alone, or fused into the sum of squares of the clipping path) sets a device flag; a one-thread bookkeeping
// kernel advances the optimiser's device step count and writes the step size only when the flag is clear; the guarded
// update kernels read the flag and then either compute exactly what the unguarded ones compute or take the EMA-only path.
// Flags are set with plain stores of the value 1 (any order gives the same result: deterministic).
#include "common.h"

namespace {

__device__ __forceinline__ void adam_ema_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, float* __restrict__ ema, int64_t numel, float lr_t,
                                              float b1, float b2, float eps, float gscale, float ema_decay) {
  const int64_t nv = numel / 4;
  const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const float omd = 1.f - ema_decay;
  for (int64_t i = tid0; i < nv; i += stride) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    if (g) {
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * gscale;
      f32x4 mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
      mm = b1 * mm + (1.f - b1) * gg;
      vv = b2 * vv + (1.f - b2) * gg * gg;
#pragma unroll
      for (int e = 0; e < 4; ++e) pp[e] -= lr_t * mm[e] / (sqrtf(vv[e]) + eps);
      reinterpret_cast<f32x4*>(m)[i] = mm;
      SG_STORE16_GUARD(mm);
      reinterpret_cast<f32x4*>(v)[i] = vv;
      SG_STORE16_GUARD(vv);
      reinterpret_cast<f32x4*>(p)[i] = pp;
      SG_STORE16_GUARD(pp);
    }
    if (ema) {
      f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
      ee -= omd * (ee - pp);
      reinterpret_cast<f32x4*>(ema)[i] = ee;
      SG_STORE16_GUARD(ee);
    }
  }
  for (int64_t i = nv * 4 + tid0; i < numel; i += stride) {
    float pp = p[i];
    if (g) {
      const float gg = g[i] * gscale;
      const float mm = b1 * m[i] + (1.f - b1) * gg;
      const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
      pp -= lr_t * mm / (sqrtf(vv) + eps);
      m[i] = mm; v[i] = vv; p[i] = pp;
    }
    if (ema) ema[i] -= omd * (ema[i] - pp);
  }
}

__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                float* __restrict__ v, float* __restrict__ ema, int64_t numel, float lr_t, float b1,
                                float b2, float eps, float gscale, float ema_decay, const float* __restrict__ lr_dev) {
  if (lr_dev) lr_t = *lr_dev;      // captured step: the bias-corrected step size is written by the host before each replay
  adam_ema_body(p, g, m, v, ema, numel, lr_t, b1, b2, eps, gscale, ema_decay);
}

// Guarded step: a set skip flag turns the launch into the EMA-only one (g NULL), a clear one computes what adam_ema_kernel
// computes with lr_t read from device memory (written by guard_step_kernel).
__global__ void adam_ema_guard_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                      float* __restrict__ v, float* __restrict__ ema, int64_t numel,
                                      const float* __restrict__ lr_dev, float b1, float b2, float eps, float gscale,
                                      float ema_decay, const int32_t* __restrict__ skip) {
  const bool skipped = *skip != 0;
  if (skipped && !ema) return;
  adam_ema_body(p, skipped ? nullptr : g, m, v, ema, numel, skipped ? 0.f : *lr_dev, b1, b2, eps, gscale, ema_decay);
}

// tf.train.GradientDescentOptimizer / MomentumOptimizer(use_nesterov) / AdadeltaOptimizer(rho, epsilon) as created
// at SURFGAN_3D/optimization.py:17-22,29-35, fused with the EMA update like Adam above.  TF's update rules
// (training_ops: ApplyGradientDescent, ApplyMomentum, ApplyAdadelta):
//   SGD       p -= lr * g
//   Momentum  a = h * a + g;  p -= nesterov ? lr * g + lr * h * a : lr * a
//   Adadelta  a = h * a + (1-h) g^2;  u = sqrt(a2 + eps) * rsqrt(a + eps) * g;  p -= lr * u;  a2 = h * a2 + (1-h) u^2
template <int KIND>
__device__ __forceinline__ void optim_rule(float& p, float g, float& s1, float& s2, float lr, float h, float eps,
                                           int nesterov) {
  if (KIND == SG_OPT_SGD) {
    p -= lr * g;
  } else if (KIND == SG_OPT_MOMENTUM) {
    s1 = h * s1 + g;
    p -= nesterov ? (lr * g + lr * h * s1) : lr * s1;
  } else {
    s1 = h * s1 + (1.f - h) * g * g;
    const float u = sqrtf(s2 + eps) * rsqrtf(s1 + eps) * g;
    p -= lr * u;
    s2 = h * s2 + (1.f - h) * u * u;
  }
}

template <int KIND>
__device__ __forceinline__ void optim_step_body(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                                float* __restrict__ s2, float* __restrict__ ema, int64_t numel, float lr,
                                                float h, float eps, int nesterov, float gscale, float ema_decay) {
  const int64_t nv = numel / 4;
  const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const float omd = 1.f - ema_decay;
  for (int64_t i = tid0; i < nv; i += stride) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * gscale;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (KIND != SG_OPT_SGD) a = reinterpret_cast<f32x4*>(s1)[i];
    if (KIND == SG_OPT_ADADELTA) b = reinterpret_cast<f32x4*>(s2)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // (ext-vector elements cannot bind to references)
      float pe = pp[e], ae = a[e], be = b[e];
      optim_rule<KIND>(pe, gg[e], ae, be, lr, h, eps, nesterov);
      pp[e] = pe; a[e] = ae; b[e] = be;
    }
    if (KIND != SG_OPT_SGD) reinterpret_cast<f32x4*>(s1)[i] = a;
    SG_STORE16_GUARD(a);
    if (KIND == SG_OPT_ADADELTA) reinterpret_cast<f32x4*>(s2)[i] = b;
    SG_STORE16_GUARD(b);
    reinterpret_cast<f32x4*>(p)[i] = pp;
    SG_STORE16_GUARD(pp);
    if (ema) {
      f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
      ee -= omd * (ee - pp);
      reinterpret_cast<f32x4*>(ema)[i] = ee;
      SG_STORE16_GUARD(ee);
    }
  }
  for (int64_t i = nv * 4 + tid0; i < numel; i += stride) {
    float pp = p[i], a = KIND != SG_OPT_SGD ? s1[i] : 0.f, b = KIND == SG_OPT_ADADELTA ? s2[i] : 0.f;
    optim_rule<KIND>(pp, g[i] * gscale, a, b, lr, h, eps, nesterov);
    if (KIND != SG_OPT_SGD) s1[i] = a;
    if (KIND == SG_OPT_ADADELTA) s2[i] = b;
    p[i] = pp;
    if (ema) ema[i] -= omd * (ema[i] - pp);
  }
}

template <int KIND>
__global__ void optim_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                  float* __restrict__ s2, float* __restrict__ ema, int64_t numel, float lr, float h,
                                  float eps, int nesterov, float gscale, float ema_decay, const float* __restrict__ lr_dev) {
  if (lr_dev) lr = *lr_dev;
  optim_step_body<KIND>(p, g, s1, s2, ema, numel, lr, h, eps, nesterov, gscale, ema_decay);
}

// The EMA-only pass of a skipped step: the arithmetic of adam_ema_body's `g == NULL` path.
__device__ __forceinline__ void ema_only_body(const float* __restrict__ p, float* __restrict__ ema, int64_t numel,
                                              float ema_decay) {
  const int64_t nv = numel / 4;
  const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  const float omd = 1.f - ema_decay;
  for (int64_t i = tid0; i < nv; i += stride) {
    const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
    f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
    ee -= omd * (ee - pp);
    reinterpret_cast<f32x4*>(ema)[i] = ee;
    SG_STORE16_GUARD(ee);
  }
  for (int64_t i = nv * 4 + tid0; i < numel; i += stride) ema[i] -= omd * (ema[i] - p[i]);
}

template <int KIND>
__global__ void optim_step_guard_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s1,
                                        float* __restrict__ s2, float* __restrict__ ema, int64_t numel,
                                        const float* __restrict__ lr_dev, float h, float eps, int nesterov, float gscale,
                                        float ema_decay, const int32_t* __restrict__ skip) {
  if (*skip) {
    if (ema) ema_only_body(p, ema, numel, ema_decay);
    return;
  }
  optim_step_body<KIND>(p, g, s1, s2, ema, numel, *lr_dev, h, eps, nesterov, gscale, ema_decay);
}

__device__ __forceinline__ bool finite4(const f32x4 v) {
  return __builtin_isfinite(v[0]) & __builtin_isfinite(v[1]) & __builtin_isfinite(v[2]) & __builtin_isfinite(v[3]);
}

// flag = 1 if any of x[0..numel) is NaN or +-Inf (the caller clears it first).  f32x4 loads, scalar tail for numel % 4.
__global__ __launch_bounds__(256) void nonfinite_flag_kernel(const float* __restrict__ x, int64_t numel,
                                                             int32_t* __restrict__ flag) {
  const int64_t nv = numel / 4;
  const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  bool ok = true;
  for (int64_t i = tid0; i < nv; i += stride) ok &= finite4(reinterpret_cast<const f32x4*>(x)[i]);
  for (int64_t i = nv * 4 + tid0; i < numel; i += stride) ok &= __builtin_isfinite(x[i]);
  if (!ok) *flag = 1;
}

// One bookkeeping thread per guarded train op, between the flag and the update: an applied step advances the device step
// count t and writes the step size the update reads (Adam: lr*sqrt(1-b2^t)/(1-b1^t) in double, as the host computes it,
// then rounded to float; the other rules: lr); a skipped one counts.  cnt: [skipped, consecutive skips, longest run].
__global__ void guard_step_kernel(const int32_t* __restrict__ flag, int64_t* __restrict__ t, int64_t* __restrict__ cnt,
                                  double lr, const double* __restrict__ lr_dev, float* __restrict__ lr_t, int adam, double b1,
                                  double b2) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (*flag) {
    const int64_t run = cnt[1] + 1;
    cnt[0] += 1;
    cnt[1] = run;
    if (run > cnt[2]) cnt[2] = run;
    return;
  }
  if (lr_dev) lr = *lr_dev;
  const int64_t s = *t + 1;
  *t = s;
  cnt[1] = 0;
  *lr_t = adam ? (float)(lr * sqrt(1.0 - pow(b2, (double)s)) / (1.0 - pow(b1, (double)s))) : (float)lr;
}

// flag (may be NULL): the all-finite test of nonfinite_flag_kernel on the values this pass reads anyway.  It is a separate
// test: a finite gradient whose squares overflow (3e38) is not flagged.
__device__ __forceinline__ void segment_sumsq_body(const float* __restrict__ flat, const int64_t* __restrict__ offsets,
                                                   float* __restrict__ out, int32_t* __restrict__ flag) {
  __shared__ float red[256];
  const int seg = blockIdx.x;
  const int64_t b = offsets[seg], e = offsets[seg + 1];
  float s = 0.f;
  bool ok = true;
  for (int64_t i = b + threadIdx.x; i < e; i += 256) {
    const float x = flat[i];
    s += x * x;
    if (flag) ok &= __builtin_isfinite(x);
  }
  if (flag && !ok) *flag = 1;
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[seg] = red[0];
}

__global__ __launch_bounds__(256) void segment_sumsq_kernel(const float* __restrict__ flat,
                                                            const int64_t* __restrict__ offsets,
                                                            float* __restrict__ out) {
  segment_sumsq_body(flat, offsets, out, nullptr);
}

__global__ __launch_bounds__(256) void segment_sumsq_flag_kernel(const float* __restrict__ flat,
                                                                 const int64_t* __restrict__ offsets,
                                                                 float* __restrict__ out, int32_t* __restrict__ flag) {
  segment_sumsq_body(flat, offsets, out, flag);
}

}  // namespace

static int adam_ema_launch(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, float lr_t, const float* lr_dev,
                           float b1, float b2, float eps, float gscale, float ema_decay, sg_stream_t st) {
  if (!p || numel < 1 || (g && (!m || !v)) || (!g && !ema)) return SG_EINVAL;
  if (!sg_aligned16(p) || (g && (!sg_aligned16(g) || !sg_aligned16(m) || !sg_aligned16(v))) ||
      (ema && !sg_aligned16(ema)))
    return SG_EALIGN;
  int64_t blocks = (numel / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adam_ema_kernel, dim3((unsigned)blocks), dim3(256), 0, sg_st(st), p, g, m, v, ema, numel, lr_t,
                     b1, b2, eps, gscale, ema_decay, lr_dev);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, float lr_t,
                           float b1, float b2, float eps, float gscale, float ema_decay, sg_stream_t st) {
  return adam_ema_launch(p, g, m, v, ema, numel, lr_t, nullptr, b1, b2, eps, gscale, ema_decay, st);
}

extern "C" int sg_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, const float* lr_t,
                               float b1, float b2, float eps, float gscale, float ema_decay, sg_stream_t st) {
  if (!lr_t) return SG_EINVAL;
  return adam_ema_launch(p, g, m, v, ema, numel, 0.f, lr_t, b1, b2, eps, gscale, ema_decay, st);
}

static int optim_step_launch(int kind, float* p, const float* g, float* s1, float* s2, float* ema, int64_t numel,
                             float lr, const float* lr_dev, float h, float eps, int nesterov, float gscale, float ema_decay,
                             sg_stream_t st) {
  if (!p || !g || numel < 1) return SG_EINVAL;
  if (kind != SG_OPT_SGD && kind != SG_OPT_MOMENTUM && kind != SG_OPT_ADADELTA) return SG_EINVAL;
  if ((kind != SG_OPT_SGD && !s1) || (kind == SG_OPT_ADADELTA && !s2)) return SG_EINVAL;
  if (!sg_aligned16(p) || !sg_aligned16(g) || (s1 && !sg_aligned16(s1)) || (s2 && !sg_aligned16(s2)) ||
      (ema && !sg_aligned16(ema)))
    return SG_EALIGN;
  int64_t blocks = (numel / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  const dim3 grid((unsigned)blocks), blk(256);
  if (kind == SG_OPT_SGD)
    hipLaunchKernelGGL(optim_step_kernel<SG_OPT_SGD>, grid, blk, 0, sg_st(st), p, g, s1, s2, ema, numel, lr, h, eps,
                       nesterov, gscale, ema_decay, lr_dev);
  else if (kind == SG_OPT_MOMENTUM)
    hipLaunchKernelGGL(optim_step_kernel<SG_OPT_MOMENTUM>, grid, blk, 0, sg_st(st), p, g, s1, s2, ema, numel, lr, h,
                       eps, nesterov, gscale, ema_decay, lr_dev);
  else
    hipLaunchKernelGGL(optim_step_kernel<SG_OPT_ADADELTA>, grid, blk, 0, sg_st(st), p, g, s1, s2, ema, numel, lr, h,
                       eps, nesterov, gscale, ema_decay, lr_dev);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_optim_step(int kind, float* p, const float* g, float* s1, float* s2, float* ema, int64_t numel,
                             float lr, float h, float eps, int nesterov, float gscale, float ema_decay,
                             sg_stream_t st) {
  return optim_step_launch(kind, p, g, s1, s2, ema, numel, lr, nullptr, h, eps, nesterov, gscale, ema_decay, st);
}

extern "C" int sg_optim_step_dev(int kind, float* p, const float* g, float* s1, float* s2, float* ema, int64_t numel,
                                 const float* lr, float h, float eps, int nesterov, float gscale, float ema_decay,
                                 sg_stream_t st) {
  if (!lr) return SG_EINVAL;
  return optim_step_launch(kind, p, g, s1, s2, ema, numel, 0.f, lr, h, eps, nesterov, gscale, ema_decay, st);
}

extern "C" int sg_segment_sumsq(const float* flat, const int64_t* offsets, float* out, int32_t nseg,
                                sg_stream_t st) {
  if (!flat || !offsets || !out || nseg < 1) return SG_EINVAL;
  hipLaunchKernelGGL(segment_sumsq_kernel, dim3(nseg), dim3(256), 0, sg_st(st), flat, offsets, out);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

// ---- non-finite step guard ------------------------------------------------------------------------------------------
static int clear_flag(int32_t* flag, sg_stream_t st) {
  const hipError_t e = hipMemsetAsync(flag, 0, sizeof(int32_t), sg_st(st));
  return e == hipSuccess ? SG_OK : (int)e;
}

extern "C" int sg_nonfinite_flag(const float* x, int64_t numel, int32_t* flag, int32_t accumulate, sg_stream_t st) {
  if (!x || !flag || numel < 1) return SG_EINVAL;
  if (!sg_aligned16(x)) return SG_EALIGN;
  if (!accumulate) {
    const int rc = clear_flag(flag, st);
    if (rc != SG_OK) return rc;
  }
  int64_t blocks = (numel / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(nonfinite_flag_kernel, dim3((unsigned)blocks), dim3(256), 0, sg_st(st), x, numel, flag);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_segment_sumsq_flag(const float* flat, const int64_t* offsets, float* out, int32_t nseg, int32_t* flag,
                                     int32_t accumulate, sg_stream_t st) {
  if (!flat || !offsets || !out || !flag || nseg < 1) return SG_EINVAL;
  if (!accumulate) {
    const int rc = clear_flag(flag, st);
    if (rc != SG_OK) return rc;
  }
  hipLaunchKernelGGL(segment_sumsq_flag_kernel, dim3(nseg), dim3(256), 0, sg_st(st), flat, offsets, out, flag);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_guard_step(const int32_t* flag, int64_t* t, int64_t* counters, double lr, const double* lr_dev, float* lr_t,
                             int32_t adam, double b1, double b2, sg_stream_t st) {
  if (!flag || !t || !counters || !lr_t) return SG_EINVAL;
  hipLaunchKernelGGL(guard_step_kernel, dim3(1), dim3(64), 0, sg_st(st), flag, t, counters, lr, lr_dev, lr_t, adam, b1, b2);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_adam_ema_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, const float* lr_t,
                                   const int32_t* skip, float b1, float b2, float eps, float gscale, float ema_decay,
                                   sg_stream_t st) {
  if (!p || !g || !m || !v || !lr_t || !skip || numel < 1) return SG_EINVAL;
  if (!sg_aligned16(p) || !sg_aligned16(g) || !sg_aligned16(m) || !sg_aligned16(v) || (ema && !sg_aligned16(ema)))
    return SG_EALIGN;
  int64_t blocks = (numel / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(adam_ema_guard_kernel, dim3((unsigned)blocks), dim3(256), 0, sg_st(st), p, g, m, v, ema, numel, lr_t,
                     b1, b2, eps, gscale, ema_decay, skip);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_optim_step_guarded(int kind, float* p, const float* g, float* s1, float* s2, float* ema, int64_t numel,
                                     const float* lr, const int32_t* skip, float h, float eps, int nesterov, float gscale,
                                     float ema_decay, sg_stream_t st) {
  if (!p || !g || !lr || !skip || numel < 1) return SG_EINVAL;
  if (kind != SG_OPT_SGD && kind != SG_OPT_MOMENTUM && kind != SG_OPT_ADADELTA) return SG_EINVAL;
  if ((kind != SG_OPT_SGD && !s1) || (kind == SG_OPT_ADADELTA && !s2)) return SG_EINVAL;
  if (!sg_aligned16(p) || !sg_aligned16(g) || (s1 && !sg_aligned16(s1)) || (s2 && !sg_aligned16(s2)) ||
      (ema && !sg_aligned16(ema)))
    return SG_EALIGN;
  int64_t blocks = (numel / 4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  const dim3 grid((unsigned)blocks), blk(256);
  if (kind == SG_OPT_SGD)
    hipLaunchKernelGGL(optim_step_guard_kernel<SG_OPT_SGD>, grid, blk, 0, sg_st(st), p, g, s1, s2, ema, numel, lr, h, eps,
                       nesterov, gscale, ema_decay, skip);
  else if (kind == SG_OPT_MOMENTUM)
    hipLaunchKernelGGL(optim_step_guard_kernel<SG_OPT_MOMENTUM>, grid, blk, 0, sg_st(st), p, g, s1, s2, ema, numel, lr, h,
                       eps, nesterov, gscale, ema_decay, skip);
  else
    hipLaunchKernelGGL(optim_step_guard_kernel<SG_OPT_ADADELTA>, grid, blk, 0, sg_st(st), p, g, s1, s2, ema, numel, lr, h,
                       eps, nesterov, gscale, ema_decay, skip);
  SG_LAUNCH_CHECK();
  return SG_OK;
}
