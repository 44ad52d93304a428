// Layer-wise adaptive optimisers over the segments of a flat f32 parameter buffer, fused with the EMA update: LAMB and AdamW
// (weight-decayed Adam without bias correction) as SURFGAN_2D/optim.py:60-80 instantiates them (rules: optim.py:246-267,
// optim.py:354-398).  Per variable w with gradient g (already multiplied by gscale), moments m, v, t applied updates:
//   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g^2
//   AdamW  u = m / (sqrt(v) + eps) + lam*w;                          w -= lr*u
//   LAMB   u = (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) + lam*w;      r = |w| / |u| if both > 0 else 1;   w -= lr*r*u
// lam is the decay rate of segments whose decay flag is set and 0 elsewhere (names containing `bias`).
//
// A train op's variables are segments [start, start + count) of one flat buffer with alignment padding between them.  One
// device table per train op (built once by the host) describes them; every launch below covers the whole train op whatever
// the number of variables: block b works on chunk blocks[b].y (SG_SEG_CHUNK elements) of segment blocks[b].x.  Padding is
// neither read nor written.
//   sg_adamw_ema     one launch.
//   sg_lamb_moments  pass 1: reads w, g, m, v; writes m, v; leaves the block's sums of w^2 and u^2 in partials[2b], [2b+1].
//   sg_lamb_ratios   nseg blocks of one wave: sums a segment's partials in double, in an order fixed by the table (lane
//                    l takes partials l, l + 64, ...; the lanes are combined by a tree), and writes r; unguarded, it also
//                    advances the device step count.
//   sg_lamb_update   pass 2: recomputes u from the stored m, v and the old w, w -= lr*r*u, EMA.  (Two kernels: the compiler
//                    may contract lamb_u's multiply-adds differently, so the u applied can differ in the last bit from the
//                    u whose norm pass 1 took -- far below the norm's own rounding, and the same bits on every run.)
// No atomics: two runs from the same state give the same bits.  1 - b^t comes from the device step count in double (one
// thread per block), as guard_step_kernel computes Adam's step size.  Guarded (skip flag set): pass 1 and the ratio launch
// do nothing, pass 2 is the EMA-only update.
#include "common.h"

namespace {

constexpr int CHUNK = SG_SEG_CHUNK;      // elements per block: 256 threads x 4 x f32x4
constexpr int SEG_FIELDS = 4;            // segs[s] = {start, count, decay flag, first block}

struct seg_view {
  int64_t base;      // first element of this block's chunk in the flat buffers
  int n;             // elements of the chunk (CHUNK, or the segment's ragged end); 0: nothing to do
  int seg;
  bool decay;
};

// The table is trusted to describe [0, total): a chunk that would reach outside it is dropped as a whole.
__device__ __forceinline__ seg_view block_view(const int64_t* __restrict__ segs, const int32_t* __restrict__ blocks,
                                               int64_t total) {
  seg_view s;
  s.seg = blocks[2 * blockIdx.x];
  const int64_t chunk = blocks[2 * blockIdx.x + 1];
  const int64_t start = segs[SEG_FIELDS * s.seg], count = segs[SEG_FIELDS * s.seg + 1];
  s.decay = segs[SEG_FIELDS * s.seg + 2] != 0;
  s.base = start + chunk * CHUNK;
  const int64_t left = count - chunk * CHUNK;
  s.n = (int)(left < CHUNK ? left : CHUNK);
  if (start < 0 || (start & 3) || left <= 0 || start + count > total) s.n = 0;
  return s;
}

// 1/(1-b1^t), 1/(1-b2^t) rounded to float once, by one thread; every thread of the block gets the same two floats.
__device__ __forceinline__ void bias_corrections(const int64_t* __restrict__ t, int advance, double b1, double b2, float& c1,
                                                 float& c2) {
  __shared__ float bc[2];
  if (threadIdx.x == 0) {
    const double s = (double)(*t + advance);
    bc[0] = (float)(1.0 / (1.0 - pow(b1, s)));
    bc[1] = (float)(1.0 / (1.0 - pow(b2, s)));
  }
  __syncthreads();
  c1 = bc[0];
  c2 = bc[1];
}

__device__ __forceinline__ float lamb_u(float m, float v, float w, float c1, float c2, float eps, float lam) {
  return (m * c1) / (sqrtf(v * c2) + eps) + lam * w;
}

__device__ __forceinline__ float adamw_u(float m, float v, float w, float eps, float lam) {
  return m / (sqrtf(v) + eps) + lam * w;
}

// Sum over the block in a fixed order (a tree over the 256 threads); the result is valid in thread 0.
__device__ __forceinline__ float block_sum(float x, float* red) {
  red[threadIdx.x] = x;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  return red[0];
}

__device__ __forceinline__ void ema_only_chunk(const float* __restrict__ p, float* __restrict__ ema, int n, float omd) {
  const int nv = n / 4;
  for (int i = threadIdx.x; i < nv; i += 256) {
    const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
    f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
    ee -= omd * (ee - pp);
    reinterpret_cast<f32x4*>(ema)[i] = ee;
    SG_STORE16_GUARD(ee);
  }
  for (int i = nv * 4 + threadIdx.x; i < n; i += 256) ema[i] -= omd * (ema[i] - p[i]);
}

__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, int64_t total,
                                                        const int64_t* __restrict__ segs, const int32_t* __restrict__ blocks,
                                                        float lr, const float* __restrict__ lr_dev, float b1, float b2,
                                                        float eps, float decay, float gscale, float ema_decay,
                                                        const int32_t* __restrict__ skip) {
  const seg_view s = block_view(segs, blocks, total);
  if (s.n == 0) return;
  const float omd = 1.f - ema_decay;
  p += s.base;
  if (ema) ema += s.base;
  if (skip && *skip) {
    if (ema) ema_only_chunk(p, ema, s.n, omd);
    return;
  }
  g += s.base; m += s.base; v += s.base;
  if (lr_dev) lr = *lr_dev;
  const float lam = s.decay ? decay : 0.f;
  const int nv = s.n / 4;
  for (int i = threadIdx.x; i < nv; i += 256) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * gscale;
    f32x4 mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
    mm = b1 * mm + (1.f - b1) * gg;
    vv = b2 * vv + (1.f - b2) * gg * gg;
#pragma unroll
    for (int e = 0; e < 4; ++e) pp[e] -= lr * adamw_u(mm[e], vv[e], pp[e], eps, lam);
    reinterpret_cast<f32x4*>(m)[i] = mm;
    SG_STORE16_GUARD(mm);
    reinterpret_cast<f32x4*>(v)[i] = vv;
    SG_STORE16_GUARD(vv);
    reinterpret_cast<f32x4*>(p)[i] = pp;
    SG_STORE16_GUARD(pp);
    if (ema) {
      f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
      ee -= omd * (ee - pp);
      reinterpret_cast<f32x4*>(ema)[i] = ee;
      SG_STORE16_GUARD(ee);
    }
  }
  for (int i = nv * 4 + threadIdx.x; i < s.n; i += 256) {
    const float gg = g[i] * gscale;
    const float mm = b1 * m[i] + (1.f - b1) * gg;
    const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
    const float pp = p[i] - lr * adamw_u(mm, vv, p[i], eps, lam);
    m[i] = mm; v[i] = vv; p[i] = pp;
    if (ema) ema[i] -= omd * (ema[i] - pp);
  }
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, int64_t total,
                                                           const int64_t* __restrict__ segs,
                                                           const int32_t* __restrict__ blocks, float* __restrict__ partials,
                                                           const int64_t* __restrict__ t, int advance, double b1d, double b2d,
                                                           float b1, float b2, float eps, float decay, float gscale,
                                                           const int32_t* __restrict__ skip) {
  __shared__ float red[256];
  if (skip && *skip) return;
  const seg_view s = block_view(segs, blocks, total);
  float c1, c2;
  bias_corrections(t, advance, b1d, b2d, c1, c2);
  float sw = 0.f, su = 0.f;
  if (s.n > 0) {
    p += s.base; g += s.base; m += s.base; v += s.base;
    const float lam = s.decay ? decay : 0.f;
    const int nv = s.n / 4;
    for (int i = threadIdx.x; i < nv; i += 256) {
      const f32x4 pp = reinterpret_cast<const f32x4*>(p)[i];
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i] * gscale;
      f32x4 mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i];
      mm = b1 * mm + (1.f - b1) * gg;
      vv = b2 * vv + (1.f - b2) * gg * gg;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float u = lamb_u(mm[e], vv[e], pp[e], c1, c2, eps, lam);
        sw += pp[e] * pp[e];
        su += u * u;
      }
      reinterpret_cast<f32x4*>(m)[i] = mm;
      SG_STORE16_GUARD(mm);
      reinterpret_cast<f32x4*>(v)[i] = vv;
      SG_STORE16_GUARD(vv);
    }
    for (int i = nv * 4 + threadIdx.x; i < s.n; i += 256) {
      const float gg = g[i] * gscale;
      const float mm = b1 * m[i] + (1.f - b1) * gg;
      const float vv = b2 * v[i] + (1.f - b2) * gg * gg;
      const float u = lamb_u(mm, vv, p[i], c1, c2, eps, lam);
      sw += p[i] * p[i];
      su += u * u;
      m[i] = mm; v[i] = vv;
    }
  }
  sw = block_sum(sw, red);
  __syncthreads();
  su = block_sum(su, red);
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = sw;
    partials[2 * (int64_t)blockIdx.x + 1] = su;
  }
}

// One wave per segment.  The segment's blocks are first .. first + ceil(count / CHUNK) - 1.
__global__ __launch_bounds__(64) void lamb_ratios_kernel(const int64_t* __restrict__ segs, int32_t nblocks,
                                                         const float* __restrict__ partials, float* __restrict__ ratios,
                                                         int64_t* __restrict__ t, int advance,
                                                         const int32_t* __restrict__ skip) {
  __shared__ double red[2][64];
  if (skip && *skip) return;
  const int seg = blockIdx.x;
  const int64_t count = segs[SEG_FIELDS * seg + 1], first = segs[SEG_FIELDS * seg + 3];
  int64_t nb = (count + CHUNK - 1) / CHUNK;
  if (first < 0 || first + nb > nblocks) nb = 0;      // (a table that does not fit its workspace: the ratio stays 1)
  double sw = 0.0, su = 0.0;
  for (int64_t i = threadIdx.x; i < nb; i += 64) {
    sw += (double)partials[2 * (first + i)];
    su += (double)partials[2 * (first + i) + 1];
  }
  red[0][threadIdx.x] = sw;
  red[1][threadIdx.x] = su;
  __syncthreads();
  for (int k = 32; k >= 1; k >>= 1) {
    if (threadIdx.x < k) {
      red[0][threadIdx.x] += red[0][threadIdx.x + k];
      red[1][threadIdx.x] += red[1][threadIdx.x + k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double w2 = red[0][0], u2 = red[1][0];
    ratios[seg] = (w2 > 0.0 && u2 > 0.0) ? (float)(sqrt(w2) / sqrt(u2)) : 1.f;
    if (seg == 0 && advance) *t += advance;      // (pass 1 is complete; pass 2 reads the advanced count)
  }
}

__global__ __launch_bounds__(256) void lamb_update_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                          const float* __restrict__ v, float* __restrict__ ema, int64_t total,
                                                          const int64_t* __restrict__ segs,
                                                          const int32_t* __restrict__ blocks, const float* __restrict__ ratios,
                                                          const int64_t* __restrict__ t, float lr,
                                                          const float* __restrict__ lr_dev, double b1d, double b2d, float eps,
                                                          float decay, float ema_decay, const int32_t* __restrict__ skip) {
  const seg_view s = block_view(segs, blocks, total);
  const float omd = 1.f - ema_decay;
  if (skip && *skip) {
    if (ema && s.n > 0) ema_only_chunk(p + s.base, ema + s.base, s.n, omd);
    return;
  }
  float c1, c2;
  bias_corrections(t, 0, b1d, b2d, c1, c2);
  if (s.n == 0) return;
  p += s.base; m += s.base; v += s.base;
  if (ema) ema += s.base;
  if (lr_dev) lr = *lr_dev;
  const float step = lr * ratios[s.seg];
  const float lam = s.decay ? decay : 0.f;
  const int nv = s.n / 4;
  for (int i = threadIdx.x; i < nv; i += 256) {
    f32x4 pp = reinterpret_cast<f32x4*>(p)[i];
    const f32x4 mm = reinterpret_cast<const f32x4*>(m)[i], vv = reinterpret_cast<const f32x4*>(v)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) pp[e] -= step * lamb_u(mm[e], vv[e], pp[e], c1, c2, eps, lam);
    reinterpret_cast<f32x4*>(p)[i] = pp;
    SG_STORE16_GUARD(pp);
    if (ema) {
      f32x4 ee = reinterpret_cast<f32x4*>(ema)[i];
      ee -= omd * (ee - pp);
      reinterpret_cast<f32x4*>(ema)[i] = ee;
      SG_STORE16_GUARD(ee);
    }
  }
  for (int i = nv * 4 + threadIdx.x; i < s.n; i += 256) {
    const float pp = p[i] - step * lamb_u(m[i], v[i], p[i], c1, c2, eps, lam);
    p[i] = pp;
    if (ema) ema[i] -= omd * (ema[i] - pp);
  }
}

bool bad_table(const int64_t* segs, const int32_t* blocks, int32_t nseg, int32_t nblocks, int64_t total) {
  return !segs || !blocks || nseg < 1 || nblocks < nseg || total < 1;
}

}  // namespace

extern "C" int sg_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t total, const int64_t* segs,
                            const int32_t* blocks, int32_t nseg, int32_t nblocks, float lr, const float* lr_dev,
                            const int32_t* skip, float b1, float b2, float eps, float decay, float gscale, float ema_decay,
                            sg_stream_t st) {
  if (!p || !g || !m || !v || bad_table(segs, blocks, nseg, nblocks, total) || (skip && !lr_dev)) return SG_EINVAL;
  if (!sg_aligned16(p) || !sg_aligned16(g) || !sg_aligned16(m) || !sg_aligned16(v) || (ema && !sg_aligned16(ema)))
    return SG_EALIGN;
  hipLaunchKernelGGL(adamw_ema_kernel, dim3((unsigned)nblocks), dim3(256), 0, sg_st(st), p, g, m, v, ema, total, segs, blocks,
                     lr, lr_dev, b1, b2, eps, decay, gscale, ema_decay, skip);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t total, const int64_t* segs,
                               const int32_t* blocks, int32_t nseg, int32_t nblocks, float* partials, const int64_t* t,
                               int32_t advance, const int32_t* skip, double b1, double b2, float eps, float decay,
                               float gscale, sg_stream_t st) {
  if (!p || !g || !m || !v || !partials || !t || bad_table(segs, blocks, nseg, nblocks, total)) return SG_EINVAL;
  if (advance != 0 && advance != 1) return SG_EINVAL;
  if (!sg_aligned16(p) || !sg_aligned16(g) || !sg_aligned16(m) || !sg_aligned16(v)) return SG_EALIGN;
  hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)nblocks), dim3(256), 0, sg_st(st), p, g, m, v, total, segs, blocks,
                     partials, t, (int)advance, b1, b2, (float)b1, (float)b2, eps, decay, gscale, skip);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_lamb_ratios(const int64_t* segs, int32_t nseg, int32_t nblocks, const float* partials, float* ratios,
                              int64_t* t, int32_t advance, const int32_t* skip, sg_stream_t st) {
  if (!segs || !partials || !ratios || !t || nseg < 1 || nblocks < nseg) return SG_EINVAL;
  if (advance != 0 && advance != 1) return SG_EINVAL;
  hipLaunchKernelGGL(lamb_ratios_kernel, dim3((unsigned)nseg), dim3(64), 0, sg_st(st), segs, nblocks, partials, ratios, t,
                     (int)advance, skip);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_lamb_update(float* p, const float* m, const float* v, float* ema, int64_t total, const int64_t* segs,
                              const int32_t* blocks, int32_t nseg, int32_t nblocks, const float* ratios, const int64_t* t,
                              float lr, const float* lr_dev, const int32_t* skip, double b1, double b2, float eps, float decay,
                              float ema_decay, sg_stream_t st) {
  if (!p || !m || !v || !ratios || !t || bad_table(segs, blocks, nseg, nblocks, total) || (skip && !lr_dev)) return SG_EINVAL;
  if (!sg_aligned16(p) || !sg_aligned16(m) || !sg_aligned16(v) || (ema && !sg_aligned16(ema))) return SG_EALIGN;
  hipLaunchKernelGGL(lamb_update_kernel, dim3((unsigned)nblocks), dim3(256), 0, sg_st(st), p, m, v, ema, total, segs, blocks,
                     ratios, t, lr, lr_dev, b1, b2, eps, decay, ema_decay, skip);
  SG_LAUNCH_CHECK();
  return SG_OK;
}
