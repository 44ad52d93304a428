// Discriminator augmentation (Karras et al. 2020, "Training GANs with limited data"), pixel-blitting transforms only:
// axis flips, 90-degree rotations in the (h, w) plane, integer translations with a constant fill.  All three are index
// gathers: values are COPIED, never recomputed, so a permutation reproduces its input's bits in f32 and bf16, and the
// adjoint is another gather.  (Not in the reference, whose only regulariser is the instance noise.)
//
// Per-sample parameters: int32 params[n][8] = {flip_d, flip_h, flip_w, rot_k, t_d, t_h, t_w, 0}.
//
// sg_augment_draw -- one thread per sample i.  ctr = offset + i (64 bit), key = seed ^ SG_AUG_KEY (the instance noise keeps
// `seed`: its streams are untouched).  Three Philox4x32-10 blocks with counter (lo32(ctr), hi32(ctr), j, 0), j = 0, 1, 2:
//     A = block 0: gate flip_w, gate flip_h, gate flip_d, gate rot90
//     B = block 1: gate translate, value flip_w, value flip_h, value flip_d
//     C = block 2: value rot_k, value t_d, value t_h, value t_w
//   gate(r)       = (uint64)r < (uint64)((double)p * 4294967296.0)          (p <= 0 or NaN: never; p >= 1: always)
//   value(r, cnt) = (int)(((uint64)r * cnt) >> 32)                         uniform in [0, cnt)
//   flip_a = gate ? value(r, 2) : 0;  rot_k = gate ? value(r, 4) : 0;  t_a = gate ? value(r, 2 m_a + 1) - m_a : 0
// Integer arithmetic only after the one float -> double -> uint64 conversion of p.  A transform whose bit is clear in `ops`
// (SG_AUG_*) yields 0.
//
// sg_augment_apply -- forward  y[i] = shift(rot90(flip(x[i], axes), k, plane (h, w)), t, fill), numpy's flip / rot90
// conventions on the sample's [d, h, w, c] array, shift(a, t, fill)[v] = a[v - t] where v - t is in range, else fill;
// adjoint  y[i] = flip(rot90(shift(x[i], -t, 0), -k), axes): the exact transpose of the forward's linear part.
//
// sg_ada_update -- the adaptive probability's controller, one thread.  state = {sum_sign, count, steps, adjustments} (int64):
//     sum_sign += sum_i sign(logits[i])   (+1 for > 0, -1 for < 0, 0 for zeros and NaN);  count += n;  steps += 1
//     if steps % interval == 0:
//         up = sum_sign * target_den > target_num * count                  (int64: r_t = sum_sign / count against the target)
//         p  = min(max(p + (up ? delta : -delta), 0), p_max)               (f32)
//         adjustments += 1;  sum_sign = count = 0
#include "common.h"

namespace {

constexpr uint64_t SG_AUG_KEY = 0x4155474D454E5431ull;      // "AUGMENT1"

__device__ __forceinline__ bool aug_gate(uint32_t r, uint64_t thr) { return (uint64_t)r < thr; }
__device__ __forceinline__ int32_t aug_value(uint32_t r, uint32_t cnt) { return (int32_t)(((uint64_t)r * cnt) >> 32); }

__global__ void augment_draw_kernel(int32_t* __restrict__ params, int32_t n, uint32_t ops, int32_t m_d, int32_t m_h,
                                    int32_t m_w, float p, const float* __restrict__ p_dev, uint64_t seed, uint64_t offset,
                                    const uint64_t* __restrict__ offset_dev) {
  const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  if (p_dev != nullptr) p = *p_dev;
  if (offset_dev != nullptr) offset = *offset_dev;
  const uint64_t thr = p > 0.f ? (p >= 1.f ? 0x100000000ull : (uint64_t)((double)p * 4294967296.0)) : 0ull;
  const uint64_t ctr = offset + (uint64_t)i, key = seed ^ SG_AUG_KEY;
  uint32_t a[4], b[4], c[4];
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)key, (uint32_t)(key >> 32), a);
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 1u, 0u, (uint32_t)key, (uint32_t)(key >> 32), b);
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 2u, 0u, (uint32_t)key, (uint32_t)(key >> 32), c);
  const bool g_fw = (ops & SG_AUG_FLIP_W) && aug_gate(a[0], thr), g_fh = (ops & SG_AUG_FLIP_H) && aug_gate(a[1], thr);
  const bool g_fd = (ops & SG_AUG_FLIP_D) && aug_gate(a[2], thr), g_rot = (ops & SG_AUG_ROT90) && aug_gate(a[3], thr);
  const bool g_tr = (ops & SG_AUG_TRANSLATE) && aug_gate(b[0], thr);
  int32_t* o = params + (int64_t)i * 8;
  o[0] = g_fd ? aug_value(b[3], 2u) : 0;
  o[1] = g_fh ? aug_value(b[2], 2u) : 0;
  o[2] = g_fw ? aug_value(b[1], 2u) : 0;
  o[3] = g_rot ? aug_value(c[0], 4u) : 0;
  o[4] = g_tr ? aug_value(c[1], 2u * (uint32_t)m_d + 1u) - m_d : 0;
  o[5] = g_tr ? aug_value(c[2], 2u * (uint32_t)m_h + 1u) - m_h : 0;
  o[6] = g_tr ? aug_value(c[3], 2u * (uint32_t)m_w + 1u) - m_w : 0;
  o[7] = 0;
}

__global__ void aug_counter_add_kernel(uint64_t* ctr, uint64_t inc) { *ctr += inc; }

// rot90(m, k, axes (h, w))[i, j] = m[a, b] on an e x e plane (numpy: k = 1 turns the first axis towards the second)
__device__ __forceinline__ void rot_source(int k, int64_t e, int64_t i, int64_t j, int64_t& a, int64_t& b) {
  a = k == 0 ? i : (k == 1 ? j : (k == 2 ? e - 1 - i : e - 1 - j));
  b = k == 0 ? j : (k == 1 ? e - 1 - i : (k == 2 ? e - 1 - j : i));
}

// One output piece of 16 bytes (E elements) of a (w, c) row per thread and trip: a row is w*c contiguous elements of one
// (n, d, h).  VEC: w*c is a multiple of E and y is 16-byte aligned, so every piece is whole and aligned -- one vector store.
// Otherwise rows start at any element and the last piece of a row is short: the scalar path stores element by element.
// Sources are read element-wise (any of the three transforms may separate neighbours; the tensor is D's input, cache-resident).
// Parameters come from device memory and are not trusted: rot_k is taken mod 4 and ignored unless `ops` allows it (the host
// has checked h == w in that case), shifts are 64-bit, every source voxel is range-checked.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void augment_apply_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                            const int32_t* __restrict__ params, int64_t total, uint32_t P,
                                                            int small, int32_t d, int32_t h, int32_t w, int32_t c,
                                                            uint32_t ops, float fill, int adjoint) {
  constexpr int E = 16 / (int)sizeof(T);
  const int32_t L = w * c;
  const T fillv = sg_traits<T>::from_f(adjoint ? 0.f : fill);
  const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid0; i < total; i += stride) {
    uint32_t row, piece;
    if (small) {      // fewer than 2^32 pieces: 32-bit division
      row = (uint32_t)i / P;
      piece = (uint32_t)i - row * P;
    } else {
      const uint64_t r = (uint64_t)i / P;
      row = (uint32_t)r;
      piece = (uint32_t)((uint64_t)i - r * P);
    }
    const uint32_t t1 = row / (uint32_t)h;
    const int32_t hh = (int32_t)(row - t1 * (uint32_t)h);
    const uint32_t nn = t1 / (uint32_t)d;
    const int32_t dd = (int32_t)(t1 - nn * (uint32_t)d);
    const int32_t* pr = params + (int64_t)nn * 8;
    const bool fd = (ops & SG_AUG_FLIP_D) && pr[0] != 0, fh = (ops & SG_AUG_FLIP_H) && pr[1] != 0;
    const bool fw = (ops & SG_AUG_FLIP_W) && pr[2] != 0;
    int k = (ops & SG_AUG_ROT90) ? (pr[3] & 3) : 0;
    if (adjoint) k = (4 - k) & 3;
    const bool tr = (ops & SG_AUG_TRANSLATE) != 0;
    const int64_t td = tr ? pr[4] : 0, th = tr ? pr[5] : 0, tw = tr ? pr[6] : 0;
    const T* xs = x + (int64_t)nn * d * h * L;
    const int32_t q0 = (int32_t)piece * E;
    int32_t ww = q0 / c, ch = q0 - ww * c;
    alignas(16) T out[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      T v = fillv;
      if (VEC || q0 + e < L) {
        int64_t sd, sh, sw, a, b;
        bool ok;
        if (!adjoint) {
          const int64_t ud = dd - td, uh = hh - th, uw = ww - tw;
          ok = (uint64_t)ud < (uint64_t)d && (uint64_t)uh < (uint64_t)h && (uint64_t)uw < (uint64_t)w;
          rot_source(k, h, uh, uw, a, b);
          sd = fd ? d - 1 - ud : ud;
          sh = fh ? h - 1 - a : a;
          sw = fw ? w - 1 - b : b;
        } else {
          const int64_t pd = fd ? d - 1 - dd : dd, ph = fh ? h - 1 - hh : hh, pw = fw ? w - 1 - ww : ww;
          rot_source(k, h, ph, pw, a, b);
          sd = pd + td;
          sh = a + th;
          sw = b + tw;
          ok = (uint64_t)sd < (uint64_t)d && (uint64_t)sh < (uint64_t)h && (uint64_t)sw < (uint64_t)w;
        }
        if (ok) v = xs[((sd * h + sh) * w + sw) * c + ch];
      }
      out[e] = v;
      if (++ch == c) {
        ch = 0;
        ++ww;
      }
    }
    T* dst = y + (int64_t)row * L + q0;
    if (VEC) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(out);
      *reinterpret_cast<u32x4*>(dst) = raw;
      SG_STORE16_GUARD(raw);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (q0 + e < L) dst[e] = out[e];
    }
  }
}

__global__ void ada_update_kernel(const float* __restrict__ logits, int32_t n, int64_t* __restrict__ state,
                                  float* __restrict__ p, int32_t interval, int64_t target_num, int64_t target_den,
                                  float delta, float p_max) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  int64_t s = 0;
  for (int32_t i = 0; i < n; ++i) {
    const float v = logits[i];
    s += v > 0.f ? 1 : (v < 0.f ? -1 : 0);
  }
  const int64_t sum_sign = state[0] + s, count = state[1] + n, steps = state[2] + 1;
  state[2] = steps;
  if (steps % interval == 0) {
    const bool up = sum_sign * target_den > target_num * count;
    const float q = *p + (up ? delta : -delta);
    *p = fminf(fmaxf(q, 0.f), p_max);
    state[3] += 1;
    state[0] = 0;
    state[1] = 0;
  } else {
    state[0] = sum_sign;
    state[1] = count;
  }
}

}  // namespace

extern "C" int sg_augment_draw(int32_t* params, int32_t n, uint32_t ops, int32_t m_d, int32_t m_h, int32_t m_w, float p,
                               const float* p_dev, uint64_t seed, uint64_t offset, uint64_t* offset_dev, uint64_t bump,
                               sg_stream_t st) {
  if (!params || n < 1 || (ops & ~(uint32_t)SG_AUG_ALL) || m_d < 0 || m_h < 0 || m_w < 0) return SG_EINVAL;
  if (m_d > (1 << 30) || m_h > (1 << 30) || m_w > (1 << 30)) return SG_EINVAL;      // 2m + 1 fits 32 bits
  hipStream_t hs = sg_st(st);
  hipLaunchKernelGGL(augment_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, hs, params, n, ops, m_d, m_h, m_w, p, p_dev,
                     seed, offset, (const uint64_t*)offset_dev);
  SG_LAUNCH_CHECK();
  if (offset_dev && bump) {      // stream order: every block of the launch above has read the counter before this runs
    hipLaunchKernelGGL(aug_counter_add_kernel, dim3(1), dim3(1), 0, hs, offset_dev, bump);
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}

extern "C" int sg_augment_apply(const void* x, void* y, const int32_t* params, int32_t n, int32_t d, int32_t h, int32_t w,
                                int32_t c, uint32_t ops, float fill, int32_t adjoint, sg_dtype dt, sg_stream_t st) {
  if (!x || !y || !params || x == y || n < 1 || d < 1 || h < 1 || w < 1 || c < 1) return SG_EINVAL;
  if (dt != SG_F32 && dt != SG_BF16) return SG_EINVAL;
  if ((ops & ~(uint32_t)SG_AUG_ALL) || ((ops & SG_AUG_ROT90) && h != w)) return SG_EINVAL;
  const int64_t L = (int64_t)w * c, rows = (int64_t)n * d * h;
  if (L >= (1ll << 31) || rows >= (1ll << 32)) return SG_EINVAL;
  const int E = 16 / (int)sg_esize(dt);
  const int64_t P = (L + E - 1) / E, total = rows * P;
  const bool vec = L % E == 0 && sg_aligned16(y);
  const int small = total < (1ll << 32) ? 1 : 0;
  // two trips per thread at every size of more than one block (the grid-stride loop is never a path of large tensors only)
  int64_t blocks = (total + 255) / 256;
  if (blocks > 1) blocks = (blocks + 1) / 2;
  if (blocks > (1ll << 30)) blocks = 1ll << 30;
  hipStream_t hs = sg_st(st);
#define L_(T, V)                                                                                                          \
  hipLaunchKernelGGL((augment_apply_kernel<T, V>), dim3((unsigned)blocks), dim3(256), 0, hs, (const T*)x, (T*)y, params,  \
                     total, (uint32_t)P, small, d, h, w, c, ops, fill, adjoint ? 1 : 0)
  if (dt == SG_BF16) {
    if (vec) L_(bf16_t, true); else L_(bf16_t, false);
  } else {
    if (vec) L_(float, true); else L_(float, false);
  }
#undef L_
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_ada_update(const float* logits, int32_t n, int64_t* state, float* p, int32_t interval, int64_t target_num,
                             int64_t target_den, float delta, float p_max, sg_stream_t st) {
  if (!logits || !state || !p || n < 1 || interval < 1 || target_den < 1) return SG_EINVAL;
  hipLaunchKernelGGL(ada_update_kernel, dim3(1), dim3(64), 0, sg_st(st), logits, n, state, p, interval, target_num,
                     target_den, delta, p_max);
  SG_LAUNCH_CHECK();
  return SG_OK;
}
