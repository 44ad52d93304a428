// Minibatch standard deviation as a per-sample statistic (networks/ops.py:313-325 without the concatenation):
// the statistic, its gradient and the gradient of that gradient, and the three bilinear kernels of the rank-1 term the
// statistic channel adds to the SAME-padded convolution that follows it.  Every sum below has one fixed order (serial per
// thread, a tree over the block's LDS, serial over the blocks' partial sums): no float atomics, two runs give the same bits.
// All arithmetic is f32; tensors are NDHWC, read and written element by element along the flattened (voxel, channel) axis,
// so any channel count and any base alignment is accepted.
#include "common.h"

namespace {

constexpr int MB_THREADS = 256;
constexpr int MB_MAX_PARTS = 64;      // partial sums per group (blocks of the reducing launches)

static int mb_parts(int64_t per_sample) {
  const int64_t b = (per_sample + MB_THREADS - 1) / MB_THREADS;
  return (int)(b < MB_MAX_PARTS ? b : MB_MAX_PARTS);
}

// Where a group's samples are: the batch is nseg sub-batches of seg_samples = G * M samples; group (seg, m) holds the samples
// seg * seg_samples + g * M + m, g < G (the reference's reshape [G, M, ...] inside each sub-batch).
struct mb_group {
  int64_t first;       // first sample of the group
  int64_t stride;      // samples between two members: M
};

__device__ __forceinline__ mb_group mb_locate(int grp, int G, int M) {
  const int seg = grp / M, m = grp - seg * M;
  return {(int64_t)seg * G * M + m, (int64_t)M};
}

// sum over the group in pairs: (x0 + x1) + (x2 + x3) + ... -- two or four equal values give an exact mean
template <typename T>
__device__ __forceinline__ float mb_mean(const T* __restrict__ p, int64_t step, int G) {
  float s = 0.f;
  int g = 0;
  for (; g + 1 < G; g += 2) s += sg_traits<T>::to_f(p[g * step]) + sg_traits<T>::to_f(p[(g + 1) * step]);
  if (g < G) s += sg_traits<T>::to_f(p[g * step]);
  return s / (float)G;
}

template <typename T>
__device__ __forceinline__ float mb_sigma(const T* __restrict__ p, int64_t step, int G, float mean) {
  float var = 0.f;
  for (int g = 0; g < G; ++g) {
    const float d = sg_traits<T>::to_f(p[g * step]) - mean;
    var += d * d;
  }
  return sqrtf(var / (float)G + 1e-8f);
}

// the block's sum of s in a fixed order, valid in thread 0
__device__ __forceinline__ float mb_block_sum(float s, float* red) {
  red[threadIdx.x] = s;
  __syncthreads();
  for (int k = MB_THREADS / 2; k >= 1; k >>= 1) {
    if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  return red[0];
}

// part[grp][blockIdx.x] = sum over this block's positions of sigma_i
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mbstd_sigma_kernel(const T* __restrict__ x, float* __restrict__ part, int G, int M,
                                                                 int64_t P) {
  __shared__ float red[MB_THREADS];
  const mb_group gr = mb_locate(blockIdx.y, G, M);
  const int64_t step = gr.stride * P;
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * MB_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * MB_THREADS) {
    const T* p = x + gr.first * P + i;
    s += mb_sigma(p, step, G, mb_mean(p, step, G));
  }
  const float t = mb_block_sum(s, red);
  if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
}

// out[sample] = scale * (part[grp][0] + part[grp][1] + ...) for every sample of the group
__global__ __launch_bounds__(64) void mbstd_finish_kernel(const float* __restrict__ part, int nparts, float scale,
                                                          float* __restrict__ out, int G, int M) {
  __shared__ float total;
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int k = 0; k < nparts; ++k) t += part[(int64_t)blockIdx.x * nparts + k];
    total = t * scale;
  }
  __syncthreads();
  const mb_group gr = mb_locate(blockIdx.x, G, M);
  for (int g = threadIdx.x; g < G; g += blockDim.x) out[gr.first + g * gr.stride] = total;
}

__device__ __forceinline__ float mb_group_sum(const float* __restrict__ v, mb_group gr, int G) {
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += v[gr.first + g * gr.stride];
  return s;
}

// dx_gi = S / (P G) * d_gi / sigma_i
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mbstd_bwd_kernel(const float* __restrict__ gstat, const T* __restrict__ x,
                                                               T* __restrict__ dx, int G, int M, int64_t P) {
  const mb_group gr = mb_locate(blockIdx.y, G, M);
  const int64_t step = gr.stride * P;
  const float k = mb_group_sum(gstat, gr, G) / ((float)P * (float)G);
  for (int64_t i = (int64_t)blockIdx.x * MB_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * MB_THREADS) {
    const T* p = x + gr.first * P + i;
    const float mean = mb_mean(p, step, G);
    const float r = k / mb_sigma(p, step, G, mean);
    T* o = dx + gr.first * P + i;
    for (int g = 0; g < G; ++g) o[g * step] = sg_traits<T>::from_f(r * (sg_traits<T>::to_f(p[g * step]) - mean));
  }
}

// gx_gi = S / (P G) * [(h_gi - hbar_i) / sigma_i - d_gi * (sum_g' h_g'i d_g'i) / (G sigma_i^3)]   (gx may be NULL)
// part[grp][blockIdx.x] = sum over this block's positions of (sum_g h_gi d_gi) / sigma_i          (part may be NULL)
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mbstd_bwd2_kernel(const T* __restrict__ h, const T* __restrict__ x,
                                                                const float* __restrict__ gstat, T* __restrict__ gx,
                                                                float* __restrict__ part, int G, int M, int64_t P) {
  __shared__ float red[MB_THREADS];
  const mb_group gr = mb_locate(blockIdx.y, G, M);
  const int64_t step = gr.stride * P;
  const float k = mb_group_sum(gstat, gr, G) / ((float)P * (float)G);
  float s = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * MB_THREADS + threadIdx.x; i < P; i += (int64_t)gridDim.x * MB_THREADS) {
    const T* p = x + gr.first * P + i;
    const T* ph = h + gr.first * P + i;
    const float mean = mb_mean(p, step, G);
    const float rs = 1.f / mb_sigma(p, step, G, mean);
    const float hbar = mb_mean(ph, step, G);
    float q = 0.f;
    for (int g = 0; g < G; ++g) q += sg_traits<T>::to_f(ph[g * step]) * (sg_traits<T>::to_f(p[g * step]) - mean);
    s += q * rs;
    if (gx) {
      T* o = gx + gr.first * P + i;
      if (G == 2) {
        // Two samples: h - hbar and d are both (t, -t), so the bracket's two terms cancel down to
        // (h_g - hbar) * 1e-8 / sigma^2 -- some 1e-5 of either term, below what their f32 difference resolves.  That closed
        // form is evaluated instead (the general one with sum_g' h_g' d_g' = 2 (h_g - hbar) d_g and 2 d_g^2 = 2 (sigma^2 - 1e-8)).
        const float c2 = k * 1e-8f * rs * rs * rs;
        for (int g = 0; g < 2; ++g) o[g * step] = sg_traits<T>::from_f(c2 * (sg_traits<T>::to_f(ph[g * step]) - hbar));
      } else {
        const float c3 = q * rs * rs * rs / (float)G;
        for (int g = 0; g < G; ++g) {
          const float d = sg_traits<T>::to_f(p[g * step]) - mean;
          o[g * step] = sg_traits<T>::from_f(k * ((sg_traits<T>::to_f(ph[g * step]) - hbar) * rs - d * c3));
        }
      }
    }
  }
  if (part) {      // (uniform over the block)
    const float t = mb_block_sum(s, red);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
  }
}

// out[n][j] = y[n][j] + s[n] * B[j], one f32 add, one rounding (y NULL: the outer product alone)
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mbstd_term_kernel(const T* __restrict__ y, const float* __restrict__ s,
                                                                const float* __restrict__ B, T* __restrict__ out, int64_t plane) {
  const int64_t base = (int64_t)blockIdx.y * plane;
  const float sn = s[blockIdx.y];
  for (int64_t j = (int64_t)blockIdx.x * MB_THREADS + threadIdx.x; j < plane; j += (int64_t)gridDim.x * MB_THREADS) {
    const float v = y ? sg_traits<T>::to_f(y[base + j]) : 0.f;
    out[base + j] = sg_traits<T>::from_f(v + sn * B[j]);
  }
}

// r[n] = sum_j g[n][j] * B[j]: one block per sample
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mbstd_dot_kernel(const T* __restrict__ g, const float* __restrict__ B,
                                                               float* __restrict__ r, int64_t plane) {
  __shared__ float red[MB_THREADS];
  const int64_t base = (int64_t)blockIdx.x * plane;
  float s = 0.f;
  for (int64_t j = threadIdx.x; j < plane; j += MB_THREADS) s += sg_traits<T>::to_f(g[base + j]) * B[j];
  const float t = mb_block_sum(s, red);
  if (threadIdx.x == 0) r[blockIdx.x] = t;
}

// Bg[j] = s[0] g[0][j] + s[1] g[1][j] + ... in this order
template <typename T>
__global__ __launch_bounds__(MB_THREADS) void mbstd_outer_kernel(const float* __restrict__ s, const T* __restrict__ g,
                                                                 float* __restrict__ Bg, int n, int64_t plane) {
  for (int64_t j = (int64_t)blockIdx.x * MB_THREADS + threadIdx.x; j < plane; j += (int64_t)gridDim.x * MB_THREADS) {
    float t = 0.f;
    for (int nn = 0; nn < n; ++nn) t += s[nn] * sg_traits<T>::to_f(g[(int64_t)nn * plane + j]);
    Bg[j] = t;
  }
}

#define MB_DISPATCH(dt, BF, FL) \
  do {                          \
    if ((dt) == SG_BF16) {      \
      BF;                       \
    } else {                    \
      FL;                       \
    }                           \
  } while (0)

struct mb_geom {
  int G, M, groups;
  int64_t P;
};

// SG_EINVAL unless the batch splits into nseg sub-batches of whole groups
static int mb_geometry(int32_t n, int64_t vox, int32_t c, int32_t group_size, int32_t nseg, sg_dtype dt, mb_geom* o) {
  if (n < 1 || vox < 1 || c < 1 || group_size < 1 || nseg < 1 || (dt != SG_F32 && dt != SG_BF16)) return SG_EINVAL;
  if (n % nseg != 0) return SG_EINVAL;
  const int sub = n / nseg;
  o->G = group_size < sub ? group_size : sub;
  if (sub % o->G != 0) return SG_EINVAL;      // tf.reshape at networks/ops.py:317 fails likewise
  o->M = sub / o->G;
  o->groups = nseg * o->M;
  o->P = vox * (int64_t)c;
  return SG_OK;
}

static int mb_blocks(int64_t count, int cap) {
  const int64_t b = (count + MB_THREADS - 1) / MB_THREADS;
  return (int)(b < cap ? b : cap);
}

}  // namespace

extern "C" size_t sg_mbstd_stat_workspace(int32_t n, int64_t vox_per_sample, int32_t c, int32_t group_size, int32_t nseg) {
  mb_geom ge;
  if (mb_geometry(n, vox_per_sample, c, group_size, nseg, SG_F32, &ge) != SG_OK) return 0;
  return (size_t)ge.groups * mb_parts(ge.P) * sizeof(float);
}

extern "C" int sg_mbstd_stat_fwd(const void* x, float* stat, float* workspace, size_t workspace_bytes, int32_t n,
                                 int64_t vox_per_sample, int32_t c, int32_t group_size, int32_t nseg, sg_dtype dt,
                                 sg_stream_t st) {
  mb_geom ge;
  if (!x || !stat || !workspace) return SG_EINVAL;
  const int rc = mb_geometry(n, vox_per_sample, c, group_size, nseg, dt, &ge);
  if (rc != SG_OK) return rc;
  const int parts = mb_parts(ge.P);
  if (workspace_bytes < (size_t)ge.groups * parts * sizeof(float)) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
#define L(T) hipLaunchKernelGGL((mbstd_sigma_kernel<T>), dim3(parts, ge.groups), dim3(MB_THREADS), 0, hs, (const T*)x, workspace, ge.G, ge.M, ge.P)
  MB_DISPATCH(dt, L(bf16_t), L(float));
#undef L
  SG_LAUNCH_CHECK();
  hipLaunchKernelGGL(mbstd_finish_kernel, dim3(ge.groups), dim3(64), 0, hs, workspace, parts, 1.f / (float)ge.P, stat, ge.G, ge.M);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_mbstd_stat_bwd(const float* gstat, const void* x, void* dx, int32_t n, int64_t vox_per_sample, int32_t c,
                                 int32_t group_size, int32_t nseg, sg_dtype dt, sg_stream_t st) {
  mb_geom ge;
  if (!gstat || !x || !dx) return SG_EINVAL;
  const int rc = mb_geometry(n, vox_per_sample, c, group_size, nseg, dt, &ge);
  if (rc != SG_OK) return rc;
  hipStream_t hs = sg_st(st);
  const int bx = mb_blocks(ge.P, 1024);
#define L(T) hipLaunchKernelGGL((mbstd_bwd_kernel<T>), dim3(bx, ge.groups), dim3(MB_THREADS), 0, hs, gstat, (const T*)x, (T*)dx, ge.G, ge.M, ge.P)
  MB_DISPATCH(dt, L(bf16_t), L(float));
#undef L
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_mbstd_stat_bwd2(const void* h, const void* x, const float* gstat, void* gx, float* ggstat, float* workspace,
                                  size_t workspace_bytes, int32_t n, int64_t vox_per_sample, int32_t c, int32_t group_size,
                                  int32_t nseg, sg_dtype dt, sg_stream_t st) {
  mb_geom ge;
  if (!h || !x || !gstat || (!gx && !ggstat) || (ggstat && !workspace)) return SG_EINVAL;
  const int rc = mb_geometry(n, vox_per_sample, c, group_size, nseg, dt, &ge);
  if (rc != SG_OK) return rc;
  const int parts = mb_parts(ge.P);
  if (ggstat && workspace_bytes < (size_t)ge.groups * parts * sizeof(float)) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
  float* part = ggstat ? workspace : nullptr;
#define L(T) hipLaunchKernelGGL((mbstd_bwd2_kernel<T>), dim3(parts, ge.groups), dim3(MB_THREADS), 0, hs, (const T*)h, (const T*)x, gstat, (T*)gx, part, ge.G, ge.M, ge.P)
  MB_DISPATCH(dt, L(bf16_t), L(float));
#undef L
  SG_LAUNCH_CHECK();
  if (ggstat) {
    hipLaunchKernelGGL(mbstd_finish_kernel, dim3(ge.groups), dim3(64), 0, hs, workspace, parts, 1.f / ((float)ge.P * (float)ge.G),
                       ggstat, ge.G, ge.M);
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}

extern "C" int sg_mbstd_term_fwd(const void* y, const float* s, const float* B, void* out, int32_t n, int64_t plane,
                                 sg_dtype dt, sg_stream_t st) {
  if (!s || !B || !out || n < 1 || plane < 1 || (dt != SG_F32 && dt != SG_BF16)) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
  const int bx = mb_blocks(plane, 1024);
#define L(T) hipLaunchKernelGGL((mbstd_term_kernel<T>), dim3(bx, n), dim3(MB_THREADS), 0, hs, (const T*)y, s, B, (T*)out, plane)
  MB_DISPATCH(dt, L(bf16_t), L(float));
#undef L
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_mbstd_term_dot(const void* g, const float* B, float* r, int32_t n, int64_t plane, sg_dtype dt,
                                 sg_stream_t st) {
  if (!g || !B || !r || n < 1 || plane < 1 || (dt != SG_F32 && dt != SG_BF16)) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
#define L(T) hipLaunchKernelGGL((mbstd_dot_kernel<T>), dim3(n), dim3(MB_THREADS), 0, hs, (const T*)g, B, r, plane)
  MB_DISPATCH(dt, L(bf16_t), L(float));
#undef L
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_mbstd_term_outer(const float* s, const void* g, float* Bg, int32_t n, int64_t plane, sg_dtype dt,
                                   sg_stream_t st) {
  if (!s || !g || !Bg || n < 1 || plane < 1 || (dt != SG_F32 && dt != SG_BF16)) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
  const int bx = mb_blocks(plane, 1024);
#define L(T) hipLaunchKernelGGL((mbstd_outer_kernel<T>), dim3(bx), dim3(MB_THREADS), 0, hs, s, (const T*)g, Bg, n, plane)
  MB_DISPATCH(dt, L(bf16_t), L(float));
#undef L
  SG_LAUNCH_CHECK();
  return SG_OK;
}
