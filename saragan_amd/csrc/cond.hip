// Label conditioning of the 3-D pgan: the generator's label embedding concatenated to the latents and the
// discriminator's label-weighted sum of its outputs, each with its adjoint.  N x latent_dim elements at most: one launch per
// call, one thread per output element, every sum serial in one thread in ascending index order (no atomics: two runs give
// the same bits).  Labels c [n, l] and the embedding W [l, zdim] are f32; z, out / o, out are f32 or bf16, sums in f32.
#include "common.h"

namespace {

constexpr int CD_THREADS = 256;

// out[n, :Z] = z[n], out[n, Z + j] = sum_l c[n, l] * W[l, j]
template <typename T>
__global__ __launch_bounds__(CD_THREADS) void cond_embed_fwd_kernel(const T* __restrict__ z, const float* __restrict__ c,
                                                                    const float* __restrict__ W, T* __restrict__ out, int n, int Z,
                                                                    int L) {
  const int64_t total = (int64_t)n * 2 * Z;
  const int64_t i = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
  if (i >= total) return;
  const int row = (int)(i / (2 * Z)), col = (int)(i - (int64_t)row * 2 * Z);
  if (col < Z) {
    out[i] = z[(int64_t)row * Z + col];
    return;
  }
  const int j = col - Z;
  float s = 0.f;
  for (int l = 0; l < L; ++l) s += c[(int64_t)row * L + l] * W[(int64_t)l * Z + j];
  out[i] = sg_traits<T>::from_f(s);
}

// dW[l, j] = sum_n c[n, l] * g[n, Z + j] (n ascending; dW may be NULL), dz[n, j] = g[n, j] (dz may be NULL)
template <typename T>
__global__ __launch_bounds__(CD_THREADS) void cond_embed_adj_kernel(T* __restrict__ dz, const float* __restrict__ c,
                                                                    float* __restrict__ dW, const T* __restrict__ g, int n, int Z,
                                                                    int L) {
  const int64_t nw = dW ? (int64_t)L * Z : 0;
  const int64_t total = nw + (dz ? (int64_t)n * Z : 0);
  const int64_t i = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
  if (i >= total) return;
  if (i < nw) {
    const int l = (int)(i / Z), j = (int)(i - (int64_t)l * Z);
    float s = 0.f;
    for (int r = 0; r < n; ++r) s += c[(int64_t)r * L + l] * sg_traits<T>::to_f(g[(int64_t)r * 2 * Z + Z + j]);
    dW[i] = s;
    return;
  }
  const int64_t k = i - nw;
  const int row = (int)(k / Z), j = (int)(k - (int64_t)row * Z);
  dz[k] = g[(int64_t)row * 2 * Z + j];
}

// out[n] = sum_l o[n, l] * c[n, l]
template <typename T>
__global__ __launch_bounds__(CD_THREADS) void cond_project_fwd_kernel(const T* __restrict__ o, const float* __restrict__ c,
                                                                      T* __restrict__ out, int n, int L) {
  const int row = blockIdx.x * CD_THREADS + threadIdx.x;
  if (row >= n) return;
  float s = 0.f;
  for (int l = 0; l < L; ++l) s += sg_traits<T>::to_f(o[(int64_t)row * L + l]) * c[(int64_t)row * L + l];
  out[row] = sg_traits<T>::from_f(s);
}

// go[n, l] = g[n] * c[n, l]
template <typename T>
__global__ __launch_bounds__(CD_THREADS) void cond_project_adj_kernel(const T* __restrict__ g, const float* __restrict__ c,
                                                                      T* __restrict__ go, int n, int L) {
  const int64_t i = (int64_t)blockIdx.x * CD_THREADS + threadIdx.x;
  if (i >= (int64_t)n * L) return;
  go[i] = sg_traits<T>::from_f(sg_traits<T>::to_f(g[i / L]) * c[i]);
}

static inline unsigned cd_blocks(int64_t count) { return (unsigned)((count + CD_THREADS - 1) / CD_THREADS); }

}  // namespace

extern "C" int sg_cond_embed(void* z, const float* c, float* W, void* out, int32_t n, int32_t zdim, int32_t l, int32_t adjoint,
                             sg_dtype dt, sg_stream_t st) {
  if (!c || !out || n < 1 || zdim < 1 || l < 1 || (dt != SG_F32 && dt != SG_BF16)) return SG_EINVAL;
  if ((int64_t)n * 2 * zdim + (int64_t)l * zdim > (int64_t)1 << 30) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
  if (!adjoint) {
    if (!z || !W) return SG_EINVAL;
    const unsigned bx = cd_blocks((int64_t)n * 2 * zdim);
    if (dt == SG_BF16)
      hipLaunchKernelGGL((cond_embed_fwd_kernel<bf16_t>), dim3(bx), dim3(CD_THREADS), 0, hs, (const bf16_t*)z, c, (const float*)W,
                         (bf16_t*)out, n, zdim, l);
    else
      hipLaunchKernelGGL((cond_embed_fwd_kernel<float>), dim3(bx), dim3(CD_THREADS), 0, hs, (const float*)z, c, (const float*)W,
                         (float*)out, n, zdim, l);
  } else {
    if (!z && !W) return SG_EINVAL;
    const unsigned bx = cd_blocks((W ? (int64_t)l * zdim : 0) + (z ? (int64_t)n * zdim : 0));
    if (dt == SG_BF16)
      hipLaunchKernelGGL((cond_embed_adj_kernel<bf16_t>), dim3(bx), dim3(CD_THREADS), 0, hs, (bf16_t*)z, c, W, (const bf16_t*)out, n,
                         zdim, l);
    else
      hipLaunchKernelGGL((cond_embed_adj_kernel<float>), dim3(bx), dim3(CD_THREADS), 0, hs, (float*)z, c, W, (const float*)out, n,
                         zdim, l);
  }
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_cond_project(const void* o, const float* c, void* out, int32_t n, int32_t l, int32_t adjoint, sg_dtype dt,
                               sg_stream_t st) {
  if (!o || !c || !out || n < 1 || l < 1 || (dt != SG_F32 && dt != SG_BF16)) return SG_EINVAL;
  if ((int64_t)n * l > (int64_t)1 << 30) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
  if (!adjoint) {
    const unsigned bx = cd_blocks(n);
    if (dt == SG_BF16)
      hipLaunchKernelGGL((cond_project_fwd_kernel<bf16_t>), dim3(bx), dim3(CD_THREADS), 0, hs, (const bf16_t*)o, c, (bf16_t*)out, n, l);
    else
      hipLaunchKernelGGL((cond_project_fwd_kernel<float>), dim3(bx), dim3(CD_THREADS), 0, hs, (const float*)o, c, (float*)out, n, l);
  } else {
    const unsigned bx = cd_blocks((int64_t)n * l);
    if (dt == SG_BF16)
      hipLaunchKernelGGL((cond_project_adj_kernel<bf16_t>), dim3(bx), dim3(CD_THREADS), 0, hs, (const bf16_t*)o, c, (bf16_t*)out, n, l);
    else
      hipLaunchKernelGGL((cond_project_adj_kernel<float>), dim3(bx), dim3(CD_THREADS), 0, hs, (const float*)o, c, (float*)out, n, l);
  }
  SG_LAUNCH_CHECK();
  return SG_OK;
}
