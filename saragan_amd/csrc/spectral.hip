// Spectral normalisation of the weights of one network (SURFGAN_3D/networks/ops.py:80-127: spectral_norm) over the segments of
// its flat f32 parameter buffer, batched: every launch covers all normalised layers.  For a weight W = reshape(w, [R, C]),
// C = cout, with persistent state u [C], one refresh with `iteration` = k is, k times,
//   v_ = u W^T;  v = v_ / sqrt(max(sum v_^2, 1e-12));   u_ = v W;  u = u_ / sqrt(max(sum u_^2, 1e-12))
// then sigma = v W u^T and Wbar = W / sigma.  With t = W u^T, s = W^T t, T = sum t^2, S = sum s^2, nt = sqrt(max(T, 1e-12)):
//   v = t / nt;  u_ = s / nt;  U2 = sum u_^2 = S / nt^2;  nu = sqrt(max(U2, 1e-12));  u = s / (nt nu);  sigma = U2 / nu
// (sigma = sqrt(S / T) when no clamp engages), so W is read from memory once per iteration for both products.
//
// One device table per network (built once by the host, functional.SpectralTable):
//   segs   int64[nseg][8]    {start (a multiple of 4), R, C, first block, rows per block, u offset, v offset, column offset}
//   blocks int32[nblocks][2] {segment, row block}: block b covers rows [rb*rpb, min(R, (rb+1)*rpb)) of its segment, whole rows
//          only; a segment's ceil(R / rpb) blocks are consecutive, starting at its `first block`.
// Padding between the segments is neither read nor written.
//   spectral_products    grid nblocks: t for the block's rows (left unnormalised in v), the block's sum of t^2 in partials[b]
//                        and its partial column sums of W^T t in cols[column offset + rb*C + c]
//   spectral_normalise   grid nseg: sums the segment's partials and column partials in an order fixed by the table (in
//                        double), writes u, sigma and nt
//   spectral_scale       grid nblocks: Wbar = W / sigma into the effective-weight buffer (same offsets), v = t / nt
//   spectral_dot         grid nblocks: the block's part of <g, Wbar> in partials[b]
//   spectral_pullback    grid nblocks: every block sums its segment's partials itself (same order, same bits), then
//                        g = (g - <g, Wbar> v_r u_c) / sigma on its rows
// A refresh is 2k + 1 launches, a pull-back two, whatever the number of layers.  No atomics: equal inputs give equal bits.
#include "common.h"

namespace {

constexpr int SEG_FIELDS = SG_SPECTRAL_SEG_FIELDS;
constexpr int MAX_RPB = SG_SEG_CHUNK;      // rows per block the LDS copy of t is sized for
constexpr double CLAMP = 1e-12;

struct sn_view {
  int64_t base;      // first element of the block's rows in the flat buffers
  int64_t uoff, voff, coloff;
  int rows;          // 0: nothing to do
  int r0, C, seg, nb;
};

struct sn_limits {
  int64_t total, ulen, vlen, collen;
  int32_t nblocks, nseg;
};

// The table is trusted to describe its buffers: a segment that would reach outside one of them is dropped as a whole.
__device__ __forceinline__ sn_view segment_view(const int64_t* __restrict__ segs, int seg, int rb, sn_limits lim) {
  sn_view s;
  s.seg = seg;
  s.uoff = s.voff = s.coloff = 0;
  s.rows = 0; s.r0 = 0; s.C = 0; s.nb = 0; s.base = 0;
  if (seg < 0 || seg >= lim.nseg) return s;      // (a block entry that names no segment)
  const int64_t* e = segs + (int64_t)SEG_FIELDS * seg;
  const int64_t start = e[0], R = e[1], C = e[2], first = e[3], rpb = e[4];
  s.uoff = e[5]; s.voff = e[6]; s.coloff = e[7];
  s.C = (int)C;
  if (start < 0 || (start & 3) || R < 1 || C < 1 || C > 0x7fffffff || R > 0x7fffffff || rpb < 1 || rpb > MAX_RPB) return s;
  const int64_t nb = (R + rpb - 1) / rpb;
  if (start + R * C > lim.total || first < 0 || first + nb > lim.nblocks) return s;
  if (s.uoff < 0 || s.uoff + C > lim.ulen || s.voff < 0 || s.voff + R > lim.vlen) return s;
  if (s.coloff < 0 || s.coloff + nb * C > lim.collen) return s;
  s.nb = (int)nb;
  if (rb < 0 || rb >= nb) return s;
  s.r0 = (int)(rb * rpb);
  const int64_t left = R - s.r0;
  s.rows = (int)(left < rpb ? left : rpb);
  s.base = start + (int64_t)s.r0 * C;
  s.coloff += (int64_t)rb * C;
  return s;
}

__device__ __forceinline__ sn_view block_view(const int64_t* __restrict__ segs, const int32_t* __restrict__ blocks,
                                              sn_limits lim) {
  return segment_view(segs, blocks[2 * blockIdx.x], blocks[2 * blockIdx.x + 1], lim);
}

// Lanes of a wave that share one row: the smallest power of two >= min(C, 64).
__device__ __forceinline__ int lanes_per_row(int C) {
  int L = 1;
  while (L < C && L < 64) L <<= 1;
  return L;
}

template <typename T>
__device__ __forceinline__ T block_sum(T x, T* red) {      // a tree over the 256 threads; valid in every thread
  red[threadIdx.x] = x;
  __syncthreads();
  for (int k = 128; k >= 1; k >>= 1) {
    if (threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
    __syncthreads();
  }
  const T r = red[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void spectral_products_kernel(const float* __restrict__ p, const int64_t* __restrict__ segs,
                                                                const int32_t* __restrict__ blocks, sn_limits lim,
                                                                const float* __restrict__ u, float* __restrict__ v,
                                                                float* __restrict__ partials, float* __restrict__ cols) {
  __shared__ float t[MAX_RPB];
  __shared__ float red[256];
  const sn_view s = block_view(segs, blocks, lim);
  if (s.rows == 0) return;
  const float* w = p + s.base;
  const float* us = u + s.uoff;
  const int C = s.C, L = lanes_per_row(C);
  // t_r = sum_c W[r, c] u[c]: L lanes per row, 256 / L rows at a time; the lanes of a row are combined by a butterfly
  {
    const int sub = threadIdx.x / L, cl = threadIdx.x % L, per = 256 / L;
    for (int r = 0; r < s.rows; r += per) {      // (uniform bounds: every lane takes part in the shuffles)
      const int row = r + sub;
      float acc = 0.f;
      if (row < s.rows)
        for (int c = cl; c < C; c += L) acc += w[(int64_t)row * C + c] * us[c];
      for (int k = L >> 1; k >= 1; k >>= 1) acc += __shfl_xor(acc, k);
      if (cl == 0 && row < s.rows) t[row] = acc;
    }
  }
  __syncthreads();
  float tt = 0.f;
  for (int r = threadIdx.x; r < s.rows; r += 256) {
    const float x = t[r];
    v[s.voff + s.r0 + r] = x;
    tt += x * x;
  }
  tt = block_sum(tt, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = tt;
  // the block's column sums of W^T t: LC threads over the columns, 256 / LC groups over the rows, groups added in order
  int LC = 1;
  while (LC < C && LC < 256) LC <<= 1;
  const int G = 256 / LC, g = threadIdx.x / LC, cl = threadIdx.x % LC;
  for (int c0 = 0; c0 < C; c0 += LC) {
    const int c = c0 + cl;
    float acc = 0.f;
    if (c < C)
      for (int r = g; r < s.rows; r += G) acc += w[(int64_t)r * C + c] * t[r];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (g == 0 && c < C) {
      float sum = red[cl];
      for (int k = 1; k < G; ++k) sum += red[k * LC + cl];
      cols[s.coloff + c] = sum;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void spectral_normalise_kernel(const int64_t* __restrict__ segs, sn_limits lim,
                                                                 const float* __restrict__ partials,
                                                                 const float* __restrict__ cols, float* __restrict__ u,
                                                                 float* __restrict__ sigma, float* __restrict__ nt_out) {
  __shared__ double red[256];
  const sn_view s = segment_view(segs, blockIdx.x, 0, lim);
  if (s.rows == 0) return;
  const int64_t first = segs[(int64_t)SEG_FIELDS * s.seg + 3];
  const int C = s.C;
  double T = 0.0;
  for (int b = threadIdx.x; b < s.nb; b += 256) T += (double)partials[first + b];
  T = block_sum(T, red);
  float* us = u + s.uoff;
  // s_c: LC threads over the columns, 256 / LC groups over the row blocks (group g takes blocks g, g + G, ...), groups added in order
  int LC = 1;
  while (LC < C && LC < 256) LC <<= 1;
  const int G = 256 / LC, g = threadIdx.x / LC, cl = threadIdx.x % LC;
  double S = 0.0;
  for (int c0 = 0; c0 < C; c0 += LC) {
    const int c = c0 + cl;
    double sc = 0.0;
    if (c < C)
      for (int b = g; b < s.nb; b += G) sc += (double)cols[s.coloff + (int64_t)b * C + c];
    red[threadIdx.x] = sc;
    __syncthreads();
    if (g == 0 && c < C) {
      for (int k = 1; k < G; ++k) sc += red[k * LC + cl];
      const float sf = (float)sc;      // (u holds the raw column sum until the norms are known)
      us[c] = sf;
      S += (double)sf * (double)sf;
    }
    __syncthreads();
  }
  S = block_sum(S, red);
  const double nt = sqrt(T > CLAMP ? T : CLAMP);
  const double U2 = S / (nt * nt);
  const double nu = sqrt(U2 > CLAMP ? U2 : CLAMP);
  const double inv = 1.0 / (nt * nu);
  __threadfence_block();
  __syncthreads();      // (the raw sums were written by the column groups' first threads)
  for (int c = threadIdx.x; c < C; c += 256) us[c] = (float)((double)us[c] * inv);
  if (threadIdx.x == 0) {
    sigma[s.seg] = (float)(U2 / nu);
    nt_out[s.seg] = (float)nt;
  }
}

__global__ __launch_bounds__(256) void spectral_scale_kernel(const float* __restrict__ p, float* __restrict__ eff,
                                                             const int64_t* __restrict__ segs,
                                                             const int32_t* __restrict__ blocks, sn_limits lim,
                                                             float* __restrict__ v, const float* __restrict__ sigma,
                                                             const float* __restrict__ nt) {
  const sn_view s = block_view(segs, blocks, lim);
  if (s.rows == 0) return;
  const float sg = sigma[s.seg], n = nt[s.seg];
  const int64_t count = (int64_t)s.rows * s.C;
  const float* w = p + s.base;
  float* o = eff + s.base;
  const int64_t nv = (s.base & 3) ? 0 : count / 4;      // 16-byte loads only where the block's first row is aligned
  for (int64_t i = threadIdx.x; i < nv; i += 256) {
    f32x4 x = reinterpret_cast<const f32x4*>(w)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = x[e] / sg;
    reinterpret_cast<f32x4*>(o)[i] = x;
    SG_STORE16_GUARD(x);
  }
  for (int64_t i = nv * 4 + threadIdx.x; i < count; i += 256) o[i] = w[i] / sg;
  for (int r = threadIdx.x; r < s.rows; r += 256) v[s.voff + s.r0 + r] = v[s.voff + s.r0 + r] / n;
}

__global__ __launch_bounds__(256) void spectral_dot_kernel(const float* __restrict__ g, const float* __restrict__ eff,
                                                           const int64_t* __restrict__ segs,
                                                           const int32_t* __restrict__ blocks, sn_limits lim,
                                                           float* __restrict__ partials) {
  __shared__ float red[256];
  const sn_view s = block_view(segs, blocks, lim);
  if (s.rows == 0) return;
  const int64_t count = (int64_t)s.rows * s.C;
  const float* a = g + s.base;
  const float* b = eff + s.base;
  const int64_t nv = (s.base & 3) ? 0 : count / 4;
  float acc = 0.f;
  for (int64_t i = threadIdx.x; i < nv; i += 256) {
    const f32x4 x = reinterpret_cast<const f32x4*>(a)[i], y = reinterpret_cast<const f32x4*>(b)[i];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc += x[e] * y[e];
  }
  for (int64_t i = nv * 4 + threadIdx.x; i < count; i += 256) acc += a[i] * b[i];
  acc = block_sum(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void spectral_pullback_kernel(float* __restrict__ g, const int64_t* __restrict__ segs,
                                                                const int32_t* __restrict__ blocks, sn_limits lim,
                                                                const float* __restrict__ partials,
                                                                const float* __restrict__ u, const float* __restrict__ v,
                                                                const float* __restrict__ sigma) {
  __shared__ double red[256];
  const sn_view s = block_view(segs, blocks, lim);
  if (s.rows == 0) return;
  const int64_t first = segs[(int64_t)SEG_FIELDS * s.seg + 3];
  double dd = 0.0;
  for (int b = threadIdx.x; b < s.nb; b += 256) dd += (double)partials[first + b];
  const float d = (float)block_sum(dd, red);
  const float sg = sigma[s.seg];
  const float* us = u + s.uoff;
  const float* vs = v + s.voff + s.r0;
  float* a = g + s.base;
  const int C = s.C, L = lanes_per_row(C);
  const int sub = threadIdx.x / L, cl = threadIdx.x % L, per = 256 / L;
  for (int row = sub; row < s.rows; row += per) {
    const float dv = d * vs[row];
    for (int c = cl; c < C; c += L) {
      const int64_t i = (int64_t)row * C + c;
      a[i] = (a[i] - dv * us[c]) / sg;
    }
  }
}

bool bad_table(const int64_t* segs, const int32_t* blocks, int32_t nseg, int32_t nblocks, int64_t total) {
  return !segs || !blocks || nseg < 1 || nblocks < nseg || total < 1;
}

}  // namespace

extern "C" int sg_spectral_refresh(const float* p, float* eff, int64_t total, const int64_t* segs, const int32_t* blocks,
                                   int32_t nseg, int32_t nblocks, float* u, int64_t ulen, float* v, int64_t vlen,
                                   float* sigma, float* nt, float* partials, float* cols, int64_t collen, int32_t iteration,
                                   sg_stream_t st) {
  if (!p || !eff || !u || !v || !sigma || !nt || !partials || !cols || bad_table(segs, blocks, nseg, nblocks, total))
    return SG_EINVAL;
  if (p == eff || iteration < 1 || ulen < 1 || vlen < 1 || collen < 1) return SG_EINVAL;
  if (!sg_aligned16(p) || !sg_aligned16(eff)) return SG_EALIGN;
  const sn_limits lim = {total, ulen, vlen, collen, nblocks, nseg};
  for (int32_t k = 0; k < iteration; ++k) {
    hipLaunchKernelGGL(spectral_products_kernel, dim3((unsigned)nblocks), dim3(256), 0, sg_st(st), p, segs, blocks, lim, u, v,
                       partials, cols);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(spectral_normalise_kernel, dim3((unsigned)nseg), dim3(256), 0, sg_st(st), segs, lim, partials, cols, u,
                       sigma, nt);
    SG_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(spectral_scale_kernel, dim3((unsigned)nblocks), dim3(256), 0, sg_st(st), p, eff, segs, blocks, lim, v,
                     sigma, nt);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_spectral_pullback(float* g, const float* eff, int64_t total, const int64_t* segs, const int32_t* blocks,
                                    int32_t nseg, int32_t nblocks, const float* u, int64_t ulen, const float* v,
                                    int64_t vlen, const float* sigma, float* partials, sg_stream_t st) {
  if (!g || !eff || !u || !v || !sigma || !partials || bad_table(segs, blocks, nseg, nblocks, total)) return SG_EINVAL;
  if (g == eff || ulen < 1 || vlen < 1) return SG_EINVAL;
  if (!sg_aligned16(g) || !sg_aligned16(eff)) return SG_EALIGN;
  const sn_limits lim = {total, ulen, vlen, INT64_MAX, nblocks, nseg};      // (the column workspace is not touched here)
  hipLaunchKernelGGL(spectral_dot_kernel, dim3((unsigned)nblocks), dim3(256), 0, sg_st(st), g, eff, segs, blocks, lim,
                     partials);
  SG_LAUNCH_CHECK();
  hipLaunchKernelGGL(spectral_pullback_kernel, dim3((unsigned)nblocks), dim3(256), 0, sg_st(st), g, segs, blocks, lim, partials,
                     u, v, sigma);
  SG_LAUNCH_CHECK();
  return SG_OK;
}
