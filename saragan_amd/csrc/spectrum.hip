// Shell-binned power spectra: per sample x [d, h, w] of any sg_src_dtype, the half spectrum
//   F(kd, kh, kw) = sum t * exp(-2 pi i (kd d / D + kh h / H + kw w / W)),  kw = 0 .. W / 2,  t = (double)x * scale + shift,
// as three one-axis passes (W, then H, then D) of small f64 matrix products on v_mfma_f64_16x16x4_f64, and of it only
//   radial[c] = sum g P over the coefficients of radial column c,   P = Fr^2 + Fi^2,  g = 1 at kw = 0 and kw = W / 2, else 2
//   axis_d[q], axis_h[q], axis_w[q]: the same sums over min(kd, D - kd) = q, min(kh, H - kh) = q, kw = q.
// The host supplies the per-axis matrices (transposed: Mt[j][k] = trig[(k j) mod n] * win[j], k contiguous), the three tables
// of squared frequencies and the squared column edges; the file is built with -ffp-contract=off, so t rounds twice and
// r2 = (f2_d + f2_h) + f2_w has numpy's bits.
//
// f64 MFMA operand maps (16x16x4): lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; of C/D it holds
// col l & 15, rows (l >> 4) + 4 * reg, reg = 0..3.  Fragments are loaded with guarded scalar loads: what lies past an extent
// is a zero in a register, nothing is read past a row.  A wave owns ONE 16-row tile of the matrix and SP_TILES 16-wide data
// tiles: a matrix fragment (two loads per lane) feeds 4 * SP_TILES MFMAs in the complex passes.
//
// Complex pass: Yr = C Xr + S Xi, Yi = C Xi - S Xr (the W pass has Xi = 0).  Intermediates are planar f64 [n, D, H, Wf] in
// the workspace (two pairs of planes).  The D pass writes no coefficient: it squares and weights its tiles and adds them to
// a wave-private image of the sample's row (radial columns, then the three profiles) in LDS.  Lanes of one instruction that
// meet in one bin are summed by a fixed butterfly over the wave (the others contribute +0.0) and added by lane 0, so the
// order of every sum is fixed by (D, H, W, bins) alone: no floating-point atomics, and a sample's bits do not depend on the
// batch around it.  A block sums its waves' images in wave order into one partial row; sp_finalize sums a sample's
// partial rows in index order.
//
// What bounds it: the matrix pipe in the W and H passes (10 and 6 operand loads per 8 and 16 MFMAs, every MFMA 4 x 16 x 16 x 2
// flop); the D pass adds the binning, 10 bin-adds per 16 x 16 tile, each a loop over the distinct bins of the wave.
#include "common.h"
#include <math.h>

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int SP_MAX_EXTENT = 1024;
constexpr int SP_MAX_BINS = 4096;
constexpr int SP_WAVES = 4;                    // waves per block (the D pass may take fewer: its LDS holds one image per wave)
constexpr int SP_TILES = 4;                    // data tiles per wave
constexpr int SP_SPAN = 16 * SP_TILES;         // data rows (W pass) or columns (H, D passes) of a wave
constexpr int SP_LDS_BYTES = 64 * 1024;        // the D pass's dynamic LDS never passes this
constexpr int64_t SP_MAX_PARTIALS = 1024;      // partial rows per sample, at most
constexpr int64_t SP_SLAB = 32768;             // samples per launch sequence (grid.z)

template <typename S>
__device__ __forceinline__ double sp_to_d(S v) { return (double)v; }      // exact for every source type
struct sp_bf16 { uint16_t bits; };
template <>
__device__ __forceinline__ double sp_to_d<sp_bf16>(sp_bf16 v) { return (double)__uint_as_float((uint32_t)v.bits << 16); }

__device__ __forceinline__ f64x4 sp_mfma(double a, double b, f64x4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// ---- W pass: Y[r][k] = sum_j t[r][j] M[k][j] over the contiguous index.  A = the data (16 rows x 4 j), B = Mt.
template <typename S>
__global__ __launch_bounds__(SP_WAVES * 64) void sp_pass_w(const S* __restrict__ x, int64_t rows, int W, int Wf, double scale,
                                                          double shift, const double* __restrict__ Ct,
                                                          const double* __restrict__ St, double* __restrict__ yr,
                                                          double* __restrict__ yi) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const int64_t KT = (Wf + 15) / 16, RG = (rows + SP_SPAN - 1) / SP_SPAN;
  const int64_t item = (int64_t)blockIdx.x * SP_WAVES + (threadIdx.x >> 6);
  if (item >= KT * RG) return;
  const int kt = (int)(item % KT);
  const int64_t r0 = (item / KT) * SP_SPAN, samp = blockIdx.z;
  const S* __restrict__ xs = x + samp * rows * (int64_t)W;
  const int k = kt * 16 + lr;
  f64x4 ar[SP_TILES], ai[SP_TILES];
#pragma unroll
  for (int t = 0; t < SP_TILES; ++t) { ar[t] = f64x4{0., 0., 0., 0.}; ai[t] = f64x4{0., 0., 0., 0.}; }
  for (int j0 = 0; j0 < W; j0 += 4) {
    const int j = j0 + lk;
    const bool mok = j < W && k < Wf;
    const double bc = mok ? Ct[(int64_t)j * Wf + k] : 0.0;
    const double bs = mok ? -St[(int64_t)j * Wf + k] : 0.0;
#pragma unroll
    for (int t = 0; t < SP_TILES; ++t) {
      if (r0 + t * 16 < rows) {      // (wave-uniform)
        const int64_t r = r0 + t * 16 + lr;
        double a = 0.0;
        if (r < rows && j < W) a = __dadd_rn(__dmul_rn(sp_to_d(xs[r * W + j]), scale), shift);
        ar[t] = sp_mfma(a, bc, ar[t]);
        ai[t] = sp_mfma(a, bs, ai[t]);
      }
    }
  }
  if (k >= Wf) return;
  double* __restrict__ outr = yr + samp * rows * (int64_t)Wf;
  double* __restrict__ outi = yi + samp * rows * (int64_t)Wf;
#pragma unroll
  for (int t = 0; t < SP_TILES; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int64_t r = r0 + t * 16 + lk + 4 * g;
      if (r < rows) {
        outr[r * Wf + k] = ar[t][g];
        outi[r * Wf + k] = ai[t][g];
      }
    }
}

// ---- the D pass's tables and the layout of a sample's row
struct sp_bins {
  const double* f2d;
  const double* f2h;
  const double* f2w;
  const double* edges2;      // [bins + 1]
  int32_t bins, D, H, W, Wf;
  int32_t row_len;           // (bins + 1) + (D / 2 + 1) + (H / 2 + 1) + (W / 2 + 1)
  int32_t edges_in_lds;
  int32_t items_per_wave;
};

// the radial column of r2 > 0: the smallest b >= 1 with b == bins + 1 or ed[b] > r2, capped at bins (the top edge is closed).
// The square root only says where to start looking: the answer is decided by comparisons with the table alone.
__device__ __forceinline__ int sp_column(double r2, const double* ed, int bins, double inv_top) {
  if (r2 == 0.0) return 0;
  int b = (int)(sqrt(r2 * inv_top) * (double)bins) + 1;
  b = max(1, min(b, bins + 1));
  while (b > 1 && ed[b - 1] > r2) --b;
  while (b <= bins && ed[b] <= r2) ++b;
  return min(b, bins);
}

// img[key] += the sum of v over the lanes that hold `key`, for every distinct key >= 0 of the wave: one fixed butterfly per key
// (lanes with another key add +0.0, which changes no bit of a sum of non-negative terms), added by lane 0 in the order of the
// keys' first lanes.
__device__ __forceinline__ void sp_wave_bin_add(double* img, int key, double v, int lane) {
  unsigned long long todo = __ballot(key >= 0);
  while (todo) {
    const int leader = __ffsll(todo) - 1;
    const int kk = __shfl(key, leader);
    const bool m = key == kk;
    double s = m ? v : 0.0;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) img[kk] += s;
    todo &= ~__ballot(m);
  }
}

// ---- H and D passes: Y[o][k][i] = sum_j M[k][j] X[o][j][i] on [outer, N, inner] views.  A = M (16 k x 4 j), B = the data.
template <bool LAST>
__global__ __launch_bounds__(SP_WAVES * 64) void sp_pass_left(const double* __restrict__ xr, const double* __restrict__ xi, int N,
                                                             int64_t inner, const double* __restrict__ Ct,
                                                             const double* __restrict__ St, double* __restrict__ yr,
                                                             double* __restrict__ yi, sp_bins sb, double* __restrict__ partial) {
  extern __shared__ double sp_lds[];
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
  const int64_t KT = (N + 15) / 16, CG = (inner + SP_SPAN - 1) / SP_SPAN, items = KT * CG;
  const int64_t plane = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * (int64_t)N * inner;
  const double* __restrict__ pr = xr + plane;
  const double* __restrict__ pi = xi + plane;
  double* img = nullptr;
  const double* ed = sb.edges2;
  double inv_top = 0.0;      // 1 / edges2[bins] (0 where that is 0): only the first guess of a column uses it
  if (LAST) {
    const double top = sb.edges2[sb.bins];
    inv_top = top > 0.0 ? 1.0 / top : 0.0;
    double* base = sp_lds;
    if (sb.edges_in_lds) {
      for (int b = threadIdx.x; b <= sb.bins; b += blockDim.x) base[b] = sb.edges2[b];
      ed = base;
      base += sb.bins + 1;
    }
    for (int b = threadIdx.x; b < waves * sb.row_len; b += blockDim.x) base[b] = 0.0;
    img = base + wave * sb.row_len;
    __syncthreads();
  }
  const int per = LAST ? sb.items_per_wave : 1;
  for (int q = 0; q < per; ++q) {
    const int64_t item = ((int64_t)blockIdx.x * waves + wave) * per + q;
    if (item >= items) break;
    const int kt = (int)(item % KT);
    const int64_t i0 = (item / KT) * SP_SPAN;
    const int k = kt * 16 + lr;
    f64x4 ar[SP_TILES], ai[SP_TILES];
#pragma unroll
    for (int t = 0; t < SP_TILES; ++t) { ar[t] = f64x4{0., 0., 0., 0.}; ai[t] = f64x4{0., 0., 0., 0.}; }
    for (int j0 = 0; j0 < N; j0 += 4) {
      const int j = j0 + lk;
      const bool mok = j < N && k < N;
      const double mc = mok ? Ct[(int64_t)j * N + k] : 0.0;
      const double ms = mok ? St[(int64_t)j * N + k] : 0.0;
      const double mn = -ms;
#pragma unroll
      for (int t = 0; t < SP_TILES; ++t) {
        if (i0 + t * 16 < inner) {      // (wave-uniform)
          const int64_t i = i0 + t * 16 + lr;
          const bool ok = j < N && i < inner;
          const double vr = ok ? pr[(int64_t)j * inner + i] : 0.0;
          const double vi = ok ? pi[(int64_t)j * inner + i] : 0.0;
          ar[t] = sp_mfma(mc, vr, ar[t]);
          ar[t] = sp_mfma(ms, vi, ar[t]);
          ai[t] = sp_mfma(mc, vi, ai[t]);
          ai[t] = sp_mfma(mn, vr, ai[t]);
        }
      }
    }
    if (!LAST) {
      double* __restrict__ outr = yr + plane;
      double* __restrict__ outi = yi + plane;
#pragma unroll
      for (int t = 0; t < SP_TILES; ++t) {
        const int64_t i = i0 + t * 16 + lr;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int kk = kt * 16 + lk + 4 * g;
          if (kk < N && i < inner) {
            outr[(int64_t)kk * inner + i] = ar[t][g];
            outi[(int64_t)kk * inner + i] = ai[t][g];
          }
        }
      }
    } else {
      const int off_d = sb.bins + 1, off_h = off_d + sb.D / 2 + 1, off_w = off_h + sb.H / 2 + 1;
#pragma unroll
      for (int t = 0; t < SP_TILES; ++t) {
        if (i0 + t * 16 >= inner) break;      // (wave-uniform)
        const int64_t i = i0 + t * 16 + lr;
        const bool iok = i < inner;
        const int kh = iok ? (int)(i / sb.Wf) : 0;
        const int kw = iok ? (int)(i - (int64_t)kh * sb.Wf) : 0;
        const double wgt = (kw == 0 || 2 * kw == sb.W) ? 1.0 : 2.0;
        const double fh = sb.f2h[kh], fw = sb.f2w[kw];
        double colsum = 0.0;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int kd = kt * 16 + lk + 4 * g;
          const bool ok = iok && kd < sb.D;
          const double fr = ar[t][g], fi = ai[t][g];
          const double p = (fr * fr + fi * fi) * wgt;
          const double r2 = (sb.f2d[ok ? kd : 0] + fh) + fw;
          sp_wave_bin_add(img, ok ? sp_column(r2, ed, sb.bins, inv_top) : -1, p, lane);
          sp_wave_bin_add(img + off_d, ok ? min(kd, sb.D - kd) : -1, p, lane);
          colsum += ok ? p : 0.0;
        }
        sp_wave_bin_add(img + off_h, iok ? min(kh, sb.H - kh) : -1, colsum, lane);
        sp_wave_bin_add(img + off_w, iok ? kw : -1, colsum, lane);
      }
    }
  }
  if (LAST) {
    __syncthreads();
    const double* base = sp_lds + (sb.edges_in_lds ? sb.bins + 1 : 0);
    double* __restrict__ dst = partial + ((int64_t)blockIdx.z * gridDim.x + blockIdx.x) * (int64_t)sb.row_len;
    for (int b = threadIdx.x; b < sb.row_len; b += blockDim.x) {
      double s = base[b];
      for (int w = 1; w < waves; ++w) s += base[w * sb.row_len + b];
      dst[b] = s;
    }
  }
}

// a sample's partial rows, summed in index order
__global__ __launch_bounds__(256) void sp_finalize(const double* __restrict__ partial, int64_t parts, int row_len, int nrad,
                                                  double* __restrict__ radial, double* __restrict__ axes) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= row_len) return;
  const int64_t samp = blockIdx.y;
  const double* __restrict__ src = partial + samp * parts * (int64_t)row_len + b;
  double s = src[0];
  for (int64_t p = 1; p < parts; ++p) s += src[p * row_len];
  if (b < nrad) radial[samp * nrad + b] = s;
  else axes[samp * (int64_t)(row_len - nrad) + (b - nrad)] = s;
}

// the launch structure of one shape: a function of (d, h, w, bins) alone
struct sp_plan {
  int64_t vol;         // D * H * Wf: elements of one plane of one sample
  int32_t row_len, edges_in_lds, waves, items_per_wave;
  int64_t parts;       // partial rows (= D-pass blocks) per sample
  size_t lds;
};

sp_plan sp_make_plan(int64_t d, int64_t h, int64_t w, int32_t bins) {
  sp_plan p;
  const int64_t wf = w / 2 + 1;
  p.vol = d * h * wf;
  p.row_len = (int32_t)((bins + 1) + (d / 2 + 1) + (h / 2 + 1) + (w / 2 + 1));
  const int64_t row_bytes = (int64_t)p.row_len * 8, edge_bytes = (int64_t)(bins + 1) * 8;
  p.edges_in_lds = edge_bytes + row_bytes <= SP_LDS_BYTES ? 1 : 0;
  const int64_t room = SP_LDS_BYTES - (p.edges_in_lds ? edge_bytes : 0);
  int64_t waves = room / row_bytes;
  p.waves = (int32_t)(waves > SP_WAVES ? SP_WAVES : waves);      // >= 1: a row is at most 45088 bytes
  p.lds = (size_t)((p.edges_in_lds ? edge_bytes : 0) + p.waves * row_bytes);
  const int64_t items = ((d + 15) / 16) * ((h * wf + SP_SPAN - 1) / SP_SPAN);
  p.items_per_wave = (int32_t)((items + p.waves * SP_MAX_PARTIALS - 1) / (p.waves * SP_MAX_PARTIALS));
  const int64_t per_block = (int64_t)p.waves * p.items_per_wave;
  p.parts = (items + per_block - 1) / per_block;
  return p;
}

// The workspace does not depend on `bins`: the partial rows are sized for the most columns and the most blocks any bins give
// (one wave per block: min(items, SP_MAX_PARTIALS) rows).
size_t sp_workspace(int64_t n, int64_t d, int64_t h, int64_t w) {
  const int64_t wf = w / 2 + 1, vol = d * h * wf;
  const int64_t items = ((d + 15) / 16) * ((h * wf + SP_SPAN - 1) / SP_SPAN);
  const int64_t parts = items < SP_MAX_PARTIALS ? items : SP_MAX_PARTIALS;
  const int64_t row = (SP_MAX_BINS + 1) + (d / 2 + 1) + (h / 2 + 1) + (w / 2 + 1);
  return (size_t)n * ((size_t)4 * (size_t)vol + (size_t)parts * (size_t)row) * sizeof(double);
}

template <typename S>
int sp_run(const void* x, int64_t n, int64_t d, int64_t h, int64_t w, double scale, double shift, const double* mats,
           const double* f2, const double* edges2, int32_t bins, double* radial, double* axes, double* ws,
           const sp_plan& p, hipStream_t hs) {
  if (((uintptr_t)x) % sizeof(S) != 0) return SG_EALIGN;
  const int64_t wf = w / 2 + 1, rows = d * h;
  const double* Cd = mats;
  const double* Sd = Cd + d * d;
  const double* Ch = Sd + d * d;
  const double* Sh = Ch + h * h;
  const double* Cw = Sh + h * h;
  const double* Sw = Cw + w * wf;
  sp_bins sb;
  sb.f2d = f2; sb.f2h = f2 + d; sb.f2w = f2 + d + h; sb.edges2 = edges2;
  sb.bins = bins; sb.D = (int32_t)d; sb.H = (int32_t)h; sb.W = (int32_t)w; sb.Wf = (int32_t)wf;
  sb.row_len = p.row_len; sb.edges_in_lds = p.edges_in_lds; sb.items_per_wave = p.items_per_wave;
  const int nrad = bins + 1;
  for (int64_t n0 = 0; n0 < n; n0 += SP_SLAB) {
    const int64_t m = n - n0 < SP_SLAB ? n - n0 : SP_SLAB;
    double* ar = ws;                       // after the W pass
    double* ai = ar + m * p.vol;
    double* br = ai + m * p.vol;           // after the H pass
    double* bi = br + m * p.vol;
    double* partial = bi + m * p.vol;
    const S* xs = (const S*)x + n0 * rows * w;
    const int64_t items_w = ((wf + 15) / 16) * ((rows + SP_SPAN - 1) / SP_SPAN);
    hipLaunchKernelGGL((sp_pass_w<S>), dim3((unsigned)((items_w + SP_WAVES - 1) / SP_WAVES), 1, (unsigned)m), dim3(SP_WAVES * 64),
                       0, hs, xs, rows, (int)w, (int)wf, scale, shift, Cw, Sw, ar, ai);
    SG_LAUNCH_CHECK();
    const int64_t items_h = ((h + 15) / 16) * ((wf + SP_SPAN - 1) / SP_SPAN);
    hipLaunchKernelGGL((sp_pass_left<false>), dim3((unsigned)((items_h + SP_WAVES - 1) / SP_WAVES), (unsigned)d, (unsigned)m),
                       dim3(SP_WAVES * 64), 0, hs, ar, ai, (int)h, wf, Ch, Sh, br, bi, sb, (double*)nullptr);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL((sp_pass_left<true>), dim3((unsigned)p.parts, 1, (unsigned)m), dim3(p.waves * 64), p.lds, hs, br, bi,
                       (int)d, h * wf, Cd, Sd, (double*)nullptr, (double*)nullptr, sb, partial);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(sp_finalize, dim3((unsigned)((p.row_len + 255) / 256), (unsigned)m), dim3(256), 0, hs, partial, p.parts,
                       p.row_len, nrad, radial + n0 * nrad, axes + n0 * (int64_t)(p.row_len - nrad));
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}

bool sp_shape_ok(int64_t d, int64_t h, int64_t w) {
  return d >= 1 && h >= 1 && w >= 1 && d <= SP_MAX_EXTENT && h <= SP_MAX_EXTENT && w <= SP_MAX_EXTENT;
}

}  // namespace

extern "C" int32_t sg_power_spectrum_max_extent(void) { return SP_MAX_EXTENT; }

extern "C" size_t sg_power_spectrum_workspace(int64_t n, int64_t d, int64_t h, int64_t w) {
  if (n < 1 || !sp_shape_ok(d, h, w)) return 0;
  return sp_workspace(n < SP_SLAB ? n : SP_SLAB, d, h, w);      // slabs of samples reuse one workspace
}

extern "C" int sg_power_spectrum(const void* x, sg_src_dtype dt, int64_t n, int64_t d, int64_t h, int64_t w, double scale,
                                 double shift, const double* mats, const double* f2, const double* edges2,
                                 int32_t bins, double* radial, double* axes, void* workspace, size_t workspace_bytes,
                                 sg_stream_t st) {
  if (n < 0 || !sp_shape_ok(d, h, w) || bins < 1 || bins > SP_MAX_BINS) return SG_EINVAL;
  if ((int)dt < (int)SG_SRC_U8 || (int)dt > (int)SG_SRC_BF16) return SG_EINVAL;
  if (!isfinite(scale) || !isfinite(shift)) return SG_EINVAL;
  if (n == 0) return SG_OK;
  if (!x || !mats || !f2 || !edges2 || !radial || !axes || !workspace) return SG_EINVAL;
  const sp_plan p = sp_make_plan(d, h, w, bins);
  if (workspace_bytes < sp_workspace(n < SP_SLAB ? n : SP_SLAB, d, h, w)) return SG_EWORKSPACE;
  if (((uintptr_t)mats | (uintptr_t)f2 | (uintptr_t)edges2 | (uintptr_t)radial | (uintptr_t)axes | (uintptr_t)workspace) % 8 != 0)
    return SG_EALIGN;
  hipStream_t hs = sg_st(st);
  double* ws = (double*)workspace;
  switch (dt) {
    case SG_SRC_U8:   return sp_run<uint8_t>(x, n, d, h, w, scale, shift, mats, f2, edges2, bins, radial, axes, ws, p, hs);
    case SG_SRC_I8:   return sp_run<int8_t>(x, n, d, h, w, scale, shift, mats, f2, edges2, bins, radial, axes, ws, p, hs);
    case SG_SRC_I16:  return sp_run<int16_t>(x, n, d, h, w, scale, shift, mats, f2, edges2, bins, radial, axes, ws, p, hs);
    case SG_SRC_U16:  return sp_run<uint16_t>(x, n, d, h, w, scale, shift, mats, f2, edges2, bins, radial, axes, ws, p, hs);
    case SG_SRC_F16:  return sp_run<_Float16>(x, n, d, h, w, scale, shift, mats, f2, edges2, bins, radial, axes, ws, p, hs);
    case SG_SRC_F32:  return sp_run<float>(x, n, d, h, w, scale, shift, mats, f2, edges2, bins, radial, axes, ws, p, hs);
    case SG_SRC_BF16: return sp_run<sp_bf16>(x, n, d, h, w, scale, shift, mats, f2, edges2, bins, radial, axes, ws, p, hs);
  }
  return SG_EINVAL;
}
