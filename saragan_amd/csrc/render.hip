// Sample previews: one launch renders one VIEW of every sample of a batch x [n, d, h, w, c] (any sg_src_dtype)
// into a u8 canvas on the device.  A view collapses one axis -- a plane of it (SLICE), its maximum (MAX) or its mean (MEAN) -- and
// the two remaining axes, in their original order, are the image's rows and columns:
//   axis 0 (D) -> H x W (axial)     axis 1 (H) -> D x W (coronal)     axis 2 (W) -> D x H (sagittal)
//
// The definition is exact (tests compare with ==).  Per image pixel, in this order:
//   v = f32(x)                                        SLICE
//       max over the axis from -inf, NaN ignored      MAX   (a comparison per voxel: an all-NaN column stays -inf)
//       f32(f64 sum over the axis / extent)           MEAN  (the f64 sum in any order: one f64 division, one rounding)
//   t = v * scale + shift                             two correctly rounded f32 operations (the file is built with
//   u = (t - lo) * inv                                -ffp-contract=off as well); inv = f32(255 / (f64(hi) - f64(lo))), the caller's
//   g = u8(floor(min(max(u, 0), 255) + 0.5f))         a NaN u gives 0
// and g is stored zoom_r x zoom_c times (nearest repeat, on the store side) into the sample's tile.
//
// Two kernels, by where the collapsed axis lies in memory:
//   * render_cols_kernel: the lanes run along the image's columns and every lane walks the collapsed axis in registers -- the
//     collapse along D and along H (columns = W, contiguous: 16-byte loads where c == 1 and every row starts at the same
//     offset from a 16-byte boundary, the columns in front of the first boundary and behind the last whole load by element) and
//     every SLICE (a strided copy through the same map; the W slice reads one element per row).
//   * render_rows_kernel: the collapse along W.  The collapsed axis is the contiguous one, so a group of lanes -- a wave for
//     short rows, the block for long ones -- reads a row with 16-byte loads (from the row's OWN first boundary: the head and tail
//     are per row), reduces with shuffles across the wave and, for the block, through LDS across its four waves.
// No atomics: every image pixel has one owner, which writes its zoom_r x zoom_c bytes.  All offsets are 64-bit.
#include "common.h"
#include <math.h>
#include <initializer_list>
#include <type_traits>

namespace {

constexpr int RV_THREADS = 256;
constexpr int RV_WAVE = 64;
constexpr int RV_UNROLL = 8;                       // loads in flight per lane along the collapsed axis
constexpr int64_t RV_MAX_BLOCKS = 1 << 20;         // grid-stride beyond
constexpr int64_t RV_WAVE_ROW_BYTES = 2 * RV_WAVE * 16;      // rows up to two 16-byte loads per lane take a wave, longer ones the block

struct rv_tone {
  float scale, shift, lo, inv;
};

struct rv_canvas {
  uint8_t* p;
  int64_t w, r0, c0, pitch_r, pitch_c;
  int32_t grid_cols, zoom_r, zoom_c;
};

// the image in the volume: pixel (r, q) of sample i collapses x[off + i * sN + r * sR + q * sQ + k * sK], k < K  (element strides)
struct rv_geom {
  int64_t n, R, Q, K, sN, sR, sQ, sK, off;
};

template <typename S>
__device__ __forceinline__ float rv_to_f(S v) { return (float)v; }      // exact for every source type
struct rv_bf16 { uint16_t bits; };                                      // bf16 is the upper half of an f32
template <>
__device__ __forceinline__ float rv_to_f<rv_bf16>(rv_bf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }

template <int MODE>
using rv_acc_t = std::conditional_t<MODE == SG_VIEW_MEAN, double, float>;

template <int MODE>
__device__ __forceinline__ rv_acc_t<MODE> rv_init() {
  if constexpr (MODE == SG_VIEW_MEAN) return 0.0;
  else return -INFINITY;
}
template <int MODE>
__device__ __forceinline__ void rv_add(rv_acc_t<MODE>& a, float x) {
  if constexpr (MODE == SG_VIEW_MEAN) a += (double)x;
  else if constexpr (MODE == SG_VIEW_MAX) a = x > a ? x : a;      // false for a NaN x: ignored
  else a = x;
}
template <int MODE>
__device__ __forceinline__ void rv_merge(rv_acc_t<MODE>& a, rv_acc_t<MODE> b) {
  if constexpr (MODE == SG_VIEW_MEAN) a += b;
  else a = b > a ? b : a;
}
template <int MODE>
__device__ __forceinline__ float rv_finish(rv_acc_t<MODE> a, int64_t K) {
  if constexpr (MODE == SG_VIEW_MEAN) return (float)(a / (double)K);
  else return a;
}

__device__ __forceinline__ uint8_t rv_grey(float v, const rv_tone& tn) {
  const float t = __fadd_rn(__fmul_rn(v, tn.scale), tn.shift);
  float u = __fmul_rn(__fsub_rn(t, tn.lo), tn.inv);
  u = u > 0.f ? u : 0.f;      // (a NaN u: 0)
  u = u < 255.f ? u : 255.f;
  return (uint8_t)floorf(__fadd_rn(u, 0.5f));
}

// pixel (r, q) of sample i's tile, repeated zoom_r x zoom_c times
__device__ __forceinline__ void rv_put(const rv_canvas& cv, int64_t i, int64_t r, int64_t q, uint8_t g) {
  const int64_t tr = i / cv.grid_cols, tc = i - tr * cv.grid_cols;
  uint8_t* __restrict__ dst = cv.p + (cv.r0 + tr * cv.pitch_r + r * cv.zoom_r) * cv.w + cv.c0 + tc * cv.pitch_c + q * cv.zoom_c;
  for (int a = 0; a < cv.zoom_r; ++a)
    for (int b = 0; b < cv.zoom_c; ++b) dst[(int64_t)a * cv.w + b] = g;
}

// ---- lanes along the image's columns.  A row of Q columns is `units` pieces of work: with VEC (sQ == 1 and every row starts
// `head` elements in front of a 16-byte boundary) the first `pieces` units are whole 16-byte loads of E columns from column
// `head` on, then come the `head` columns in front and the columns behind the last whole load, one each; without, a unit is a column.
template <typename S, int MODE, bool VEC>
__global__ __launch_bounds__(RV_THREADS) void render_cols_kernel(const S* __restrict__ x, rv_geom g, int64_t head, int64_t pieces,
                                                                 int64_t units, rv_tone tn, rv_canvas cv) {
  constexpr int E = VEC ? 16 / (int)sizeof(S) : 1;
  const int64_t total = g.n * g.R * units, stride = (int64_t)gridDim.x * RV_THREADS;
  for (int64_t t = (int64_t)blockIdx.x * RV_THREADS + threadIdx.x; t < total; t += stride) {
    const int64_t row = t / units, u = t - row * units;
    const int64_t i = row / g.R, r = row - i * g.R;
    const bool whole = VEC && u < pieces;
    int64_t q0;
    if (!VEC) q0 = u;
    else if (whole) q0 = head + u * E;
    else q0 = u - pieces < head ? u - pieces : pieces * E + (u - pieces);      // (head + pieces * E + (u - pieces - head))
    const S* __restrict__ src = x + g.off + i * g.sN + r * g.sR + q0 * g.sQ;
    if (whole) {
      rv_acc_t<MODE> acc[E];
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = rv_init<MODE>();
      for (int64_t k0 = 0; k0 < g.K; k0 += RV_UNROLL) {
        u32x4 raw[RV_UNROLL];
#pragma unroll
        for (int j = 0; j < RV_UNROLL; ++j)
          if (k0 + j < g.K) raw[j] = *reinterpret_cast<const u32x4*>(src + (k0 + j) * g.sK);
#pragma unroll
        for (int j = 0; j < RV_UNROLL; ++j) {
          if (k0 + j < g.K) {
            const S* s = reinterpret_cast<const S*>(&raw[j]);
#pragma unroll
            for (int e = 0; e < E; ++e) rv_add<MODE>(acc[e], rv_to_f(s[e]));
          }
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) rv_put(cv, i, r, q0 + e, rv_grey(rv_finish<MODE>(acc[e], g.K), tn));
    } else {
      rv_acc_t<MODE> acc = rv_init<MODE>();
      for (int64_t k0 = 0; k0 < g.K; k0 += RV_UNROLL) {
        S raw[RV_UNROLL];
#pragma unroll
        for (int j = 0; j < RV_UNROLL; ++j)
          if (k0 + j < g.K) raw[j] = src[(k0 + j) * g.sK];
#pragma unroll
        for (int j = 0; j < RV_UNROLL; ++j)
          if (k0 + j < g.K) rv_add<MODE>(acc, rv_to_f(raw[j]));
      }
      rv_put(cv, i, r, q0, rv_grey(rv_finish<MODE>(acc, g.K), tn));
    }
  }
}

// ---- the collapse along the contiguous axis: G lanes (a wave, or the block) per image pixel; K elements sK apart (sK = c).
// With VEC (c == 1) the row is read as: the elements in front of ITS first 16-byte boundary, whole 16-byte loads, the rest.
template <typename S, int MODE, bool VEC, int G>
__global__ __launch_bounds__(RV_THREADS) void render_rows_kernel(const S* __restrict__ x, rv_geom g, rv_tone tn, rv_canvas cv) {
  constexpr int E = 16 / (int)sizeof(S);
  constexpr int WAVES = RV_THREADS / RV_WAVE;
  __shared__ rv_acc_t<MODE> part[WAVES];
  const int tid = threadIdx.x, lane = tid % G, wave = tid / RV_WAVE;
  const int64_t per_block = RV_THREADS / G, total = g.n * g.R * g.Q;
  // (every lane of a group, and with G = the block every wave of it, sees the same pixel: the barriers below are uniform)
  for (int64_t px = (int64_t)blockIdx.x * per_block + tid / G; px < total; px += (int64_t)gridDim.x * per_block) {
    const int64_t row = px / g.Q, q = px - row * g.Q;
    const int64_t i = row / g.R, r = row - i * g.R;
    const S* __restrict__ src = x + g.off + i * g.sN + r * g.sR + q * g.sQ;
    rv_acc_t<MODE> acc = rv_init<MODE>();
    int64_t head = g.K, pieces = 0;
    if (VEC) {
      head = (int64_t)(((16u - (uint32_t)((uintptr_t)src & 15u)) & 15u) / (uint32_t)sizeof(S));
      if (head > g.K) head = g.K;
      pieces = (g.K - head) / E;
    }
    const int64_t tail0 = head + pieces * E;
    for (int64_t e = lane; e < head; e += G) rv_add<MODE>(acc, rv_to_f(src[e * g.sK]));
    for (int64_t e = tail0 + lane; e < g.K; e += G) rv_add<MODE>(acc, rv_to_f(src[e * g.sK]));
    if (VEC) {
      const u32x4* __restrict__ vsrc = reinterpret_cast<const u32x4*>(src + head);
      for (int64_t p = lane; p < pieces; p += (int64_t)G * 2) {
        u32x4 raw[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
          if (p + (int64_t)j * G < pieces) raw[j] = vsrc[p + (int64_t)j * G];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (p + (int64_t)j * G < pieces) {
            const S* s = reinterpret_cast<const S*>(&raw[j]);
#pragma unroll
            for (int e = 0; e < E; ++e) rv_add<MODE>(acc, rv_to_f(s[e]));
          }
        }
      }
    }
#pragma unroll
    for (int m = RV_WAVE / 2; m >= 1; m >>= 1) rv_merge<MODE>(acc, __shfl_xor(acc, m, RV_WAVE));
    if constexpr (G == RV_WAVE) {
      if (lane == 0) rv_put(cv, i, r, q, rv_grey(rv_finish<MODE>(acc, g.K), tn));
    } else {
      if (tid % RV_WAVE == 0) part[wave] = acc;
      __syncthreads();
      if (tid == 0) {
        rv_acc_t<MODE> a = part[0];
#pragma unroll
        for (int wv = 1; wv < WAVES; ++wv) rv_merge<MODE>(a, part[wv]);
        rv_put(cv, i, r, q, rv_grey(rv_finish<MODE>(a, g.K), tn));
      }
      __syncthreads();      // part[] is written again for the block's next pixel
    }
  }
}

unsigned rv_blocks(int64_t work_items, int64_t per_block) {
  int64_t b = (work_items + per_block - 1) / per_block;
  if (b > RV_MAX_BLOCKS) b = RV_MAX_BLOCKS;
  return (unsigned)b;
}

template <typename S, int MODE>
int rv_launch_cols(const S* x, const rv_geom& g, bool vec, const rv_tone& tn, const rv_canvas& cv, hipStream_t hs) {
  constexpr int64_t E = 16 / (int64_t)sizeof(S);
  if (vec) {
    int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)(x + g.off) & 15u)) & 15u) / (uint32_t)sizeof(S));
    if (head > g.Q) head = g.Q;
    const int64_t pieces = (g.Q - head) / E, units = pieces + (g.Q - pieces * E);
    hipLaunchKernelGGL((render_cols_kernel<S, MODE, true>), dim3(rv_blocks(g.n * g.R * units, RV_THREADS)), dim3(RV_THREADS), 0,
                       hs, x, g, head, pieces, units, tn, cv);
  } else {
    hipLaunchKernelGGL((render_cols_kernel<S, MODE, false>), dim3(rv_blocks(g.n * g.R * g.Q, RV_THREADS)), dim3(RV_THREADS), 0,
                       hs, x, g, (int64_t)0, (int64_t)0, g.Q, tn, cv);
  }
  SG_LAUNCH_CHECK();
  return SG_OK;
}

template <typename S, int MODE>
int rv_launch_rows(const S* x, const rv_geom& g, bool vec, const rv_tone& tn, const rv_canvas& cv, hipStream_t hs) {
  const int64_t total = g.n * g.R * g.Q;
  const bool by_wave = g.K * (int64_t)sizeof(S) <= RV_WAVE_ROW_BYTES;
  const dim3 grid(rv_blocks(total, by_wave ? RV_THREADS / RV_WAVE : 1)), block(RV_THREADS);
  if (by_wave && vec) hipLaunchKernelGGL((render_rows_kernel<S, MODE, true, RV_WAVE>), grid, block, 0, hs, x, g, tn, cv);
  else if (by_wave) hipLaunchKernelGGL((render_rows_kernel<S, MODE, false, RV_WAVE>), grid, block, 0, hs, x, g, tn, cv);
  else if (vec) hipLaunchKernelGGL((render_rows_kernel<S, MODE, true, RV_THREADS>), grid, block, 0, hs, x, g, tn, cv);
  else hipLaunchKernelGGL((render_rows_kernel<S, MODE, false, RV_THREADS>), grid, block, 0, hs, x, g, tn, cv);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

struct rv_request {
  int64_t d, h, w, index;
  int32_t c, channel, axis, mode;
};

template <typename S>
int rv_launch(const void* xv, int64_t n, const rv_request& q, const rv_tone& tn, const rv_canvas& cv, hipStream_t hs) {
  const S* x = (const S*)xv;
  const int64_t c = q.c, sW = c, sH = q.w * c, sD = q.h * sH;
  rv_geom g;
  g.n = n; g.sN = q.d * sD; g.off = q.channel;
  if (q.axis == 0)      { g.R = q.h; g.Q = q.w; g.K = q.d; g.sR = sH; g.sQ = sW; g.sK = sD; }
  else if (q.axis == 1) { g.R = q.d; g.Q = q.w; g.K = q.h; g.sR = sD; g.sQ = sW; g.sK = sH; }
  else                  { g.R = q.d; g.Q = q.h; g.K = q.w; g.sR = sD; g.sQ = sH; g.sK = sW; }
  if (q.mode == SG_VIEW_SLICE) {
    g.off += q.index * g.sK;
    g.K = 1;
    // columns = W and c == 1 and every row 16-byte periodic: whole loads (the W slice reads one element per row)
    const bool vec = q.axis != 2 && c == 1 && (q.w * (int64_t)sizeof(S)) % 16 == 0;
    return rv_launch_cols<S, SG_VIEW_SLICE>(x, g, vec, tn, cv, hs);
  }
  if (q.axis == 2)
    return q.mode == SG_VIEW_MAX ? rv_launch_rows<S, SG_VIEW_MAX>(x, g, c == 1, tn, cv, hs)
                                 : rv_launch_rows<S, SG_VIEW_MEAN>(x, g, c == 1, tn, cv, hs);
  const bool vec = c == 1 && (q.w * (int64_t)sizeof(S)) % 16 == 0;
  return q.mode == SG_VIEW_MAX ? rv_launch_cols<S, SG_VIEW_MAX>(x, g, vec, tn, cv, hs)
                               : rv_launch_cols<S, SG_VIEW_MEAN>(x, g, vec, tn, cv, hs);
}

}  // namespace

extern "C" int sg_render_view(const void* x, sg_src_dtype dt, int64_t n, int64_t d, int64_t h, int64_t w, int32_t c, int32_t channel,
                              int32_t axis, int32_t mode, int64_t index, int32_t zoom_r, int32_t zoom_c, float scale, float shift,
                              float lo, float hi, float inv, uint8_t* canvas, int64_t canvas_h, int64_t canvas_w, int64_t r0,
                              int64_t c0, int32_t grid_cols, int64_t pitch_r, int64_t pitch_c, sg_stream_t st) {
  if (n < 0 || d < 0 || h < 0 || w < 0 || c < 1 || channel < 0 || channel >= c) return SG_EINVAL;
  if ((int)dt < (int)SG_SRC_U8 || (int)dt > (int)SG_SRC_BF16) return SG_EINVAL;
  if (axis < 0 || axis > 2 || mode < SG_VIEW_SLICE || mode > SG_VIEW_MEAN) return SG_EINVAL;
  if (zoom_r < 1 || zoom_c < 1 || grid_cols < 1) return SG_EINVAL;
  if (!isfinite(lo) || !isfinite(hi) || !isfinite(scale) || !(hi > lo)) return SG_EINVAL;
  if (canvas_h < 0 || canvas_w < 0 || r0 < 0 || c0 < 0 || pitch_r < 0 || pitch_c < 0) return SG_EINVAL;
  const int64_t extent = axis == 0 ? d : axis == 1 ? h : w;
  if (mode == SG_VIEW_SLICE && extent > 0 && (index < 0 || index >= extent)) return SG_EINVAL;
  if (n == 0 || d == 0 || h == 0 || w == 0) return SG_OK;
  if (!x || !canvas) return SG_EINVAL;
  // every tile inside the canvas, no two tiles on one pixel (128-bit products: nothing here can wrap)
  typedef __int128 i128;
  const i128 tile_h = (i128)(axis == 0 ? h : d) * zoom_r, tile_w = (i128)(axis == 2 ? h : w) * zoom_c;
  const int64_t tiles_down = (n - 1) / grid_cols + 1, tiles_across = n < grid_cols ? n : grid_cols;
  if ((i128)r0 + (i128)(tiles_down - 1) * pitch_r + tile_h > (i128)canvas_h) return SG_EINVAL;
  if ((i128)c0 + (i128)(tiles_across - 1) * pitch_c + tile_w > (i128)canvas_w) return SG_EINVAL;
  if ((tiles_down > 1 && (i128)pitch_r < tile_h) || (tiles_across > 1 && (i128)pitch_c < tile_w)) return SG_EINVAL;
  if ((i128)canvas_h * canvas_w > (i128)INT64_MAX) return SG_EINVAL;
  i128 elems = 1;      // (checked factor by factor: five 63-bit factors would wrap even 128 bits)
  for (int64_t f : {n, d, h, w, (int64_t)c}) {
    elems *= f;
    if (elems > (i128)INT64_MAX) return SG_EINVAL;
  }
  static const size_t esize[] = {1, 1, 2, 2, 2, 4, 2};
  if (((uintptr_t)x) % esize[(int)dt] != 0) return SG_EALIGN;
  const rv_tone tn = {scale, shift, lo, inv};
  const rv_canvas cv = {canvas, canvas_w, r0, c0, pitch_r, pitch_c, grid_cols, zoom_r, zoom_c};
  const rv_request q = {d, h, w, index, c, channel, axis, mode};
  hipStream_t hs = sg_st(st);
  switch (dt) {
    case SG_SRC_U8:   return rv_launch<uint8_t>(x, n, q, tn, cv, hs);
    case SG_SRC_I8:   return rv_launch<int8_t>(x, n, q, tn, cv, hs);
    case SG_SRC_I16:  return rv_launch<int16_t>(x, n, q, tn, cv, hs);
    case SG_SRC_U16:  return rv_launch<uint16_t>(x, n, q, tn, cv, hs);
    case SG_SRC_F16:  return rv_launch<_Float16>(x, n, q, tn, cv, hs);
    case SG_SRC_F32:  return rv_launch<float>(x, n, q, tn, cv, hs);
    case SG_SRC_BF16: return rv_launch<rv_bf16>(x, n, q, tn, cv, hs);
  }
  return SG_EINVAL;
}
