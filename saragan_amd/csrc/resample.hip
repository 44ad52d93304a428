// Resampling to a common voxel spacing (prepare_data.py --spacing): one launch turns a batch of source volumes
// x [n, sd, sh, sw] into y [n, od, oh, ow], separably, through one tap table per axis that the caller built on the host
// (table_ops.resample_taps): for every output index an `inside` flag and T taps (a source index and an f32 weight each).
//
// The definition is exact (tests compare with ==); include/saragan_hip.h states it operation by operation.  In short: an output
// voxel that is outside on any axis is the fill value; any other is the f64 sum over the d taps of wd * (the f64 sum over the h
// taps of wh * (the f64 sum over the w taps of ww * x)), every sum sequential in table order from 0.0, a tap of weight 0 skipped
// without reading its voxel; one rounding to f32, or rint and a clamp to the integer type.
//
// The scheme.  A block of 256 threads owns RS_TD x RS_TH x RS_TW = 4 x 4 x 64 output voxels: a wave is one output row segment (its
// lanes run along w, the contiguous axis of source and output), the block's four waves are four rows, and every thread walks
// the tile's four planes.  The block first copies its slice of the three tables into LDS (indices clamped to the extents on the
// way, so nothing outside x is read whatever the tables hold): after that the only global loads are the source voxels, and no
// load waits for a table entry that is itself a load away.  A thread then evaluates its voxels' taps itself: lanes read
// neighbouring source elements of one row, and rows that neighbouring outputs share are re-read through the vector L1 / L2, not
// staged (at a step of 1 or more along d and h -- the case this is built for -- nothing is shared).  Every output voxel has one
// writer; there are no atomics; every offset is 64-bit; source rows need only element alignment (every load is one element).
#include "common.h"
#include <math.h>
#include <limits.h>
#include <initializer_list>
#include <type_traits>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_TD = 4, RS_TH = 4, RS_TW = 64;
constexpr int RS_MAX_TAPS = SG_RESAMPLE_MAX_TAPS;

// (extents are at most 2^29, host-checked: coordinates are 32-bit, only linear offsets 64-bit)
struct rs_geom {
  int32_t sd, sh, sw, od, oh, ow;
  int32_t td, th, tw;                  // taps per axis
  uint32_t tiles_h, tiles_w, tiles;      // tiles: per sample
};

// a tap table of an axis with O outputs and T taps, tap-major: int32 [1 + 2 T][O] = inside, T rows of indices, T rows of weights
struct rs_tab {
  const int32_t* __restrict__ p;
  int64_t O;
  int T;
  __device__ __forceinline__ bool inside(int o) const { return p[o] != 0; }
  __device__ __forceinline__ int index(int k, int o) const { return p[(int64_t)(1 + k) * O + o]; }
  __device__ __forceinline__ float weight(int k, int o) const { return __int_as_float(p[(int64_t)(1 + T + k) * O + o]); }
};

__device__ __forceinline__ int rs_clampi(int i, int s) { return i < 0 ? 0 : i >= s ? s - 1 : i; }

// the stored value of an accumulator
template <typename O>
__device__ __forceinline__ O rs_store(double acc) {
  if constexpr (std::is_same_v<O, float>) {
    return (float)acc;      // one rounding
  } else {
    constexpr double lo = std::is_same_v<O, int16_t> ? -32768.0 : 0.0, hi = std::is_same_v<O, int16_t> ? 32767.0 : 65535.0;
    double r = rint(acc);      // ties to even
    r = r < lo ? lo : r;
    r = r > hi ? hi : r;
    return (O)(int32_t)r;
  }
}

// The taps of `count` output indices from o0 on into LDS, tap-major: idx / wgt [k * count + i], k < kt (kt >= T: the slots from T
// on, and every slot of an index past the axis's end, get weight 0), indices clamped to [0, S - 1]; ins[i]: the inside flags.
__device__ __forceinline__ void rs_stage(const rs_tab& t, int o0, int count, int kt, int S, int* __restrict__ idx,
                                         float* __restrict__ wgt, int* __restrict__ ins) {
  for (int e = threadIdx.x; e < kt * count; e += RS_THREADS) {
    const int k = e / count, i = e - k * count, o = o0 + i;
    const bool ok = k < t.T && o < (int)t.O;
    idx[e] = ok ? rs_clampi(t.index(k, o), S) : 0;
    wgt[e] = ok ? t.weight(k, o) : 0.0f;
  }
  for (int i = threadIdx.x; i < count; i += RS_THREADS) ins[i] = o0 + i < (int)t.O && t.inside(o0 + i);
}

__device__ __forceinline__ int rs_uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float rs_uni(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// One thread computes the RS_TD voxels (o_d, o_h, o_w) of its tile column side by side, so that their loads are in flight together:
// per tap (i, j, k) the RS_TD planes' voxels are loaded before the first of them is summed; each voxel keeps its own accumulators,
// and its sums run in table order.  The d and h taps of a wave are the same in every lane (a wave is one output row): they are
// held in scalar registers, and a tap of weight 0 is a scalar branch around everything behind it.  The w taps differ from lane
// to lane: a tap whose weight is 0 in every lane is skipped, one whose weight is 0 in no lane runs unpredicated, and only a
// mixed tap pays for lane masks.
template <typename S, typename O>
__global__ __launch_bounds__(RS_THREADS) void resample_kernel(const S* __restrict__ x, rs_geom g, const int32_t* __restrict__ tab_d,
                                                              const int32_t* __restrict__ tab_h, const int32_t* __restrict__ tab_w,
                                                              double fill, O* __restrict__ y) {
  __shared__ int s_id[RS_TD * RS_MAX_TAPS], s_ih[RS_TH * RS_MAX_TAPS], s_iw[RS_TW * RS_MAX_TAPS];
  __shared__ float s_wd[RS_TD * RS_MAX_TAPS], s_wh[RS_TH * RS_MAX_TAPS], s_ww[RS_TW * RS_MAX_TAPS];
  __shared__ int s_in_d[RS_TD], s_in_h[RS_TH], s_in_w[RS_TW];

  const uint32_t sample32 = blockIdx.x / g.tiles, t = blockIdx.x - sample32 * g.tiles;
  const int64_t sample = sample32;
  const uint32_t tq = t / g.tiles_w, tqq = tq / g.tiles_h;
  const int W0 = (int)(t - tq * g.tiles_w) * RS_TW, H0 = (int)(tq - tqq * g.tiles_h) * RS_TH, D0 = (int)tqq * RS_TD;
  const int lw = (int)(threadIdx.x % RS_TW), lh = rs_uni((int)(threadIdx.x / RS_TW));      // lh: one per wave
  const int o_w = W0 + lw, o_h = H0 + lh;
  const rs_tab td{tab_d, g.od, g.td}, th{tab_h, g.oh, g.th}, tw{tab_w, g.ow, g.tw};
  const bool has_source = g.sd > 0 && g.sh > 0 && g.sw > 0;
  const int nd = g.td, nh = g.th, nw = g.tw;
  if (has_source) {
    rs_stage(td, D0, RS_TD, nd, g.sd, s_id, s_wd, s_in_d);
    rs_stage(th, H0, RS_TH, nh, g.sh, s_ih, s_wh, s_in_h);
    rs_stage(tw, W0, RS_TW, nw, g.sw, s_iw, s_ww, s_in_w);
  }
  __syncthreads();
  if (o_w >= g.ow || o_h >= g.oh) return;      // (no barrier follows)
  const uint64_t lanes = __ballot(1);           // the lanes that are left
  const bool row_in = has_source && rs_uni(s_in_h[lh]) != 0;      // (uniform)
  const bool in_w = s_in_w[lw] != 0;
  const S* __restrict__ xs = x + sample * g.sd * g.sh * g.sw;
  const int64_t plane_elems = (int64_t)g.sh * g.sw;
  bool rowd[RS_TD];      // (uniform) the plane exists and is inside along d and h
  double acc[RS_TD];
#pragma unroll
  for (int ld = 0; ld < RS_TD; ++ld) {
    rowd[ld] = row_in && D0 + ld < g.od && rs_uni(s_in_d[ld]) != 0;
    acc[ld] = 0.0;
  }
#pragma unroll 1
  for (int i = 0; i < nd; ++i) {
    float wd[RS_TD];
    bool on[RS_TD], any = false;
    const S* __restrict__ plane[RS_TD];
    double mid[RS_TD];
#pragma unroll
    for (int ld = 0; ld < RS_TD; ++ld) {
      wd[ld] = rs_uni(s_wd[i * RS_TD + ld]);
      on[ld] = rowd[ld] && wd[ld] != 0.0f;
      any = any || on[ld];
      plane[ld] = xs + (int64_t)rs_uni(s_id[i * RS_TD + ld]) * plane_elems;
      mid[ld] = 0.0;
    }
    if (!any) continue;
#pragma unroll 1
    for (int j = 0; j < nh; ++j) {
      const float wh = rs_uni(s_wh[j * RS_TH + lh]);
      if (wh == 0.0f) continue;
      const int64_t row = (int64_t)rs_uni(s_ih[j * RS_TH + lh]) * g.sw;
      double inner[RS_TD];
#pragma unroll
      for (int ld = 0; ld < RS_TD; ++ld) inner[ld] = 0.0;
#pragma unroll 1
      for (int k = 0; k < nw; ++k) {
        const float ww = s_ww[k * RS_TW + lw];
        const uint64_t nz = __ballot(ww != 0.0f);
        if (nz == 0) continue;
        const int64_t at = row + s_iw[k * RS_TW + lw];
        S raw[RS_TD];
        if (nz == lanes) {
#pragma unroll
          for (int ld = 0; ld < RS_TD; ++ld)
            if (on[ld]) raw[ld] = plane[ld][at];
#pragma unroll
          for (int ld = 0; ld < RS_TD; ++ld)
            if (on[ld]) inner[ld] = inner[ld] + (double)ww * (double)raw[ld];
        } else {
#pragma unroll
          for (int ld = 0; ld < RS_TD; ++ld) {
            raw[ld] = S(0);
            if (on[ld] && ww != 0.0f) raw[ld] = plane[ld][at];
          }
#pragma unroll
          for (int ld = 0; ld < RS_TD; ++ld)
            if (on[ld]) inner[ld] = ww != 0.0f ? inner[ld] + (double)ww * (double)raw[ld] : inner[ld];
        }
      }
#pragma unroll
      for (int ld = 0; ld < RS_TD; ++ld)
        if (on[ld]) mid[ld] = mid[ld] + (double)wh * inner[ld];
    }
#pragma unroll
    for (int ld = 0; ld < RS_TD; ++ld)
      if (on[ld]) acc[ld] = acc[ld] + (double)wd[ld] * mid[ld];
  }
  const O filled = rs_store<O>(fill);
#pragma unroll
  for (int ld = 0; ld < RS_TD; ++ld)
    if (D0 + ld < g.od) y[((sample * g.od + (D0 + ld)) * g.oh + o_h) * g.ow + o_w] = rowd[ld] && in_w ? rs_store<O>(acc[ld]) : filled;
}

struct rs_args {
  int64_t n;
  rs_geom g;
  const int32_t *tab_d, *tab_h, *tab_w;
  double fill;
  void* y;
};

template <typename S, typename O>
int rs_launch2(const void* x, const rs_args& q, hipStream_t hs) {
  const dim3 grid((unsigned)(q.n * q.g.tiles)), block(RS_THREADS);
  hipLaunchKernelGGL((resample_kernel<S, O>), grid, block, 0, hs, (const S*)x, q.g, q.tab_d, q.tab_h, q.tab_w, q.fill, (O*)q.y);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

template <typename S>
int rs_launch(const void* x, sg_src_dtype odt, const rs_args& q, hipStream_t hs) {
  if constexpr (std::is_integral_v<S>) {
    if (odt == SG_SRC_U16) return rs_launch2<S, uint16_t>(x, q, hs);
    if (odt == SG_SRC_I16) return rs_launch2<S, int16_t>(x, q, hs);
  }
  return rs_launch2<S, float>(x, q, hs);
}

}  // namespace

extern "C" int sg_resample_axes(const void* x, sg_src_dtype dt, int64_t n, int64_t sd, int64_t sh, int64_t sw, int64_t od, int64_t oh,
                                int64_t ow, const int32_t* tab_d, int32_t taps_d, const int32_t* tab_h, int32_t taps_h,
                                const int32_t* tab_w, int32_t taps_w, int32_t fill_i, float fill_f, sg_src_dtype out_dt, void* y,
                                sg_stream_t st) {
  if (n < 0 || sd < 0 || sh < 0 || sw < 0 || od < 0 || oh < 0 || ow < 0) return SG_EINVAL;
  for (int32_t t : {taps_d, taps_h, taps_w})
    if (t < 1 || t > RS_MAX_TAPS) return SG_EINVAL;
  if ((int)dt < (int)SG_SRC_U8 || (int)dt > (int)SG_SRC_F32) return SG_EINVAL;      // (bf16: not a source here)
  if (out_dt != SG_SRC_U16 && out_dt != SG_SRC_I16 && out_dt != SG_SRC_F32) return SG_EINVAL;
  const bool is_int = dt == SG_SRC_U8 || dt == SG_SRC_I8 || dt == SG_SRC_I16 || dt == SG_SRC_U16;
  if (!is_int && out_dt != SG_SRC_F32) return SG_EINVAL;
  const int64_t big = (int64_t)1 << 29;      // extents that are 32-bit coordinates in the kernel
  for (int64_t v : {sd, sh, sw, od, oh, ow})
    if (v > big) return SG_EINVAL;
  typedef __int128 i128;
  if ((i128)n * sd * sh * sw > (i128)INT64_MAX / 8 || (i128)n * od * oh * ow > (i128)INT64_MAX / 8) return SG_EINVAL;
  if (n == 0 || od == 0 || oh == 0 || ow == 0) return SG_OK;
  if (!y || !tab_d || !tab_h || !tab_w) return SG_EINVAL;
  const bool has_source = sd > 0 && sh > 0 && sw > 0;
  if (has_source && !x) return SG_EINVAL;
  static const size_t esize[] = {1, 1, 2, 2, 2, 4};
  if (x && ((uintptr_t)x) % esize[(int)dt] != 0) return SG_EALIGN;
  if (((uintptr_t)y) % (out_dt == SG_SRC_F32 ? 4 : 2) != 0) return SG_EALIGN;
  for (const int32_t* t : {tab_d, tab_h, tab_w})
    if (((uintptr_t)t) % 4 != 0) return SG_EALIGN;
  rs_args q;
  q.n = n;
  q.g.sd = (int32_t)sd; q.g.sh = (int32_t)sh; q.g.sw = (int32_t)sw; q.g.od = (int32_t)od; q.g.oh = (int32_t)oh; q.g.ow = (int32_t)ow;
  q.g.td = taps_d; q.g.th = taps_h; q.g.tw = taps_w;
  const int64_t tiles_d = (od + RS_TD - 1) / RS_TD, tiles_h = (oh + RS_TH - 1) / RS_TH, tiles_w = (ow + RS_TW - 1) / RS_TW;
  const int64_t tiles = tiles_d * tiles_h * tiles_w;
  if (tiles > (int64_t)INT32_MAX || n * tiles > (int64_t)INT32_MAX) return SG_EINVAL;
  q.g.tiles_h = (uint32_t)tiles_h; q.g.tiles_w = (uint32_t)tiles_w; q.g.tiles = (uint32_t)tiles;
  q.tab_d = tab_d; q.tab_h = tab_h; q.tab_w = tab_w;
  q.fill = is_int ? (double)fill_i : (double)fill_f;
  q.y = y;
  hipStream_t hs = sg_st(st);
  switch (dt) {
    case SG_SRC_U8:  return rs_launch<uint8_t>(x, out_dt, q, hs);
    case SG_SRC_I8:  return rs_launch<int8_t>(x, out_dt, q, hs);
    case SG_SRC_I16: return rs_launch<int16_t>(x, out_dt, q, hs);
    case SG_SRC_U16: return rs_launch<uint16_t>(x, out_dt, q, hs);
    case SG_SRC_F16: return rs_launch<_Float16>(x, out_dt, q, hs);
    case SG_SRC_F32: return rs_launch<float>(x, out_dt, q, hs);
    default: break;
  }
  return SG_EINVAL;
}
