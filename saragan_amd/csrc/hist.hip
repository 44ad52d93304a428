// Voxel-intensity histograms: out[row][col] += the number of elements of row `row` whose value, mapped to data
// units, falls into unit-wide bin `col` of [lo, lo + bins].  x [rows, row_elems] of any sg_src_dtype, row-major, contiguous.
//
// The definition is exact (tests compare with ==).  Per element, in f32:
//   t   = x * scale + shift        two correctly rounded operations (__fmul_rn, __fadd_rn; the file is built with
//                                  -ffp-contract=off as well): the bits of numpy's x * np.float32(scale) + np.float32(shift)
//   t is NaN         -> column `bins` (the extra column)
//   t >= lo + bins   -> column bins - 1  (saturated; the top edge is closed, so hi - 1 and hi share the last bin)
//   t <  lo          -> column 0         (saturated)
//   otherwise        -> min(floor(t) - lo, bins - 1)
// The saturation is decided on the FLOAT, before any conversion: t is clamped to [flo, fhi], the largest f32 <= lo and the
// smallest f32 >= lo + bins (for an f32 t and an integer k, t >= k  <=>  t >= the smallest f32 >= k).  +-inf saturate.  What is
// converted then has its floor in [flo, fhi], inside the int32 range (the host refuses lo + bins above the largest int32 an
// f32 holds), and the column is clamped to [0, bins - 1] as an integer.
//
// The pass reads the input once: its roof is the HBM read rate.  A block takes one (row, chunk of the row) at a time: it
// zeroes a u32 image of the histogram in LDS, counts its chunk into it, and adds the non-zero counts to `out` with 64-bit
// global atomics -- integer sums, so the result does not depend on the order and two calls give the same tensor.  A chunk has
// at most 2^30 elements, so no u32 of the image can wrap between two flushes.
//
// Contention (CT volumes put half their voxels into the air bin, and neighbours are alike):
//   * a lane reads 16 bytes of consecutive elements per load and keeps (last column, count) in registers: a run of equal
//     columns costs ONE LDS atomic when it ends, however long it is, also across the lane's loads.  A volume that sits in one
//     bin issues two LDS atomics per lane per chunk (the empty run it starts with, and the one it ends with).
//   * where the image is small, the LDS holds `copies` (a power of two, <= 32) lane-interleaved replicas of it, image word
//     col * copies + (lane % copies): lanes that do hit one column in one instruction land on `copies` different banks.
//   Worst case: columns that alternate element by element with bins > HG_WORDS / 2 - 1 (one copy) -- every element is an LDS
//   atomic and the 64 lanes of an instruction share two addresses.
#include "common.h"
#include <math.h>

namespace {

constexpr int HG_THREADS = 256;
constexpr int HG_WORDS = 8192;                   // u32 words of LDS per block (32 KiB: four blocks of a CU fit its 160 KiB)
constexpr int HG_MAX_BINS = HG_WORDS - 1;        // one image of bins + 1 columns
constexpr int HG_MAX_COPIES = 32;                // one replica per bank of a ds atomic
constexpr int HG_UNROLL = 4;                     // 16-byte loads in flight per lane
constexpr int64_t HG_MAX_CHUNK = (int64_t)1 << 30;
constexpr int64_t HG_MAX_HI = 2147483520;       // the largest int32 that an f32 holds: lo + bins may not pass it

struct hg_map {
  float scale, shift, flo, fhi;      // flo: the largest f32 <= lo; fhi: the smallest f32 >= lo + bins
  int32_t lo, bins;
};

template <typename S>
__device__ __forceinline__ float hg_to_f(S v) { return (float)v; }      // exact for every source type
struct hg_bf16 { uint16_t bits; };                                      // bf16 is the upper half of an f32
template <>
__device__ __forceinline__ float hg_to_f<hg_bf16>(hg_bf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }

// Branch-free (nine vector operations): the float is clamped to [flo, fhi] first -- a float comparison, +-inf included -- so
// the conversion sees a value whose floor fits an int32 and whose distance from lo fits one too; then the column is clamped.
// t < lo ends at or under 0 (flo <= t < lo: floor(t) - lo < 0; t < flo: flo - lo <= 0) and t >= lo + bins, which is t >= fhi, at
// fhi - lo >= bins.
__device__ __forceinline__ int hg_column(float x, const hg_map& m) {
  const float t = __fadd_rn(__fmul_rn(x, m.scale), m.shift);
  const int c = (int)floorf(__builtin_amdgcn_fmed3f(t, m.flo, m.fhi)) - m.lo;
  const int col = max(min(c, m.bins - 1), 0);
  return t != t ? m.bins : col;
}

// the lane's open run: `cnt` elements that are not in LDS yet, of the column whose word in the lane's replica is `word`
// (word = (col << lg) + copy, lg = log2(copies): runs are compared by their word, which the atomic then needs anyway)
struct hg_run {
  int word;
  uint32_t cnt;
};

__device__ __forceinline__ void hg_count(hg_run& r, int col, uint32_t* img, int lg, int copy) {
  const int word = (col << lg) + copy;
  const bool change = word != r.word;
  if (change) atomicAdd(&img[r.word], r.cnt);      // (the first run of a lane closes an empty one: it adds 0)
  r.cnt = change ? 1u : r.cnt + 1u;
  r.word = word;
}

template <typename S>
__global__ __launch_bounds__(HG_THREADS) void intensity_hist_kernel(const S* __restrict__ x, int64_t rows, int64_t row_elems,
                                                                    int64_t chunk, hg_map m, int lg,
                                                                    unsigned long long* __restrict__ out) {
  constexpr int E = 16 / (int)sizeof(S);      // elements of one 16-byte load
  __shared__ uint32_t img[HG_WORDS];
  const int tid = threadIdx.x, nb = m.bins + 1, copies = 1 << lg, words = nb << lg, copy = tid & (copies - 1);
  const int64_t e0 = (int64_t)blockIdx.x * chunk;      // the block's chunk of every row it visits
  const int64_t len = row_elems - e0 < chunk ? row_elems - e0 : chunk;
  for (int64_t row = blockIdx.y; row < rows; row += gridDim.y) {
    for (int i = tid; i < words; i += HG_THREADS) img[i] = 0u;
    __syncthreads();
    const S* __restrict__ src = x + row * row_elems + e0;
    // elements in front of the first 16-byte boundary (rows start misaligned when row_elems is odd), whole loads, the rest
    int64_t head = (int64_t)(((16u - (uint32_t)((uintptr_t)src & 15u)) & 15u) / (uint32_t)sizeof(S));
    if (head > len) head = len;
    const int64_t pieces = (len - head) / E, tail0 = head + pieces * E;
    if (tid < head) atomicAdd(&img[(hg_column(hg_to_f(src[tid]), m) << lg) + copy], 1u);
    if (tail0 + tid < len) atomicAdd(&img[(hg_column(hg_to_f(src[tail0 + tid]), m) << lg) + copy], 1u);
    const u32x4* __restrict__ vsrc = reinterpret_cast<const u32x4*>(src + head);
    hg_run run = {copy, 0u};
    for (int64_t p = tid; p < pieces; p += (int64_t)HG_THREADS * HG_UNROLL) {
      u32x4 raw[HG_UNROLL];
#pragma unroll
      for (int j = 0; j < HG_UNROLL; ++j)
        if (p + (int64_t)j * HG_THREADS < pieces) raw[j] = vsrc[p + (int64_t)j * HG_THREADS];
#pragma unroll
      for (int j = 0; j < HG_UNROLL; ++j) {
        if (p + (int64_t)j * HG_THREADS < pieces) {
          const S* s = reinterpret_cast<const S*>(&raw[j]);
#pragma unroll
          for (int e = 0; e < E; ++e) hg_count(run, hg_column(hg_to_f(s[e]), m), img, lg, copy);
        }
      }
    }
    atomicAdd(&img[run.word], run.cnt);
    __syncthreads();
    unsigned long long* __restrict__ dst = out + row * (int64_t)nb;
    for (int b = tid; b < nb; b += HG_THREADS) {
      uint32_t sum = 0u;      // (the replicas of a column sum to at most the chunk's 2^30 elements)
      for (int c = 0; c < copies; ++c) sum += img[(b << lg) + c];
      if (sum) atomicAdd(&dst[b], (unsigned long long)sum);
    }
    __syncthreads();      // the image is zeroed again for the next row
  }
}

// the smallest f32 that is >= k, the largest that is <= k
float hg_f32_at_least(int64_t k) {
  float f = (float)k;
  if ((double)f < (double)k) f = nextafterf(f, INFINITY);
  return f;
}
float hg_f32_at_most(int64_t k) {
  float f = (float)k;
  if ((double)f > (double)k) f = nextafterf(f, -INFINITY);
  return f;
}

template <typename S>
int hg_launch(const void* x, int64_t rows, int64_t row_elems, const hg_map& m, int64_t* out, hipStream_t hs) {
  if (((uintptr_t)x) % sizeof(S) != 0) return SG_EALIGN;
  constexpr int64_t E = 16 / (int64_t)sizeof(S);
  const int nb = m.bins + 1;
  int lg = 0;      // log2 of the replicas that fit
  while ((2 << lg) <= HG_MAX_COPIES && (2 << lg) * nb <= HG_WORDS) ++lg;
  // rows x chunks blocks: about eight per CU, a chunk no shorter than four rounds of the block's loads (zeroing and flushing
  // the image is paid per chunk) and no longer than 2^30 elements
  const int64_t round = (int64_t)HG_THREADS * HG_UNROLL * E;
  const int64_t gy = rows < 65535 ? rows : 65535;
  int64_t per_row = (2048 + gy - 1) / gy;
  const int64_t most = (row_elems + 4 * round - 1) / (4 * round);
  if (per_row > most) per_row = most;
  if (per_row < 1) per_row = 1;
  int64_t chunk = (row_elems + per_row - 1) / per_row;
  chunk = (chunk + round - 1) / round * round;
  if (chunk > HG_MAX_CHUNK) chunk = HG_MAX_CHUNK;
  const int64_t gx = (row_elems + chunk - 1) / chunk;
  if (gx > 0x7FFFFFFF) return SG_EINVAL;
  hipLaunchKernelGGL((intensity_hist_kernel<S>), dim3((unsigned)gx, (unsigned)gy), dim3(HG_THREADS), 0, hs, (const S*)x, rows,
                     row_elems, chunk, m, lg, reinterpret_cast<unsigned long long*>(out));
  SG_LAUNCH_CHECK();
  return SG_OK;
}

}  // namespace

extern "C" int32_t sg_intensity_hist_max_bins(void) { return HG_MAX_BINS; }

extern "C" int sg_intensity_hist(const void* x, sg_src_dtype dt, int64_t rows, int64_t row_elems, float scale, float shift,
                                 int32_t lo, int32_t bins, int64_t* out, int accumulate, sg_stream_t st) {
  if (rows < 0 || row_elems < 0 || bins < 1 || bins > HG_MAX_BINS || !isfinite(scale)) return SG_EINVAL;
  if ((int)dt < (int)SG_SRC_U8 || (int)dt > (int)SG_SRC_BF16) return SG_EINVAL;
  if ((int64_t)lo + bins > HG_MAX_HI) return SG_EINVAL;
  if (rows == 0) return SG_OK;
  if (!out || (row_elems > 0 && !x)) return SG_EINVAL;
  if (((uintptr_t)out) % 8 != 0) return SG_EALIGN;
  hipStream_t hs = sg_st(st);
  if (!accumulate) {
    hipError_t e = hipMemsetAsync(out, 0, (size_t)rows * (size_t)(bins + 1) * sizeof(int64_t), hs);
    if (e != hipSuccess) return (int)e;
  }
  if (row_elems == 0) return SG_OK;
  hg_map m;
  m.scale = scale; m.shift = shift; m.lo = lo; m.bins = bins;
  m.flo = hg_f32_at_most(lo);
  m.fhi = hg_f32_at_least((int64_t)lo + bins);
  switch (dt) {
    case SG_SRC_U8:   return hg_launch<uint8_t>(x, rows, row_elems, m, out, hs);
    case SG_SRC_I8:   return hg_launch<int8_t>(x, rows, row_elems, m, out, hs);
    case SG_SRC_I16:  return hg_launch<int16_t>(x, rows, row_elems, m, out, hs);
    case SG_SRC_U16:  return hg_launch<uint16_t>(x, rows, row_elems, m, out, hs);
    case SG_SRC_F16:  return hg_launch<_Float16>(x, rows, row_elems, m, out, hs);
    case SG_SRC_F32:  return hg_launch<float>(x, rows, row_elems, m, out, hs);
    case SG_SRC_BF16: return hg_launch<hg_bf16>(x, rows, row_elems, m, out, hs);
  }
  return SG_EINVAL;
}
