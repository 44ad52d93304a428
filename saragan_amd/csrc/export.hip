// Typed volumes from the generator's output (generate.py): the mirror image of sg_gather_rows.  One pass reads a
// batch x [n, c, d, h, w] (f32 / bf16 / f16; NCDHW-contiguous or channels-last) once, maps it back to data units, clips, rounds,
// casts and writes out [n, c, d, h, w] contiguous (i16 / u16 / u8 / f32), and sums every sample's statistics on the way.
//
// The definition is exact (tests compare with ==); include/saragan_hip.h states it operation by operation.  Per element, in f32:
//   t      = x * scale + shift      two correctly rounded operations (__fmul_rn, __fadd_rn; the file is built with
//                                   -ffp-contract=off as well): the bits of numpy's x * np.float32(scale) + np.float32(shift)
//   nan, below, above               t != t, t < lo, t > hi: float comparisons, made before any conversion
//   u      = nan or below ? lo : above ? hi : t
//   stored = T(trunc(u)) or T(rint(u)) for an integer T (lo and hi are integers of T: the conversion cannot overflow);
//            nan ? the quiet NaN 0x7FC00000 : u for f32.
//
// The pass reads 2 or 4 bytes and writes 1, 2 or 4 per element: its roof is the HBM rate.  Two kernels, chosen per launch on the
// host.  The PIECE kernel: a sample's c * v elements are one contiguous row of both tensors (NCDHW, or one channel); a lane takes
// pieces of E = 16 / min(element sizes) consecutive elements, so that its loads AND its stores are whole 16-byte accesses.  It needs
// a row length that is a multiple of E and one `head` < E at which source and output are both 16-byte aligned: then every row
// starts with the same `head` elements by element, continues in aligned pieces and ends with E - head elements by element.  The
// ELEMENT kernel: one voxel per lane and a loop over the channels; any alignment, any row length, and the transposition of a
// channels-last source (consecutive lanes read consecutive voxels' channel groups and write c coalesced rows).
//
// The statistics are integers: summed per lane (a piece's sum in 32 bits, its squares in one multiply-add each), per wave by lane
// exchanges, per block in LDS, then ONE 64-bit integer atomic per (block, row, statistic) -- exact and independent of the order,
// so two calls give the same bits.
#include "common.h"
#include <math.h>
#include <limits.h>
#include <type_traits>

namespace {

constexpr int SV_WAVE = 64;
// blocks of 256 lanes, about sixteen per CU, share the rows between them.  With statistics every block ends each of its rows with
// up to seven atomics on ONE 56-byte record, and atomics on one cache line are served one after the other (measured: 7-10 ns
// each; 4096 blocks of 256 lanes added 40 us to an 11 us pass): then the same lanes come as 512 blocks of 1024.
constexpr int SV_THREADS = 256, SV_BLOCKS = 4096;
constexpr int SV_THREADS_STATS = 1024, SV_BLOCKS_STATS = 512;

struct sv_bf16 { uint16_t bits; };      // bf16 is the upper half of an f32

template <typename S>
__device__ __forceinline__ float sv_to_f(S v) { return (float)v; }      // exact
template <>
__device__ __forceinline__ float sv_to_f<sv_bf16>(sv_bf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }

struct sv_map {
  float scale, shift, lo, hi;
  int32_t rint;      // 0: trunc, 1: rint (ties to even)
};

// a lane's statistics; the counts of a whole row fit 64 bits, a piece's fit 32
struct sv_stat {
  int64_t s, ss, below, above, nan;
  int32_t mn, mx;
  __device__ __forceinline__ void clear() { s = 0; ss = 0; below = 0; above = 0; nan = 0; mn = INT32_MAX; mx = INT32_MIN; }
};

// the stored value of x; the three flags are added to the counters given
template <typename T>
__device__ __forceinline__ T sv_value(float x, const sv_map& m, int32_t& below, int32_t& above, int32_t& nan) {
  const float t = __fadd_rn(__fmul_rn(x, m.scale), m.shift);
  const bool isn = t != t, b = t < m.lo, a = t > m.hi;
  below += b ? 1 : 0;
  above += a ? 1 : 0;
  nan += isn ? 1 : 0;
  const float u = (isn || b) ? m.lo : a ? m.hi : t;
  if constexpr (std::is_same_v<T, float>) {
    return isn ? __uint_as_float(0x7FC00000u) : u;
  } else {
    const float r = m.rint ? rintf(u) : truncf(u);
    return (T)(int32_t)r;      // lo <= r <= hi, integers of T
  }
}

template <typename T>
__device__ __forceinline__ void sv_add(sv_stat& a, T q) {
  if constexpr (!std::is_same_v<T, float>) {
    const int32_t v = (int32_t)q;
    a.s += v;
    a.ss += (int64_t)v * v;
    a.mn = v < a.mn ? v : a.mn;
    a.mx = v > a.mx ? v : a.mx;
  }
}

// every lane of the wave calls; lane 0 adds the wave's totals to the block's LDS slots
template <bool INT>
__device__ __forceinline__ void sv_wave_to_lds(sv_stat a, int64_t* slot) {
#pragma unroll
  for (int m = SV_WAVE / 2; m >= 1; m >>= 1) {
    if constexpr (INT) {
      a.s += __shfl_xor(a.s, m, SV_WAVE);
      a.ss += __shfl_xor(a.ss, m, SV_WAVE);
      const int32_t on = __shfl_xor(a.mn, m, SV_WAVE), ox = __shfl_xor(a.mx, m, SV_WAVE);
      a.mn = on < a.mn ? on : a.mn;
      a.mx = ox > a.mx ? ox : a.mx;
    }
    a.below += __shfl_xor(a.below, m, SV_WAVE);
    a.above += __shfl_xor(a.above, m, SV_WAVE);
    a.nan += __shfl_xor(a.nan, m, SV_WAVE);
  }
  if (threadIdx.x % SV_WAVE == 0) {
    if constexpr (INT) {
      __hip_atomic_fetch_add(slot + 0, a.s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_add(slot + 1, a.ss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_min(slot + 2, (int64_t)a.mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      __hip_atomic_fetch_max(slot + 3, (int64_t)a.mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __hip_atomic_fetch_add(slot + 4, a.below, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(slot + 5, a.above, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(slot + 6, a.nan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

__device__ __forceinline__ int64_t sv_identity(int k, bool is_int) { return !is_int ? 0 : k == 2 ? INT64_MAX : k == 3 ? INT64_MIN : 0; }

// the block's row statistics: cleared, summed per wave, flushed with one global atomic per statistic (block-uniform calls)
template <bool INT>
__device__ __forceinline__ void sv_block_flush(const sv_stat& a, int64_t* st, int64_t* __restrict__ dst) {
  const int tid = threadIdx.x;
  if (tid < 7) st[tid] = sv_identity(tid, INT);
  __syncthreads();
  sv_wave_to_lds<INT>(a, st);
  __syncthreads();
  if (tid < 7) {
    const int64_t v = st[tid];
    if (INT && tid == 2) __hip_atomic_fetch_min(dst + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (INT && tid == 3) __hip_atomic_fetch_max(dst + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if ((INT || tid >= 4) && v != 0) __hip_atomic_fetch_add(dst + tid, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // (a sum of 0 adds nothing)
  }
  __syncthreads();      // the slots are cleared again for the block's next row
}

__global__ void store_stats_init_kernel(int64_t* stats, int64_t n, int is_int) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n * 7) stats[i] = sv_identity((int)(i % 7), is_int != 0);
}

// ---- whole 16-byte loads and stores: rows of `row` = c * v elements, row % E == 0, both tensors 16-byte aligned at `head`
template <typename S, typename T>
__global__ __launch_bounds__(SV_THREADS_STATS) void store_volumes_piece_kernel(const S* __restrict__ x, T* __restrict__ out, int64_t n,
                                                                         int64_t row, int head, sv_map m,
                                                                         int64_t* __restrict__ stats) {
  constexpr int ES = 16 / (int)sizeof(S), ET = 16 / (int)sizeof(T), E = ES > ET ? ES : ET;      // elements of a piece
  constexpr int NL = E / ES, NS = E / ET;                                                       // its 16-byte loads and stores
  constexpr int U = 32 / (E * (int)sizeof(S)) > 1 ? 32 / (E * (int)sizeof(S)) : 1;              // pieces in flight: 32 bytes of loads
  constexpr bool INT = !std::is_same_v<T, float>;
  __shared__ int64_t st[8];
  const int tid = threadIdx.x;
  // with a head the row's last piece is cut in two: `head` elements in front, E - head behind
  const int64_t pieces = head ? row / E - 1 : row / E, tail0 = (int64_t)head + pieces * E;
  const int tail = (int)(row - tail0);
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
    const S* __restrict__ src = x + i * row;
    T* __restrict__ dst = out + i * row;
    sv_stat a;
    a.clear();
    if (blockIdx.x == 0 && tid < head + tail) {      // the elements outside the aligned run
      const int64_t e = tid < head ? (int64_t)tid : tail0 + (tid - head);
      int32_t pb = 0, pa = 0, pn = 0;
      const T q = sv_value<T>(sv_to_f(src[e]), m, pb, pa, pn);
      dst[e] = q;
      sv_add<T>(a, q);
      a.below += pb; a.above += pa; a.nan += pn;
    }
    const u32x4* __restrict__ vsrc = reinterpret_cast<const u32x4*>(src + head);
    u32x4* __restrict__ vdst = reinterpret_cast<u32x4*>(dst + head);
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + tid; p < pieces; p += step * U) {
      u32x4 raw[U][NL];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if (p + j * step < pieces) {
#pragma unroll
          for (int k = 0; k < NL; ++k) raw[j][k] = vsrc[(p + j * step) * NL + k];
        }
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
        if (p + j * step < pieces) {
          const S* s = reinterpret_cast<const S*>(&raw[j][0]);
          T q[E];
          int32_t pb = 0, pa = 0, pn = 0;
#pragma unroll
          for (int e = 0; e < E; ++e) q[e] = sv_value<T>(sv_to_f(s[e]), m, pb, pa, pn);
          if constexpr (INT) {      // a piece's sum fits 32 bits (16 * 65535), its squares one multiply-add each
            int32_t ps = 0;
            uint64_t pss = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const int32_t v = (int32_t)q[e];
              const uint32_t mag = (uint32_t)(v < 0 ? -v : v);
              ps += v;
              pss = (uint64_t)mag * mag + pss;
              a.mn = v < a.mn ? v : a.mn;
              a.mx = v > a.mx ? v : a.mx;
            }
            a.s += ps;
            a.ss += (int64_t)pss;
          }
          a.below += pb; a.above += pa; a.nan += pn;
#pragma unroll
          for (int k = 0; k < NS; ++k) {
            u32x4 w;
            __builtin_memcpy(&w, reinterpret_cast<const char*>(q) + 16 * k, 16);
            vdst[(p + j * step) * NS + k] = w;
            SG_STORE16_GUARD(w);
          }
        }
      }
    }
    if (stats) sv_block_flush<INT>(a, st, stats + i * 7);      // (uniform)
  }
}

// ---- one voxel per lane, a loop over the channels: any alignment, any length, and the transposition of a channels-last source
template <typename S, typename T>
__global__ __launch_bounds__(SV_THREADS_STATS) void store_volumes_elem_kernel(const S* __restrict__ x, T* __restrict__ out, int64_t n,
                                                                        int64_t c, int64_t v, int channels_last, sv_map m,
                                                                        int64_t* __restrict__ stats) {
  constexpr bool INT = !std::is_same_v<T, float>;
  __shared__ int64_t st[8];
  const int64_t e0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (int64_t)gridDim.x * blockDim.x;
  // the source's strides between the voxels and between the channels of a sample
  const int64_t sv = channels_last ? c : 1, sc = channels_last ? 1 : v;
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
    const S* __restrict__ src = x + i * c * v;
    T* __restrict__ dst = out + i * c * v;
    sv_stat a;
    a.clear();
    for (int64_t e = e0; e < v; e += step) {
      for (int64_t ch = 0; ch < c; ++ch) {
        int32_t pb = 0, pa = 0, pn = 0;
        const T q = sv_value<T>(sv_to_f(src[e * sv + ch * sc]), m, pb, pa, pn);
        dst[ch * v + e] = q;
        sv_add<T>(a, q);
        a.below += pb; a.above += pa; a.nan += pn;
      }
    }
    if (stats) sv_block_flush<INT>(a, st, stats + i * 7);      // (uniform)
  }
}

struct sv_args {
  const void* x;
  void* out;
  int64_t n, c, v;
  int channels_last;
  sv_map m;
  int64_t* stats;
};

template <typename S, typename T>
int sv_launch(const sv_args& q, hipStream_t hs) {
  constexpr int64_t ES = 16 / (int64_t)sizeof(S), ET = 16 / (int64_t)sizeof(T), E = ES > ET ? ES : ET;
  if (((uintptr_t)q.x) % sizeof(S) != 0 || ((uintptr_t)q.out) % sizeof(T) != 0) return SG_EALIGN;
  if (q.stats) {
    hipLaunchKernelGGL(store_stats_init_kernel, dim3((unsigned)((q.n * 7 + 255) / 256)), dim3(256), 0, hs, q.stats, q.n,
                       std::is_same_v<T, float> ? 0 : 1);
    SG_LAUNCH_CHECK();
  }
  const int64_t row = q.c * q.v;
  const int64_t gy = q.n < 65535 ? q.n : 65535;
  const int threads = q.stats ? SV_THREADS_STATS : SV_THREADS;
  const int64_t most = ((q.stats ? SV_BLOCKS_STATS : SV_BLOCKS) + gy - 1) / gy;      // blocks along a row
  const bool flat = !q.channels_last || q.c == 1;      // a sample is one contiguous row of both tensors
  // the head (in elements) at which both tensors are 16-byte aligned, if there is one
  const int64_t head_s = (int64_t)((16u - (uint32_t)((uintptr_t)q.x & 15u)) & 15u) / (int64_t)sizeof(S);
  const int64_t head_t = (int64_t)((16u - (uint32_t)((uintptr_t)q.out & 15u)) & 15u) / (int64_t)sizeof(T);
  const int64_t head = ES > ET ? head_s : head_t;      // the coarser of the two decides; the other must agree
  const bool vec = flat && row % E == 0 && head % ES == head_s && head % ET == head_t;
  if (vec) {
    int64_t gx = (row / E + threads - 1) / threads;
    gx = gx > most ? most : gx;
    hipLaunchKernelGGL((store_volumes_piece_kernel<S, T>), dim3((unsigned)gx, (unsigned)gy), dim3(threads), 0, hs,
                       (const S*)q.x, (T*)q.out, q.n, row, (int)head, q.m, q.stats);
  } else {
    // NCDHW rows that take the element path are walked as c * v voxels of one channel: the same memory, no inner loop
    const int64_t c = flat ? 1 : q.c, v = flat ? row : q.v;
    int64_t gx = (v + threads - 1) / threads;
    gx = gx > most ? most : gx;
    hipLaunchKernelGGL((store_volumes_elem_kernel<S, T>), dim3((unsigned)gx, (unsigned)gy), dim3(threads), 0, hs,
                       (const S*)q.x, (T*)q.out, q.n, c, v, flat ? 0 : 1, q.m, q.stats);
  }
  SG_LAUNCH_CHECK();
  return SG_OK;
}

template <typename S>
int sv_launch_out(sg_src_dtype odt, const sv_args& q, hipStream_t hs) {
  switch (odt) {
    case SG_SRC_I16: return sv_launch<S, int16_t>(q, hs);
    case SG_SRC_U16: return sv_launch<S, uint16_t>(q, hs);
    case SG_SRC_U8:  return sv_launch<S, uint8_t>(q, hs);
    case SG_SRC_F32: return sv_launch<S, float>(q, hs);
    default: break;
  }
  return SG_EINVAL;
}

}  // namespace

extern "C" int sg_store_volumes(const void* x, sg_src_dtype dt, int32_t channels_last, int64_t n, int64_t c, int64_t d, int64_t h,
                                int64_t w, float scale, float shift, float lo, float hi, int32_t rounding, sg_src_dtype out_dt,
                                void* out, int64_t* stats, sg_stream_t st) {
  if (n < 0 || c < 1 || d < 0 || h < 0 || w < 0) return SG_EINVAL;
  if (dt != SG_SRC_F32 && dt != SG_SRC_BF16 && dt != SG_SRC_F16) return SG_EINVAL;
  if (rounding != SG_ROUND_TRUNC && rounding != SG_ROUND_RINT) return SG_EINVAL;
  if (!isfinite(scale) || !(lo <= hi)) return SG_EINVAL;      // (a NaN bound too)
  float tlo, thi;
  switch (out_dt) {
    case SG_SRC_I16: tlo = -32768.f; thi = 32767.f; break;
    case SG_SRC_U16: tlo = 0.f; thi = 65535.f; break;
    case SG_SRC_U8:  tlo = 0.f; thi = 255.f; break;
    case SG_SRC_F32: tlo = -INFINITY; thi = INFINITY; break;
    default: return SG_EINVAL;
  }
  if (out_dt != SG_SRC_F32 && (lo < tlo || hi > thi || lo != truncf(lo) || hi != truncf(hi))) return SG_EINVAL;
  typedef __int128 i128;
  if ((i128)n * c * d * h * w > (i128)INT64_MAX / 8) return SG_EINVAL;
  const int64_t v = d * h * w;
  if (n == 0 || v == 0) return SG_OK;
  if (!x || !out) return SG_EINVAL;
  if (stats && ((uintptr_t)stats) % 8 != 0) return SG_EALIGN;
  sv_args q;
  q.x = x; q.out = out; q.n = n; q.c = c; q.v = v; q.channels_last = channels_last ? 1 : 0; q.stats = stats;
  q.m.scale = scale; q.m.shift = shift; q.m.lo = lo; q.m.hi = hi; q.m.rint = rounding == SG_ROUND_RINT ? 1 : 0;
  hipStream_t hs = sg_st(st);
  switch (dt) {
    case SG_SRC_F32:  return sv_launch_out<float>(out_dt, q, hs);
    case SG_SRC_BF16: return sv_launch_out<sv_bf16>(out_dt, q, hs);
    case SG_SRC_F16:  return sv_launch_out<_Float16>(out_dt, q, hs);
    default: break;
  }
  return SG_EINVAL;
}
