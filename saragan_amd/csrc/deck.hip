// Batches from a device-resident table: out[i] = f32(table[idx[i]]), optionally (x - mean) / stddev.  A phase's
// whole `.npy` table sits in HBM in the files' own dtype ([rows, row_elems]: u8 / i8 / i16 / u16 / f16 / f32) and a training
// batch is ONE launch over N drawn positions, instead of N np.load calls, two numpy passes and a host-to-device copy
// (dataset.PinnedPrefetcher).  The label table (f32 [F, L]) goes through the same entry point with normalise = 0.
//
// Bit-identity with the host path: every source type converts to f32 exactly, and the normalisation is two correctly rounded
// f32 operations, __fdiv_rn(__fsub_rn(x, mean), stddev) -- what np.subtract / np.divide with np.float32 scalars compute.  No
// reciprocal, no fused form (the file is built with -ffp-contract=off as well).
//
// A block works on one output row at a time (blockIdx.y, strided), so the drawn position is block-uniform: the range check is
// one scalar compare, and a position outside [0, rows) makes the block write quiet NaNs WITHOUT forming a table address.  Row
// offsets are 64-bit: rows * row_elems * sizeof(S) passes 4 GiB for ordinary data sets.  Two kernels, chosen per launch on the
// host: 16-byte loads and 16-byte stores when the table base, the row length in bytes and the output base are multiples of 16
// (then every row of both is), an element-per-lane kernel otherwise (a 3 x 5 x 7 u8 volume has 105-byte rows).
#include "common.h"

namespace {

template <typename S>
__device__ __forceinline__ float dk_to_f(S v) { return (float)v; }      // exact for every source type below

__device__ __forceinline__ float dk_norm(float x, int normalise, float mean, float stddev) {
  return normalise ? __fdiv_rn(__fsub_rn(x, mean), stddev) : x;
}

template <typename S>
__global__ __launch_bounds__(256) void gather_rows_vec_kernel(const S* __restrict__ table, int64_t rows, int64_t row_elems,
                                                              const int32_t* __restrict__ idx, int n, float* __restrict__ out,
                                                              int normalise, float mean, float stddev) {
  constexpr int E = 16 / (int)sizeof(S);      // elements of one 16-byte load = E / 4 stores of 16 bytes
  const int64_t pieces = row_elems / E;
  const int64_t p0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const int64_t r = idx[i];
    float* __restrict__ dst = out + (int64_t)i * row_elems;
    if (r < 0 || r >= rows) {      // block-uniform; the table is not addressed
      const float q = __builtin_nanf("");
      const f32x4 nan4 = {q, q, q, q};
      for (int64_t p = p0; p < pieces; p += stride) {
#pragma unroll
        for (int j = 0; j < E / 4; ++j) {
          *reinterpret_cast<f32x4*>(dst + p * E + 4 * j) = nan4;
          SG_STORE16_GUARD(nan4);
        }
      }
      continue;
    }
    const S* __restrict__ src = table + r * row_elems;
    for (int64_t p = p0; p < pieces; p += stride) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(src + p * E);
      const S* s = reinterpret_cast<const S*>(&raw);
#pragma unroll
      for (int j = 0; j < E / 4; ++j) {
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = dk_norm(dk_to_f(s[4 * j + e]), normalise, mean, stddev);
        *reinterpret_cast<f32x4*>(dst + p * E + 4 * j) = v;
        SG_STORE16_GUARD(v);
      }
    }
  }
}

template <typename S>
__global__ __launch_bounds__(256) void gather_rows_elem_kernel(const S* __restrict__ table, int64_t rows, int64_t row_elems,
                                                               const int32_t* __restrict__ idx, int n, float* __restrict__ out,
                                                               int normalise, float mean, float stddev) {
  const int64_t e0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int i = blockIdx.y; i < n; i += gridDim.y) {
    const int64_t r = idx[i];
    float* __restrict__ dst = out + (int64_t)i * row_elems;
    if (r < 0 || r >= rows) {
      for (int64_t e = e0; e < row_elems; e += stride) dst[e] = __builtin_nanf("");
      continue;
    }
    const S* __restrict__ src = table + r * row_elems;
    for (int64_t e = e0; e < row_elems; e += stride) dst[e] = dk_norm(dk_to_f(src[e]), normalise, mean, stddev);
  }
}

template <typename S>
int dk_launch(const void* table, int64_t rows, int64_t row_elems, const int32_t* idx, int32_t n, float* out, int32_t normalise,
              float mean, float stddev, hipStream_t hs) {
  if (((uintptr_t)table) % sizeof(S) != 0) return SG_EALIGN;
  const bool vec = sg_aligned16(table) && sg_aligned16(out) && (row_elems * (int64_t)sizeof(S)) % 16 == 0;
  const int64_t items = vec ? row_elems / (16 / (int64_t)sizeof(S)) : row_elems;      // lanes' worth of work per row
  const int threads = items <= 64 ? 64 : 256;
  int64_t gx = (items + threads - 1) / threads;
  if (gx > 1024) gx = 1024;      // (the kernels stride over what is left)
  const dim3 grid((unsigned)gx, (unsigned)(n < 65535 ? n : 65535));
  if (vec)
    hipLaunchKernelGGL((gather_rows_vec_kernel<S>), grid, dim3(threads), 0, hs, (const S*)table, rows, row_elems, idx, n, out,
                       normalise, mean, stddev);
  else
    hipLaunchKernelGGL((gather_rows_elem_kernel<S>), grid, dim3(threads), 0, hs, (const S*)table, rows, row_elems, idx, n, out,
                       normalise, mean, stddev);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

}  // namespace

extern "C" int sg_gather_rows(const void* table, sg_src_dtype sdt, int64_t rows, int64_t row_elems, const int32_t* idx, int32_t n,
                              float* out, int32_t normalise, float mean, float stddev, sg_stream_t st) {
  if (!table || !idx || !out || rows < 0 || row_elems < 1 || n < 0) return SG_EINVAL;
  if ((int)sdt < (int)SG_SRC_U8 || (int)sdt > (int)SG_SRC_F32) return SG_EINVAL;
  if (((uintptr_t)out) % 4 != 0 || ((uintptr_t)idx) % 4 != 0) return SG_EALIGN;
  if (n == 0) return SG_OK;
  hipStream_t hs = sg_st(st);
  normalise = normalise ? 1 : 0;
  switch (sdt) {
    case SG_SRC_U8:  return dk_launch<uint8_t>(table, rows, row_elems, idx, n, out, normalise, mean, stddev, hs);
    case SG_SRC_I8:  return dk_launch<int8_t>(table, rows, row_elems, idx, n, out, normalise, mean, stddev, hs);
    case SG_SRC_I16: return dk_launch<int16_t>(table, rows, row_elems, idx, n, out, normalise, mean, stddev, hs);
    case SG_SRC_U16: return dk_launch<uint16_t>(table, rows, row_elems, idx, n, out, normalise, mean, stddev, hs);
    case SG_SRC_F16: return dk_launch<_Float16>(table, rows, row_elems, idx, n, out, normalise, mean, stddev, hs);
    case SG_SRC_F32: return dk_launch<float>(table, rows, row_elems, idx, n, out, normalise, mean, stddev, hs);
    case SG_SRC_BF16: break;      // sg_intensity_hist's input type, no table type: refused above
  }
  return SG_EINVAL;
}
