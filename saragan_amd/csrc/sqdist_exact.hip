// Exact squared Euclidean distances between typed integer rows (metrics/memorisation.py):
//   out[i][j] = sum_e (q[i][e] - r[j][e])^2  as int64,  q [mq, v], r [mr, v] of u8 / i8 / i16 / u16 -- no rounding anywhere.
// A 16-bit voxel s (u16: after flipping the top bit, a common shift that a difference does not see) splits into two signed
// bytes h = s >> 8 and l = (s & 255) - 128 with t = 256 h + l = s - 128 (again a common shift), so
//   out = |tq|^2 + |tr|^2 - 2 tq.tr,   tq.tr = 65536 h.h + 256 (h.l + l.h) + l.l,
// and the four byte dot products run on v_mfma_i32_16x16x64_i8 (8-bit types: t = s, u8 shifted by 128; one product).
//   * i32 accumulators hold at most SQX_CHUNK consecutive voxels: |byte product| <= 2^14, the cross accumulator takes two
//     per voxel, 2 * 2^14 * SQX_CHUNK = 2^29; every chunk is then combined into i64 registers;
//   * the grid comes from splitting K as in pdist.hip: block (tile, split) writes its i64 tile to the workspace,
//     sqx_final_kernel adds a tile's splits -- integer sums, no atomics, the same bits on every call and for every split;
//   * the row norms are i64 from the start (sqx_norm_kernel), over the same K splits; the combination is i64;
//   * r == q: only tiles on and above the diagonal are computed, (i, j) with i > j reads what (j, i) wrote, the diagonal is 0.
// Block = 4 waves in 2 x 2 on a 64 x 64 tile, each wave 2 x 2 MFMA tiles of 16 x 16.  A staged row is 128 bytes in two 64-byte
// regions: 16-bit types stage 64 voxels a K step, their h bytes in region 0 and their l bytes in region 1 (split while
// staging: no conversion pass over memory); 8-bit types stage 128 voxels, 64 in each region.  The next step's global loads are
// issued before the MFMAs of the current one and written to the other of two LDS buffers after them: one barrier a step.
// Both MFMA operands take a lane's 16 bytes from the same K positions of their rows, so the sum does not depend on the
// instruction's K order inside a fragment.
// A thread stages 16 bytes of a row at a time.  When every row starts on a 16-byte boundary (decided by the host) a whole step
// is four plain 16-byte loads; otherwise, and at the ragged end, each 16 bytes are one load where they are aligned and inside
// the split and element loads where not (rows of an odd v, views that start mid-buffer).  Rows past mq / mr and voxels
// past the split's end are staged as zero bytes (t = 0 adds nothing to a dot product), never read.  Every offset is 64-bit.
//
// sg_topk_merge keeps the k nearest per query row while the reference set streams by: one wave per row, k selection rounds
// over (distance, id) pairs in lexicographic order, so ties go to the lower id and the chunking of the reference set cannot
// show; lane 0 is the row's only writer.
#include "common.h"

namespace {

constexpr int SQX_CHUNK = 16384;      // longest i32 accumulation, in voxels: 2 * 2^14 * 2^14 = 2^29 < 2^31
constexpr int SQX_BM = 64;            // tile side
constexpr int SQX_LDS_ROW = 144;      // bytes per staged row: 128 + 16, so 16 rows' 16-byte reads cover the 64 banks once
constexpr int SQX_BLOCKS_PER_CU = 3;  // resident blocks a CU holds (at most 168 registers a lane, 36 KB of LDS a block)
constexpr int SQX_MAX_ROUNDS = 2;     // most rounds of the chip (blocks / resident blocks) a K split may be chosen for
constexpr int SQX_TOPK_MAX = 16;

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

struct SqxPlan {
  int nti, ntj, sym;
  int64_t tiles;
  int S;           // K splits
  int64_t span;    // voxels per split (a multiple of SQX_CHUNK)
  size_t dot_words, norm_words;
};

int sqx_cus() {
  static int cus = 0;
  static std::once_flag once;
  std::call_once(once, [] {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
      cus = n;
    else
      cus = 256;
    (void)hipGetLastError();
  });
  return cus;
}

SqxPlan sqx_plan(int32_t mq, int32_t mr, int64_t v, bool sym) {
  SqxPlan p;
  p.sym = sym ? 1 : 0;
  p.nti = (mq + SQX_BM - 1) / SQX_BM;
  p.ntj = (mr + SQX_BM - 1) / SQX_BM;
  p.tiles = sym ? (int64_t)p.nti * (p.nti + 1) / 2 : (int64_t)p.nti * p.ntj;
  const int64_t chunks = (v + SQX_CHUNK - 1) / SQX_CHUNK;
  // tiles x splits = a small multiple of the blocks the chip holds at once, chosen as pdist.hip chooses it: among the splits
  // that keep the grid within SQX_MAX_ROUNDS rounds of the chip, the smallest whose last round is filled to within 5 % of the
  // best filling.  The bound on the grid bounds the workspace: at most max(tiles, rounds * resident blocks) partial tiles.
  const int64_t cus = (int64_t)sqx_cus() * SQX_BLOCKS_PER_CU;
  int64_t smax = SQX_MAX_ROUNDS * cus / p.tiles;
  if (smax < 1) smax = 1;
  if (smax > chunks) smax = chunks;
  auto splits_of = [&](int64_t s) { const int64_t per = (chunks + s - 1) / s; return (chunks + per - 1) / per; };
  auto fill_of = [&](int64_t s) {
    const int64_t blocks = p.tiles * splits_of(s), rounds = (blocks + cus - 1) / cus;
    return (double)blocks / (double)(rounds * cus);
  };
  double best = 0.0;
  for (int64_t s = 1; s <= smax; ++s) best = fill_of(s) > best ? fill_of(s) : best;
  int64_t pick = 1;
  while (fill_of(pick) < 0.95 * best) ++pick;
  const int64_t per = (chunks + pick - 1) / pick;
  p.S = (int)((chunks + per - 1) / per);
  p.span = per * SQX_CHUNK;
  p.dot_words = (size_t)p.tiles * p.S * SQX_BM * SQX_BM;
  p.norm_words = (size_t)(sym ? mq : (int64_t)mq + mr) * p.S;
  return p;
}

// upper-triangle tile (ti <= tj) of an nt x nt grid <-> linear index, rows first
__host__ __device__ __forceinline__ int64_t sqx_tri_index(int ti, int tj, int nt) {
  return (int64_t)ti * nt - (int64_t)ti * (ti - 1) / 2 + (tj - ti);
}

// 16 raw bytes of a row (k_left elements remain in the split) for the slow path: one 16-byte load where they are aligned and
// whole, element loads otherwise.  Elements past the split's end come back as the flip pattern, which staging turns into 0.
template <int ES>
__device__ __forceinline__ u32x4 sqx_fetch(const uint8_t* __restrict__ row, int64_t k_left, uint32_t flip) {
  constexpr int G = 16 / ES;
  u32x4 w = {flip, flip, flip, flip};
  if (k_left <= 0) return w;
  if (k_left >= G && (((uintptr_t)row) & 15) == 0) return *reinterpret_cast<const u32x4*>(row);
#pragma unroll
  for (int e = 0; e < G; ++e) {
    if (e < k_left) {
      const int sh = 8 * ((e * ES) & 3);
      const uint32_t x = ES == 2 ? (uint32_t)(*reinterpret_cast<const uint16_t*>(row + 2 * e)) : (uint32_t)row[e];
      w[(e * ES) >> 2] = (w[(e * ES) >> 2] & ~((ES == 2 ? 0xFFFFu : 0xFFu) << sh)) | (x << sh);
    }
  }
  return w;
}

template <int ES>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SQX_BLOCKS_PER_CU))) void sqx_dot_kernel(
    const uint8_t* __restrict__ q, const uint8_t* __restrict__ r, int64_t* __restrict__ ws, int mq, int mr, int64_t v, int nt_j,
    int sym, int64_t span, uint32_t flip, int vec) {
  constexpr int G = 16 / ES;                 // voxels per 16 bytes
  constexpr int BK = 8 * G;                  // voxels per K step: 8 sixteen-byte groups a row
  constexpr int NA = ES == 2 ? 3 : 1;        // i32 accumulators per MFMA tile: hh, hl + lh, ll  /  one
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][2][SQX_BM][SQX_LDS_ROW];      // [buffer][operand]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lg = lane >> 4;

  int ti, tj;
  if (sym) {
    int rest = (int)blockIdx.x;
    ti = 0;
    while (rest >= nt_j - ti) { rest -= nt_j - ti; ++ti; }
    tj = ti + rest;
  } else {
    ti = (int)blockIdx.x / nt_j;
    tj = (int)blockIdx.x - ti * nt_j;
  }
  const int split = blockIdx.y;
  const int64_t k_begin = (int64_t)split * span;
  const int64_t k_end = k_begin + span < v ? k_begin + span : v;
  const int row_q0 = ti * SQX_BM, row_r0 = tj * SQX_BM;

  // A thread stages the same two 16-byte groups of both operands every step.  Its row pointers are fixed here; a row past the
  // end points at the last row (so that the fast path below loads without a branch) and is staged through a zero mask.
  const uint8_t* pq[2];
  const uint8_t* pr[2];
  uint32_t mask_q[2], mask_r[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int idx = tid + 256 * i, row = idx >> 3, c = idx & 7;
    const int rowq = row_q0 + row < mq ? row_q0 + row : mq - 1, rowr = row_r0 + row < mr ? row_r0 + row : mr - 1;
    mask_q[i] = row_q0 + row < mq ? 0xFFFFFFFFu : 0u;
    mask_r[i] = row_r0 + row < mr ? 0xFFFFFFFFu : 0u;
    pq[i] = q + ((int64_t)rowq * v + k_begin + c * G) * ES;
    pr[i] = r + ((int64_t)rowr * v + k_begin + c * G) * ES;
  }
  // The raw bytes of the next step.  Nothing here uses a loaded value on the fast path (every row 16-byte aligned, the step
  // whole: vec, decided by the host), so the loads stay in flight across the MFMAs; flipping and masking wait until staging.
  u32x4 rq[2], rr[2];
  auto load = [&](int64_t k0) {
    const int64_t off = (k0 - k_begin) * ES;
    if (vec && k0 + BK <= k_end) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        rq[i] = *reinterpret_cast<const u32x4*>(pq[i] + off);
        rr[i] = *reinterpret_cast<const u32x4*>(pr[i] + off);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int64_t k_left = k_end - k0 - ((tid + 256 * i) & 7) * G;
        rq[i] = sqx_fetch<ES>(pq[i] + off, mask_q[i] ? k_left : 0, flip);
        rr[i] = sqx_fetch<ES>(pr[i] + off, mask_r[i] ? k_left : 0, flip);
      }
    }
  };
  auto stage_one = [&](int buf, int op, int row, int c, u32x4 w, uint32_t mask) {
#pragma unroll
    for (int d = 0; d < 4; ++d) w[d] = (w[d] ^ flip) & mask;      // signed bytes / halves; rows past the end: zeros
    if (ES == 2) {
      // dword = [l0, h0, l1, h1]: the high bytes of four voxels into one dword, the low bytes into another
      u32x2 h, l;
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        h[p] = __builtin_amdgcn_perm(w[2 * p + 1], w[2 * p], 0x07050301u);
        l[p] = __builtin_amdgcn_perm(w[2 * p + 1], w[2 * p], 0x06040200u);
      }
      *reinterpret_cast<u32x2*>(&lds[buf][op][row][8 * c]) = h;
      *reinterpret_cast<u32x2*>(&lds[buf][op][row][64 + 8 * c]) = l;
    } else {
      *reinterpret_cast<u32x4*>(&lds[buf][op][row][16 * c]) = w;
    }
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int idx = tid + 256 * i, row = idx >> 3, c = idx & 7;
      stage_one(buf, 0, row, c, rq[i], mask_q[i]);
      stage_one(buf, 1, row, c, rr[i], mask_r[i]);
    }
  };

  i32x4 acc[2][2][NA];
  int64_t dacc[2][2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int a = 0; a < NA; ++a) acc[m][n][a] = i32x4{0, 0, 0, 0};
#pragma unroll
      for (int e = 0; e < 4; ++e) dacc[m][n][e] = 0;
    }
  auto flush = [&]() {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (ES == 2)
            dacc[m][n][e] += 65536 * (int64_t)acc[m][n][0][e] + 256 * (int64_t)acc[m][n][NA > 1 ? 1 : 0][e] +
                             (int64_t)acc[m][n][NA > 2 ? 2 : 0][e];
          else
            dacc[m][n][e] += (int64_t)acc[m][n][0][e];
        }
#pragma unroll
        for (int a = 0; a < NA; ++a) acc[m][n][a] = i32x4{0, 0, 0, 0};
      }
  };
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;

  // step i reads buffer i & 1 and, after its MFMAs are issued, stages step i + 1 into the other one: one barrier a step
  load(k_begin);
  stage(0);
  __syncthreads();
  int in_chunk = 0, buf = 0;
  for (int64_t k0 = k_begin; k0 < k_end; k0 += BK, buf ^= 1) {
    const bool more = k0 + BK < k_end;
    if (more) load(k0 + BK);
    i32x4 fa[2][2], fb[2][2];      // [tile][region]
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        fa[m][g] = *reinterpret_cast<const i32x4*>(&lds[buf][0][wr + 16 * m + lr][64 * g + 16 * lg]);
        fb[m][g] = *reinterpret_cast<const i32x4*>(&lds[buf][1][wc + 16 * m + lr][64 * g + 16 * lg]);
      }
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n) {
        if (ES == 2) {
          constexpr int X = NA > 1 ? 1 : 0, L = NA > 2 ? 2 : 0;
          acc[m][n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m][0], fb[n][0], acc[m][n][0], 0, 0, 0);
          acc[m][n][X] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m][0], fb[n][1], acc[m][n][X], 0, 0, 0);
          acc[m][n][X] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m][1], fb[n][0], acc[m][n][X], 0, 0, 0);
          acc[m][n][L] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m][1], fb[n][1], acc[m][n][L], 0, 0, 0);
        } else {
          acc[m][n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m][0], fb[n][0], acc[m][n][0], 0, 0, 0);
          acc[m][n][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m][1], fb[n][1], acc[m][n][0], 0, 0, 0);
        }
      }
    if (++in_chunk == SQX_CHUNK / BK) {      // the split starts on a chunk boundary: at most SQX_CHUNK voxels per i32 sum
      in_chunk = 0;
      flush();
    }
    if (more) stage(buf ^ 1);
    __syncthreads();      // the next buffer is whole, and this one's fragment reads are done before step i + 2 overwrites it
  }
  flush();
  // C/D map of the 16x16 MFMA: column = lane & 15, row = 4 * (lane >> 4) + reg
  int64_t* tile = ws + ((int64_t)blockIdx.x * gridDim.y + split) * (int64_t)(SQX_BM * SQX_BM);
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n) {
#pragma unroll
      for (int e = 0; e < 4; ++e) tile[(wr + 16 * m + 4 * lg + e) * SQX_BM + wc + 16 * n + lr] = dacc[m][n][e];
    }
}

template <int ES>
__device__ __forceinline__ int64_t sqx_sq(uint32_t raw, uint32_t top) {
  // raw: the element's bits; top: the bit that turns an unsigned type into its shifted signed twin
  const int32_t t = ES == 2 ? (int32_t)(int16_t)(uint16_t)(raw ^ top) - 128 : (int32_t)(int8_t)(uint8_t)(raw ^ top);
  return (int64_t)(t * t);
}

// nws[row * S + split] = sum over the split's voxels of t^2 in i64; rows mq.. are r's.  One block per (row, split): the
// elements up to the first 16-byte boundary one by one, 16-byte loads from there, the rest one by one.
template <int ES>
__global__ __launch_bounds__(256) void sqx_norm_kernel(const uint8_t* __restrict__ q, const uint8_t* __restrict__ r,
                                                       int64_t* __restrict__ nws, int mq, int64_t v, int64_t span,
                                                       uint32_t top) {
  constexpr int G = 16 / ES;
  __shared__ int64_t sh[4];
  const int row = blockIdx.x, split = blockIdx.y;
  const int64_t k_begin = (int64_t)split * span;
  const int64_t k_end = k_begin + span < v ? k_begin + span : v;
  const uint8_t* x = (row < mq ? q + (int64_t)row * v * ES : r + (int64_t)(row - mq) * v * ES) + k_begin * ES;
  const int64_t n = k_end - k_begin;
  int64_t head = (int64_t)(((16 - (((uintptr_t)x) & 15)) & 15) / ES);
  if (head > n) head = n;
  const int64_t groups = (n - head) / G, tail0 = head + groups * G;
  auto elem = [&](int64_t k) {
    return ES == 2 ? (uint32_t)(*reinterpret_cast<const uint16_t*>(x + 2 * k)) : (uint32_t)x[k];
  };
  int64_t s = 0;
  if ((int64_t)threadIdx.x < head) s += sqx_sq<ES>(elem(threadIdx.x), top);
  for (int64_t g = threadIdx.x; g < groups; g += 256) {
    const u32x4 w = *reinterpret_cast<const u32x4*>(x + (head + g * G) * ES);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (ES == 2) {
        s += sqx_sq<ES>(w[d] & 0xFFFFu, top) + sqx_sq<ES>(w[d] >> 16, top);
      } else {
        s += sqx_sq<ES>(w[d] & 0xFFu, top) + sqx_sq<ES>((w[d] >> 8) & 0xFFu, top) + sqx_sq<ES>((w[d] >> 16) & 0xFFu, top) +
             sqx_sq<ES>(w[d] >> 24, top);
      }
    }
  }
  if (tail0 + (int64_t)threadIdx.x < n) s += sqx_sq<ES>(elem(tail0 + threadIdx.x), top);      // (fewer than G <= 16 elements)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) nws[(int64_t)row * gridDim.y + split] = sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(256) void sqx_final_kernel(const int64_t* __restrict__ ws, const int64_t* __restrict__ nws,
                                                        int64_t* __restrict__ out, int mq, int mr, int nt_j, int sym, int S) {
  constexpr int64_t TILE = SQX_BM * SQX_BM;
  const int64_t total = (int64_t)mq * mr;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / mr), j = (int)(e - (int64_t)i * mr);
    if (sym && i == j) { out[e] = 0; continue; }
    const int p = (sym && i > j) ? j : i, c = (sym && i > j) ? i : j;     // the lower half reads what the upper half wrote
    const int ti = p / SQX_BM, tj = c / SQX_BM;
    const int64_t t = sym ? sqx_tri_index(ti, tj, nt_j) : (int64_t)ti * nt_j + tj;
    const int64_t* src = ws + t * S * TILE + (int64_t)(p - ti * SQX_BM) * SQX_BM + (c - tj * SQX_BM);
    const int64_t* np_ = nws + (int64_t)p * S;
    const int64_t* nc_ = nws + (int64_t)(sym ? c : mq + c) * S;
    int64_t dot = 0, np = 0, nc = 0;
    for (int s = 0; s < S; ++s) {
      dot += src[(int64_t)s * TILE];
      np += np_[s];
      nc += nc_[s];
    }
    out[e] = np + nc - 2 * dot;
  }
}

__device__ __forceinline__ bool sqx_less(int64_t d0, int64_t i0, int64_t d1, int64_t i1) {
  return d0 < d1 || (d0 == d1 && i0 < i1);
}

// One wave per query row.  Candidates: the row's mr new distances (ids r_base + j, the row's own id skipped) and the k entries
// it already holds (id -1: empty).  Round t picks the smallest (distance, id) above round t - 1's pick.
__global__ __launch_bounds__(64) void sqx_topk_kernel(const int64_t* __restrict__ d, int mr, int64_t r_base,
                                                      const int64_t* __restrict__ q_ids, int k, int64_t* __restrict__ best_d,
                                                      int64_t* __restrict__ best_id) {
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t* dr = d + row * mr;
  const int64_t own = q_ids != nullptr ? q_ids[row] : -1;
  const int64_t imax = 0x7FFFFFFFFFFFFFFFll, imin = -imax - 1;
  int64_t old_d = imax, old_id = -1;
  if (lane < k) { old_d = best_d[row * k + lane]; old_id = best_id[row * k + lane]; }
  int64_t last_d = imin, last_id = -1;
  for (int t = 0; t < k; ++t) {
    int64_t cd = imax, ci = imax;      // (no candidate yet)
    if (old_id >= 0 && sqx_less(last_d, last_id, old_d, old_id)) { cd = old_d; ci = old_id; }
    for (int j = lane; j < mr; j += 64) {
      const int64_t id = r_base + j, dj = dr[j];
      if ((q_ids == nullptr || id != own) && sqx_less(last_d, last_id, dj, id) && sqx_less(dj, id, cd, ci)) { cd = dj; ci = id; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int64_t od = __shfl_xor(cd, o), oi = __shfl_xor(ci, o);
      if (sqx_less(od, oi, cd, ci)) { cd = od; ci = oi; }
    }
    const bool none = ci == imax;
    if (lane == 0) {
      best_d[row * k + t] = none ? imax : cd;
      best_id[row * k + t] = none ? -1 : ci;
    }
    if (none) {      // nothing above the last pick: the tail stays empty
      if (lane == 0)
        for (int u = t + 1; u < k; ++u) { best_d[row * k + u] = imax; best_id[row * k + u] = -1; }
      break;
    }
    last_d = cd;
    last_id = ci;
  }
}

bool sqx_dtype(sg_src_dtype dt, int* es, uint32_t* flip, uint32_t* top) {
  switch (dt) {
    case SG_SRC_U8: *es = 1; *flip = 0x80808080u; *top = 0x80u; return true;
    case SG_SRC_I8: *es = 1; *flip = 0u; *top = 0u; return true;
    case SG_SRC_I16: *es = 2; *flip = 0x00800080u; *top = 0u; return true;        // l - 128 == l ^ 0x80 as a signed byte
    case SG_SRC_U16: *es = 2; *flip = 0x80808080u; *top = 0x8000u; return true;   // and the top bit: u - 32768
    default: return false;
  }
}

}  // namespace

extern "C" {

int32_t sg_sqdist_exact_chunk(void) { return SQX_CHUNK; }

size_t sg_sqdist_exact_workspace(int32_t mq, int32_t mr, int64_t v) {
  if (mq < 1 || mr < 1 || v < 1) return 0;
  // the caller may pass r == q: fewer tiles, but possibly more splits
  const SqxPlan p = sqx_plan(mq, mr, v, false);
  size_t n = p.dot_words + p.norm_words;
  if (mq == mr) {
    const SqxPlan s = sqx_plan(mq, mr, v, true);
    if (s.dot_words + s.norm_words > n) n = s.dot_words + s.norm_words;
  }
  return n * sizeof(int64_t);
}

int sg_sqdist_exact(const void* q, const void* r, sg_src_dtype dt, int32_t mq, int32_t mr, int64_t v, int64_t* out,
                    void* workspace, size_t workspace_bytes, sg_stream_t st) {
  if (q == nullptr || r == nullptr || out == nullptr || workspace == nullptr) return SG_EINVAL;
  if (mq < 1 || mr < 1 || v < 1 || v >= ((int64_t)1 << 31)) return SG_EINVAL;
  int es = 0;
  uint32_t flip = 0, top = 0;
  if (!sqx_dtype(dt, &es, &flip, &top)) return SG_EINVAL;
  if ((((uintptr_t)q | (uintptr_t)r) & (uintptr_t)(es - 1)) != 0 || (((uintptr_t)out | (uintptr_t)workspace) & 7) != 0)
    return SG_EALIGN;
  const bool sym = q == r && mq == mr;
  const SqxPlan p = sqx_plan(mq, mr, v, sym);
  if (p.tiles > 0x7FFFFFFF) return SG_EINVAL;
  if (workspace_bytes < (p.dot_words + p.norm_words) * sizeof(int64_t)) return SG_EWORKSPACE;
  int64_t* ws = reinterpret_cast<int64_t*>(workspace);
  int64_t* nws = ws + p.dot_words;
  const uint8_t* qb = reinterpret_cast<const uint8_t*>(q);
  const uint8_t* rb = reinterpret_cast<const uint8_t*>(r);
  // every row starts on a 16-byte boundary: the dot kernel's whole steps load without looking at an address
  const int vec = (sg_aligned16(q) && sg_aligned16(r) && (v * es) % 16 == 0) ? 1 : 0;
  const dim3 ngrid((unsigned)(sym ? mq : mq + mr), (unsigned)p.S), dgrid((unsigned)p.tiles, (unsigned)p.S);
  if (es == 2) {
    hipLaunchKernelGGL(sqx_norm_kernel<2>, ngrid, dim3(256), 0, sg_st(st), qb, rb, nws, mq, v, p.span, top);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(sqx_dot_kernel<2>, dgrid, dim3(256), 0, sg_st(st), qb, rb, ws, mq, mr, v, p.ntj, p.sym, p.span, flip, vec);
  } else {
    hipLaunchKernelGGL(sqx_norm_kernel<1>, ngrid, dim3(256), 0, sg_st(st), qb, rb, nws, mq, v, p.span, top);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(sqx_dot_kernel<1>, dgrid, dim3(256), 0, sg_st(st), qb, rb, ws, mq, mr, v, p.ntj, p.sym, p.span, flip, vec);
  }
  SG_LAUNCH_CHECK();
  const int64_t total = (int64_t)mq * mr;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(sqx_final_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, sg_st(st), ws, nws, out,
                     mq, mr, p.ntj, p.sym, p.S);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

int sg_topk_merge(const int64_t* d, int32_t mq, int32_t mr, int64_t r_base, const int64_t* q_ids, int32_t k, int64_t* best_d,
                  int64_t* best_id, sg_stream_t st) {
  if (d == nullptr || best_d == nullptr || best_id == nullptr) return SG_EINVAL;
  if (mq < 1 || mr < 1 || k < 1 || k > SQX_TOPK_MAX || r_base < 0) return SG_EINVAL;
  if ((((uintptr_t)d | (uintptr_t)q_ids | (uintptr_t)best_d | (uintptr_t)best_id) & 7) != 0) return SG_EALIGN;
  hipLaunchKernelGGL(sqx_topk_kernel, dim3((unsigned)mq), dim3(64), 0, sg_st(st), d, mr, r_base, q_ids, k, best_d, best_id);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

}  // extern "C"
