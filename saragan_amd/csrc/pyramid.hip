// The per-phase dataset pyramid (prepare_data.py): one launch reads a batch of source volumes x [n, sd, sh, sw] once
// and writes up to SG_PYRAMID_LEVELS_PER_LAUNCH levels [n, D >> i, H >> i, W >> i] of their block reduction, after placing every
// volume in the target window (D, H, W): target voxel t of axis a is source voxel t + off[a], pad_value outside the source.
//
// The definition is exact (tests compare with ==); include/saragan_hip.h states it operation by operation.  In short: v = x -
// intercept; level i is the sum (MEAN: an int64 or f64 partial) or the maximum of v over the aligned 2^i cube; MEAN divides by 8^i
// (integers: truncation toward zero; floats: one f64 division, one rounding); the stored value is that, clamped.  Level i is
// built from level i - 1's unclamped partials, never from stored values.
//
// The brick scheme.  A block owns tiles of PY_TD x 32 x 64 target voxels, PY_TD = max(2^(L-1), 4): every 2^(L-1) brick lies
// inside one tile, so all levels finish inside the block.  A tile is walked in slabs of 4 x 32 x 64:
//   fill    the slab's source rows are read with 16-byte loads from each row's first 16-byte boundary (the elements in front of it
//           and behind the last whole load one by one: no byte is read twice, none outside the source), converted to v and written
//           to LDS in TARGET coordinates; voxels outside the source get pad_value - intercept;
//   sticks  every thread takes a 2 x 2 x 8 stick of the slab from LDS: it stores 4 x 8 voxels of level 0 (16-byte stores), holds
//           the four 2-cube partials of level 1 in registers and stores them, and completes level 2 with its three neighbours of
//           the 4-cube by two lane exchanges.  The level-2 partials stay in LDS for
//   tail    levels 3, 4, 5: eight partials of the level below per output voxel, level by level, once the tile's slabs are done.
// No output voxel has two writers and no atomics touch the outputs.  The statistics (integer outputs) are summed per thread, per
// wave by lane exchanges and per block in LDS: one 64-bit integer atomic per (block, level, statistic).
#include "common.h"
#include <math.h>
#include <limits.h>
#include <initializer_list>
#include <type_traits>

namespace {

constexpr int PY_THREADS = 256;
constexpr int PY_WAVE = 64;
constexpr int PY_TH = 32, PY_TW = 64, PY_SD = 4;      // tile rows and columns; slab depth
constexpr int PY_PITCH = PY_TW + 4;                   // LDS row pitch in 32-bit words (16-byte aligned rows, staggered banks)
constexpr int PY_MAXL = SG_PYRAMID_LEVELS_PER_LAUNCH;

struct py_out {
  void* p[PY_MAXL];
};

// (extents and offsets are at most 2^29 in magnitude, host-checked: coordinates are 32-bit, only linear offsets 64-bit)
struct py_geom {
  int32_t sd, sh, sw, D, H, W, od, oh, ow;
  uint32_t tiles_h, tiles_w, tiles, chunks;      // chunks: blocks per sample
  int32_t levels, TD;
};

template <bool INT>
struct py_scal {
  std::conditional_t<INT, int32_t, float> intercept, pad, lo, hi;
};

template <typename S>
constexpr bool py_int = std::is_integral_v<S>;
template <typename S>
using py_v_t = std::conditional_t<py_int<S>, int32_t, float>;
// the unclamped partial of a level: exact integer sums, f64 sums, running maxima
template <bool INT, int MODE>
using py_acc_t = std::conditional_t<MODE == SG_PYR_MAX, std::conditional_t<INT, int32_t, float>, std::conditional_t<INT, int64_t, double>>;

template <int MODE, typename A>
__device__ __forceinline__ void py_merge(A& a, A b) {
  if constexpr (MODE == SG_PYR_MEAN) a += b;
  else a = b > a ? b : a;      // (false for a NaN b: ignored)
}
template <bool INT, int MODE>
__device__ __forceinline__ py_acc_t<INT, MODE> py_identity() {
  if constexpr (MODE == SG_PYR_MEAN) return 0;
  else if constexpr (INT) return INT32_MIN;
  else return -INFINITY;
}

__device__ __forceinline__ double py_pow2_neg(int k) { return __longlong_as_double((int64_t)(1023 - k) << 52); }      // 2^-k, exact

// the stored value of a partial s of absolute level `lv`
template <typename O, bool INT, int MODE, typename A>
__device__ __forceinline__ O py_finish(A s, int lv, const py_scal<INT>& sc) {
  if constexpr (INT && !std::is_same_v<O, float>) {
    int64_t q = (int64_t)s;
    if constexpr (MODE == SG_PYR_MEAN) q = (q + ((q >> 63) & (((int64_t)1 << (3 * lv)) - 1))) >> (3 * lv);      // toward zero
    q = q < (int64_t)sc.lo ? (int64_t)sc.lo : q;
    q = q > (int64_t)sc.hi ? (int64_t)sc.hi : q;
    return (O)q;
  } else {
    float r;
    if constexpr (MODE == SG_PYR_MEAN) r = (float)((double)s * py_pow2_neg(3 * lv));      // one rounding (the product is exact)
    else r = (float)s;
    const float lo = (float)sc.lo, hi = (float)sc.hi;
    r = r < lo ? lo : r;      // (a NaN r stays NaN)
    r = r > hi ? hi : r;
    return r;
  }
}

// `valid` leading elements of v[N] to p: whole and aligned runs as 16-, 8- or 4-byte stores, anything else by element
template <typename T, int N>
__device__ __forceinline__ void py_store_run(T* __restrict__ p, const T (&v)[N], int valid) {
  constexpr int BYTES = N * (int)sizeof(T), UNIT = BYTES >= 16 ? 16 : BYTES;
  if (valid >= N && ((uintptr_t)p & (uintptr_t)(UNIT - 1)) == 0) {
    if constexpr (BYTES >= 16) {
#pragma unroll
      for (int k = 0; k < BYTES / 16; ++k) {
        u32x4 q;
        __builtin_memcpy(&q, reinterpret_cast<const char*>(v) + 16 * k, 16);
        *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(p) + 16 * k) = q;
        SG_STORE16_GUARD(q);
      }
    } else if constexpr (BYTES == 8) {
      u32x2 q;
      __builtin_memcpy(&q, v, 8);
      *reinterpret_cast<u32x2*>(p) = q;
    } else if constexpr (BYTES == 4) {
      uint32_t q;
      __builtin_memcpy(&q, v, 4);
      *reinterpret_cast<uint32_t*>(p) = q;
    } else {
#pragma unroll
      for (int e = 0; e < N; ++e) p[e] = v[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e)
      if (e < valid) p[e] = v[e];
  }
}

// ---- statistics of the stored values: sum, sum of squares, minimum, maximum
struct py_stat {
  int64_t s, ss;
  int32_t mn, mx;
  __device__ __forceinline__ void clear() { s = 0; ss = 0; mn = INT32_MAX; mx = INT32_MIN; }
  __device__ __forceinline__ void add(int32_t q) {
    s += q;
    ss += (int64_t)q * q;
    mn = q < mn ? q : mn;
    mx = q > mx ? q : mx;
  }
};

__device__ __forceinline__ void py_stat_to_lds(const py_stat& a, int64_t* slot) {
  __hip_atomic_fetch_add(slot + 0, a.s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(slot + 1, a.ss, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_min(slot + 2, (int64_t)a.mn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_max(slot + 3, (int64_t)a.mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// every lane of the wave calls; lane 0 adds the wave's total to the block's LDS slot
__device__ __forceinline__ void py_stat_wave_to_lds(py_stat a, int64_t* slot) {
#pragma unroll
  for (int m = PY_WAVE / 2; m >= 1; m >>= 1) {
    a.s += __shfl_xor(a.s, m, PY_WAVE);
    a.ss += __shfl_xor(a.ss, m, PY_WAVE);
    const int32_t on = __shfl_xor(a.mn, m, PY_WAVE), ox = __shfl_xor(a.mx, m, PY_WAVE);
    a.mn = on < a.mn ? on : a.mn;
    a.mx = ox > a.mx ? ox : a.mx;
  }
  if (threadIdx.x % PY_WAVE == 0) py_stat_to_lds(a, slot);
}

__device__ __forceinline__ void py_stat_lds_clear(int64_t* st, int slots) {
  for (int i = threadIdx.x; i < slots * 4; i += PY_THREADS) st[i] = (i & 3) == 2 ? INT64_MAX : (i & 3) == 3 ? INT64_MIN : 0;
}

// one global atomic per (block, level, statistic); dst: the int64 [4] of each slot, `pitch` apart
__device__ __forceinline__ void py_stat_flush(const int64_t* st, int slots, int64_t* dst) {
  const int i = threadIdx.x;
  if (i < slots * 4) {
    int64_t* d = dst + i;
    const int64_t v = st[i];
    if ((i & 3) == 2) __hip_atomic_fetch_min(d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if ((i & 3) == 3) __hip_atomic_fetch_max(d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_add(d, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void pyramid_stats_init_kernel(int64_t* stats, int64_t slots) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < slots * 4) stats[i] = (i & 3) == 2 ? INT64_MAX : (i & 3) == 3 ? INT64_MIN : 0;
}

// ---- the pyramid of a batch of source volumes
template <typename S, typename O, int MODE>
__global__ __launch_bounds__(PY_THREADS) void pyramid_kernel(const S* __restrict__ x, py_geom g, py_scal<py_int<S>> sc, py_out out,
                                                             int64_t* __restrict__ stats) {
  constexpr bool INT = py_int<S>;
  constexpr bool STATS_OK = !std::is_same_v<O, float>;
  using V = py_v_t<S>;
  using A = py_acc_t<INT, MODE>;
  constexpr int E = 16 / (int)sizeof(S);              // elements per 16-byte load
  constexpr int NL = PY_TW / E + 1;                   // 16-byte pieces a slab row can touch
  constexpr int ROWS = PY_SD * PY_TH;
  constexpr int ITEMS = ROWS * NL, ITER = (ITEMS + PY_THREADS - 1) / PY_THREADS;

  __shared__ __attribute__((aligned(16))) V tile[ROWS * PY_PITCH];
  __shared__ A acc2[8 * 8 * 16];      // level-2 partials of the tile: [TD / 4][8][16]
  __shared__ A acc3[4 * 4 * 8];       // level 3: [TD / 8][4][8]
  __shared__ A acc4[2 * 2 * 4];       // level 4: [TD / 16][2][4]
  __shared__ int64_t st[PY_MAXL * 4];

  const int tid = threadIdx.x;
  const uint32_t sample32 = blockIdx.x / g.chunks, chunk = blockIdx.x - sample32 * g.chunks;
  const int64_t sample = sample32;
  const bool do_stats = STATS_OK && stats != nullptr;
  const V padv = INT ? (V)(sc.pad - sc.intercept) : (V)__fsub_rn((float)sc.pad, (float)sc.intercept);
  // this thread's stick of a slab: 2 planes x 2 rows x 8 columns.  Lane bits 0 and 1 run through the 4-cube's sticks.
  const int stick_h = (tid & 1) | ((tid >> 5) << 1), stick_d = (tid >> 1) & 1, stick_w = (tid >> 2) & 7;

  py_stat sa[3];
  sa[0].clear(); sa[1].clear(); sa[2].clear();
  if (do_stats) py_stat_lds_clear(st, PY_MAXL);

  {
    const uint32_t t = chunk;      // one tile per block
    const uint32_t tq = t / g.tiles_w, tqq = tq / g.tiles_h;
    const int W0 = (int)(t - tq * g.tiles_w) * PY_TW, D0 = (int)tqq * g.TD, H0 = (int)(tq - tqq * g.tiles_h) * PY_TH;
    const int twc = g.W - W0 < PY_TW ? g.W - W0 : PY_TW;      // columns of the tile inside the target
    // the source columns this tile needs: [a, b)
    const int a = W0 + g.ow > 0 ? W0 + g.ow : 0, b = W0 + twc + g.ow < g.sw ? W0 + twc + g.ow : g.sw;

    for (int slab = 0; slab * PY_SD < g.TD; ++slab) {
      const int Ds = D0 + slab * PY_SD;
      if (Ds >= g.D) break;      // (uniform)
      // ---- fill: source rows -> v in LDS, target coordinates
      // (an opaque copy of the thread index as well: the per-piece rows, columns and lane masks are computed per slab, not held)
      int ftid = threadIdx.x;
      asm volatile("" : "+v"(ftid));
      u32x4 raw[ITER];
      int at[ITER];      // where a whole 16-byte piece in raw[] goes in the tile; -1: none
      bool partial = false;
#pragma unroll
      for (int k = 0; k < ITER; ++k) {
        const int it = ftid + k * PY_THREADS;
        at[k] = -1;
        if (it < ITEMS && a < b) {
          const int r = it / NL, c = it - r * NL;
          const int td = Ds + r / PY_TH, th = H0 + r % PY_TH;
          const int zd = td + g.od, zh = th + g.oh;
          if (td < g.D && th < g.H && zd >= 0 && zd < g.sd && zh >= 0 && zh < g.sh) {
            const S* __restrict__ row = x + ((sample * g.sd + zd) * g.sh + zh) * g.sw;
            // the piece's first element as a column of the row (the base is element-aligned: the difference is whole elements)
            const int e0 = a - (int)((uintptr_t)(row + a) & 15u) / (int)sizeof(S) + c * E;
            if (e0 >= a && e0 + E <= b) {
              raw[k] = *reinterpret_cast<const u32x4*>(row + e0);
              at[k] = r * PY_PITCH + (e0 - g.ow - W0);
            } else if (e0 + E > a && e0 < b) {
              partial = true;
            }
          }
        }
      }
#pragma unroll
      for (int k = 0; k < ITER; ++k) {
        if (at[k] >= 0) {
          const S* s = reinterpret_cast<const S*>(&raw[k]);
          V* __restrict__ dst = tile + at[k];
#pragma unroll
          for (int e = 0; e < E; ++e) {
            if constexpr (INT) dst[e] = (V)((int32_t)s[e] - sc.intercept);
            else dst[e] = __fsub_rn((float)s[e], sc.intercept);
          }
        }
      }
      if (partial) {      // in front of a row's first 16-byte boundary and behind its last whole load: by element
#pragma unroll 1
        for (int it = ftid; it < ITEMS; it += PY_THREADS) {
          const int r = it / NL, c = it - r * NL;
          const int td = Ds + r / PY_TH, th = H0 + r % PY_TH;
          const int zd = td + g.od, zh = th + g.oh;
          if (td < g.D && th < g.H && zd >= 0 && zd < g.sd && zh >= 0 && zh < g.sh) {
            const S* __restrict__ row = x + ((sample * g.sd + zd) * g.sh + zh) * g.sw;
            const int e0 = a - (int)((uintptr_t)(row + a) & 15u) / (int)sizeof(S) + c * E;
            if (!(e0 >= a && e0 + E <= b)) {
              const int ea = e0 > a ? e0 : a, eb = e0 + E < b ? e0 + E : b;
#pragma unroll 1
              for (int e = ea; e < eb; ++e) {
                V* __restrict__ dst = tile + r * PY_PITCH + (e - g.ow - W0);
                if constexpr (INT) *dst = (V)((int32_t)row[e] - sc.intercept);
                else *dst = __fsub_rn((float)row[e], sc.intercept);
              }
            }
          }
        }
      }
      // the pad: target voxels of the slab that no source voxel reaches (uniform test: most tiles lie inside the source)
      const bool inside = a == W0 + g.ow && b == W0 + twc + g.ow && Ds + g.od >= 0 && H0 + g.oh >= 0 &&
                          (Ds + PY_SD < g.D ? Ds + PY_SD : g.D) + g.od <= g.sd && (H0 + PY_TH < g.H ? H0 + PY_TH : g.H) + g.oh <= g.sh;
      if (!inside) {
        for (int i = ftid; i < ROWS * PY_TW; i += PY_THREADS) {
          const int r = i / PY_TW, cw = i % PY_TW;
          const int zd = Ds + r / PY_TH + g.od, zh = H0 + r % PY_TH + g.oh, zw = W0 + cw + g.ow;
          if (zd < 0 || zd >= g.sd || zh < 0 || zh >= g.sh || zw < 0 || zw >= g.sw) tile[r * PY_PITCH + cw] = padv;
        }
      }
      __syncthreads();

      // ---- sticks: levels 0, 1, 2
      {
        // (opaque copies: what derives from them -- every level's extents, strides and branch conditions -- is computed here, where
        // it is used, not hoisted out of the tile loop into scalar registers that then spill)
        int L = g.levels, gD = g.D, gH = g.H, gW = g.W;
        asm volatile("" : "+s"(L), "+s"(gD), "+s"(gH), "+s"(gW));
        const int td0 = Ds + 2 * stick_d, th0 = H0 + 2 * stick_h, tw0 = W0 + 8 * stick_w;
        A p1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) p1[k] = py_identity<INT, MODE>();
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            V v[8];
            const V* src = tile + ((2 * stick_d + j) * PY_TH + 2 * stick_h + i) * PY_PITCH + 8 * stick_w;
            *reinterpret_cast<u32x4*>(&v[0]) = *reinterpret_cast<const u32x4*>(src);
            *reinterpret_cast<u32x4*>(&v[4]) = *reinterpret_cast<const u32x4*>(src + 4);
            const int td = td0 + j, th = th0 + i;
            int valid = 0;
            if (td < gD && th < gH && tw0 < gW) valid = gW - tw0 < 8 ? gW - tw0 : 8;
            O o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              A s0 = py_identity<INT, MODE>();      // (level 0 is a cube of one voxel: a NaN voxel's maximum is -inf there too)
              py_merge<MODE, A>(s0, (A)v[e]);
              o[e] = py_finish<O, INT, MODE, A>(s0, 0, sc);
              py_merge<MODE, A>(p1[e >> 1], (A)v[e]);
            }
            if constexpr (STATS_OK) {
              if (do_stats) {
                if (valid == 8) {      // a whole run: a 32-bit sum (8 * 65535), one multiply-add per square, no per-element test
                  int32_t ps = 0;
                  uint64_t pss = 0;
#pragma unroll
                  for (int e = 0; e < 8; ++e) {
                    const int32_t q = (int32_t)o[e];
                    const uint32_t m = (uint32_t)(q < 0 ? -q : q);
                    ps += q;
                    pss = (uint64_t)m * m + pss;
                    sa[0].mn = q < sa[0].mn ? q : sa[0].mn;
                    sa[0].mx = q > sa[0].mx ? q : sa[0].mx;
                  }
                  sa[0].s += ps;
                  sa[0].ss += (int64_t)pss;
                } else {
#pragma unroll
                  for (int e = 0; e < 8; ++e)
                    if (e < valid) sa[0].add((int32_t)o[e]);
                }
              }
            }
            if (valid > 0) py_store_run<O, 8>((O*)out.p[0] + ((sample * gD + td) * gH + th) * gW + tw0, o, valid);
          }
        }
        if (L >= 2) {
          const int D1 = gD >> 1, H1 = gH >> 1, W1 = gW >> 1, d1 = td0 >> 1, h1 = th0 >> 1, w1 = tw0 >> 1;
          int valid = 0;
          if (d1 < D1 && h1 < H1 && w1 < W1) valid = W1 - w1 < 4 ? W1 - w1 : 4;
          O o[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            o[k] = py_finish<O, INT, MODE, A>(p1[k], 1, sc);
            if constexpr (STATS_OK)
              if (do_stats && k < valid) sa[1].add((int32_t)o[k]);
          }
          if (valid > 0) {
            const int64_t at = ((sample * D1 + d1) * H1 + h1) * W1 + w1;
            py_store_run<O, 4>((O*)out.p[1] + at, o, valid);
          }
        }
        if (L >= 3) {      // (uniform: every lane takes part in the exchanges)
          A p2[2];
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            p2[k] = p1[2 * k];
            py_merge<MODE, A>(p2[k], p1[2 * k + 1]);
            py_merge<MODE, A>(p2[k], (A)__shfl_xor(p2[k], 1, PY_WAVE));
            py_merge<MODE, A>(p2[k], (A)__shfl_xor(p2[k], 2, PY_WAVE));
          }
          if ((tid & 3) == 0) {
            const int D2 = gD >> 2, H2 = gH >> 2, W2 = gW >> 2, d2 = td0 >> 2, h2 = th0 >> 2, w2 = tw0 >> 2;
            int valid = 0;
            if (d2 < D2 && h2 < H2 && w2 < W2) valid = W2 - w2 < 2 ? W2 - w2 : 2;
            O o[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              o[k] = py_finish<O, INT, MODE, A>(p2[k], 2, sc);
              if constexpr (STATS_OK)
                if (do_stats && k < valid) sa[2].add((int32_t)o[k]);
            }
            if (valid > 0) {
              const int64_t at = ((sample * D2 + d2) * H2 + h2) * W2 + w2;
              py_store_run<O, 2>((O*)out.p[2] + at, o, valid);
            }
            if (L > 3) {
              A* q = acc2 + (slab * 8 + (stick_h >> 1)) * 16 + 2 * stick_w;
              q[0] = p2[0];
              q[1] = p2[1];
            }
          }
        }
      }
      __syncthreads();      // the tile is filled again for the next slab; acc2 is read below
    }

    // ---- tail: levels 3, 4, 5 from the partials of the level below, eight each
    if (g.levels > 3) {
#pragma unroll 1
      for (int lv = 3; lv < PY_MAXL; ++lv) {
        int L = g.levels, gD = g.D, gH = g.H, gW = g.W;
        asm volatile("" : "+s"(L), "+s"(gD), "+s"(gH), "+s"(gW));
        if (lv < L) {      // (uniform)
          const A* below = lv == 3 ? acc2 : lv == 4 ? acc3 : acc4;
          A* mine = lv == 3 ? acc3 : acc4;
          const int bh = PY_TH >> lv, bw = PY_TW >> lv;      // this level's [TD >> lv][bh][bw] inside the tile
          const int cnt = (g.TD >> lv) * bh * bw;
          if (tid < cnt) {
            const int cw = tid % bw, ch = (tid / bw) % bh, cd = tid / (bw * bh);
            A s = py_identity<INT, MODE>();
#pragma unroll
            for (int q = 0; q < 8; ++q)
              py_merge<MODE, A>(s, below[((2 * cd + (q >> 2)) * (2 * bh) + 2 * ch + ((q >> 1) & 1)) * (2 * bw) + 2 * cw + (q & 1)]);
            if (lv + 1 < L) mine[(cd * bh + ch) * bw + cw] = s;
            const int Dl = gD >> lv, Hl = gH >> lv, Wl = gW >> lv;
            const int dl = (D0 >> lv) + cd, hl = (H0 >> lv) + ch, wl = (W0 >> lv) + cw;
            if (dl < Dl && hl < Hl && wl < Wl) {
              const int64_t at = ((sample * Dl + dl) * Hl + hl) * Wl + wl;
              const O o = py_finish<O, INT, MODE, A>(s, lv, sc);
              ((O*)out.p[lv])[at] = o;
              if constexpr (STATS_OK)
                if (do_stats) {
                  py_stat one;
                  one.clear();
                  one.add((int32_t)o);
                  py_stat_to_lds(one, st + 4 * lv);
                }
            }
          }
          __syncthreads();
        }
      }
    }
  }

  if constexpr (STATS_OK) {
    if (do_stats) {      // (uniform)
#pragma unroll
      for (int lv = 0; lv < 3; ++lv)
        if (lv < g.levels) py_stat_wave_to_lds(sa[lv], st + 4 * lv);
      __syncthreads();
      py_stat_flush(st, g.levels, stats + sample * g.levels * 4);
    }
  }
}

struct py_args {
  int64_t n, sd, sh, sw, D, H, W, od, oh, ow;
  int32_t levels, mode;
  int32_t ii, ip, ilo, ihi;
  float fi, fp, flo, fhi;
  py_out out;
  int64_t* stats;
};

int py_stats_init(int64_t* stats, int64_t slots, hipStream_t hs) {
  if (!stats || slots == 0) return SG_OK;
  hipLaunchKernelGGL(pyramid_stats_init_kernel, dim3((unsigned)((slots * 4 + 255) / 256)), dim3(256), 0, hs, stats, slots);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

template <typename S, typename O, int MODE>
int py_launch3(const void* x, const py_args& q, hipStream_t hs) {
  constexpr bool INT = py_int<S>;
  py_geom g;
  g.sd = (int32_t)q.sd; g.sh = (int32_t)q.sh; g.sw = (int32_t)q.sw; g.D = (int32_t)q.D; g.H = (int32_t)q.H; g.W = (int32_t)q.W;
  g.od = (int32_t)q.od; g.oh = (int32_t)q.oh; g.ow = (int32_t)q.ow;
  g.levels = q.levels;
  const int brick = 1 << (q.levels - 1);
  g.TD = brick > PY_SD ? brick : PY_SD;
  const int64_t tiles_d = (q.D + g.TD - 1) / g.TD;
  const int64_t tiles_h = (q.H + PY_TH - 1) / PY_TH, tiles_w = (q.W + PY_TW - 1) / PY_TW, tiles = tiles_d * tiles_h * tiles_w;
  const int64_t chunks = tiles;      // one block per (sample, tile)
  if (tiles > (int64_t)INT32_MAX || q.n * chunks > (int64_t)INT32_MAX) return SG_EINVAL;
  g.tiles_h = (uint32_t)tiles_h; g.tiles_w = (uint32_t)tiles_w; g.tiles = (uint32_t)tiles; g.chunks = (uint32_t)chunks;
  py_scal<INT> sc;
  if constexpr (INT) { sc.intercept = q.ii; sc.pad = q.ip; sc.lo = q.ilo; sc.hi = q.ihi; }
  else { sc.intercept = q.fi; sc.pad = q.fp; sc.lo = q.flo; sc.hi = q.fhi; }
  int64_t* stats = std::is_same_v<O, float> ? nullptr : q.stats;
  const int rc = py_stats_init(stats, q.n * q.levels, hs);
  if (rc != SG_OK) return rc;
  hipLaunchKernelGGL((pyramid_kernel<S, O, MODE>), dim3((unsigned)(q.n * g.chunks)), dim3(PY_THREADS), 0, hs, (const S*)x, g, sc,
                     q.out, stats);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

template <typename S, typename O>
int py_launch2(const void* x, const py_args& q, hipStream_t hs) {
  return q.mode == SG_PYR_MAX ? py_launch3<S, O, SG_PYR_MAX>(x, q, hs) : py_launch3<S, O, SG_PYR_MEAN>(x, q, hs);
}

template <typename S>
int py_launch(const void* x, sg_src_dtype odt, const py_args& q, hipStream_t hs) {
  if constexpr (py_int<S>) {
    if (odt == SG_SRC_U16) return py_launch2<S, uint16_t>(x, q, hs);
    if (odt == SG_SRC_I16) return py_launch2<S, int16_t>(x, q, hs);
  }
  return py_launch2<S, float>(x, q, hs);
}

bool py_is_int_dt(sg_src_dtype dt) { return dt == SG_SRC_U8 || dt == SG_SRC_I8 || dt == SG_SRC_I16 || dt == SG_SRC_U16; }

// the checks both entry points share; SG_OK: go on
int py_check_common(sg_src_dtype dt, int32_t levels, int32_t mode, sg_src_dtype odt, const py_args& q) {
  if ((int)dt < (int)SG_SRC_U8 || (int)dt > (int)SG_SRC_F32) return SG_EINVAL;      // (bf16: not a source here)
  if (levels < 1 || levels > PY_MAXL) return SG_EINVAL;
  if (mode != SG_PYR_MEAN && mode != SG_PYR_MAX) return SG_EINVAL;
  if (odt != SG_SRC_U16 && odt != SG_SRC_I16 && odt != SG_SRC_F32) return SG_EINVAL;
  if (py_is_int_dt(dt)) {
    if (q.ilo > q.ihi) return SG_EINVAL;
    if (odt == SG_SRC_U16 && (q.ilo < 0 || q.ihi > 65535)) return SG_EINVAL;
    if (odt == SG_SRC_I16 && (q.ilo < -32768 || q.ihi > 32767)) return SG_EINVAL;
    // v = x - intercept and pad_value - intercept stay 32-bit integers
    if (q.ii < -(1 << 30) || q.ii > (1 << 30) || q.ip < -(1 << 30) || q.ip > (1 << 30)) return SG_EINVAL;
  } else {
    if (odt != SG_SRC_F32) return SG_EINVAL;
    if (!(q.flo <= q.fhi)) return SG_EINVAL;      // (a NaN bound too)
  }
  return SG_OK;
}

}  // namespace

extern "C" int sg_block_pyramid(const void* x, sg_src_dtype dt, int64_t n, int64_t sd, int64_t sh, int64_t sw, int64_t D, int64_t H,
                                int64_t W, int64_t off_d, int64_t off_h, int64_t off_w, int32_t levels, int32_t mode,
                                int32_t intercept_i, int32_t pad_i, int32_t clip_lo_i, int32_t clip_hi_i, float intercept_f,
                                float pad_f, float clip_lo_f, float clip_hi_f, sg_src_dtype out_dt, void* const* out, int64_t* stats,
                                sg_stream_t st) {
  py_args q;
  q.n = n; q.sd = sd; q.sh = sh; q.sw = sw; q.D = D; q.H = H; q.W = W; q.od = off_d; q.oh = off_h; q.ow = off_w;
  q.levels = levels; q.mode = mode;
  q.ii = intercept_i; q.ip = pad_i; q.ilo = clip_lo_i; q.ihi = clip_hi_i;
  q.fi = intercept_f; q.fp = pad_f; q.flo = clip_lo_f; q.fhi = clip_hi_f;
  q.stats = stats;
  if (n < 0 || sd < 0 || sh < 0 || sw < 0 || D < 0 || H < 0 || W < 0) return SG_EINVAL;
  const int rc = py_check_common(dt, levels, mode, out_dt, q);
  if (rc != SG_OK) return rc;
  const int64_t brick = (int64_t)1 << (levels - 1);
  if (D % brick || H % brick || W % brick) return SG_EINVAL;
  // extents and offsets that are 32-bit coordinates in the kernel
  const int64_t big = (int64_t)1 << 29;
  for (int64_t v : {sd, sh, sw, D, H, W, off_d, off_h, off_w})
    if (v > big || v < -big) return SG_EINVAL;
  typedef __int128 i128;
  if ((i128)n * sd * sh * sw > (i128)INT64_MAX / 8 || (i128)n * D * H * W > (i128)INT64_MAX / 8) return SG_EINVAL;
  if (n == 0 || D == 0 || H == 0 || W == 0) return SG_OK;
  if (!out) return SG_EINVAL;
  const bool has_source = sd > 0 && sh > 0 && sw > 0;
  if (has_source && !x) return SG_EINVAL;
  static const size_t esize[] = {1, 1, 2, 2, 2, 4};
  const size_t osize = out_dt == SG_SRC_F32 ? 4 : 2;
  for (int i = 0; i < levels; ++i) {
    if (!out[i]) return SG_EINVAL;
    if (((uintptr_t)out[i]) % osize != 0) return SG_EALIGN;
    q.out.p[i] = out[i];
  }
  for (int i = levels; i < PY_MAXL; ++i) q.out.p[i] = nullptr;
  if (x && ((uintptr_t)x) % esize[(int)dt] != 0) return SG_EALIGN;
  if (stats && ((uintptr_t)stats) % 8 != 0) return SG_EALIGN;
  hipStream_t hs = sg_st(st);
  switch (dt) {
    case SG_SRC_U8:  return py_launch<uint8_t>(x, out_dt, q, hs);
    case SG_SRC_I8:  return py_launch<int8_t>(x, out_dt, q, hs);
    case SG_SRC_I16: return py_launch<int16_t>(x, out_dt, q, hs);
    case SG_SRC_U16: return py_launch<uint16_t>(x, out_dt, q, hs);
    case SG_SRC_F16: return py_launch<_Float16>(x, out_dt, q, hs);
    case SG_SRC_F32: return py_launch<float>(x, out_dt, q, hs);
    default: break;
  }
  return SG_EINVAL;
}
