// Squared Euclidean distances between every pair of volumes (metrics/sample_metrics.py: kernel MMD, 1-NN two-sample
// accuracy, k-NN precision / recall):  out[i][j] = max(0, |a_i|^2 + |b_j|^2 - 2 a_i.b_j),  a [ma, v], b [mb, v] f32, out f64.
// The shape is a skinny, very deep GEMM (tens to a few thousand rows, 0.5M - 4M voxels per row), so:
//   * the dot products run on v_mfma_f32_32x32x2_f32 (exact f32 products in an f32 fmaf chain, the f32 vector rate) over
//     PD_CHUNK consecutive voxels at most; every chunk's accumulators are then added into f64 registers;
//   * the grid comes from splitting K: block (tile, split) writes its f64 tile to the workspace, pdist_final_kernel adds a
//     tile's splits in ascending order -- no atomics, the same bits on every call;
//   * the row norms are summed in f64 from the start (pdist_norm_kernel, products of two f32 are exact in f64), over the
//     same K splits, and the combination is f64;
//   * b == a: only tiles on and above the diagonal are computed, element (i, j) with i > j is read from where (j, i) was
//     written, and the diagonal is written as 0.
// Block = 4 waves in 2 x 2, each wave R x R accumulators of 32 x 32 (R = 1 up to 64 rows a side, else 2: a 64 x 64 or a
// 128 x 128 tile).  A K step is 32 voxels: the next step's global loads are issued before the MFMAs of the current one
// and written to LDS after them.  Within a K step lane half h multiplies voxels 8g + 4h + e (g, e < 4) of both operands:
// one 16-byte LDS read per 4 MFMAs; the order inside a chunk does not matter to the sum's bound.
// Rows past ma / mb and voxels past the split's end are staged as zeros (fma(0, 0, c) == c), never read from memory.
#include "common.h"

namespace {

constexpr int PD_CHUNK = 1024;   // longest f32 accumulation chain, in voxels (9 * PD_CHUNK < 2^24: small integers stay exact)
constexpr int PD_BK = 32;        // voxels per K step
constexpr int PD_LDS_ROW = 36;   // floats per staged row: 16-byte aligned, 9 sixteen-byte slots -> rows spread over the banks
constexpr int PD_MAX_ROUNDS = 6;  // most rounds of the chip (blocks / CUs) a K split may be chosen for

struct PdPlan {
  int R, BM, nti, ntj, sym;
  int64_t tiles;
  int S;           // K splits
  int64_t span;    // voxels per split (a multiple of PD_CHUNK)
  size_t dot_doubles, norm_doubles;
};

int pd_cus() {
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

PdPlan pd_plan(int32_t ma, int32_t mb, int64_t v, bool sym) {
  PdPlan p;
  p.sym = sym ? 1 : 0;
  p.R = (ma > 64 || mb > 64) ? 2 : 1;
  p.BM = 64 * p.R;
  p.nti = (ma + p.BM - 1) / p.BM;
  p.ntj = (mb + p.BM - 1) / p.BM;
  p.tiles = sym ? (int64_t)p.nti * (p.nti + 1) / 2 : (int64_t)p.nti * p.ntj;
  const int64_t chunks = (v + PD_CHUNK - 1) / PD_CHUNK;
  // tiles x splits = a small multiple of the CU count (the 128 x 128 kernel holds one block per CU): among the splits that
  // keep the grid within PD_MAX_ROUNDS rounds of the chip, the smallest whose last round is filled to within 5 % of the
  // best filling.  The bound on the grid bounds the workspace: at most max(tiles, PD_MAX_ROUNDS * CUs) partial tiles.
  const int64_t cus = pd_cus();
  int64_t smax = PD_MAX_ROUNDS * cus / p.tiles;
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
  p.span = per * PD_CHUNK;
  p.dot_doubles = (size_t)p.tiles * p.S * p.BM * p.BM;
  p.norm_doubles = (size_t)(sym ? ma : (int64_t)ma + mb) * p.S;
  return p;
}

// upper-triangle tile (ti <= tj) of an nt x nt grid <-> linear index, rows first
__host__ __device__ __forceinline__ int64_t pd_tri_index(int ti, int tj, int nt) {
  return (int64_t)ti * nt - (int64_t)ti * (ti - 1) / 2 + (tj - ti);
}

template <int R, bool VEC>
__global__ __launch_bounds__(256) void pdist_dot_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                        double* __restrict__ ws, int ma, int mb, int64_t v, int nt_j,
                                                        int sym, int64_t span) {
  constexpr int BM = 64 * R;
  constexpr int NL = BM * PD_BK / 256;      // floats per thread and operand per K step
  __shared__ __attribute__((aligned(16))) float lds[2][BM][PD_LDS_ROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 31, lh = lane >> 5;

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
  const int row_a0 = ti * BM, row_b0 = tj * BM;

  float ra[NL], rb[NL];
  auto load = [&](int64_t k0) {
    if (VEC) {
#pragma unroll
      for (int i = 0; i < NL / 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 3, c = (idx & 7) * 4;
        const int64_t k = k0 + c;
        f32x4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
        if (k < k_end) {     // v % 4 == 0 and k % 4 == 0: the four voxels are inside together
          if (row_a0 + r < ma) va = *reinterpret_cast<const f32x4*>(a + (int64_t)(row_a0 + r) * v + k);
          if (row_b0 + r < mb) vb = *reinterpret_cast<const f32x4*>(b + (int64_t)(row_b0 + r) * v + k);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { ra[4 * i + e] = va[e]; rb[4 * i + e] = vb[e]; }
      }
    } else {
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int idx = tid + 256 * i, r = idx >> 5, c = idx & 31;
        const int64_t k = k0 + c;
        ra[i] = (k < k_end && row_a0 + r < ma) ? a[(int64_t)(row_a0 + r) * v + k] : 0.f;
        rb[i] = (k < k_end && row_b0 + r < mb) ? b[(int64_t)(row_b0 + r) * v + k] : 0.f;
      }
    }
  };
  auto stage = [&]() {
    if (VEC) {
#pragma unroll
      for (int i = 0; i < NL / 4; ++i) {
        const int idx = tid + 256 * i, r = idx >> 3, c = (idx & 7) * 4;
        const f32x4 va = {ra[4 * i], ra[4 * i + 1], ra[4 * i + 2], ra[4 * i + 3]};
        const f32x4 vb = {rb[4 * i], rb[4 * i + 1], rb[4 * i + 2], rb[4 * i + 3]};
        *reinterpret_cast<f32x4*>(&lds[0][r][c]) = va;
        *reinterpret_cast<f32x4*>(&lds[1][r][c]) = vb;
      }
    } else {
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int idx = tid + 256 * i, r = idx >> 5, c = idx & 31;
        lds[0][r][c] = ra[i];
        lds[1][r][c] = rb[i];
      }
    }
  };

  f32x16 acc[R][R];
  double dacc[R][R][16];
#pragma unroll
  for (int m = 0; m < R; ++m)
#pragma unroll
    for (int n = 0; n < R; ++n) {
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc[m][n][e] = 0.f; dacc[m][n][e] = 0.0; }
    }
  const int wr = (wave >> 1) * 32 * R, wc = (wave & 1) * 32 * R;

  load(k_begin);
  int in_chunk = 0;
  for (int64_t k0 = k_begin; k0 < k_end; k0 += PD_BK) {
    __syncthreads();      // the previous step's fragment reads are done
    stage();
    __syncthreads();
    if (k0 + PD_BK < k_end) load(k0 + PD_BK);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      f32x4 fa[R], fb[R];
#pragma unroll
      for (int m = 0; m < R; ++m) fa[m] = *reinterpret_cast<const f32x4*>(&lds[0][wr + 32 * m + lr][8 * g + 4 * lh]);
#pragma unroll
      for (int n = 0; n < R; ++n) fb[n] = *reinterpret_cast<const f32x4*>(&lds[1][wc + 32 * n + lr][8 * g + 4 * lh]);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int m = 0; m < R; ++m)
#pragma unroll
          for (int n = 0; n < R; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[m][e], fb[n][e], acc[m][n], 0, 0, 0);
    }
    if (++in_chunk == PD_CHUNK / PD_BK) {      // the split starts on a chunk boundary: at most PD_CHUNK voxels per chain
      in_chunk = 0;
#pragma unroll
      for (int m = 0; m < R; ++m)
#pragma unroll
        for (int n = 0; n < R; ++n) {
#pragma unroll
          for (int e = 0; e < 16; ++e) { dacc[m][n][e] += (double)acc[m][n][e]; acc[m][n][e] = 0.f; }
        }
    }
  }
  // C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  double* tile = ws + ((int64_t)blockIdx.x * gridDim.y + split) * (int64_t)(BM * BM);
#pragma unroll
  for (int m = 0; m < R; ++m)
#pragma unroll
    for (int n = 0; n < R; ++n) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int row = wr + 32 * m + (e & 3) + 8 * (e >> 2) + 4 * lh, col = wc + 32 * n + lr;
        tile[row * BM + col] = dacc[m][n][e] + (double)acc[m][n][e];
      }
    }
}

// nws[row * S + split] = sum over the split's voxels of x^2 in f64; rows ma.. are b's.  One block per (row, split); every
// thread's stride-256 sum, the wave shuffles and the 4 wave sums are added in a fixed order.
__global__ __launch_bounds__(256) void pdist_norm_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         double* __restrict__ nws, int ma, int64_t v, int64_t span) {
  __shared__ double sh[4];
  const int row = blockIdx.x, split = blockIdx.y;
  const float* x = row < ma ? a + (int64_t)row * v : b + (int64_t)(row - ma) * v;
  const int64_t k_begin = (int64_t)split * span;
  const int64_t k_end = k_begin + span < v ? k_begin + span : v;
  double s = 0.0;
  for (int64_t k = k_begin + threadIdx.x; k < k_end; k += 256) {
    const double t = (double)x[k];
    s += t * t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) nws[(int64_t)row * gridDim.y + split] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void pdist_final_kernel(const double* __restrict__ ws, const double* __restrict__ nws,
                                                          double* __restrict__ out, int ma, int mb, int BM, int nt_j,
                                                          int sym, int S) {
  const int64_t total = (int64_t)ma * mb;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
    const int i = (int)(e / mb), j = (int)(e - (int64_t)i * mb);
    if (sym && i == j) { out[e] = 0.0; continue; }
    const int p = (sym && i > j) ? j : i, q = (sym && i > j) ? i : j;     // the lower half reads what the upper half wrote
    const int ti = p / BM, tj = q / BM;
    const int64_t t = sym ? pd_tri_index(ti, tj, nt_j) : (int64_t)ti * nt_j + tj;
    const double* src = ws + t * S * (int64_t)(BM * BM) + (int64_t)(p - ti * BM) * BM + (q - tj * BM);
    const double* np_ = nws + (int64_t)p * S;
    const double* nq_ = nws + (int64_t)(sym ? q : ma + q) * S;
    double dot = 0.0, np = 0.0, nq = 0.0;
    for (int s = 0; s < S; ++s) {
      dot += src[(int64_t)s * (BM * BM)];
      np += np_[s];
      nq += nq_[s];
    }
    const double d = (np + nq) - 2.0 * dot;
    out[e] = d < 0.0 ? 0.0 : d;
  }
}

template <int R>
void pd_launch_dot(const PdPlan& p, bool vec, const float* a, const float* b, double* ws, int32_t ma, int32_t mb, int64_t v,
                   hipStream_t st) {
  const dim3 grid((unsigned)p.tiles, (unsigned)p.S);
  if (vec)
    hipLaunchKernelGGL((pdist_dot_kernel<R, true>), grid, dim3(256), 0, st, a, b, ws, ma, mb, v, p.ntj, p.sym, p.span);
  else
    hipLaunchKernelGGL((pdist_dot_kernel<R, false>), grid, dim3(256), 0, st, a, b, ws, ma, mb, v, p.ntj, p.sym, p.span);
}

}  // namespace

extern "C" {

int32_t sg_pairwise_sqdist_chunk(void) { return PD_CHUNK; }

size_t sg_pairwise_sqdist_workspace(int32_t ma, int32_t mb, int64_t v) {
  if (ma < 1 || mb < 1 || v < 1) return 0;
  // the caller may pass b == a: fewer tiles, but possibly more splits
  const PdPlan p = pd_plan(ma, mb, v, false);
  size_t n = p.dot_doubles + p.norm_doubles;
  if (ma == mb) {
    const PdPlan q = pd_plan(ma, mb, v, true);
    if (q.dot_doubles + q.norm_doubles > n) n = q.dot_doubles + q.norm_doubles;
  }
  return n * sizeof(double);
}

int sg_pairwise_sqdist(const float* a, const float* b, double* out, int32_t ma, int32_t mb, int64_t v, void* workspace,
                       size_t workspace_bytes, sg_stream_t st) {
  if (a == nullptr || b == nullptr || out == nullptr || workspace == nullptr) return SG_EINVAL;
  if (ma < 1 || mb < 1 || v < 1) return SG_EINVAL;
  if ((((uintptr_t)a | (uintptr_t)b) & 3) != 0 || (((uintptr_t)out | (uintptr_t)workspace) & 7) != 0) return SG_EALIGN;
  const bool sym = a == b && ma == mb;
  const PdPlan p = pd_plan(ma, mb, v, sym);
  if (p.tiles > 0x7FFFFFFF) return SG_EINVAL;
  if (workspace_bytes < (p.dot_doubles + p.norm_doubles) * sizeof(double)) return SG_EWORKSPACE;
  double* ws = reinterpret_cast<double*>(workspace);
  double* nws = ws + p.dot_doubles;
  const bool vec = (v & 3) == 0 && sg_aligned16(a) && sg_aligned16(b);
  hipLaunchKernelGGL(pdist_norm_kernel, dim3((unsigned)(sym ? ma : ma + mb), (unsigned)p.S), dim3(256), 0, sg_st(st), a, b,
                     nws, ma, v, p.span);
  SG_LAUNCH_CHECK();
  if (p.R == 1) pd_launch_dot<1>(p, vec, a, b, ws, ma, mb, v, sg_st(st));
  else pd_launch_dot<2>(p, vec, a, b, ws, ma, mb, v, sg_st(st));
  SG_LAUNCH_CHECK();
  const int64_t total = (int64_t)ma * mb;
  const int64_t blocks = (total + 255) / 256;
  hipLaunchKernelGGL(pdist_final_kernel, dim3((unsigned)(blocks < 16384 ? blocks : 16384)), dim3(256), 0, sg_st(st), ws, nws,
                     out, ma, mb, p.BM, p.ntj, p.sym, p.S);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

}  // extern "C"
