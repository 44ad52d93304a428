// Projection of volumes onto the generator (project.py): the multi-scale residual loss with its gradient, one read
// of each operand and one write, and the per-sample update of the latents.
//
// sg_multiscale_residual.  Per sample i, with x = table[idx[i]] in its stored type and y the generator's output:
//   t = (f32(x) - mean) / stddev       two correctly rounded f32 operations, as sg_gather_rows
//   r = f32(y) - t                     one rounding
//   S_0 = f64(r); S_l(B) of a cube B of edge 2^l = the sum of its eight children's S_(l-1) in the octree's order: the w pairs
//                                      first, then the h pairs, then the d pair -- ((a + b) + (c + d)) + ((e + f) + (g + h))
//   m_l(B) = S_l(B) * 8^-l             exact
//   Q_l = m_l^2, carried up the SAME tree to the cubes of edge 8 that tile the volume from its origin (a child outside the
//                                      volume counts as +0); the cubes of a sample are then added along w, those sums along h and
//                                      those over (channel, d) in index order, each sum sequential from its first element
//   terms[i][l] = that total / N_l     N_l = c d h w / 8^l, the number of cubes of level l
//   loss[i] = f32(lambda_0 terms_0 + lambda_1 terms_1 + ...)            f64, in this order
//   grad[v] = round(k_0 r + (k_1 m_1 + (k_2 m_2 + k_3 m_3)))            f64, from the coarsest level down, k_l = lambda_l (2 / N_l)
//                                      / 8^l (given by the caller); rounded ONCE to y's type: f64 -> f32 for f32, and for bf16 /
//                                      f16 through an f32 rounded to odd, which makes the second rounding the only one
// Nothing in this depends on the launch: two calls give the same bits, and the numpy twin (table_ops._msr_numpy) gives them too.
// The file is built with -ffp-contract=off, and every product that feeds a sum is written __dmul_rn / __dadd_rn as well.
//
// A wave owns a strip of eight edge-8 cubes along w: lane = 8 hh + cw reads, for the eight planes of the strip, the eight
// consecutive w elements of row hh of cube cw -- 16 bytes of a 2-byte type, so eight lanes read 128 consecutive bytes of a row.
// The w and d steps of the octree are sums inside a lane, the h steps are exchanges with the lanes 8, 16 and 32 away (addition
// commutes, so both lanes of a pair hold the same bits afterwards).  The residuals stay in registers between the reduction and
// the gradient: no LDS, no second read.  Per cube and level one f64 goes to a workspace; a second small launch (one block per
// sample) adds them in the defined order.  Aligned path: whole 8-element loads and stores (W % 8 == 0, bases aligned to eight
// elements, NCDHW or one channel); element path otherwise (any extent, any alignment, channels-last).  64-bit offsets throughout.
// A position outside the table is never formed into an address: its targets read as NaN, which the arithmetic carries into
// every gradient, term and the loss of that sample.
//
// sg_latent_step: one wave per sample; see include/saragan_hip.h for the order of the operations.
#include "common.h"
#include <math.h>
#include <type_traits>

namespace {

constexpr int MSR_MAX_LEVELS = 4;      // the cube a wave reduces in registers has edge 8 = 2^(4 - 1)

struct pj_bf16 { uint16_t bits; };

template <typename T>
__device__ __forceinline__ float pj_to_f(T v) { return (float)v; }      // exact for every type below
template <>
__device__ __forceinline__ float pj_to_f<pj_bf16>(pj_bf16 v) { return __uint_as_float((uint32_t)v.bits << 16); }

// f64 -> f32 rounded to odd: the truncated value, its last bit set when anything was cut off.  A following rounding to nearest
// even into a type with at least two bits fewer equals ONE rounding of the f64.
__device__ __forceinline__ float pj_round_odd(double x) {
  const float f = __double2float_rz(x);
  uint32_t b = __float_as_uint(f);
  if ((double)f != x) b |= 1u;      // (a NaN stays a NaN)
  return __uint_as_float(b);
}

template <typename Y>
__device__ __forceinline__ Y pj_from_d(double g) {
  if constexpr (std::is_same_v<Y, float>) {
    return (float)g;
  } else if constexpr (std::is_same_v<Y, pj_bf16>) {
    const float f = pj_round_odd(g);
    const uint32_t b = __float_as_uint(f);
    pj_bf16 o;
    if (f != f) o.bits = 0x7FC0u;
    else o.bits = (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16);      // to nearest, ties to even
    return o;
  } else {
    return (_Float16)pj_round_odd(g);
  }
}

template <typename T>
struct alignas(sizeof(T) * 8 > 16 ? 16 : sizeof(T) * 8) pj_pack8 { T v[8]; };

struct msr_args {
  const void* y;
  const void* table;
  const int32_t* idx;
  void* grad;
  double* part;      // [n][levels][cubes]
  int64_t rows, n, c, d, h, w;
  int64_t nd8, nh8, nw8, strips, waves;
  int32_t levels, channels_last;
  float mean, stddev;
  double k[MSR_MAX_LEVELS];
};

__device__ __forceinline__ double pj_shfl_xor(double v, int mask) { return __shfl_xor(v, mask, 64); }

// one step up the octree of a lane's [D][W] cells; the h pair sits `hmask` lanes away
template <int D, int W>
__device__ __forceinline__ void pj_up(const double (&in)[D][W], double (&out)[D / 2][W / 2], int hmask) {
#pragma unroll
  for (int dp = 0; dp < D / 2; ++dp) {
#pragma unroll
    for (int wc = 0; wc < W / 2; ++wc) {
      double a0 = __dadd_rn(in[2 * dp][2 * wc], in[2 * dp][2 * wc + 1]);
      double a1 = __dadd_rn(in[2 * dp + 1][2 * wc], in[2 * dp + 1][2 * wc + 1]);
      a0 = __dadd_rn(a0, pj_shfl_xor(a0, hmask));
      a1 = __dadd_rn(a1, pj_shfl_xor(a1, hmask));
      out[dp][wc] = __dadd_rn(a0, a1);
    }
  }
}

template <typename Y, typename S, bool VEC>
__global__ __launch_bounds__(256) void multiscale_residual_kernel(msr_args a) {
  const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (wv >= a.waves) return;      // (whole waves leave; nothing below synchronises a block)
  const int lane = threadIdx.x & 63, cw = lane & 7, hh = lane >> 3;
  int64_t t = wv;
  const int64_t strip = t % a.strips; t /= a.strips;
  const int64_t bh = t % a.nh8; t /= a.nh8;
  const int64_t bd = t % a.nd8; t /= a.nd8;
  const int64_t ch = t % a.c;
  const int64_t i = t / a.c;
  const int64_t bw = strip * 8 + cw, w0 = bw * 8, hrow = bh * 8 + hh, d0 = bd * 8;
  const int64_t V = a.d * a.h * a.w;
  const int64_t row = a.idx[i];
  const bool inside = row >= 0 && row < a.rows;      // (wave-uniform)
  const bool lane_ok = bw < a.nw8 && hrow < a.h;
  const Y* __restrict__ y = (const Y*)a.y;
  Y* __restrict__ grad = (Y*)a.grad;
  const S* __restrict__ tab = (const S*)a.table;
  // element (dd, j) of this lane: voxel ((d0 + dd) * h + hrow) * w + w0 + j of channel ch
  const int64_t es = a.channels_last ? a.c : 1;                                     // between the voxels of y / grad
  const int64_t ybase = a.channels_last ? i * a.c * V * 1 + ch : (i * a.c + ch) * V;      // + voxel * es
  const int64_t tbase = inside ? (row * a.c + ch) * V : 0;
  const float qnan = __builtin_nanf("");

  float r[8][8];
#pragma unroll
  for (int dd = 0; dd < 8; ++dd) {
    const bool ok = lane_ok && d0 + dd < a.d;
    const int64_t vox = ((d0 + dd) * a.h + hrow) * a.w + w0;
    if constexpr (VEC) {
      if (ok) {
        const pj_pack8<Y> py = *reinterpret_cast<const pj_pack8<Y>*>(y + ybase + vox);
        pj_pack8<S> pt;
        if (inside) pt = *reinterpret_cast<const pj_pack8<S>*>(tab + tbase + vox);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float tv = inside ? __fdiv_rn(__fsub_rn(pj_to_f(pt.v[j]), a.mean), a.stddev) : qnan;
          r[dd][j] = __fsub_rn(pj_to_f(py.v[j]), tv);
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) r[dd][j] = 0.f;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float v = 0.f;
        if (ok && w0 + j < a.w) {
          const float tv = inside ? __fdiv_rn(__fsub_rn(pj_to_f(tab[tbase + vox + j]), a.mean), a.stddev) : qnan;
          v = __fsub_rn(pj_to_f(y[ybase + (vox + j) * es]), tv);
        }
        r[dd][j] = v;
      }
    }
  }

  // ---- up the octree: s1 .. s3 the sums, q<l> the squares of level l carried to the level reached so far.  Level 1 is formed
  // plane pair by plane pair, so that no f64 image of the 64 residuals is ever live.
  double s1[4][4], q0a[4][4];
#pragma unroll
  for (int dp = 0; dp < 4; ++dp) {
#pragma unroll
    for (int wc = 0; wc < 4; ++wc) {
      const double e0 = (double)r[2 * dp][2 * wc], e1 = (double)r[2 * dp][2 * wc + 1];
      const double f0 = (double)r[2 * dp + 1][2 * wc], f1 = (double)r[2 * dp + 1][2 * wc + 1];
      double a0 = __dadd_rn(__dmul_rn(e0, e0), __dmul_rn(e1, e1)), a1 = __dadd_rn(__dmul_rn(f0, f0), __dmul_rn(f1, f1));
      a0 = __dadd_rn(a0, pj_shfl_xor(a0, 8));
      a1 = __dadd_rn(a1, pj_shfl_xor(a1, 8));
      q0a[dp][wc] = __dadd_rn(a0, a1);
      if (a.levels > 1) {
        double b0 = __dadd_rn(e0, e1), b1 = __dadd_rn(f0, f1);
        b0 = __dadd_rn(b0, pj_shfl_xor(b0, 8));
        b1 = __dadd_rn(b1, pj_shfl_xor(b1, 8));
        s1[dp][wc] = __dadd_rn(b0, b1);
      }
    }
  }
  double q0b[2][2], q1b[2][2], s2[2][2];
  pj_up<4, 4>(q0a, q0b, 16);
  if (a.levels > 1) {
    double m2[4][4];
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double m = __dmul_rn(s1[p][k], 0.125);
        m2[p][k] = __dmul_rn(m, m);
      }
    pj_up<4, 4>(m2, q1b, 16);
  }
  if (a.levels > 2) pj_up<4, 4>(s1, s2, 16);
  double q0c[1][1], q1c[1][1], q2c[1][1], s3[1][1];
  pj_up<2, 2>(q0b, q0c, 32);
  if (a.levels > 1) pj_up<2, 2>(q1b, q1c, 32);
  if (a.levels > 2) {
    double m2[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const double m = __dmul_rn(s2[p][k], 0.015625);
        m2[p][k] = __dmul_rn(m, m);
      }
    pj_up<2, 2>(m2, q2c, 32);
  }
  double q3 = 0.0, m3 = 0.0;
  if (a.levels > 3) {
    pj_up<2, 2>(s2, s3, 32);
    m3 = __dmul_rn(s3[0][0], 0.001953125);
    q3 = __dmul_rn(m3, m3);
  }
  // every lane of a cube's eight rows holds the cube's totals: row 0 writes them
  if (hh == 0 && bw < a.nw8) {
    const int64_t cubes = a.c * a.nd8 * a.nh8 * a.nw8;
    const int64_t cube = ((ch * a.nd8 + bd) * a.nh8 + bh) * a.nw8 + bw;
    double* __restrict__ p = a.part + i * a.levels * cubes + cube;
    p[0] = q0c[0][0];
    if (a.levels > 1) p[cubes] = q1c[0][0];
    if (a.levels > 2) p[2 * cubes] = q2c[0][0];
    if (a.levels > 3) p[3 * cubes] = q3;
  }

  // ---- the gradient, from the coarsest level down
  const double g3 = __dmul_rn(a.k[3], m3);
#pragma unroll
  for (int dd = 0; dd < 8; ++dd) {
    Y out[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double g = __dmul_rn(a.k[0], (double)r[dd][j]);
      if (a.levels > 1) {
        double up = __dmul_rn(a.k[1], __dmul_rn(s1[dd >> 1][j >> 1], 0.125));
        if (a.levels > 2) {
          double up2 = __dmul_rn(a.k[2], __dmul_rn(s2[dd >> 2][j >> 2], 0.015625));
          if (a.levels > 3) up2 = __dadd_rn(up2, g3);
          up = __dadd_rn(up, up2);
        }
        g = __dadd_rn(g, up);
      }
      out[j] = pj_from_d<Y>(g);
    }
    const bool ok = lane_ok && d0 + dd < a.d;
    const int64_t vox = ((d0 + dd) * a.h + hrow) * a.w + w0;
    if constexpr (VEC) {
      if (ok) {
        constexpr int NS = (int)sizeof(Y) * 8 / 16;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
          u32x4 wd;
          __builtin_memcpy(&wd, reinterpret_cast<const char*>(out) + 16 * s, 16);
          *reinterpret_cast<u32x4*>(reinterpret_cast<char*>(grad + ybase + vox) + 16 * s) = wd;
          SG_STORE16_GUARD(wd);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (ok && w0 + j < a.w) grad[ybase + (vox + j) * es] = out[j];
    }
  }
}

// one block per sample: the cubes' partial sums added along w, then along h, then over (channel, d), each in index order
__global__ __launch_bounds__(256) void multiscale_finish_kernel(double* __restrict__ part, int64_t rows_cd, int64_t nh8, int64_t nw8,
                                                                int32_t levels, const float* __restrict__ lambda, double n0,
                                                                double* __restrict__ terms, float* __restrict__ loss) {
  const int64_t i = blockIdx.x, cubes = rows_cd * nh8 * nw8;
  double* __restrict__ p = part + i * levels * cubes;
  for (int l = 0; l < levels; ++l) {
    double* __restrict__ q = p + (int64_t)l * cubes;
    for (int64_t rw = threadIdx.x; rw < rows_cd * nh8; rw += blockDim.x) {
      double acc = q[rw * nw8];
      for (int64_t k = 1; k < nw8; ++k) acc = __dadd_rn(acc, q[rw * nw8 + k]);
      q[rw * nw8] = acc;
    }
  }
  __syncthreads();
  for (int l = 0; l < levels; ++l) {
    double* __restrict__ q = p + (int64_t)l * cubes;
    for (int64_t pl = threadIdx.x; pl < rows_cd; pl += blockDim.x) {
      double acc = q[pl * nh8 * nw8];
      for (int64_t k = 1; k < nh8; ++k) acc = __dadd_rn(acc, q[(pl * nh8 + k) * nw8]);
      q[pl * nh8 * nw8] = acc;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0, nl = n0;
    for (int l = 0; l < levels; ++l) {
      const double* __restrict__ q = p + (int64_t)l * cubes;
      double acc = q[0];
      for (int64_t k = 1; k < rows_cd; ++k) acc = __dadd_rn(acc, q[k * nh8 * nw8]);
      const double term = __ddiv_rn(acc, nl);
      terms[i * levels + l] = term;
      const double wt = __dmul_rn((double)lambda[l], term);
      total = l ? __dadd_rn(total, wt) : wt;
      nl = nl * 0.125;      // (exact: every extent is a multiple of 2^(levels - 1))
    }
    loss[i] = (float)total;
  }
}

template <typename Y, typename S>
int msr_launch(const msr_args& a, bool vec, hipStream_t hs) {
  const int64_t blocks = (a.waves + 3) / 4;
  if (blocks > 0x7FFFFFFFll) return SG_EINVAL;
  if (vec)
    hipLaunchKernelGGL((multiscale_residual_kernel<Y, S, true>), dim3((unsigned)blocks), dim3(256), 0, hs, a);
  else
    hipLaunchKernelGGL((multiscale_residual_kernel<Y, S, false>), dim3((unsigned)blocks), dim3(256), 0, hs, a);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

template <typename Y>
int msr_launch_src(sg_src_dtype sdt, const msr_args& a, bool yvec, hipStream_t hs) {
  const bool base = yvec && a.w % 8 == 0;
  switch (sdt) {
    case SG_SRC_U8:  return msr_launch<Y, uint8_t>(a, base && ((uintptr_t)a.table) % 8 == 0, hs);
    case SG_SRC_I8:  return msr_launch<Y, int8_t>(a, base && ((uintptr_t)a.table) % 8 == 0, hs);
    case SG_SRC_I16: return msr_launch<Y, int16_t>(a, base && ((uintptr_t)a.table) % 16 == 0, hs);
    case SG_SRC_U16: return msr_launch<Y, uint16_t>(a, base && ((uintptr_t)a.table) % 16 == 0, hs);
    case SG_SRC_F16: return msr_launch<Y, _Float16>(a, base && ((uintptr_t)a.table) % 16 == 0, hs);
    case SG_SRC_F32: return msr_launch<Y, float>(a, base && ((uintptr_t)a.table) % 16 == 0, hs);
    default: break;
  }
  return SG_EINVAL;
}

// ---- the latents' update: one wave per sample
__global__ __launch_bounds__(64) void latent_step_kernel(float* __restrict__ z, float* __restrict__ m, float* __restrict__ v,
                                                         const float* __restrict__ gz, const float* __restrict__ loss,
                                                         float* __restrict__ best_loss, float* __restrict__ z_best,
                                                         int32_t* __restrict__ best_step, int64_t L, float lr, float b1, float b2,
                                                         float omb1, float omb2, float bc1, float bc2, float eps, int32_t step,
                                                         int32_t sphere) {
  const int64_t i = blockIdx.x;
  const int lane = threadIdx.x;
  float* __restrict__ zi = z + i * L;
  const float li = loss[i];
  const bool take = li < best_loss[i];      // (false for a NaN loss: a NaN never wins; equal losses keep the earlier step)
  if (take) {
    for (int64_t k = lane; k < L; k += 64) z_best[i * L + k] = zi[k];
  }
  __syncthreads();      // (every lane has read best_loss[i])
  if (take && lane == 0) {
    best_loss[i] = li;
    best_step[i] = step;
  }
  if (lr == 0.f) return;      // the scoring launch: nothing moves
  // (sqrtf, not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS the latter is the native, approximate square root; the plain
  // f32 square root and division are correctly rounded -- hipcc's -fhip-fp32-correctly-rounded-divide-sqrt is on by default)
  double part = 0.0;
  for (int64_t k = lane; k < L; k += 64) {
    const float g = gz[i * L + k];
    const float mk = __fadd_rn(__fmul_rn(b1, m[i * L + k]), __fmul_rn(omb1, g));
    const float vk = __fadd_rn(__fmul_rn(b2, v[i * L + k]), __fmul_rn(__fmul_rn(omb2, g), g));
    m[i * L + k] = mk;
    v[i * L + k] = vk;
    const float mh = __fdiv_rn(mk, bc1), vh = __fdiv_rn(vk, bc2);
    const float zn = __fsub_rn(zi[k], __fdiv_rn(__fmul_rn(lr, mh), __fadd_rn(sqrtf(vh), eps)));
    zi[k] = zn;
    part = __dadd_rn(part, __dmul_rn((double)zn, (double)zn));
  }
  if (!sphere) return;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) part = __dadd_rn(part, pj_shfl_xor(part, s));
  if (!(part > 0.0) || part == INFINITY) return;      // a zero, NaN or infinite row is left as it is (wave-uniform)
  const double scale = __ddiv_rn(__dsqrt_rn((double)L), __dsqrt_rn(part));
  for (int64_t k = lane; k < L; k += 64) zi[k] = (float)__dmul_rn((double)zi[k], scale);      // (the lane's own stores, read back)
}

}  // namespace

extern "C" int32_t sg_multiscale_residual_max_levels(void) { return MSR_MAX_LEVELS; }

extern "C" size_t sg_multiscale_residual_workspace(int64_t n, int64_t c, int64_t d, int64_t h, int64_t w, int32_t levels) {
  if (n < 0 || c < 1 || d < 0 || h < 0 || w < 0 || levels < 1) return 0;
  const int64_t cubes = c * ((d + 7) / 8) * ((h + 7) / 8) * ((w + 7) / 8);
  return (size_t)(n * levels * cubes) * sizeof(double);
}

extern "C" int sg_multiscale_residual(const void* y, sg_src_dtype ydt, int32_t channels_last, const void* table, sg_src_dtype tdt,
                                      int64_t rows, const int32_t* idx, int64_t n, int64_t c, int64_t d, int64_t h, int64_t w,
                                      float mean, float stddev, int32_t levels, const float* lambda, const double* k, void* grad,
                                      double* terms, float* loss, void* workspace, size_t workspace_bytes, sg_stream_t st) {
  if (n < 0 || c < 1 || d < 1 || h < 1 || w < 1 || rows < 0) return SG_EINVAL;
  if (levels < 1) return SG_EINVAL;
  if (levels > MSR_MAX_LEVELS) return SG_EUNSUPPORTED;
  if (ydt != SG_SRC_F32 && ydt != SG_SRC_BF16 && ydt != SG_SRC_F16) return SG_EINVAL;
  if ((int)tdt < (int)SG_SRC_U8 || (int)tdt > (int)SG_SRC_F32) return SG_EINVAL;
  const int64_t edge = (int64_t)1 << (levels - 1);
  if (d % edge || h % edge || w % edge) return SG_EINVAL;
  typedef __int128 i128;
  if ((i128)n * c * d * h * w > (i128)INT64_MAX / 8 || (i128)rows * c * d * h * w > (i128)INT64_MAX / 8) return SG_EINVAL;
  if (n == 0) return SG_OK;
  if (!y || !table || !idx || !lambda || !k || !grad || !terms || !loss || !workspace) return SG_EINVAL;
  const size_t ysz = ydt == SG_SRC_F32 ? 4 : 2;
  if (((uintptr_t)y) % ysz || ((uintptr_t)grad) % ysz || ((uintptr_t)idx) % 4 || ((uintptr_t)lambda) % 4 || ((uintptr_t)loss) % 4 ||
      ((uintptr_t)terms) % 8 || ((uintptr_t)workspace) % 8)
    return SG_EALIGN;
  const size_t tsz = (tdt == SG_SRC_U8 || tdt == SG_SRC_I8) ? 1 : tdt == SG_SRC_F32 ? 4 : 2;
  if (((uintptr_t)table) % tsz) return SG_EALIGN;
  if (workspace_bytes < sg_multiscale_residual_workspace(n, c, d, h, w, levels)) return SG_EINVAL;
  msr_args a;
  a.y = y; a.table = table; a.idx = idx; a.grad = grad; a.part = (double*)workspace;
  a.rows = rows; a.n = n; a.c = c; a.d = d; a.h = h; a.w = w;
  a.nd8 = (d + 7) / 8; a.nh8 = (h + 7) / 8; a.nw8 = (w + 7) / 8; a.strips = (a.nw8 + 7) / 8;
  a.waves = n * c * a.nd8 * a.nh8 * a.strips;
  a.levels = levels;
  a.channels_last = (channels_last && c > 1) ? 1 : 0;
  a.mean = mean; a.stddev = stddev;
  for (int l = 0; l < MSR_MAX_LEVELS; ++l) a.k[l] = l < levels ? k[l] : 0.0;
  const size_t ypack = ysz * 8 > 16 ? 16 : ysz * 8;
  const bool yvec = !a.channels_last && ((uintptr_t)y) % ypack == 0 && ((uintptr_t)grad) % 16 == 0;
  hipStream_t hs = sg_st(st);
  int rc;
  switch (ydt) {
    case SG_SRC_F32:  rc = msr_launch_src<float>(tdt, a, yvec, hs); break;
    case SG_SRC_BF16: rc = msr_launch_src<pj_bf16>(tdt, a, yvec, hs); break;
    default:          rc = msr_launch_src<_Float16>(tdt, a, yvec, hs); break;
  }
  if (rc != SG_OK) return rc;
  hipLaunchKernelGGL(multiscale_finish_kernel, dim3((unsigned)n), dim3(256), 0, hs, a.part, c * a.nd8, a.nh8, a.nw8, levels, lambda,
                     (double)c * (double)d * (double)h * (double)w, terms, loss);
  SG_LAUNCH_CHECK();
  return SG_OK;
}

extern "C" int sg_latent_step(float* z, float* m, float* v, const float* grad_z, const float* loss, float* best_loss, float* z_best,
                              int32_t* best_step, int64_t n, int64_t L, float lr, float beta1, float beta2, float eps, int32_t step,
                              int32_t sphere, sg_stream_t st) {
  if (n < 0 || L < 1 || step < 1 || n > 0x7FFFFFFFll) return SG_EINVAL;
  if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f) || !(eps > 0.f) || !(lr >= 0.f)) return SG_EINVAL;
  if (n == 0) return SG_OK;
  if (!z || !m || !v || !grad_z || !loss || !best_loss || !z_best || !best_step) return SG_EINVAL;
  const void* ps[] = {z, m, v, grad_z, loss, best_loss, z_best, best_step};
  for (const void* p : ps)
    if (((uintptr_t)p) % 4) return SG_EALIGN;
  const float omb1 = 1.f - beta1, omb2 = 1.f - beta2;
  const float bc1 = (float)(1.0 - pow((double)beta1, (double)step)), bc2 = (float)(1.0 - pow((double)beta2, (double)step));
  hipLaunchKernelGGL(latent_step_kernel, dim3((unsigned)n), dim3(64), 0, sg_st(st), z, m, v, grad_z, loss, best_loss, z_best,
                     best_step, L, lr, beta1, beta2, omb1, omb2, bc1, bc2, eps, step, sphere ? 1 : 0);
  SG_LAUNCH_CHECK();
  return SG_OK;
}
