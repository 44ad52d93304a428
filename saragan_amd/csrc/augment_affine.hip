// Discriminator augmentation, second family (Karras et al. 2020: "geom" and "color"): isotropic scaling, rotation in the
// (h, w) plane, sub-voxel translation, brightness and contrast.  One trilinear resampling pass with a per-sample 3 x 4 matrix,
// a gain and a bias; its adjoint is a GATHER over a bounded window of output voxels, so there are no atomics and two runs give
// the same bits.  (Not in the reference.  The pixel-blitting family stays in augment.hip, untouched.)
//
// Per-sample parameters: float params[n][16] = {A (row-major 3 x 4), gain a, bias b, 0, 0}.  The SOURCE coordinate of output
// voxel v = (vd, vh, vw) is u = A[:, :3] v + A[:, 3], in voxel units.
//
// sg_augment_affine_draw -- one thread per sample i, ctr = offset + i, key = seed ^ "AUGMENT2" (the blitting draws and the
// instance noise keep their streams).  Three Philox4x32-10 blocks, counter (lo32 ctr, hi32 ctr, j, 0):
//     block 0: gate scale, gate rotate, gate shift, gate brightness
//     block 1: gate contrast, value scale, value angle, value brightness
//     block 2: value contrast, value t_d, value t_h, value t_w
//   gate(r) as in sg_augment_draw;  sym(r) = 2 (r 2^-32) - 1 in double
//   s = exp2(sym log2 max_scale);  theta = sym max_angle;  t_a = sym_a max_shift_a;  b = sym max_brightness;
//   a = exp2(sym log2 max_contrast);  disabled or gated off: s = 1, theta = 0, t = 0, b = 0, a = 1
//   u = c + (1/s) R(-theta) (v - c - t), c_a = (extent_a - 1) / 2, R(-theta) = [[cos, sin], [-sin, cos]] on (h, w); in double,
//   rounded to f32 once.  The gates select literal 1 / 0 entries, never sincos(0) or exp2(0): with every gate off the row is
//   the identity's bits.
//
// sg_augment_affine_apply -- the arithmetic is fixed operation by operation (every product and every sum rounds to f32 on its
// own: this file is compiled without FMA contraction), so that a numpy float32 restatement matches bit for bit:
//   1. u_a = ((A[a][0] vd + A[a][1] vh) + A[a][2] vw) + A[a][3]
//   2. support: -1 < u_a < extent_a for all a, tested in float before any integer conversion (NaN fails).  Outside: forward
//      y = a * fill (then the bias), adjoint nothing.
//   3. f_a = floor(u_a), r_a = u_a - f_a, w0_a = 1 + (-r_a), w1_a = r_a
//   4. corner k = 4 bd + 2 bh + bw: W_k = ((wd * wh) * ww) * a at voxel f + bits; outside the volume its value is `fill`
//      forward and absent in the adjoint
//   5. forward: corners in ascending k, those with W_k == 0 skipped (never read); acc = first product, later ones added;
//      y = b != 0 ? acc + b : acc, rounded to the output type once
//   6. adjoint: gx[u] = sum over the output voxels v that have u among their in-range corners with W_k != 0 of W_k(v) * gy[v],
//      in ascending linear order of v, starting from the first term; 0 where no v reaches u.
//      One v reaches a given u through at most one corner, so per input voxel the kernel walks a window of candidate v,
//      recomputes steps 1-4 for each exactly as the forward does and keeps the hits.  The window: v reaches u only if
//      A v + t lies in the open cube u + (-1, 1)^3, that is v in A^-1 (u - t) + A^-1 (-1, 1)^3, whose half-width along axis a
//      is the absolute row sum of A^-1; a slack of 1/16 + 2^-14 sum_j |A^-1[a][j]| |u_j - t_j| -- float error is about 2^-19
//      of that sum -- covers the rounding of the forward's coordinates and of the inverse computed here.  Absolute row sums up
//      to 3 (scale <= 2 at any angle gives 2 sqrt 2) need at most 7 candidates per axis; the loops are capped at AFF_CAP = 8
//      per axis for ANY bit pattern in params, and every index is clamped to the volume before it is converted to an integer.
//   flags bit 0: adjoint; bit 1: linear part only (fill and b read as 0: what the autograd layer differentiates).
//   A row that is exactly the identity matrix skips the coordinate arithmetic: y = a * x (+ b), the same bits as the general path.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr uint64_t SG_AUGF_KEY = 0x4155474D454E5432ull;      // "AUGMENT2"
constexpr int AFF_CAP = 8;                                   // adjoint: candidates per axis, at most

__device__ __forceinline__ double aff_sym(uint32_t r) { return 2.0 * ((double)r * (1.0 / 4294967296.0)) - 1.0; }

__global__ void affine_draw_kernel(float* __restrict__ params, int32_t n, uint32_t ops, double c_d, double c_h, double c_w,
                                   double l2_scale, double max_angle, double m_d, double m_h, double m_w, double max_b,
                                   double l2_contrast, float p, const float* __restrict__ p_dev, uint64_t seed, uint64_t offset,
                                   const uint64_t* __restrict__ offset_dev) {
  const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  if (p_dev != nullptr) p = *p_dev;
  if (offset_dev != nullptr) offset = *offset_dev;
  const uint64_t thr = p > 0.f ? (p >= 1.f ? 0x100000000ull : (uint64_t)((double)p * 4294967296.0)) : 0ull;
  const uint64_t ctr = offset + (uint64_t)i, key = seed ^ SG_AUGF_KEY;
  uint32_t a[4], b[4], c[4];
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u, (uint32_t)key, (uint32_t)(key >> 32), a);
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 1u, 0u, (uint32_t)key, (uint32_t)(key >> 32), b);
  philox4x32_10((uint32_t)ctr, (uint32_t)(ctr >> 32), 2u, 0u, (uint32_t)key, (uint32_t)(key >> 32), c);
  const bool g_sc = (ops & SG_AUGF_SCALE) && (uint64_t)a[0] < thr, g_rot = (ops & SG_AUGF_ROTATE) && (uint64_t)a[1] < thr;
  const bool g_sh = (ops & SG_AUGF_SHIFT) && (uint64_t)a[2] < thr, g_br = (ops & SG_AUGF_BRIGHTNESS) && (uint64_t)a[3] < thr;
  const bool g_ct = (ops & SG_AUGF_CONTRAST) && (uint64_t)b[0] < thr;
  double inv = 1.0, cs = 1.0, sn = 0.0;
  if (g_sc) inv = 1.0 / exp2(aff_sym(b[1]) * l2_scale);
  if (g_rot) sincos(aff_sym(b[2]) * max_angle, &sn, &cs);
  const double bias = g_br ? aff_sym(b[3]) * max_b : 0.0;
  const double gain = g_ct ? exp2(aff_sym(c[0]) * l2_contrast) : 1.0;
  const double t_d = g_sh ? aff_sym(c[1]) * m_d : 0.0, t_h = g_sh ? aff_sym(c[2]) * m_h : 0.0;
  const double t_w = g_sh ? aff_sym(c[3]) * m_w : 0.0;
  // the gates pick literal entries: no product with a computed 1 or 0 stands where the identity's bits are promised
  const double a_dd = inv, a_hh = g_rot ? cs * inv : inv, a_hw = g_rot ? sn * inv : 0.0, a_wh = g_rot ? -(sn * inv) : 0.0;
  const double q_d = c_d + t_d, q_h = c_h + t_h, q_w = c_w + t_w;
  float* o = params + (int64_t)i * 16;
  o[0] = (float)a_dd; o[1] = 0.f;         o[2] = 0.f;         o[3] = (float)(c_d - a_dd * q_d);
  o[4] = 0.f;         o[5] = (float)a_hh; o[6] = (float)a_hw; o[7] = (float)(c_h - (a_hh * q_h + a_hw * q_w));
  o[8] = 0.f;         o[9] = (float)a_wh; o[10] = (float)a_hh; o[11] = (float)(c_w - (a_wh * q_h + a_hh * q_w));
  o[12] = (float)gain;
  o[13] = (float)bias;
  o[14] = 0.f;
  o[15] = 0.f;
}

__global__ void affine_counter_add_kernel(uint64_t* ctr, uint64_t inc) { *ctr += inc; }

// One sample's row.  ident: the 3 x 4 matrix is exactly the identity (a -0.0 entry compares equal and gives the same u = v).
struct aff_row {
  float A[12], a, b;
  bool ident;
};

__device__ __forceinline__ aff_row aff_load_row(const float* __restrict__ pr, bool linear) {
  aff_row r;
#pragma unroll
  for (int j = 0; j < 12; ++j) r.A[j] = pr[j];
  r.a = pr[12];
  r.b = linear ? 0.f : pr[13];
  bool id = true;
#pragma unroll
  for (int j = 0; j < 12; ++j) id = id && r.A[j] == ((j == 0 || j == 5 || j == 10) ? 1.f : 0.f);
  r.ident = id;
  return r;
}

// steps 2-3 on one axis: false if u is out of support; else the base index (in [-1, e - 1]) and the two weights
__device__ __forceinline__ bool aff_axis(float u, float ef, int32_t& f, float& w0, float& w1) {
  if (!(u > -1.f && u < ef)) return false;
  const float fl = floorf(u);
  const float r = u - fl;
  w0 = __fadd_rn(1.f, -r);
  w1 = r;
  f = (int32_t)fl;
  return true;
}

// steps 1-4 of the forward for output voxel (vd, vh, vw): the eight corner weights and the base corner
struct aff_vox {
  bool sup;
  int32_t fd, fh, fw;
  float W[8];
};

__device__ __forceinline__ void aff_forward_voxel(const aff_row& r, int32_t vd, int32_t vh, int32_t vw, float ed, float eh,
                                                  float ew, aff_vox& s) {
  if (r.ident) {
    s.sup = true;
    s.fd = vd; s.fh = vh; s.fw = vw;
    s.W[0] = r.a;      // ((1 * 1) * 1) * a
#pragma unroll
    for (int k = 1; k < 8; ++k) s.W[k] = 0.f;
    return;
  }
  const float xd = (float)vd, xh = (float)vh, xw = (float)vw;
  float u[3];
#pragma unroll
  for (int ax = 0; ax < 3; ++ax)
    u[ax] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(r.A[4 * ax], xd), __fmul_rn(r.A[4 * ax + 1], xh)),
                                __fmul_rn(r.A[4 * ax + 2], xw)), r.A[4 * ax + 3]);
  float wd[2] = {0.f, 0.f}, wh[2] = {0.f, 0.f}, ww[2] = {0.f, 0.f};
  s.fd = s.fh = s.fw = 0;
  const bool sd = aff_axis(u[0], ed, s.fd, wd[0], wd[1]), sh = aff_axis(u[1], eh, s.fh, wh[0], wh[1]);
  const bool sw = aff_axis(u[2], ew, s.fw, ww[0], ww[1]);
  s.sup = sd && sh && sw;
#pragma unroll
  for (int k = 0; k < 8; ++k)
    s.W[k] = __fmul_rn(__fmul_rn(__fmul_rn(wd[k >> 2], wh[(k >> 1) & 1]), ww[k & 1]), r.a);
}

template <typename T, int E>
__device__ __forceinline__ void aff_unpack(const T* __restrict__ src, float (&v)[E]) {
  alignas(16) T tmp[E];
  *reinterpret_cast<u32x4*>(tmp) = *reinterpret_cast<const u32x4*>(src);
#pragma unroll
  for (int e = 0; e < E; ++e) v[e] = sg_traits<T>::to_f(tmp[e]);
}

// Forward.  One output piece of 16 bytes (E elements) of a (w, c) row per thread and trip, as augment_apply_kernel.  VEC: w*c is
// a multiple of E and x, y are 16-byte aligned.  ONEVOX (VEC and c a multiple of E): a piece lies within one voxel, so the
// corners are read as 16-byte pieces too.  Otherwise the voxel's weights are computed when the piece enters it and shared by
// its channels; sources are read element-wise (the tensor is D's input, cache-resident).
template <typename T, bool VEC, bool ONEVOX>
__global__ __launch_bounds__(256) void affine_fwd_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                         const float* __restrict__ params, int64_t total, uint32_t P, int small,
                                                         int32_t d, int32_t h, int32_t w, int32_t c, float fill, int linear) {
  constexpr int E = 16 / (int)sizeof(T);
  const int32_t L = w * c;
  const float ed = (float)d, eh = (float)h, ew = (float)w;
  if (linear) fill = 0.f;
  const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid0; i < total; i += stride) {
    uint32_t row, piece;
    if (small) {      // fewer than 2^32 pieces: 32-bit division
      row = (uint32_t)i / P;
      piece = (uint32_t)i - row * P;
    } else {
      const uint64_t q = (uint64_t)i / P;
      row = (uint32_t)q;
      piece = (uint32_t)((uint64_t)i - q * P);
    }
    const uint32_t t1 = row / (uint32_t)h;
    const int32_t hh = (int32_t)(row - t1 * (uint32_t)h);
    const uint32_t nn = t1 / (uint32_t)d;
    const int32_t dd = (int32_t)(t1 - nn * (uint32_t)d);
    const aff_row r = aff_load_row(params + (int64_t)nn * 16, linear != 0);
    const T* xs = x + (int64_t)nn * d * h * L;
    const int32_t q0 = (int32_t)piece * E;
    int32_t ww = q0 / c, ch = q0 - ww * c;
    alignas(16) T out[E];
    aff_vox s;
    if (ONEVOX) {
      aff_forward_voxel(r, dd, hh, ww, ed, eh, ew, s);
      float acc[E];
      bool first = true;
#pragma unroll
      for (int e = 0; e < E; ++e) acc[e] = __fmul_rn(r.a, fill);
      if (s.sup) {
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float W = s.W[k];
          if (W != 0.f) {
            const int32_t id = s.fd + (k >> 2), ih = s.fh + ((k >> 1) & 1), iw = s.fw + (k & 1);
            float v[E];
#pragma unroll
            for (int e = 0; e < E; ++e) v[e] = fill;
            if ((uint32_t)id < (uint32_t)d && (uint32_t)ih < (uint32_t)h && (uint32_t)iw < (uint32_t)w)
              aff_unpack<T, E>(xs + (((int64_t)id * h + ih) * w + iw) * c + ch, v);
#pragma unroll
            for (int e = 0; e < E; ++e) {
              const float t = __fmul_rn(W, v[e]);
              acc[e] = first ? t : __fadd_rn(acc[e], t);
            }
            first = false;
          }
        }
      }
#pragma unroll
      for (int e = 0; e < E; ++e) out[e] = sg_traits<T>::from_f(r.b != 0.f ? __fadd_rn(acc[e], r.b) : acc[e]);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        float acc = 0.f;
        if (VEC || q0 + e < L) {
          if (e == 0 || ch == 0) aff_forward_voxel(r, dd, hh, ww, ed, eh, ew, s);
          if (s.sup) {
            bool first = true;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const float W = s.W[k];
              if (W != 0.f) {
                const int32_t id = s.fd + (k >> 2), ih = s.fh + ((k >> 1) & 1), iw = s.fw + (k & 1);
                float v = fill;
                if ((uint32_t)id < (uint32_t)d && (uint32_t)ih < (uint32_t)h && (uint32_t)iw < (uint32_t)w)
                  v = sg_traits<T>::to_f(xs[(((int64_t)id * h + ih) * w + iw) * c + ch]);
                const float t = __fmul_rn(W, v);
                acc = first ? t : __fadd_rn(acc, t);
                first = false;
              }
            }
          } else {
            acc = __fmul_rn(r.a, fill);
          }
          if (r.b != 0.f) acc = __fadd_rn(acc, r.b);
        }
        out[e] = sg_traits<T>::from_f(acc);
        if (++ch == c) {
          ch = 0;
          ++ww;
        }
      }
    }
    T* dst = y + (int64_t)row * L + q0;
    if (VEC) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(out);
      *reinterpret_cast<u32x4*>(dst) = raw;
      SG_STORE16_GUARD(raw);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (q0 + e < L) dst[e] = out[e];
    }
  }
}

// The adjoint's per-sample part: A^-1 (adjugate over determinant, f32) with the absolute row sums.  A singular or non-finite
// matrix gives NaN here; aff_window turns NaN bounds into the whole (capped) axis.
struct aff_inv {
  float I[9], hw[3];
};

__device__ __forceinline__ aff_inv aff_invert(const aff_row& r) {
  const float m00 = r.A[0], m01 = r.A[1], m02 = r.A[2], m10 = r.A[4], m11 = r.A[5], m12 = r.A[6];
  const float m20 = r.A[8], m21 = r.A[9], m22 = r.A[10];
  const float c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
  const float rd = 1.f / (m00 * c00 + m01 * c01 + m02 * c02);
  aff_inv v;
  v.I[0] = c00 * rd; v.I[1] = (m02 * m21 - m01 * m22) * rd; v.I[2] = (m01 * m12 - m02 * m11) * rd;
  v.I[3] = c01 * rd; v.I[4] = (m00 * m22 - m02 * m20) * rd; v.I[5] = (m02 * m10 - m00 * m12) * rd;
  v.I[6] = c02 * rd; v.I[7] = (m01 * m20 - m00 * m21) * rd; v.I[8] = (m00 * m11 - m01 * m10) * rd;
#pragma unroll
  for (int ax = 0; ax < 3; ++ax) v.hw[ax] = fabsf(v.I[3 * ax]) + fabsf(v.I[3 * ax + 1]) + fabsf(v.I[3 * ax + 2]);
  return v;
}

// candidates along one axis for input voxel coordinate differences q = u - t: [lo, lo + cnt), inside [0, e), cnt <= AFF_CAP
__device__ __forceinline__ void aff_window(const aff_inv& v, int ax, float q0, float q1, float q2, int32_t e, int32_t& lo,
                                           int32_t& cnt) {
  const float i0 = v.I[3 * ax], i1 = v.I[3 * ax + 1], i2 = v.I[3 * ax + 2];
  const float ctr = i0 * q0 + i1 * q1 + i2 * q2;
  const float mag = fabsf(i0) * fabsf(q0) + fabsf(i1) * fabsf(q1) + fabsf(i2) * fabsf(q2);
  const float half = v.hw[ax] + (0.0625f + 6.103515625e-05f * mag);
  // clamped in float first (fmaxf / fminf drop a NaN operand), converted afterwards: lo in [0, e], hi in [-1, e - 1]
  const float flo = fminf(fmaxf(ceilf(ctr - half), 0.f), (float)e);
  const float fhi = fmaxf(fminf(floorf(ctr + half), (float)(e - 1)), -1.f);
  lo = (int32_t)flo;
  const int32_t m = (int32_t)fhi - lo + 1;
  cnt = m < 0 ? 0 : (m > AFF_CAP ? AFF_CAP : m);
}

// Adjoint (step 6) for input voxel (pd, ph, pw), NV channels starting at `gs` + ch of every candidate's voxel.  acc[] holds
// the sums; `any` says whether a term has arrived (the first term starts the sum).
template <typename T, int NV, bool PIECE>
__device__ __forceinline__ void aff_adjoint_voxel(const T* __restrict__ gs, const aff_row& r, const aff_inv& inv, int32_t pd,
                                                  int32_t ph, int32_t pw, int32_t d, int32_t h, int32_t w, int32_t c, int32_t ch,
                                                  float (&acc)[NV]) {
#pragma unroll
  for (int e = 0; e < NV; ++e) acc[e] = 0.f;
  if (r.ident) {
    float g[NV];
    const T* src = gs + (((int64_t)pd * h + ph) * w + pw) * c + ch;
    if (PIECE) aff_unpack<T, NV>(src, g);
    else g[0] = sg_traits<T>::to_f(src[0]);
#pragma unroll
    for (int e = 0; e < NV; ++e) acc[e] = __fmul_rn(r.a, g[e]);
    return;
  }
  const float fpd = (float)pd, fph = (float)ph, fpw = (float)pw;
  const float q0 = fpd - r.A[3], q1 = fph - r.A[7], q2 = fpw - r.A[11];
  int32_t lo_d, n_d, lo_h, n_h, lo_w, n_w;
  aff_window(inv, 0, q0, q1, q2, d, lo_d, n_d);
  aff_window(inv, 1, q0, q1, q2, h, lo_h, n_h);
  aff_window(inv, 2, q0, q1, q2, w, lo_w, n_w);
  // v is in support and has this voxel as corner bit 0 (floor(u) == p) or bit 1 (floor(u) == p - 1) on an axis exactly when
  // p - 1 <= u < p + 1 and u > -1 (p + 1 <= extent): two comparisons, with the float next above -1 as the bound where p == 0.
  // NaN fails them.
  constexpr float ABOVE_M1 = -0.99999994f;
  const float lb0 = pd == 0 ? ABOVE_M1 : fpd - 1.f, lb1 = ph == 0 ? ABOVE_M1 : fph - 1.f, lb2 = pw == 0 ? ABOVE_M1 : fpw - 1.f;
  const float ub0 = fpd + 1.f, ub1 = fph + 1.f, ub2 = fpw + 1.f;
  // u_d does not depend on (vh, vw) -- every row of the draw: the d axis is only scaled -- so its test and weight are taken once
  // per vd.  ((d0 + A1 vh) + A2 vw with A1 = A2 = 0 adds zeros: the same value as d0, up to the sign of a zero, which neither
  // floor(u) == p, nor r = u - floor(u) = +0, nor the weights see.)
  const bool dsep = r.A[1] == 0.f && r.A[2] == 0.f;
  bool any = false;
  for (int32_t jd = 0; jd < n_d; ++jd) {
    const int32_t vd = lo_d + jd;
    const float xd = (float)vd;
    const float d0 = __fmul_rn(r.A[0], xd), d1 = __fmul_rn(r.A[4], xd), d2 = __fmul_rn(r.A[8], xd);
    float wd = 0.f;
    if (dsep) {
      const float u0 = __fadd_rn(d0, r.A[3]);
      if (!(u0 >= lb0 && u0 < ub0)) continue;
      const float f0 = floorf(u0), r0 = u0 - f0;
      wd = f0 != fpd ? r0 : __fadd_rn(1.f, -r0);
    }
    for (int32_t jh = 0; jh < n_h; ++jh) {
      const int32_t vh = lo_h + jh;
      const float xh = (float)vh;
      const float h0 = __fadd_rn(d0, __fmul_rn(r.A[1], xh)), h1 = __fadd_rn(d1, __fmul_rn(r.A[5], xh));
      const float h2 = __fadd_rn(d2, __fmul_rn(r.A[9], xh));
      for (int32_t jw = 0; jw < n_w; ++jw) {
        const int32_t vw = lo_w + jw;
        const float xw = (float)vw;
        const float u1 = __fadd_rn(__fadd_rn(h1, __fmul_rn(r.A[6], xw)), r.A[7]);
        const float u2 = __fadd_rn(__fadd_rn(h2, __fmul_rn(r.A[10], xw)), r.A[11]);
        if (!(u1 >= lb1 && u1 < ub1 && u2 >= lb2 && u2 < ub2)) continue;
        if (!dsep) {
          const float u0 = __fadd_rn(__fadd_rn(h0, __fmul_rn(r.A[2], xw)), r.A[3]);
          if (!(u0 >= lb0 && u0 < ub0)) continue;
          const float f0 = floorf(u0), r0 = u0 - f0;
          wd = f0 != fpd ? r0 : __fadd_rn(1.f, -r0);
        }
        const float f1 = floorf(u1), f2 = floorf(u2);
        const float r1 = u1 - f1, r2 = u2 - f2;
        const float wh = f1 != fph ? r1 : __fadd_rn(1.f, -r1), ww = f2 != fpw ? r2 : __fadd_rn(1.f, -r2);
        const float W = __fmul_rn(__fmul_rn(__fmul_rn(wd, wh), ww), r.a);
        if (W != 0.f) {
          float g[NV];
          const T* src = gs + (((int64_t)vd * h + vh) * w + vw) * c + ch;
          if (PIECE) aff_unpack<T, NV>(src, g);
          else g[0] = sg_traits<T>::to_f(src[0]);
#pragma unroll
          for (int e = 0; e < NV; ++e) {
            const float t = __fmul_rn(W, g[e]);
            acc[e] = any ? __fadd_rn(acc[e], t) : t;
          }
          any = true;
        }
      }
    }
  }
}

// Adjoint launch shape: as the forward.  ONEVOX: one window walk per piece, the hits read as 16-byte pieces and shared by the
// piece's channels.  Otherwise every element walks its own voxel's window (c = 1, D's input, has nothing to share).
template <typename T, bool VEC, bool ONEVOX>
__global__ __launch_bounds__(256) void affine_adj_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                         const float* __restrict__ params, int64_t total, uint32_t P, int small,
                                                         int32_t d, int32_t h, int32_t w, int32_t c) {
  constexpr int E = 16 / (int)sizeof(T);
  const int32_t L = w * c;
  const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = tid0; i < total; i += stride) {
    uint32_t row, piece;
    if (small) {
      row = (uint32_t)i / P;
      piece = (uint32_t)i - row * P;
    } else {
      const uint64_t q = (uint64_t)i / P;
      row = (uint32_t)q;
      piece = (uint32_t)((uint64_t)i - q * P);
    }
    const uint32_t t1 = row / (uint32_t)h;
    const int32_t hh = (int32_t)(row - t1 * (uint32_t)h);
    const uint32_t nn = t1 / (uint32_t)d;
    const int32_t dd = (int32_t)(t1 - nn * (uint32_t)d);
    const aff_row r = aff_load_row(params + (int64_t)nn * 16, true);
    aff_inv inv = {};
    if (!r.ident) inv = aff_invert(r);
    const T* gs = x + (int64_t)nn * d * h * L;
    const int32_t q0 = (int32_t)piece * E;
    int32_t ww = q0 / c, ch = q0 - ww * c;
    alignas(16) T out[E];
    if (ONEVOX) {
      float acc[E];
      aff_adjoint_voxel<T, E, true>(gs, r, inv, dd, hh, ww, d, h, w, c, ch, acc);
#pragma unroll
      for (int e = 0; e < E; ++e) out[e] = sg_traits<T>::from_f(acc[e]);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) {
        float acc[1] = {0.f};
        if (VEC || q0 + e < L) aff_adjoint_voxel<T, 1, false>(gs, r, inv, dd, hh, ww, d, h, w, c, ch, acc);
        out[e] = sg_traits<T>::from_f(acc[0]);
        if (++ch == c) {
          ch = 0;
          ++ww;
        }
      }
    }
    T* dst = y + (int64_t)row * L + q0;
    if (VEC) {
      const u32x4 raw = *reinterpret_cast<const u32x4*>(out);
      *reinterpret_cast<u32x4*>(dst) = raw;
      SG_STORE16_GUARD(raw);
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e)
        if (q0 + e < L) dst[e] = out[e];
    }
  }
}

}  // namespace

extern "C" int sg_augment_affine_draw(float* params, int32_t n, uint32_t ops, int32_t d, int32_t h, int32_t w, double max_scale,
                                      double max_angle, double max_shift_d, double max_shift_h, double max_shift_w,
                                      double max_brightness, double max_contrast, float p, const float* p_dev, uint64_t seed,
                                      uint64_t offset, uint64_t* offset_dev, uint64_t bump, sg_stream_t st) {
  if (!params || n < 1 || d < 1 || h < 1 || w < 1 || (ops & ~(uint32_t)SG_AUGF_ALL)) return SG_EINVAL;
  // (written so that a NaN is refused too)
  if (!(max_scale >= 1.0 && max_scale <= 2.0) || !(max_angle >= 0.0 && max_angle <= 3.14159265358979323846)) return SG_EINVAL;
  if (!(max_shift_d >= 0.0 && max_shift_d <= 1e9) || !(max_shift_h >= 0.0 && max_shift_h <= 1e9) ||
      !(max_shift_w >= 0.0 && max_shift_w <= 1e9))
    return SG_EINVAL;
  if (!(max_brightness >= 0.0 && max_brightness <= 3.0e38) || !(max_contrast >= 1.0 && max_contrast <= 4.0)) return SG_EINVAL;
  hipStream_t hs = sg_st(st);
  hipLaunchKernelGGL(affine_draw_kernel, dim3((n + 255) / 256), dim3(256), 0, hs, params, n, ops, (d - 1) * 0.5, (h - 1) * 0.5,
                     (w - 1) * 0.5, log2(max_scale), max_angle, max_shift_d, max_shift_h, max_shift_w, max_brightness,
                     log2(max_contrast), p, p_dev, seed, offset, (const uint64_t*)offset_dev);
  SG_LAUNCH_CHECK();
  if (offset_dev && bump) {      // stream order: every block of the launch above has read the counter before this runs
    hipLaunchKernelGGL(affine_counter_add_kernel, dim3(1), dim3(1), 0, hs, offset_dev, bump);
    SG_LAUNCH_CHECK();
  }
  return SG_OK;
}

extern "C" int sg_augment_affine_apply(const void* x, void* y, const float* params, int32_t n, int32_t d, int32_t h, int32_t w,
                                       int32_t c, float fill, uint32_t flags, sg_dtype dt, sg_stream_t st) {
  if (!x || !y || !params || x == y || n < 1 || d < 1 || h < 1 || w < 1 || c < 1 || (flags & ~3u)) return SG_EINVAL;
  if (dt != SG_F32 && dt != SG_BF16) return SG_EINVAL;
  if (d > (1 << 24) || h > (1 << 24) || w > (1 << 24)) return SG_EINVAL;      // extents and indices are exact in f32
  const int64_t L = (int64_t)w * c, rows = (int64_t)n * d * h;
  if (L >= (1ll << 31) || rows >= (1ll << 32)) return SG_EINVAL;
  const int E = 16 / (int)sg_esize(dt);
  const int64_t P = (L + E - 1) / E, total = rows * P;
  const bool vec = L % E == 0 && sg_aligned16(y);
  const bool onevox = vec && c % E == 0 && sg_aligned16(x);
  const int small = total < (1ll << 32) ? 1 : 0;
  // two trips per thread at every size of more than one block (the grid-stride loop is never a path of large tensors only)
  int64_t blocks = (total + 255) / 256;
  if (blocks > 1) blocks = (blocks + 1) / 2;
  if (blocks > (1ll << 30)) blocks = 1ll << 30;
  hipStream_t hs = sg_st(st);
  const int linear = (flags & 2u) ? 1 : 0;
#define F_(T, V, O)                                                                                                      \
  hipLaunchKernelGGL((affine_fwd_kernel<T, V, O>), dim3((unsigned)blocks), dim3(256), 0, hs, (const T*)x, (T*)y, params, \
                     total, (uint32_t)P, small, d, h, w, c, fill, linear)
#define A_(T, V, O)                                                                                                      \
  hipLaunchKernelGGL((affine_adj_kernel<T, V, O>), dim3((unsigned)blocks), dim3(256), 0, hs, (const T*)x, (T*)y, params, \
                     total, (uint32_t)P, small, d, h, w, c)
#define D_(K, T)                     \
  do {                               \
    if (onevox) K(T, true, true);    \
    else if (vec) K(T, true, false); \
    else K(T, false, false);         \
  } while (0)
  if (flags & 1u) {
    if (dt == SG_BF16) D_(A_, bf16_t); else D_(A_, float);
  } else {
    if (dt == SG_BF16) D_(F_, bf16_t); else D_(F_, float);
  }
#undef D_
#undef A_
#undef F_
  SG_LAUNCH_CHECK();
  return SG_OK;
}
