"""Helpers shared by tests/test_autograd_gen_exact_gpu.py and tests/test_gref_host.py: a plain fp64 restatement (torch, on the
device of its arguments) of the generator's autograd nodes (saragan_amd/functional.py: _ConvBiasAct with pixel_norm, _PnActBwd,
_PixelNormBwd + _BiasActBwd, _ConvPnActToRgb, _dgrad_into with pn_bwd, _upconv_dgrad, _Axpby, dense), built from tests/fwdref.py,
tests/wgref.py, tests/agref.py and tests/ewref.py, the data of the cases, their range assertions and the error bounds.

Two tiers.  Tier 1 is agref's scheme (integer data, slope 1/4, sparse +-1 filters where an intermediate is stored, q / coef
variables): everything that carries no pixel-norm factor -- the up-sampled convolution node, the mixing branch, the dense head --
must EQUAL the exact value rounded once.  Tier 2 starts at a pixel norm: the backward kernels read the forward's STORED y (bf16)
and scale (f32), so a node's reference is evaluated in fp64 on exactly the tensors the node read (y, scale, the sign words, and
the bf16 dz one kernel hands to the next, captured by the test), and each comparison is one kernel deep.  Its bounds:

  forward y, scale       pn_check(): (C / 2 + 6.5) 2^-24 |ref| + half a bf16 ulp (the count is written above it)
  rgb head               rgb_bound(): 11 roundings of partial sums <= sum |y q| + |b|, + half a bf16 ulp
  pixel-norm backward    dz = M s (g - y mean_c(g y)); bound N 2^-24 T + half a bf16 ulp(|ref| + N 2^-24 T),
                         T = M s (|g| + |y| mean_c|g y|), N = PN_BWD_ROUNDINGS[family] (counted from the kernels, see there).
                         g is an exact integer tensor by construction (integer upstream gradients, sparse +-1 consumer filter,
                         integer to_rgb filter), so g y is exact in f32, 1 / C is exact for C a power of two, and a route that
                         stores g in bf16 first holds the same value as one that keeps it in registers
  sums over a dz         every product (small integer) x (bf16 value) is exact in f32; a sum of K non-zero terms is within
                         2 K 2^-24 sum|terms| of the fp64 sum (K 2^-24 is the any-order worst case, doubled because the adds
                         inside an MFMA are not specified as individually rounded), + half a bf16 ulp for a bf16 result,
                         + 2 2^-24 |coef sum| for a filter gradient (wgref.scaled: float(coef) and the product, one rounding each)
  bias gradient          summed by the pixel-norm backward pass itself from its f32 dz BEFORE the bf16 store
                         (elementwise.hip pixel_norm_kernel: `cs[k][e] += pa[u][k].v[e]` ahead of `store`): the reference is
                         the fp64 sum of the restated dz, the bound sum_v N 2^-24 T + the sum bound; taken from the
                         weight-gradient launch or sg_bias_act_bwd it is a sum over the STORED dz like the others

Every toleranced sum has K <= KMAX = 2048 (assert_k), so 2 K 2^-24 sum|terms| stays below half the mean absolute term: one
lost, doubled or misplaced term of ordinary size leaves the bound.  Layouts as in fwdref: activations NCDHW, filters DHWIO.
Nothing here touches the GPU by itself."""
import numpy as np
import torch

from tests import agref as A
from tests import ewref as E
from tests import fwdref as R
from tests import wgref as W

BF, F32 = A.BF, A.F32
SLOPE, NNZ, K333, K111 = A.SLOPE, A.NNZ, A.K333, A.K111
EPS = 1e-8
U = 2.0 ** -24          # the unit roundoff of f32
KMAX = 2048
HE_32 = A.HE_32
UPS_COEF = 2.0 ** -5      # the up-sampled nodes' coefficient: a power of two (see Stage)
RGB_COEF = 1.0 / 32 ** 0.5      # to_rgb's own constant on 32 channels: gain 1 / sqrt(fan_in), no power of two


# ---------------------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------------------
def assert_k(k):
    """The condition that keeps a toleranced sum's bound below half its mean absolute term."""
    assert 0 < int(k) <= KMAX, f'a toleranced sum of {int(k)} terms: the case is too large for a sharp bound (K <= {KMAX})'
    return int(k)


def excess(got, ref, bound):
    """max |got - ref| / bound (<= 1: inside)."""
    err = (got.detach().double().reshape(ref.shape) - ref.to(got.device)).abs()
    return float((err / bound.to(got.device).clamp_min(1e-300)).max())


def within(got, ref, bound):
    err = (got.detach().double().reshape(ref.shape) - ref.to(got.device)).abs()
    return bool((err <= bound.to(got.device)).all())


def check(got, ref, bound, what):
    assert got is not None, what
    assert got.numel() == ref.numel(), (what, tuple(got.shape), tuple(ref.shape))
    worst = excess(got, ref, bound)
    print(f'{what}: largest error {worst:.3f} of its bound')      # (the figure before the assertion: shown with pytest -s / on failure)
    assert within(got, ref, bound), f'{what}: leaves the derived bound by a factor {worst}'


# pixel_norm: y = v * rsqrt(mean_c(v^2) + eps) on the exact f32 accumulator values v.  The f32 error, counted from the epilogues
# (conv3d.hip:205-224 and its copies): the sum of C exact squares by FMA, at most C roundings of a positive sum (C 2^-24 relative),
# the product with the rounded 1 / C (2), the eps add (1), halved by the square root; rsqrtf within 2 ulp (4 2^-24); the product
# with v (1): (C / 2 + 1.5 + 4 + 1) 2^-24 |y|.  f32 outputs get that term alone, bf16 outputs half a bf16 ulp (of |ref| + that
# term) on top.  pn_scale gets the scale's share (C / 2 + 5.5) 2^-24.
def pn_check(cid, y, scale, pre, dt, cout):
    """y (and scale) of pixel_norm over the exact activation `pre` (fp64), inside the bound above."""
    ref, s = R.pixel_norm(pre, EPS)
    f32_term = (cout / 2 + 6.5) * 2.0 ** -24 * ref.abs()
    bound = f32_term if dt == F32 else f32_term + 0.5 * R.bf16_ulp(ref.abs() + f32_term)
    err = (y.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    assert bool((err <= bound).all()), f'{cid}: y leaves the derived bound by a factor {worst}'
    if scale is not None:
        n, _, d, h, w = ref.shape
        es = (scale.double().reshape(n, 1, d, h, w) - s).abs() / s
        assert float(es.max()) <= (cout / 2 + 5.5) * 2.0 ** -24, f'{cid}: pn_scale'


def rgb_bound(y_stored, q_rgb, b_rgb, ref):
    """The rgb head on the stored y (conv3w.hip:585-610): 32 exact products (integer q_rgb) added by 8 FMAs per lane, 2 quad
    additions and the bias add, 11 roundings of partial sums no larger than sum |y q| + |b|, then the one bf16 rounding."""
    f32_term = 11 * 2.0 ** -24 * ((y_stored.double().abs() * q_rgb.double().abs().to(y_stored.device).reshape(1, -1, 1, 1, 1)).sum(1, keepdim=True)
                                  + abs(float(b_rgb)))
    return f32_term + 0.5 * R.bf16_ulp(ref.abs() + f32_term)


# f32 roundings of dz = M s (g - y mean_c(g y)), per kernel family (g y exact, 1 / C and the slope 1/4 powers of two):
#   'pass'      csrc/elementwise.hip pixel_norm_kernel (sg_pixel_norm_bwd, sg_pixel_norm_act_bwd, _pw, _pw_wg): line 349 adds the C
#               products into s (8 per lane, FMA or not) and line 352 the lanes' sums by shuffles: C - 1 roundings in the any-order
#               worst case; 360 `s * inv_c` exact; 366 `sc * (pa - py * mean)`: the product, the subtraction (one less if the
#               compiler fuses them) and the product with sc, 3; 369 `* slope` exact.  pixel_norm_scalar_kernel (446-455) the same
#               with `s / c`.  The to_rgb forms (330: fmaf(g_img, w, 0)) hand it an exact g.  N = C + 2.
#   'epilogue'  the pn_bwd_y epilogue of the consumer's data gradient: csrc/conv3d.hip:1567-1573 (conv_fwd3s) 16 FMAs into dot and
#               one add of the two half-wave sums, `* inv_c` exact, fmaf(-y, mean, g) 1, `pscale *` 1: 19; csrc/conv3w.hip:524-533
#               (conv_fwd3w) 8 FMAs, 2 quad additions, fmaf 1, `ps *` 1: 12.  The mask factor (conv3w.hip:550) is exact.  N = 19,
#               the longer of the two chains, for the family.
PN_BWD_ROUNDINGS = {'pass': lambda c: c + 2, 'epilogue': lambda c: 19}


def pn_bwd_bound(ref, t, n_round, dtype=BF):
    f = n_round * U * t
    return f if dtype == F32 else f + 0.5 * R.bf16_ulp(ref.abs() + f)


def sum_bound(abs_sum, k, ref=None, dtype=None):
    """An f32 sum of k exact terms against the fp64 sum; dtype BF: the result is stored in bf16."""
    f = 2.0 * assert_k(k) * U * abs_sum
    return f + 0.5 * R.bf16_ulp(ref.abs() + f) if dtype == BF else f


def wgrad_bound(total, abs_total, k, coef):
    """A filter gradient np.float32(coef) * f32 sum against coef * the fp64 sum."""
    return abs(coef) * sum_bound(abs_total, k) + 2.0 * U * (coef * total).abs()


def check_w(got, total, abs_total, k, coef, what):
    assert got is not None and got.dtype == F32, what
    check(got, coef * total, wgrad_bound(total, abs_total, k, coef), what)


# ---------------------------------------------------------------------------------------------------------------------------
# nodes
# ---------------------------------------------------------------------------------------------------------------------------
def stage_forward(x, q, b, ups=False, slope=SLOPE, eps=EPS):
    """pixel_norm(leaky_relu(conv3d([upscale3d] x, q) + b)): (the exact activation a, y, the factor s [n,1,d,h,w], sign words
    of the pre-activation), fp64.  The convolution's sums are integers inside the exact range (asserted)."""
    A.assert_conv_range(x, q, q.shape[0] * q.shape[1] * q.shape[2] * q.shape[3] + 1)
    pre = R.bias_act(R.conv_ref(x, q, ups=ups), b)
    a = R.bias_act(pre, None, slope)
    y, s = R.pixel_norm(a, eps)
    return a, y, s, R.sign_words(pre)


def pn_act_bwd(g, y, scale, words, slope=SLOPE):
    """(dz, T) of y = pixel_norm(leaky_relu(z)) from the GIVEN y and scale (what the kernels read): dz = M s (g - y mean_c(g y))
    (ewref.pn_bwd, then the mask), T = M s (|g| + |y| mean_c|g y|) the magnitude its roundings are relative to.
    words None: pixel_norm alone."""
    g, y = g.double(), y.double()
    n, _, d, h, w = g.shape
    s = scale.double().reshape(n, 1, d, h, w)
    dz = E.pn_bwd(g, y, s)
    t = s * (g.abs() + y.abs() * (g * y).abs().mean(1, keepdim=True))
    if words is not None:
        dz, t = R.apply_mask(dz, words, slope), R.apply_mask(t, words, slope)
    return dz, t


def check_dz(got, g, y, scale, words, family, what, dtype=BF):
    """The captured dz of one pixel-norm backward against its restatement on the stored tensors.  Returns (ref, T)."""
    ref, t = pn_act_bwd(g, y, scale, words)
    check(got, ref, pn_bwd_bound(ref, t, PN_BWD_ROUNDINGS[family](g.shape[1]), dtype), what)
    return ref, t


def check_gb_in_register(got, dz_ref, t, c, what):
    """The bias gradient the pixel-norm backward pass sums from its own f32 dz (before the bf16 store)."""
    k = dz_ref.numel() // c
    bound = (PN_BWD_ROUNDINGS['pass'](c) * U * t).sum((0, 2, 3, 4)) + sum_bound(dz_ref.abs().sum((0, 2, 3, 4)), k)
    assert got is not None and got.dtype == F32, what
    check(got, dz_ref.sum((0, 2, 3, 4)), bound, what)


def nnz_terms(q, per):
    """The largest number of non-zero filter entries one output of conv3d (per = 'out') / one element of its data gradient
    (per = 'in') sums."""
    nz = (q != 0).double()
    return int(nz.sum((0, 1, 2, 3)).max()) if per == 'out' else int(nz.sum((0, 1, 2, 4)).max())


def conv_of_stored(xs, q, b=None):
    """conv3d(xs, q) [+ b] for a stored bf16 xs and a +-1 / integer filter: (fp64 sum, bound of the bf16 result)."""
    ref, mag, k = R.conv_ref(xs, q), R.conv_ref(xs.abs(), q.abs()), nnz_terms(q, 'out')
    if b is not None:
        ref, mag, k = R.bias_act(ref, b), R.bias_act(mag, b.abs()), k + 1
    return ref, sum_bound(mag, k, ref, BF)


def behind_dz(x, q, dz, ups=False):
    """What follows a captured bf16 dz: the data gradient (fp64 sum, bound of its bf16 result), the raw filter sum with the sum of
    its absolute terms, the bias sum with its own, and K of the two voxel sums.  x: the node's input as stored."""
    dz, x, q = dz.double(), x.double(), q.double()
    gx = R.dgrad_ref(dz, q, ups=ups)
    gx_abs = R.dgrad_ref(dz.abs(), q.abs(), ups=ups)
    k_gx = nnz_terms(q, 'in') * (8 if ups else 1)
    sw, sb = W.wgrad_ref(x, dz, tuple(q.shape[:3]), ups=ups)
    sw_abs, sb_abs = W.wgrad_ref(x.abs(), dz.abs(), tuple(q.shape[:3]), ups=ups)
    k_v = dz.numel() // dz.shape[1]
    return {'gx': gx, 'gx_bound': sum_bound(gx_abs, k_gx, gx, BF), 'sw': sw, 'sw_abs': sw_abs, 'sb': sb, 'sb_abs': sb_abs, 'k': assert_k(k_v)}


def stored_dgrad(dz, q):
    """The full-resolution data gradient the generic route of _upconv_dgrad stores before its block sum: (fp64 sum over the bf16
    dz, bound of the bf16 result)."""
    dz, q = dz.double(), q.double()
    ref = R.dgrad_ref(dz, q)
    return ref, sum_bound(R.dgrad_ref(dz.abs(), q.abs()), nnz_terms(q, 'in'), ref, BF)


def stored_block_sum(full):
    """The 2x2x2 block sum of a stored bf16 tensor (sg_downscale_sum, gain 1): (fp64 sum, bound of the bf16 result)."""
    ref = R.block_sum(full.double(), (2, 2, 2))
    return ref, sum_bound(R.block_sum(full.double().abs(), (2, 2, 2)), 8, ref, BF)


def matmul_bound(a, b, ref, dtype=None):
    """a @ b with exact products in f32: K the inner extent."""
    return sum_bound(a.double().abs() @ b.double().abs(), a.shape[1], ref, dtype)


def rgb_forward(y_stored, q_rgb, b_rgb):
    return R.rgb_head(y_stored, q_rgb, b_rgb)


def rgb_backward(y_stored, q_rgb, g_img):
    """to_rgb's three gradients for an integer image gradient: the data gradient g_img (x) q_rgb (exact integers), the raw
    filter sum sum_v y g_img with the sum of its absolute terms, and the exact integer bias sum."""
    y, g = y_stored.double(), g_img.double()
    gy = g * q_rgb.double().to(g.device).reshape(1, -1, 1, 1, 1)
    sw = (y * g).sum((0, 2, 3, 4))
    sw_abs = (y * g).abs().sum((0, 2, 3, 4))
    return gy, sw, sw_abs, g.sum((0, 2, 3, 4))


def lerp_ref(a, b, alpha):
    return alpha * a + (1.0 - alpha) * b


def dense_ref(z, q, b, slope=SLOPE):
    """leaky_relu(z @ q + b) for [N, F] z and an [F, O] q: (pre-activation, output), fp64."""
    pre = z.double() @ q.double() + b.double()
    return pre, torch.where(pre >= 0, pre, pre * slope)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2 cases
# ---------------------------------------------------------------------------------------------------------------------------
class Stage:
    """One pixel-norm stage cin -> c at sp (the LOW resolution with ups), batch n.  dense: the stage's filter is a dense integer
    one (K = 27 cin terms per element of its data gradient); with ups it is sparse per input channel (K = 8 NNZ)."""

    def __init__(self, cid, n, cin, c, sp, ups=False, seed=0):
        self.id, self.n, self.cin, self.c, self.sp, self.ups, self.seed = cid, n, cin, c, tuple(sp), ups, seed
        self.fine = tuple(2 * s for s in sp) if ups else tuple(sp)
        # the sub-pixel packers add up to eight variables before they multiply by coef and round: with q / coef variables that
        # sum is the integer only for a power-of-two coef (three entries that cancel leave a 2^-21 otherwise)
        self.coef = UPS_COEF if ups else (HE_32 if cin == 32 else 1.3859292911256331 / (27 * cin) ** 0.5)

    def __repr__(self):
        return self.id


S32 = Stage('s32', 1, 32, 32, (2, 8, 32), seed=700)
S32_N2 = Stage('s32_n2', 2, 32, 32, (2, 8, 32), seed=710)
S_UPS = Stage('ups_64to32', 1, 64, 32, (2, 4, 32), ups=True, seed=720)
S_WIDE = Stage('wide_16to128', 1, 16, 128, (2, 4, 4), seed=730)
STAGES = [S32, S32_N2, S_UPS, S_WIDE]


def thin_filter(k, cin, cout, seed, keep):
    """agref.dense_filter with each entry kept with probability `keep` (the wide stage: K = 27 * 128 entries per input channel
    would pass KMAX)."""
    q = A.dense_filter(k, cin, cout, seed)
    if keep < 1.0:
        g = torch.Generator().manual_seed(seed + 7919)
        q = (q * (torch.rand(tuple(q.shape), generator=g) < keep).float() + 0).contiguous()
    return q


def stage_data(c):
    """CPU tensors of a tier-2 case: x, the stage's effective filter q1 and bias b1, an integer gradient gy for its output; the
    consumer conv's filter q2 (sparse per input channel: its data gradient sums at most NNZ integers) with bias b2 and output
    gradient gy2; to_rgb's integer filter q_rgb [c], bias b_rgb and image gradient g_img."""
    s = c.seed * 100
    d = {'x': A.ints((c.n, c.cin, *c.sp), s, BF), 'b1': W.int_data((c.c,), s + 2, F32),
         'q1': A.sparse_filter(K333, c.cin, c.c, s + 3, 'in') if c.ups else thin_filter(K333, c.cin, c.c, s + 3, 1.0 if c.c <= 64 else 0.5),
         'gy': A.ints((c.n, c.c, *c.fine), s + 4, BF),
         'q2': A.sparse_filter(K333, c.c, c.c, s + 5, 'in'), 'b2': W.int_data((c.c,), s + 6, F32),
         'gy2': A.ints((c.n, c.c, *c.fine), s + 7, BF),
         'q_rgb': A.dense_filter(K111, c.c, 1, s + 8), 'b_rgb': torch.tensor([2.0]),
         'g_img': A.ints((c.n, 1, *c.fine), s + 9, BF)}
    return d


def stage_conditions(c, d):
    """The host-side conditions of a tier-2 case: the forward's sums exact, every incoming gradient g an exact small integer
    tensor that bf16 holds, every toleranced sum K <= KMAX.  Returns the K of each sum."""
    q1, q2 = d['q1'].double(), d['q2'].double()
    A.assert_conv_range(d['x'], q1, 27 * c.cin + 1)
    g2 = R.dgrad_ref(d['gy2'].double(), q2)
    A.stored(g2, BF)
    assert float(g2.abs().max()) <= 3 * NNZ
    g_rgb = d['g_img'].double() * d['q_rgb'].double().reshape(1, -1, 1, 1, 1)
    A.stored(g_rgb, BF)
    A.stored(g_rgb + d['gy'].double(), BF)
    assert bool((g_rgb == g_rgb.round()).all()) and bool((g2 == g2.round()).all())
    nvox = c.n * c.fine[0] * c.fine[1] * c.fine[2]
    ks = {'gx': nnz_terms(q1, 'in') * (8 if c.ups else 1), 'voxels': nvox, 'y2': nnz_terms(q2, 'out'), 'channels': c.c}
    for v in ks.values():
        assert_k(v)
    assert c.c & (c.c - 1) == 0, '1 / C must be exact'
    return ks


# ---------------------------------------------------------------------------------------------------------------------------
# tier 1 cases
# ---------------------------------------------------------------------------------------------------------------------------
class Up:
    """The up-sampled convolution node cin -> cout on the low-resolution sp.  route: which branch of _upconv_dgrad the shape is
    chosen for ('subpixel', 'pool1', 'pool2', 'pool3', 'generic'); filt 'dense' / 'in' (sparse per input channel: the pooled and the
    generic route store an intermediate); density of the output gradient."""

    def __init__(self, cid, route, dtype, n, cin, cout, sp, filt, coef, density=1.0, seed=0):
        self.id, self.route, self.dtype, self.n, self.cin, self.cout, self.sp = cid, route, dtype, n, cin, cout, tuple(sp)
        self.filt, self.coef, self.density, self.seed = filt, coef, density, seed
        self.fine = tuple(2 * s for s in sp)

    def __repr__(self):
        return self.id


UP_CASES = [
    Up('up_subpixel', 'subpixel', BF, 1, 64, 32, (2, 4, 32), 'dense', UPS_COEF, seed=800),
    Up('up_gather_sparse', 'subpixel', BF, 1, 64, 32, (2, 4, 32), 'in', UPS_COEF, seed=801),
    # 32 input channels: no sub-pixel data gradient (it wants cin % 64 = 0); 16 output channels at 2^20 fine voxels in 32-wide
    # rows: pool mode 1 (32 would be mode 3, which this caller turns into 2)
    Up('up_pool1', 'pool1', BF, 1, 32, 16, (2, 256, 256), 'in', UPS_COEF, density=0.05, seed=810),
    # an odd low-resolution D (the sub-pixel tiles are 2 deep); 64 -> 16 at 2^18 <= fine voxels < 2^20: pool mode 2
    Up('up_pool2', 'pool2', BF, 6, 64, 16, (3, 8, 256), 'in', UPS_COEF, density=0.05, seed=820),
    # 32 -> 32 at 2^20 fine voxels: _pool_mode says 3 (the whole mean); _upconv_dgrad, which needs the sum, runs mode 1
    Up('up_pool3_as_1', 'pool3', BF, 1, 32, 32, (2, 256, 256), 'in', UPS_COEF, density=0.05, seed=815),
    Up('up_generic_odd_w', 'generic', BF, 1, 64, 32, (2, 4, 15), 'in', UPS_COEF, seed=830),
    Up('up_generic_f32', 'generic', F32, 1, 8, 16, (2, 4, 8), 'in', 0.25, seed=840),
]


def up_data(c):
    s = c.seed * 100
    q = A.dense_filter(K333, c.cin, c.cout, s + 1) if c.filt == 'dense' else A.sparse_filter(K333, c.cin, c.cout, s + 1, 'in')
    return {'x': A.ints((c.n, c.cin, *c.sp), s, c.dtype), 'q': q, 'b': W.int_data((c.cout,), s + 2, F32),
            'gy': A.ints((c.n, c.cout, *c.fine), s + 3, c.dtype, c.density)}


def up_reference(c, d, act):
    """Exact results of the up-sampled node: y (leaky_relu(conv3d(upscale3d(x), q) + b) with act, conv3d(upscale3d(x), q) without),
    words, gx (the 2x2x2 block sum of the data gradient of M * gy), sw, sb.  For a sparse filter the tensors the pooled and the
    generic route store -- the full-resolution data gradient and its 4-voxel means -- are asserted representable."""
    x, q, gy = d['x'].double(), d['q'].double(), d['gy'].double()
    A.assert_conv_range(x, q, 27 * c.cin + 1)
    pre = R.conv_ref(x, q, ups=True)
    out = {}
    if act:
        pre = R.bias_act(pre, d['b'].double())
        out['words'] = R.sign_words(pre)
        out['y'] = R.bias_act(pre, None, SLOPE)
        g = A.masked(gy, out['words'])
    else:
        out['y'] = pre
        g = gy
    del pre
    A.assert_conv_range(g, q, 27 * c.cout)
    full = R.dgrad_ref(g, q)
    if c.filt == 'in':
        A.stored(full, c.dtype)
        for mode in (1, 2):
            A.stored(R.pool_mean(full, mode), c.dtype)
    out['gx'] = R.block_sum(full, (2, 2, 2))
    del full
    A.assert_wgrad_range(W.up2(x), g)
    out['sw'], out['sb'] = W.wgrad_ref(x, g, K333, ups=True)
    return out


class Mix:
    def __init__(self, cid, alpha, seed):
        self.id, self.alpha, self.seed = cid, alpha, seed
        self.n, self.c, self.sp, self.dtype = 1, 32, (2, 8, 16), BF
        self.fine = tuple(2 * s for s in self.sp)

    def __repr__(self):
        return self.id


MIX_CASES = [Mix('mix_quarter', 0.25, 850), Mix('mix_half', 0.5, 851)]


def mix_data(c):
    """lerp(upscale3d(to_rgb(x)), to_rgb(x2), alpha): integer x (low resolution) and x2 (fine), filters with NNZ entries of +-1
    towards the one image channel (the images are stored: |.| <= 3 NNZ + 3), integer biases and image gradient."""
    s = c.seed * 100
    return {'x': A.ints((c.n, c.c, *c.sp), s, BF), 'x2': A.ints((c.n, c.c, *c.fine), s + 1, BF),
            'qa': A.sparse_filter(K111, c.c, 1, s + 2, 'out'), 'ba': W.int_data((1,), s + 3, F32),
            'qb': A.sparse_filter(K111, c.c, 1, s + 4, 'out'), 'bb': W.int_data((1,), s + 5, F32),
            'g': A.ints((c.n, 1, *c.fine), s + 6, BF)}


def mix_reference(c, d):
    """Exact results: the two images, the mix, and for the image gradient g the gradients of x, x2 and the four parameters (raw
    sums).  Every stored tensor (the images, alpha g, its block sum) is asserted representable."""
    x, x2, qa, qb, g = (d[k].double() for k in ('x', 'x2', 'qa', 'qb', 'g'))
    a = A.stored(R.bias_act(R.conv_ref(x, qa), d['ba'].double()), BF)
    b = A.stored(R.bias_act(R.conv_ref(x2, qb), d['bb'].double()), BF)
    out = {'a': a, 'b': b, 'y': A.stored(lerp_ref(W.up2(a), b, c.alpha), BF)}
    ga = A.stored(R.block_sum(A.stored(c.alpha * g, BF), (2, 2, 2)), BF)
    gb = A.stored((1.0 - c.alpha) * g, BF)
    A.assert_wgrad_range(x, ga), A.assert_wgrad_range(x2, gb)
    out['gx'], out['gx2'] = R.dgrad_ref(ga, qa), R.dgrad_ref(gb, qb)
    out['swa'], out['sba'] = W.wgrad_ref(x, ga, K111)
    out['swb'], out['sbb'] = W.wgrad_ref(x2, gb, K111)
    return out


class Head:
    id, n, latent, c, sp, dtype, seed = 'dense_head', 4, 32, 32, (1, 2, 2), BF, 860
    coef = 1.3859292911256331 / 32 ** 0.5       # dense's he_std on 32 latents

    def __repr__(self):
        return self.id


HEAD = Head()


def head_data(c):
    """generator_in's head: dense (32 latents -> c * 1 * 2 * 2 units, NNZ entries of +-1 per unit: its output is stored) + bias +
    LeakyReLU, reshaped to [n, c, 1, 2, 2], into a 3x3x3 convolution whose filter is sparse per input channel (its data gradient is
    stored)."""
    s = c.seed * 100
    units = c.c * c.sp[0] * c.sp[1] * c.sp[2]
    return {'z': W.int_data((c.n, c.latent), s, BF), 'q': A.sparse_filter(K111, c.latent, units, s + 1, 'out').reshape(c.latent, units).contiguous(),
            'b': W.int_data((units,), s + 2, F32), 'q2': A.sparse_filter(K333, c.c, c.c, s + 3, 'in'),
            'gy': A.ints((c.n, c.c, *c.sp), s + 4, BF)}


def head_reference(c, d):
    z, q, q2, gy = (d[k].double() for k in ('z', 'q', 'q2', 'gy'))
    pre, h = dense_ref(z, q, d['b'])
    A.stored(h, BF)
    h5 = h.reshape(c.n, c.c, *c.sp)
    out = {'h': h, 'y': R.conv_ref(h5, q2)}
    A.assert_conv_range(h5, q2)
    gh = A.stored(R.dgrad_ref(gy, q2), BF).reshape(c.n, -1)
    out['sw2'], _ = W.wgrad_ref(h5, gy, K333)
    g = A.stored(torch.where(pre >= 0, gh, gh * SLOPE), BF)
    out['gz'] = g @ q.t()
    out['sw'] = z.t() @ g
    out['sb'] = g.sum(0)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# a correct route, emulated on the host: f32 arithmetic in another order than the fp64 restatement, one bf16 rounding
# ---------------------------------------------------------------------------------------------------------------------------
def emulate_pn_act_bwd(g, y, scale, words, slope=SLOPE, channels=None, mask_words=None, round_to=BF):
    """dz as a kernel forms it: the products g y summed in f32 from the LAST channel down, times 1 / C, y * mean, the
    subtraction, the product with scale, the mask, then one rounding.  channels: sum only the first `channels` (a wrong kernel);
    mask_words: other sign words than the stage's (a wrong kernel)."""
    g32, y32 = g.float(), y.float()
    n, c, d, h, w = g32.shape
    s32 = scale.float().reshape(n, 1, d, h, w)
    p = g32 * y32
    acc = torch.zeros((n, 1, d, h, w), dtype=F32)
    for ch in reversed(range(channels if channels is not None else c)):
        acc = acc + p[:, ch:ch + 1]
    mean = acc * np.float32(1.0 / c)
    dz = s32 * (g32 - y32 * mean)
    dz = R.apply_mask(dz, words if mask_words is None else mask_words, np.float32(slope))
    return dz.to(round_to) if round_to is not None else dz


def emulate_voxel_sum(x, dz, k, skip=None):
    """sum_v x[v + tap] (x) dz[v] in f32, the voxels in reversed order of wgref's product; skip: one voxel index left out."""
    n, c, d, h, w = dz.shape
    flat = dz.float().permute(0, 2, 3, 4, 1).reshape(-1, c).clone()
    if skip is not None:
        flat[skip] = 0
    dzf = flat.reshape(n, d, h, w, c).permute(0, 4, 1, 2, 3)
    pd, ph, pw = k[0] // 2, k[1] // 2, k[2] // 2
    xp = torch.zeros((n, d + 2 * pd, h + 2 * ph, w + 2 * pw, x.shape[1]), dtype=F32)
    xp[:, pd:pd + d, ph:ph + h, pw:pw + w] = x.float().permute(0, 2, 3, 4, 1)
    dyv = dzf.permute(0, 2, 3, 4, 1).reshape(-1, c).flip(0)
    dw = torch.empty((*k, x.shape[1], c), dtype=F32)
    for a in range(k[0]):
        for b in range(k[1]):
            for cc in range(k[2]):
                xs = xp[:, a:a + d, b:b + h, cc:cc + w].reshape(-1, x.shape[1]).flip(0)
                dw[a, b, cc] = xs.t() @ dyv
    return dw


# ---------------------------------------------------------------------------------------------------------------------------
# generator_in -> generator_block -> to_rgb through networks.ops (phase 2 of a 32-channel network on the base shape (1, 2, 2))
# ---------------------------------------------------------------------------------------------------------------------------
class Gen:
    id, n, latent, c, base, seed = 'generator_p2', 4, 32, 32, (1, 2, 2), 870
    fine = (2, 4, 4)
    kernel_spec = [[K333, K333], [K333, K333]]
    filter_spec = [[32, 32], [32, 32]]


GEN = Gen()
GEN_NAMES = ['generator_in/dense', 'generator_in/conv', 'to_rgb_1', 'generator_block_2/conv_1', 'generator_block_2/conv_2', 'to_rgb_2']


def gen_data(c):
    """Integer latents and image gradient; every effective filter integer valued: dense with NNZ entries of +-1 per unit (its
    output is stored exactly), conv_1 (the up-sampled one, whose data gradient sums eight voxels) sparse per input channel, the
    other two 3x3x3 filters and the image layers dense."""
    s = c.seed * 100
    units = c.c * c.base[0] * c.base[1] * c.base[2]
    q = {'generator_in/dense': A.sparse_filter(K111, c.latent, units, s + 1, 'out').reshape(c.latent, units).contiguous(),
         'generator_in/conv': A.dense_filter(K333, c.c, c.c, s + 2), 'to_rgb_1': A.dense_filter(K111, c.c, 1, s + 3),
         'generator_block_2/conv_1': A.sparse_filter(K333, c.c, c.c, s + 4, 'in'), 'generator_block_2/conv_2': A.dense_filter(K333, c.c, c.c, s + 5),
         'to_rgb_2': A.dense_filter(K111, c.c, 1, s + 6)}
    b = {nm: W.int_data((q[nm].shape[-1],), s + 10 + i, F32) for i, nm in enumerate(GEN_NAMES)}
    return {'z': W.int_data((c.n, c.latent), s, BF), 'g': A.ints((c.n, 1, *c.fine), s + 20, BF), 'q': q, 'b': b}
