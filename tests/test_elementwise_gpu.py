"""Every dispatch branch of csrc/elementwise.hip against a plain fp64 reference on the CPU, through saragan_amd.functional.
The shapes are the smallest that reach the branch named in each case's comment; they are derived from the dispatch
constants of the file: grid_for's caps (2048 default, 4096 pixel-norm / up / down, 8192 trilinear), kBwdBlocks = 1024
(bias / pixel-norm backward with per-block partial rows), team_size (pixel-norm lanes per voxel, a power of two <= 64),
the 16,384 row blocks of the row-wise up-scale, and grid_trips (sg_axpby / sg_lerp_rows: two trips past 2048 blocks).
E is the number of elements of a 16-byte piece (bf16 8, f32 4) and P = c / E the pieces per voxel.

Inputs are drawn in fp64 and rounded to the storage type first, LeakyReLU masks are INPUTS (an activation y or its sign
words), so the reference sees exactly the kernel's inputs and every element is compared.
Tolerances: tests/test_kernels_gpu.py's (f32 1e-4 / 1e-5 x max, bf16 1e-2 / 1e-2 x max; pixel-norm backward in bf16 3e-2);
f32 sums of K terms: ewref.sum_rtol(K) of the sum of the terms' absolute values."""
import numpy as np
import pytest
import torch

from oracle import pgan_oracle as O
from tests import ewref as R
from tests.ewref import DT, SLOPE, cl, close, dev, rnd

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32


def _name(dtype):
    return 'bf16' if dtype == BF else 'f32'


def _ids(cases):
    return [f'{_name(c[0])}-' + '-'.join('x'.join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c[1:-1]) for c in cases]


# ---------------------------------------------------------------------------------------------------
# 1. pixel norm
# ---------------------------------------------------------------------------------------------------
PN_CASES = [
    # dtype, c, (n, d, h, w), dispatch condition
    (BF, 1024, (1, 1, 1, 37), 'P = 128 > tp = 64: pixel_norm_kernel<.,.,4,1>, two piece slots, ragged last block (37 = 9 * 4 + 1)'),
    (BF, 520, (1, 1, 1, 37), 'P = 65 > tp = 64: pixel_norm_kernel<.,.,4,1>, second slot live on lane 0 only'),
    (BF, 2048, (1, 1, 1, 37), 'P = 256: the last vector case, all four piece slots live'),
    (BF, 2056, (1, 1, 1, 37), 'P = 257 > 256: pixel_norm_scalar_kernel'),
    (F32, 260, (1, 1, 1, 37), 'P = 65 > tp = 64: pixel_norm_kernel<.,.,4,1>'),
    (F32, 1024, (1, 1, 1, 37), 'P = 256: the last vector case'),
    (F32, 1028, (1, 1, 1, 37), 'P = 257 > 256: pixel_norm_scalar_kernel'),
    (BF, 24, (1, 1, 1, 37), 'P = 3 < tp = 4: pixel_norm_kernel<.,.,1,2>, one idle lane per team'),
    (BF, 40, (1, 1, 1, 37), 'P = 5 < tp = 8: pixel_norm_kernel<.,.,1,2>, three idle lanes per team'),
    (F32, 12, (1, 1, 1, 37), 'P = 3 < tp = 4: pixel_norm_kernel<.,.,1,2>'),
    (BF, 512, (5, 1, 37, 101), 'P = tp = 64, 4 teams: 18,685 voxels / 4 > 4096 blocks (fwd, bwd), second U slot live'),
    (F32, 256, (5, 1, 37, 101), 'P = tp = 64, 4 teams: 18,685 voxels / 4 > 4096 blocks (fwd, bwd), second U slot live'),
    (BF, 512, (3, 1, 37, 101), 'fused act-backward: 11,211 voxels / 4 > kBwdBlocks = 1024, 1024 partial rows, two trips'),
    (F32, 256, (3, 1, 37, 101), 'fused act-backward: 11,211 voxels / 4 > kBwdBlocks = 1024, 1024 partial rows, two trips'),
]


def _pn_inputs(dtype, c, sp):
    n, d, h, w = sp
    shape = (n, c, d, h, w)
    x = rnd(shape, 101, dtype)
    scale = R.pn_scale(x).float().double()                  # the saved f32 scale, an input of the backward kernels
    y = (x * scale).to(dtype).double()                      # the stored (rounded) y, likewise
    gy = rnd(shape, 102, dtype)
    m = rnd(shape, 103, dtype)                              # the tensor whose signs are the LeakyReLU mask
    return x, scale, y, gy, m


def _pn_act_terms(dtype, c, aligned, dx_ref, m, gd, yd, sd):
    """The terms sg_pixel_norm_act_bwd's dbias sums.  The one-pass kernel (16-byte pieces, P <= 256, aligned bases) sums its
    f32 values before they are stored: mask * dx in fp64.  Every other case runs two passes -- sg_pixel_norm_bwd stores dx in
    the tensor's type, sg_bias_act_bwd_bits masks and sums what it reads back -- so in bf16 the sum's inputs are the STORED
    (rounded) dx: the same kernel's output, which the caller has compared with fp64 element by element."""
    from saragan_amd import functional as F
    e = R.elems16(dtype)
    if dtype == F32 or (aligned and c % e == 0 and c // e <= 256):
        return dx_ref * R.lrelu_mask(m)
    return F._PixelNormBwd.apply(gd, yd, sd).double().cpu() * R.lrelu_mask(m)


@pytest.mark.parametrize('case', PN_CASES, ids=_ids(PN_CASES))
def test_pixel_norm_forward_backward_and_fused_act_backward(case):
    from saragan_amd import functional as F
    dtype, c, sp, _why = case
    x, scale, y, gy, m = _pn_inputs(dtype, c, sp)
    nvox = sp[0] * sp[1] * sp[2] * sp[3]
    # forward and the saved scale
    xg = cl(x, dtype).requires_grad_(True)
    yg = F.pixel_norm(xg)
    close(yg, x * R.pn_scale(x), dtype, 'pixel_norm fwd')
    assert torch.equal(yg.grad_fn.saved_tensors[0], yg.detach())
    sc = yg.grad_fn.saved_tensors[1]
    # f32 rsqrtf plus a c-term f32 sum of squares
    np.testing.assert_allclose(sc.double().cpu().numpy(), R.pn_scale(x).reshape(-1).numpy(), rtol=1e-5, err_msg='saved scale')
    # backward from the given y and scale
    yd, gd, sd = cl(y, dtype), cl(gy, dtype), scale.reshape(-1).float().to(dev())
    bt = None if dtype == F32 else (3e-2, 3e-2)             # reads the rounded y: tests/test_kernels_gpu.py's tolerance
    dx_ref = R.pn_bwd(gy, y, scale)
    close(F._PixelNormBwd.apply(gd, yd, sd), dx_ref, dtype, 'pixel_norm bwd', bt)
    # ... and through autograd from the forward's own y and scale
    (gx,) = torch.autograd.grad(yg, xg, gd)
    close(gx, dx_ref, dtype, 'pixel_norm bwd (autograd)', bt)
    # fused LeakyReLU backward, with and without the bias gradient
    words = R.sign_words_dev(m)
    dz_ref = dx_ref * R.lrelu_mask(m)
    dz0, _ = F._PnActBwd.apply(gd, yd, sd, words, SLOPE, False)
    close(dz0, dz_ref, dtype, 'pixel_norm_act_bwd dz', bt)
    dz1, db = F._PnActBwd.apply(gd, yd, sd, words, SLOPE, True)
    assert torch.equal(dz1, dz0), 'dz differs with the bias gradient requested'
    terms = _pn_act_terms(dtype, c, True, dx_ref, m, gd, yd, sd)
    R.assert_sum_close(db, terms.sum((0, 2, 3, 4)), terms.abs().sum((0, 2, 3, 4)), nvox, 'pixel_norm_act_bwd dbias')
    # the same with a gradient |gy| + 1: dx = scale * (g - y * mean_c(g y)) is then positive almost everywhere (mean_c(g y) is
    # of the order 1 / sqrt(c) and |y| rarely above 3), the channel sums are of the order of the sums of absolute values, and
    # the K-term bound (2.7e-3 at 11,211 voxels) is far below one lost trip, block or reduction stage
    gp = (gy.abs() + 1.0).to(dtype).double()
    gpd = cl(gp, dtype)
    dxp_ref = R.pn_bwd(gp, y, scale)
    dzp, dbp = F._PnActBwd.apply(gpd, yd, sd, words, SLOPE, True)
    close(dzp, dxp_ref * R.lrelu_mask(m), dtype, 'pixel_norm_act_bwd dz (one-signed)', bt)
    terms = _pn_act_terms(dtype, c, True, dxp_ref, m, gpd, yd, sd)
    assert float(terms.sum()) > 0.8 * float(terms.abs().sum())
    R.assert_sum_close(dbp, terms.sum((0, 2, 3, 4)), terms.abs().sum((0, 2, 3, 4)), nvox, 'pixel_norm_act_bwd dbias (one-signed)')


# ---------------------------------------------------------------------------------------------------
# 2. bias + LeakyReLU
# ---------------------------------------------------------------------------------------------------
BA_CASES = [
    # dtype, c, nvox, dispatch condition
    (BF, 32, 70001, 'vec: P = 4, 64 rows per block, 70,001 / 64 > kBwdBlocks = 1024'),
    (BF, 2048, 1500, 'vec: P = 256, one row per block, ny = 1, 1500 > 1024 blocks'),
    (BF, 4096, 1500, 'vec: P = 512, ny = 2 channel slices, 1500 > 1024 blocks'),
    (BF, 96, 70001, 'scalar: P = 12 does not divide 256; 70,001 / 64 > 1024 blocks, trailing blocks past the last voxel'),
    (BF, 20, 70001, 'scalar: c % 8 != 0, c > 8'),
    (F32, 32, 70001, 'vec: P = 8, 32 rows per block, capped'),
    (F32, 2048, 1500, 'vec: P = 512, ny = 2'),
    (F32, 4096, 1500, 'vec: P = 1024, ny = 4'),
    (F32, 96, 70001, 'scalar: P = 24 does not divide 256'),
    (F32, 20, 70001, 'scalar: P = 5 does not divide 256'),
] + [(dt, c, 300001, 'small: c <= 8 without 16-byte pieces, 300,001 / 256 > 1024 blocks') for dt in (BF, F32) for c in (1, 3, 5, 7)]


def _ba_shape(c, nvox):
    return (1, c, 1, 1, nvox)


@pytest.mark.parametrize('case', BA_CASES, ids=_ids(BA_CASES))
def test_bias_act_backward_both_mask_forms(case):
    from saragan_amd import functional as F
    dtype, c, nvox, _why = case
    shape = _ba_shape(c, nvox)
    dy = rnd(shape, 111, dtype)
    y = rnd(shape, 112, dtype)
    y[0, :, 0, 0, :5] = 0.0                      # y >= 0 is the positive side
    ref = dy * R.lrelu_mask(y)
    # The bias gradients are driven with |dy|: every term mask * |dy| is positive, so a channel's sum IS the sum of its
    # terms' absolute values and the K-term bound (1.7 % at 70,001 voxels, 7 % at 300,001) is a bound relative to the result.
    # With a zero-mean dy the sum is a random walk of sqrt(nvox) terms against a bound that grows with nvox: a lost trip of
    # the capped grid (6 % / 13 % of the voxels), a lost wave of the block reduction, or zeros, would pass.
    dya = dy.abs()
    refa = dya * R.lrelu_mask(y)
    db_ref = refa.sum((0, 2, 3, 4))
    dyd, dyad = cl(dy, dtype), cl(dya, dtype)
    for what, mask in (('y', cl(y, dtype)), ('sign words', R.sign_words_dev(y))):
        dx, none = F.raw_bias_act_bwd(dyd, mask, SLOPE, True, False)
        assert none is None
        close(dx, ref, dtype, f'dx only ({what})')
        none, db = F.raw_bias_act_bwd(dyad, mask, SLOPE, False, True)
        assert none is None
        R.assert_sum_close(db, db_ref, db_ref, nvox, f'dbias only ({what})')
        dx2, db2 = F.raw_bias_act_bwd(dyad, mask, SLOPE, True, True)
        close(dx2, refa, dtype, f'dx with dbias ({what})')
        R.assert_sum_close(db2, db_ref, db_ref, nvox, f'dbias with dx ({what})')
        assert torch.equal(F.raw_bias_act_bwd(dyd, mask, SLOPE, True, True)[0], dx), f'dx differs with dbias requested ({what})'


@pytest.mark.parametrize('dtype', DT, ids=_name)
def test_bias_act_backward_without_mask(dtype):
    """y == NULL: dx = dy, dbias = column sums (a bias without an activation)."""
    from saragan_amd import functional as F
    c, nvox = 32, 1001
    dy = rnd(_ba_shape(c, nvox), 113, dtype).abs()           # one-signed terms: see test_bias_act_backward_both_mask_forms
    dx, db = F.raw_bias_act_bwd(cl(dy, dtype), None, SLOPE, True, True)
    assert torch.equal(dx.double().cpu(), dy)
    R.assert_sum_close(db, dy.sum((0, 2, 3, 4)), dy.sum((0, 2, 3, 4)), nvox, 'dbias')


@pytest.mark.parametrize('dtype', DT, ids=_name)
@pytest.mark.parametrize('c,nvox', [(c, 1001) for c in (1, 3, 5, 7, 20, 32, 96, 2048, 4096)] + [(4096, 1100)])
def test_bias_act_forward(c, nvox, dtype):
    """Vector kernel where c % E == 0, element-wise kernel otherwise.  Blocks of 256 items against grid_for's cap of 2048 (a
    second grid-stride trip): c = 4096 at nvox = 1,001 is 4,004 blocks in f32 but 2,002 in bf16, so nvox = 1,100 is added,
    where bf16 has 2,200 blocks; c = 2048 f32 at 1,001 has 2,002 (one trip)."""
    from saragan_amd import functional as F
    x = rnd(_ba_shape(c, nvox), 114, dtype)
    b = rnd((c,), 115, F32)
    xd, bd = cl(x, dtype), b.float().to(dev())
    for act in (True, False):
        close(F.bias_act(xd, bd, act, SLOPE), O.act(O.apply_bias(x, b), 'leaky_relu' if act else 'linear', SLOPE), dtype, f'act={act}')
    close(F.bias_act(xd, None, True, SLOPE), O.act(x, 'leaky_relu', SLOPE), dtype, 'no bias')


# ---------------------------------------------------------------------------------------------------
# 3. sign words
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT, ids=_name)
@pytest.mark.parametrize('c', [1, 31, 32, 33, 72])
def test_sign_words_exact(c, dtype):
    """nvox = 257 (c = 72: 257 * 3 = 771 words, four blocks of 256 threads; c <= 32: 257 words, two blocks).  -0.0 and +0.0 are not negative; the smallest negative
    subnormal is."""
    from saragan_amd import functional as F
    t = rnd((1, c, 1, 1, 257), 121, dtype)
    tiny = -(2.0 ** -133) if dtype == BF else -(2.0 ** -149)
    flat = t.permute(0, 2, 3, 4, 1).reshape(-1)             # NDHWC order (a copy: written back below)
    flat[0::7] = -0.0
    flat[1::7] = 0.0
    flat[2::7] = tiny
    t = flat.reshape(1, 1, 1, 257, c).permute(0, 4, 1, 2, 3).contiguous()
    td = cl(t, dtype)
    assert torch.equal(td.cpu().double(), t) and float(td.cpu().double().permute(0, 2, 3, 4, 1).reshape(-1)[2]) == tiny   # it survives the storage type
    ref = R.sign_words_np(t)
    got = F.sign_words(td).cpu().numpy()
    assert got.shape == ref.shape == (1, 1, 1, 257, (c + 31) // 32)
    assert np.array_equal(got, ref)
    if c % 32:                                   # bits of channels >= c
        dead = np.uint32((0xFFFFFFFF << (c % 32)) & 0xFFFFFFFF)
        assert not (got.view(np.uint32)[..., -1] & dead).any()


# ---------------------------------------------------------------------------------------------------
# 4. nearest up / sum down
# ---------------------------------------------------------------------------------------------------
UP_CASES = [
    # dtype, x shape (n, c, d, h, w), factors, dispatch condition
    (BF, (1, 64, 70, 130, 8), (2, 1, 2), 'rows<HP = 1>: OW * P = 16 * 8 = 128; 140 * 130 = 18,200 rows > 16,384 row blocks'),
    (F32, (1, 32, 70, 130, 8), (2, 1, 2), 'rows<HP = 1>: OW * P = 16 * 8 = 128; 18,200 rows > 16,384 row blocks'),
    (BF, (2, 16, 40, 32, 30), (2, 2, 2), 'flat vec: OW * P = 60 * 2 < 128; 1,228,800 output pieces > 4096 * 256'),
    (F32, (2, 8, 40, 32, 30), (2, 2, 2), 'flat vec: OW * P = 60 * 2 < 128; 1,228,800 output pieces > 4096 * 256'),
    (BF, (2, 6, 1, 5, 7), (1, 2, 2), 'flat scalar: c = 6, D = 1 (the 2-D tree)'),
    (F32, (2, 6, 1, 5, 7), (1, 2, 2), 'flat scalar: c = 6, D = 1'),
    (BF, (1, 40, 1, 410, 512), (1, 1, 2), 'masked block sum (the gradient): c = 40 has a 8-channel second word; 209,920 * 5 pieces > 4096 * 256'),
    (F32, (1, 40, 1, 206, 512), (1, 1, 2), 'masked block sum (the gradient): c = 40; 105,472 * 10 pieces > 4096 * 256'),
    (BF, (2, 64, 3, 4, 16), (2, 2, 2), 'rows<HP = 2>: H doubled, a block writes a pair of rows'),
]


@pytest.mark.parametrize('case', UP_CASES, ids=_ids(UP_CASES))
def test_upscale_nearest_and_its_gradient(case):
    """y = gain * up(x) (* mask) and, as its autograd gradient, gain * block sum of (mask *) g: sg_upscale_nn and
    sg_downscale_sum(_masked) at the shapes of one another's gradient."""
    from saragan_amd import functional as F
    dtype, shape, factors, _why = case
    gain = 0.5
    x = rnd(shape, 131, dtype)
    up = R.up_nn(x, factors)
    g = rnd(tuple(up.shape), 132, dtype)
    m = rnd(tuple(up.shape), 133, dtype)
    mk = R.lrelu_mask(m)
    xd, gd = cl(x, dtype).requires_grad_(True), cl(g, dtype)
    y = F.upscale2x(xd, gain, factors)
    close(y, gain * up, dtype, 'up')
    close(torch.autograd.grad(y, xd, gd)[0], gain * R.down_sum(g, factors), dtype, 'up gradient (block sum)')
    ym = F._Up.apply(xd, gain, R.sign_words_dev(m), SLOPE, factors)
    close(ym, gain * up * mk, dtype, 'masked up')
    close(torch.autograd.grad(ym, xd, gd)[0], gain * R.down_sum(g * mk, factors), dtype, 'masked up gradient (masked block sum)')


DOWN_CASES = [
    (BF, (2, 16, 4, 6, 10), (2, 2, 2), 'vec'),
    (F32, (2, 16, 4, 6, 10), (2, 2, 2), 'vec'),
    (BF, (2, 6, 1, 10, 14), (1, 2, 2), 'scalar: c = 6, D = 1'),
    (F32, (2, 6, 1, 10, 14), (1, 2, 2), 'scalar: c = 6, D = 1'),
    (BF, (1, 8, 1, 1030, 2048), (1, 1, 2), 'vec: 1030 * 1024 = 1,054,720 output pieces > 4096 * 256'),
]


@pytest.mark.parametrize('case', DOWN_CASES, ids=_ids(DOWN_CASES))
def test_downscale_sum_and_its_gradient(case):
    from saragan_amd import functional as F
    dtype, shape, factors, _why = case
    gain = 1.0 / (factors[0] * factors[1] * factors[2])
    x = rnd(shape, 134, dtype)
    ref = gain * R.down_sum(x, factors)
    g = rnd(tuple(ref.shape), 135, dtype)
    xd = cl(x, dtype).requires_grad_(True)
    y = F.downscale2x(xd, gain, None, factors)
    close(y, ref, dtype, 'down')
    close(torch.autograd.grad(y, xd, cl(g, dtype))[0], gain * R.up_nn(g, factors), dtype, 'down gradient (up)')
    m = rnd(shape, 136, dtype)
    ym = F._Down.apply(xd, gain, None, factors, R.sign_words_dev(m), SLOPE)
    close(ym, gain * R.down_sum(x * R.lrelu_mask(m), factors), dtype, 'masked down')
    close(torch.autograd.grad(ym, xd, cl(g, dtype))[0], gain * R.up_nn(g, factors) * R.lrelu_mask(m), dtype, 'masked down gradient (masked up)')


# ---------------------------------------------------------------------------------------------------
# 5. trilinear up and adjoint
# ---------------------------------------------------------------------------------------------------
TRI_CASES = [
    # dtype, x shape, check the adjoint at this shape too, dispatch condition
    (BF, (1, 16, 32, 66, 65), False, 'up, vec: 8 * 137,280 voxels * 2 pieces = 2,196,480 > 8192 * 256'),
    (F32, (1, 8, 32, 66, 65), False, 'up, vec: 2,196,480 pieces > 8192 * 256'),
    (BF, (2, 6, 3, 5, 7), True, 'scalar: c = 6, odd extents'),
    (F32, (2, 6, 3, 5, 7), True, 'scalar: c = 6, odd extents'),
    (BF, (2, 16, 3, 5, 7), True, 'vec, small'),
    (F32, (2, 16, 3, 5, 7), True, 'vec, small'),
]


def _adjoint_identity(up, g, x, adj, dtype):
    """<up(x), g> == <x, adj(g)> in fp64 over the returned tensors, to the storage rounding of the two outputs."""
    eps = 2.0 ** -8 if dtype == BF else 2.0 ** -23
    a, b = up.double().cpu() * g, x * adj.double().cpu()
    lim = eps * (float(a.abs().sum()) + float(b.abs().sum()))
    assert abs(float(a.sum()) - float(b.sum())) <= lim, (float(a.sum()), float(b.sum()), lim)


@pytest.mark.parametrize('case', TRI_CASES, ids=_ids(TRI_CASES))
def test_trilinear_up(case):
    from saragan_amd import functional as F
    dtype, shape, with_adj, _why = case
    x = rnd(shape, 141, dtype)
    up = F.upscale_trilinear2x(cl(x, dtype))
    close(up, R.tri_up(x), dtype, 'trilinear up')
    if with_adj:
        g = rnd(tuple(up.shape), 142, dtype)
        adj = F._TriUp.apply(cl(g, dtype), True)
        close(adj, R.tri_up_adj(g), dtype, 'trilinear adjoint')
        _adjoint_identity(up, g, x, adj, dtype)


def test_trilinear_adjoint_capped():
    """adjoint: 352,870 voxels * 6 channels = 2,117,220 items > 8192 * 256 in the element-wise kernel.  A capped grid needs
    more than 2^21 items, and g holds 8 elements per item in the element-wise kernel (33.9 MB in bf16, over 64 MB in f32) and
    8 * E per item with 16-byte pieces (over 64 MB in both types): this case is bf16 with c = 6 only."""
    from saragan_amd import functional as F
    dtype, shape = BF, (1, 6, 71, 71, 70)
    g = rnd((1, 6, 142, 142, 140), 143, dtype)
    adj = F._TriUp.apply(cl(g, dtype), True)
    close(adj, R.tri_up_adj(g), dtype, 'trilinear adjoint')
    x = rnd(shape, 144, dtype)
    up = F.upscale_trilinear2x(cl(x, dtype))                # 8 * 2,117,220 items: capped as well (element-wise kernel)
    close(up, R.tri_up(x), dtype, 'trilinear up')
    _adjoint_identity(up, g, x, adj, dtype)


# ---------------------------------------------------------------------------------------------------
# 6. lerp / sg_axpby, sg_axpby_dev, interpolate_rows
# ---------------------------------------------------------------------------------------------------
BIG = 8 * 4096 * 256 + 5      # numel / E + 1 pieces: 4097 (bf16) / 8193 (f32) blocks of 256 -> grid_trips gives 2049 / 4097
                              # blocks and a second trip; the scalar tail has BIG % 8 = 5 elements in bf16, BIG % 4 = 1 in f32


@pytest.mark.parametrize('dtype', DT, ids=_name)
@pytest.mark.parametrize('numel', [1, 7, 1003, BIG])
def test_lerp_axpby(numel, dtype):
    """numel = 1, 7: tail only (bf16) / one piece and a tail; 1003: pieces and a tail of 3; BIG: second grid trip and tail."""
    from saragan_amd import functional as F
    a, b = rnd((1, numel), 151, dtype), rnd((1, numel), 152, dtype)
    ad, bd = cl(a, dtype), cl(b, dtype)
    close(F.lerp(ad, bd, 0.3, 0.7), np.float32(0.3).item() * a + np.float32(0.7).item() * b, dtype, 'lerp')
    close(F.lerp(ad, None, 0.3, 0.0), np.float32(0.3).item() * a, dtype, 'b = None')
    if numel != BIG:
        close(F.lerp(ad, bd, -1.5, 2.25), -1.5 * a + 2.25 * b, dtype, 'weights outside [0, 1]')
    # weights exactly 0 and 1 reproduce an operand bit for bit
    assert torch.equal(F.lerp(ad, bd, 1.0, 0.0), ad), 'wa = 1, wb = 0'
    assert torch.equal(F.lerp(ad, bd, 0.0, 1.0), bd), 'wa = 0, wb = 1'
    assert torch.equal(F.lerp(ad, None, 1.0, 0.0), ad), 'wa = 1, b = None'
    # the device-coefficient entry point: same f32 weights, same arithmetic
    ds = F.DevScalars(dev())
    wa, wb = ds.coef(0, 0.3), ds.coef(1, 0.7)
    ds.flush()
    assert torch.equal(F.lerp(ad, bd, wa, wb), F.lerp(ad, bd, 0.3, 0.7)), 'sg_axpby_dev differs from sg_axpby'
    assert torch.equal(F.lerp(ad, None, wa, 0.0), F.lerp(ad, None, 0.3, 0.0)), 'sg_axpby_dev (b = None) differs from sg_axpby'


@pytest.mark.parametrize('dtype', DT, ids=_name)
@pytest.mark.parametrize('per_sample', [40, 41, 8 * 700 + 3])
def test_interpolate_rows(per_sample, dtype):
    """n = 3.  per_sample % E == 0 (40): 16-byte pieces, gamma[i / pv]; otherwise (41; 5603 = several blocks) the
    element-wise path, gamma[i / per_sample]."""
    from saragan_amd import functional as F
    a, b = rnd((3, per_sample), 153, dtype), rnd((3, per_sample), 154, dtype)
    ad, bd = cl(a, dtype), cl(b, dtype)
    for gam in (torch.tensor([0.0, 1.0, 0.3]), torch.rand(3, generator=torch.Generator().manual_seed(155))):
        g = gam.float().double().reshape(3, 1)
        out = F.interpolate_rows(gam.float().to(dev()).reshape(3, 1, 1, 1, 1), ad, bd)
        close(out, g * a + (1.0 - g) * b, dtype, 'interpolate_rows')
        for i in range(3):
            if float(gam[i]) == 0.0:
                assert torch.equal(out[i], bd[i]), 'gamma = 0 does not reproduce b'
            if float(gam[i]) == 1.0:
                assert torch.equal(out[i], ad[i]), 'gamma = 1 does not reproduce a'
    # 5-D operands take the same path (NDHWC storage, per_sample = c * d * h * w)
    a5, b5 = rnd((3, 5, 2, 2, 2), 156, dtype), rnd((3, 5, 2, 2, 2), 157, dtype)
    g = torch.tensor([0.25, 0.5, 0.75])
    close(F.interpolate_rows(g.to(dev()), cl(a5, dtype), cl(b5, dtype)),
          g.double().reshape(3, 1, 1, 1, 1) * a5 + (1 - g.double().reshape(3, 1, 1, 1, 1)) * b5, dtype, 'interpolate_rows 5-D')


# ---------------------------------------------------------------------------------------------------
# 7. instance noise
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT, ids=_name)
def test_add_noise_exact_properties(dtype):
    from saragan_amd import functional as F
    N, sd, seed = 4096, 0.5, 11
    x = rnd((1, N + 4), 161, dtype)
    xd = cl(x, dtype)
    full = F.add_noise(xd, sd, seed)
    assert int((full != xd).sum()) > 0.9 * N
    for k in (0, 1, 2, 3):          # a tail group of k elements: every element is what it is in the run with whole groups
        out = F.add_noise(xd[:, :N + k].contiguous(), sd, seed)
        assert torch.equal(out, full[:, :N + k]), k
    # the Philox offset counts groups of four elements
    z0 = F.add_noise(torch.zeros(1, N + 4 * 5, device=dev(), dtype=dtype), sd, seed, 0)
    for j in (1, 5):
        zj = F.add_noise(torch.zeros(1, N, device=dev(), dtype=dtype), sd, seed, j)
        assert torch.equal(zj, z0[:, 4 * j:4 * j + N]), j
    # ... above 2^32 too (the counter's high word)
    hi = (1 << 40) + 3
    assert torch.equal(F.add_noise(torch.zeros(1, N, device=dev(), dtype=dtype), sd, seed, hi + 2),
                       F.add_noise(torch.zeros(1, N + 8, device=dev(), dtype=dtype), sd, seed, hi)[:, 8:])
    # the device counter: read by the kernel, then advanced by 1 << 40
    j = 5
    ctr = torch.tensor([j], dtype=torch.int64, device=dev())
    xs = xd[:, :N + 1].contiguous()
    assert torch.equal(F.add_noise(xs, sd, seed, ctr), F.add_noise(xs, sd, seed, j)), 'sg_add_noise_dev differs from sg_add_noise'
    assert int(ctr.item()) == j + (1 << 40)


@pytest.mark.parametrize('dtype', DT, ids=_name)
def test_add_noise_moments(dtype):
    """N = 2^20 draws: mean, standard deviation and kurtosis of (out - x) / stddev within 6 standard errors (1/sqrt(N),
    1/sqrt(2N), sqrt(24/N)).  bf16 is measured on a zero x (so out - x is the stored noise itself).  Its rounding is a
    relative perturbation z (1 + e) with E[e^2] = v <= 2^-18: the variance becomes (1 + v) E[z^2], so v E[z^2] is added to the
    bound of the standard deviation (twice what it moves)."""
    from saragan_amd import functional as F
    N, sd = 1 << 20, 2.0
    x = torch.zeros(1, N, dtype=torch.float64) if dtype == BF else rnd((1, N), 162, dtype)
    out = F.add_noise(cl(x, dtype), sd, seed=7)
    z = ((out.float() - cl(x, dtype).float()) / sd).double().cpu()
    extra = 2.0 ** -18 * float((z * z).mean()) if dtype == BF else 0.0
    mean, std = float(z.mean()), float(z.std())
    kurt = float((((z - mean) / std) ** 4).mean())
    print('add_noise moments', _name(dtype), mean, std, kurt)
    assert abs(mean) <= 6.0 / np.sqrt(N), mean
    assert abs(std - 1.0) <= 6.0 / np.sqrt(2 * N) + extra, std
    assert abs(kurt - 3.0) <= 6.0 * np.sqrt(24.0 / N), kurt


# ---------------------------------------------------------------------------------------------------
# 8. sumsq_keep_w
# ---------------------------------------------------------------------------------------------------
SUMSQ_SHAPES = [
    (2, 1, 1, 1, 1),        # d * h = 1, w = 1: one row, one live thread
    (3, 3, 1, 9, 300),      # c = 3 (the 2-D tree's RGB); w > 256: the thread loop / the ordered kernel's w0 loop
    (2, 1, 5, 13, 257),     # d * h = 65 > 64: two rows per block, 33 blocks adding atomically into one output; w = 257
    (2, 4, 8, 40, 16),      # d * h = 320: 64 blocks of 5 rows; ordered kernel: TY = 64 row slots of 5 rows
    (1, 1, 2, 3, 1000),     # w = 1000: four trips of the thread loop / of the w0 loop
]


@pytest.mark.parametrize('dtype', DT, ids=_name)
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomic', 'ordered'])
@pytest.mark.parametrize('shape', SUMSQ_SHAPES, ids=['x'.join(map(str, s)) for s in SUMSQ_SHAPES])
def test_sumsq_keep_w(shape, deterministic, dtype, sg_env):
    """'ordered' is SG_DETERMINISTIC=1 (sumsq_keep_w_ordered_kernel), set through the sg_env fixture, which restores the
    environment it found.  That the mode took effect is asserted where the two kernels add in different orders (320 rows:
    64 blocks of 5 consecutive rows added atomically / 64 row slots striding by 64): some of the 32 f32 sums of 1,280 terms
    each must differ in their last bits, while the ordered kernel repeats itself bit for bit."""
    from saragan_amd import functional as F
    n, c, d, h, w = shape
    g = rnd(shape, 171, dtype)
    gout = rnd((n, w), 172, F32)
    ref = (g * g).sum(dim=(1, 2, 3))
    sg_env(SG_DETERMINISTIC=1 if deterministic else 0)
    gd = cl(g, dtype).requires_grad_(True)
    got = F.sumsq_keep_w(gd)
    again = F.sumsq_keep_w(gd).detach()
    (gg,) = torch.autograd.grad(got, gd, gout.float().to(dev()))
    if deterministic and shape == (2, 4, 8, 40, 16):
        sg_env(SG_DETERMINISTIC=0)
        assert not torch.equal(F.sumsq_keep_w(gd).detach(), again), 'SG_DETERMINISTIC=1 did not select the ordered kernel'
    R.assert_sum_close(got, ref, ref, c * d * h, 'sumsq_keep_w')
    if deterministic:
        assert torch.equal(got.detach(), again), 'the ordered kernel is not reproducible'
    close(gg, 2.0 * g * gout.reshape(n, 1, 1, 1, w), dtype, '_SumsqKeepW.backward')


# ---------------------------------------------------------------------------------------------------
# 9. minibatch stddev
# ---------------------------------------------------------------------------------------------------
MBSTD_CASES = [
    # n, group_size, c, (d, h, w), identical pair, dispatch condition
    (2, 4, 6, (1, 4, 4), False, 'n < group_size: one group of 2'),
    (4, 4, 6, (1, 4, 4), False, 'n == group_size: one group'),
    (8, 4, 6, (1, 4, 4), False, 'two groups'),
    (12, 4, 6, (1, 4, 4), False, 'three groups'),
    (6, 3, 6, (1, 4, 4), False, 'two groups of 3'),
    (8, 4, 7, (1, 100, 100), False, 'per_sample = 70,000 > 256 * 256: capped grid, 256 blocks add into one statistic'),
    (2, 4, 6, (1, 4, 4), True, 'the two samples of the group are identical: zero variance at every element'),
]


@pytest.mark.parametrize('dtype', DT, ids=_name)
@pytest.mark.parametrize('case', MBSTD_CASES, ids=[f'n{c[0]}g{c[1]}c{c[2]}at{"x".join(map(str, c[3]))}{"same" if c[4] else ""}' for c in MBSTD_CASES])
def test_minibatch_stddev(case, dtype):
    from saragan_amd import functional as F
    n, gs, c, sp, same, _why = case
    x = rnd((n, c, *sp), 181, dtype)
    if same:
        x[1] = x[0]
    xr = x.clone().requires_grad_(True)
    yr = O.minibatch_stddev_layer(xr, gs)
    gy = R.mbstd_grad_input(tuple(yr.shape), 182, dtype)
    (gxr,) = torch.autograd.grad(yr, [xr], gy)
    xg = cl(x, dtype).requires_grad_(True)
    yg = F.minibatch_stddev(xg, gs)
    assert torch.equal(yg[:, :c].detach().double().cpu(), x), 'the copied channels'
    stat_ref = yr[:, c:].detach()
    np.testing.assert_allclose(yg[:, c:].detach().double().cpu().numpy(), stat_ref.numpy(), rtol=R.tol(dtype)[0], err_msg='statistic')
    (gxg,) = torch.autograd.grad(yg, [xg], cl(gy, dtype))
    close(gxg, gxr, dtype, 'mbstd backward')


# ---------------------------------------------------------------------------------------------------
# base pointers that are not 16-byte aligned
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT, ids=_name)
def test_unaligned_base_selects_the_scalar_fallbacks(dtype):
    """Every dispatcher's sg_aligned16 test with a tensor that starts one element past a 16-byte boundary, at a channel
    count that would otherwise take the 16-byte kernels (c = 32): the element-wise fallbacks must give the same numbers."""
    from saragan_amd import functional as F
    shape = (2, 32, 3, 4, 6)
    x, gy, m = rnd(shape, 191, dtype), rnd(shape, 192, dtype), rnd(shape, 193, dtype)
    b = rnd((32,), 194, F32)
    xu, gu = R.unaligned(x, dtype), R.unaligned(gy, dtype)
    assert F.ndhwc(xu).data_ptr() == xu.data_ptr() and xu.data_ptr() % 16 != 0      # the wrapper keeps the pointer
    assert F.ndhwc(gu).data_ptr() == gu.data_ptr() and gu.data_ptr() % 16 != 0
    nvox = 2 * 3 * 4 * 6
    # bias_act forward and backward (y form with an unaligned y, sign-word form with an unaligned dy)
    close(F.bias_act(xu, b.float().to(dev()), True, SLOPE), O.act(O.apply_bias(x, b), 'leaky_relu', SLOPE), dtype, 'bias_act')
    ref = gy * R.lrelu_mask(x)
    for what, dy_, mask in (('y unaligned', cl(gy, dtype), xu), ('dy unaligned', gu, cl(x, dtype)), ('words', gu, R.sign_words_dev(x))):
        dx, db = F.raw_bias_act_bwd(dy_, mask, SLOPE, True, True)
        close(dx, ref, dtype, f'bias_act bwd dx ({what})')
        R.assert_sum_close(db, ref.sum((0, 2, 3, 4)), ref.abs().sum((0, 2, 3, 4)), nvox, f'bias_act bwd db ({what})')
    # pixel norm forward, backward, fused act-backward
    scale = R.pn_scale(x).float().double()
    y = (x * scale).to(dtype).double()
    close(F.pixel_norm(xu), x * R.pn_scale(x), dtype, 'pixel_norm')
    bt = None if dtype == F32 else (3e-2, 3e-2)
    sd = scale.reshape(-1).float().to(dev())
    dx_ref = R.pn_bwd(gy, y, scale)
    close(F._PixelNormBwd.apply(gu, cl(y, dtype), sd), dx_ref, dtype, 'pixel_norm bwd (dy unaligned)', bt)
    close(F._PixelNormBwd.apply(cl(gy, dtype), R.unaligned(y, dtype), sd), dx_ref, dtype, 'pixel_norm bwd (y unaligned)', bt)
    dz_ref = dx_ref * R.lrelu_mask(m)
    dz, db = F._PnActBwd.apply(gu, cl(y, dtype), sd, R.sign_words_dev(m), SLOPE, True)
    close(dz, dz_ref, dtype, 'pixel_norm_act_bwd', bt)
    terms = _pn_act_terms(dtype, 32, False, dx_ref, m, gu, cl(y, dtype), sd)
    R.assert_sum_close(db, terms.sum((0, 2, 3, 4)), terms.abs().sum((0, 2, 3, 4)), nvox, 'pixel_norm_act_bwd dbias')
    # up, down (plain and masked), trilinear and its adjoint
    f = (2, 2, 2)
    close(F.upscale2x(xu, 0.5, f), 0.5 * R.up_nn(x, f), dtype, 'up')
    mu = rnd(tuple(R.up_nn(x, f).shape), 195, dtype)
    close(F._Up.apply(xu, 0.5, R.sign_words_dev(mu), SLOPE, f), 0.5 * R.up_nn(x, f) * R.lrelu_mask(mu), dtype, 'masked up')
    x2 = rnd((2, 32, 4, 4, 6), 196, dtype)
    m2 = rnd((2, 32, 4, 4, 6), 197, dtype)
    x2u = R.unaligned(x2, dtype)
    close(F.downscale2x(x2u, 0.125, None, f), 0.125 * R.down_sum(x2, f), dtype, 'down')
    close(F._Down.apply(x2u, 0.125, None, f, R.sign_words_dev(m2), SLOPE), 0.125 * R.down_sum(x2 * R.lrelu_mask(m2), f), dtype, 'masked down')
    close(F.upscale_trilinear2x(xu), R.tri_up(x), dtype, 'trilinear up')
    close(F._TriUp.apply(x2u, True), R.tri_up_adj(x2), dtype, 'trilinear adjoint')


@pytest.mark.parametrize('dtype', DT, ids=_name)
def test_unaligned_base_is_refused_without_a_write(dtype):
    """sg_axpby, sg_axpby_dev and sg_lerp_rows have no element-wise fallback: SG_EALIGN, and the output keeps its sentinel.
    (The wrappers allocate their outputs, so the entry points are called directly.)"""
    from saragan_amd import _lib
    from saragan_amd import functional as F
    lib = _lib.load()
    SG_EALIGN = -3
    n, per = 3, 40
    a, b = rnd((n, per), 198, dtype), rnd((n, per), 199, dtype)
    ad, bd, au, bu = cl(a, dtype), cl(b, dtype), R.unaligned(a, dtype), R.unaligned(b, dtype)
    gam = torch.tensor([0.0, 1.0, 0.3], device=dev())
    w = torch.tensor([0.3, 0.7], device=dev())
    dt, st = F._dt(ad), F._stream()
    p = F._ptr
    e = R.elems16(dtype)
    obuf = torch.full((n * per + e,), 7.0, dtype=dtype, device=dev())
    out, outu = obuf[:n * per], obuf[1:1 + n * per]
    assert out.data_ptr() % 16 == 0 and outu.data_ptr() % 16 != 0
    for pa, pb, po in ((au, bd, out), (ad, bu, out), (ad, bd, outu)):
        assert lib.sg_axpby(p(pa), p(pb), p(po), 0.3, 0.7, n * per, dt, st) == SG_EALIGN
        assert lib.sg_axpby_dev(p(pa), p(pb), p(po), p(w), n * per, dt, st) == SG_EALIGN
        assert lib.sg_lerp_rows(p(pa), p(pb), p(gam), p(po), n, per, dt, st) == SG_EALIGN
    assert lib.sg_axpby(p(au), None, p(out), 0.3, 0.0, n * per, dt, st) == SG_EALIGN
    torch.cuda.synchronize()
    assert bool((obuf == 7.0).all()), 'a refused call wrote to its output'
    with pytest.raises(_lib.SgError):
        F.lerp(au, bd, 0.3, 0.7)
    with pytest.raises(_lib.SgError):
        F.interpolate_rows(gam, ad, bu)
    # and the aligned calls on the same buffers do write
    assert lib.sg_axpby(p(ad), p(bd), p(out), 0.3, 0.7, n * per, dt, st) == 0
    close(out.reshape(n, per), np.float32(0.3).item() * a + np.float32(0.7).item() * b, dtype, 'aligned sg_axpby')
