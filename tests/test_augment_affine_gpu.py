"""The affine discriminator augmentation on the device (saragan_amd/csrc/augment_affine.hip) against its numpy restatement
(tests/affref.py).  The kernel's arithmetic is fixed operation by operation, so every kernel comparison here is bit for bit;
the network-level tests state their own tolerances where two different kernel routes are compared."""
import os

import numpy as np
import pytest
import torch

from tests import affref as A
from tests import augref as R
from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
FILL = -1.0


def _to_dev(a, dtype=torch.float32):
    """numpy [n, d, h, w, c] -> device tensor of logical shape [n, c, d, h, w] stored NDHWC."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    return t.permute(0, 4, 1, 2, 3).contiguous(memory_format=torch.channels_last_3d)


def _to_np(t):
    return t.detach().float().permute(0, 2, 3, 4, 1).contiguous().cpu().numpy()


def _rows(rows):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 16))).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _data(shape, seed):
    """bf16-representable values of magnitude in [0.25, 4), some zeros and one -0.0: no product with a weight is subnormal."""
    rng = np.random.default_rng(seed)
    v = np.ldexp(1.0 + rng.integers(0, 128, shape) / 128.0, rng.integers(-2, 2, shape)) * rng.choice([-1.0, 1.0], shape)
    v = v.astype(np.float32)
    flat = v.reshape(-1)
    flat[rng.choice(flat.size, max(2, flat.size // 16), replace=False)] = 0.0
    flat[flat.size // 3] = -0.0
    return v


def _case_rows(shape):
    n, d, h, w, c = shape
    rows = [A.IDENTITY]
    for ax, e in enumerate((d, h, w)):
        for s in (0.25, -0.25, e - 1, -(e - 1), e, -(e + 0.5)):      # the last two: nothing but fill / zeros
            t = [0.0, 0.0, 0.0]
            t[ax] = s
            rows.append(A.shift_row(t))
    rows += [A.shift_row((0, 0, 2.0 ** 20)), A.shift_row((0, -2.0 ** 20, 0.25)), A.scale_row(0.5, (d, h, w)), A.scale_row(2.0, (d, h, w))]
    if h == w:
        rows += [A.quarter_turn_row(k, h) for k in (1, 2, 3)]
    rows += [A.row_of(a=1.5, b=-0.25), A.shift_row((0.25, -0.5, 0.75), a=1.5, b=-0.25)]
    # the d axis coupled to the plane (no draw does it: the adjoint's general candidate test): a dyadic shear and a turn of
    # 30 degrees in the (d, w) plane about the centre
    cs, sn, cen = np.cos(np.pi / 6), np.sin(np.pi / 6), (np.asarray((d, h, w)) - 1) / 2
    turn = np.array([[cs, 0, sn], [0, 1, 0], [-sn, 0, cs]])
    rows += [A.row_of([[1, 0.25, -0.5], [0.5, 1, 0], [0, 0.25, 1]], (0.25, 0, -0.5)), A.row_of(turn, cen - turn @ cen, a=0.75)]
    rows += list(A.draw(8, A.ALL, (d, h, w), 0.8, seed=d * 100 + w, offset=5, max_scale=2.0, max_angle=np.pi,
                        max_shift=(0.25 * d, 0.25 * h, 0.25 * w), max_brightness=0.5, max_contrast=2.0))
    while len(rows) % n:
        rows.append(rows[len(rows) % 7 + 1])
    return [np.stack(rows[i:i + n]) for i in range(0, len(rows), n)]


SHAPES = [(3, 2, 8, 8, 1),      # c = 1, one piece per row in bf16
          (2, 1, 6, 6, 3),      # D = 1; rows of 18 elements: the scalar path with its short last piece
          (2, 3, 4, 4, 32),     # pieces within one voxel's channels: corners and hits read as 16-byte pieces
          (3, 4, 64, 64, 1),    # several blocks, two trips of the grid-stride loop
          (2, 2, 4, 8, 1)]      # h != w


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_apply_is_bit_exact_forward_and_adjoint(shape, dtype):
    from saragan_amd import functional as F
    out = (lambda a: A.bf16_round(a)) if dtype == torch.bfloat16 else (lambda a: a)
    x = _data(shape, seed=shape[3])
    xd = _to_dev(x, dtype)
    for rows in _case_rows(shape):
        prm = _rows(rows)
        y = _to_np(F.augment_affine(xd, prm, fill=FILL))
        assert np.array_equal(_bits(y), _bits(out(A.forward(x, rows, FILL)))), rows
        ya = _to_np(F.augment_affine(xd, prm, fill=FILL, adjoint=True))      # the adjoint reads fill and bias as 0
        assert np.array_equal(_bits(ya), _bits(out(A.adjoint(x, rows)))), rows
    gone = np.stack([A.shift_row((0, 0, shape[3]))] * shape[0])
    assert (_to_np(F.augment_affine(xd, _rows(gone), fill=FILL)) == FILL).all()
    assert (_to_np(F.augment_affine(xd, _rows(gone), fill=FILL, adjoint=True)) == 0.0).all()
    # identity rows reproduce the input's bits, -0.0 included, in both directions
    ident = _rows(np.stack([A.IDENTITY] * shape[0]))
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(F.augment_affine(xd, ident, fill=FILL).view(iv), xd.view(iv))
    assert torch.equal(F.augment_affine(xd, ident, adjoint=True).view(iv), xd.view(iv))
    # the quarter turns equal the blitting kernel's, device against device
    if shape[2] == shape[3]:
        for k in (1, 2, 3):
            blit = torch.as_tensor(np.asarray([R.params_of(k=k)] * shape[0], np.int32)).cuda()
            turn = _rows(np.stack([A.quarter_turn_row(k, shape[2])] * shape[0]))
            assert torch.equal(F.augment_affine(xd, turn, fill=FILL).view(iv), F.augment(xd, blit, fill=FILL).view(iv))
            assert torch.equal(F.augment_affine(xd, turn, adjoint=True).view(iv), F.augment(xd, blit, adjoint=True).view(iv))


def test_parameters_outside_the_contract_stay_in_bounds():
    """Rows no draw produces -- singular, NaN, Inf, huge entries -- still give the restatement's forward bit for bit (its
    support test is the kernel's) and an adjoint that returns: nothing is asserted about the adjoint's values."""
    from saragan_amd import functional as F
    shape = (4, 2, 8, 8, 1)
    x = _data(shape, 3)
    xd = _to_dev(x)
    rows = np.stack([A.row_of(np.zeros((3, 3)), (0.5, 3.25, 2)), A.row_of(off=(np.nan, 0, 0)), A.row_of(np.eye(3) * 1e30),
                     A.row_of([[1, 0, 0], [0, np.inf, 0], [0, 0, 1]])])
    with np.errstate(all='ignore'):
        want = A.forward(x, rows, FILL)
    assert np.array_equal(_bits(_to_np(F.augment_affine(xd, _rows(rows), fill=FILL))), _bits(want))
    assert F.augment_affine(xd, _rows(rows), adjoint=True).shape == xd.shape
    torch.cuda.synchronize()


DYADIC = lambda d, h, w: [A.shift_row((0.25, -0.5, 0.75)), A.scale_row(0.5, (d, h, w)), A.scale_row(2.0, (d, h, w)),
                          A.quarter_turn_row(1, h), A.shear_row(0.25), A.shift_row((-0.75, 1.25, 2.0), a=0.5),
                          A.quarter_turn_row(3, h), A.shear_row(-0.25)]


def test_adjoint_identity_exact_on_dyadic_rows():
    """<A x, y> == <x, A^T y> exactly: dyadic matrices, integers in [-8, 8], the sums taken in float64 on the host."""
    from saragan_amd import functional as F
    shape = (4, 3, 8, 8, 2)
    rng = np.random.default_rng(3)
    x, y = (rng.integers(-8, 9, shape).astype(np.float32) for _ in range(2))
    xd, yd = _to_dev(x), _to_dev(y)
    rows = DYADIC(*shape[1:4])
    for i in range(0, 8, 4):
        prm = _rows(np.stack(rows[i:i + 4]))
        ax = _to_np(F.augment_affine(xd, prm, fill=0.0)).astype(np.float64)
        aty = _to_np(F.augment_affine(yd, prm, adjoint=True)).astype(np.float64)
        assert (ax * y).sum() == (x * aty).sum()


def test_adjoint_identity_within_the_rounding_bound_on_drawn_rows():
    """Rows from the draw, normal data: |<A x, y> - <x, A^T y>| <= (K + 2) 2^-24 sum |terms|.  Both sides evaluate the same
    bilinear form sum_v sum_k W_k(v) x[u_k(v)] y[v] with the same float32 weights; a side rounds each product once and each
    partial sum once, and K is the largest number of summands of any output of either pass (counted by the restatement).  The
    inner products themselves are taken in float64 on the host."""
    from saragan_amd import functional as F
    shape = (4, 3, 8, 8, 2)
    n, d, h, w, c = shape
    x, y = _data(shape, 5), _data(shape, 6)
    xd, yd = _to_dev(x), _to_dev(y)
    for trial in range(3):
        rows = A.draw(n, A.SCALE | A.ROTATE | A.SHIFT | A.CONTRAST, (d, h, w), 0.9, seed=trial, offset=trial, max_scale=2.0,
                      max_shift=(0.5, 1.0, 1.0), max_contrast=2.0)
        K = A.summands(rows, (d, h, w))
        terms = 0.0
        for i in range(n):
            sup, W, tgt, inr = A.geometry(rows[i], d, h, w)
            use = sup[:, None] & inr & (W != 0)
            xa = np.abs(x[i].reshape(-1, c).astype(np.float64))[tgt]                      # [V, 8, c]
            terms += (np.where(use, np.abs(W.astype(np.float64)), 0.0)[:, :, None] * xa *
                      np.abs(y[i].reshape(-1, 1, c).astype(np.float64))).sum()
        prm = _rows(rows)
        ax = _to_np(F.augment_affine(xd, prm, fill=0.0)).astype(np.float64)
        aty = _to_np(F.augment_affine(yd, prm, adjoint=True)).astype(np.float64)
        diff = abs((ax * y).sum() - (x * aty).sum())
        print(f'trial {trial}: K = {K}, |difference| = {diff:.3e}, bound = {(K + 2) * 2.0 ** -24 * terms:.3e}, '
              f'of sum |terms| = {diff / terms:.2e}')
        assert diff <= (K + 2) * 2.0 ** -24 * terms


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_autograd_first_and_second_order(dtype):
    from saragan_amd import functional as F
    shape = (4, 2, 6, 6, 2)
    rng = np.random.default_rng(9)
    x, y, v = (rng.integers(-4, 5, shape).astype(np.float32) for _ in range(3))      # (small integers: exact in both formats)
    rows = np.stack([A.shift_row((0.5, -0.5, 1.0)), A.scale_row(2.0, shape[1:4]), A.quarter_turn_row(1, 6),
                     A.shift_row((0, 0.5, 0), a=0.5, b=-0.25)])
    prm = _rows(rows)
    rnd = A.bf16_round if dtype == torch.bfloat16 else (lambda a: a)      # (each result below is one kernel's: rounded once)
    xd, yd, vd = _to_dev(x, dtype).requires_grad_(True), _to_dev(y, dtype).requires_grad_(True), _to_dev(v, dtype)
    out = F.augment_affine(xd, prm, fill=FILL)
    assert np.array_equal(_to_np(out), rnd(A.forward(x, rows, FILL)))
    (g,) = torch.autograd.grad((out * yd).sum(), xd, create_graph=True)
    assert np.array_equal(_to_np(g), rnd(A.adjoint(y, rows)))
    # g = A^T y: its derivative with respect to y, contracted with v, is the linear part of the forward (no fill, no bias)
    (gg,) = torch.autograd.grad((g * vd).sum(), yd, create_graph=True)
    assert np.array_equal(_to_np(gg), rnd(A.forward(v, rows, FILL, linear=True)))
    # and once more: the derivative of that with respect to v's slot is the adjoint again
    wd = _to_dev(x, dtype).requires_grad_(True)
    fw = F.augment_affine(wd, prm, fill=FILL, adjoint=True)
    (ga,) = torch.autograd.grad((fw * yd.detach()).sum(), wd)
    assert np.array_equal(_to_np(ga), rnd(A.forward(y, rows, FILL, linear=True)))


def _ulps(a, b):
    ia, ib = (np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return np.abs(ia - ib)


DRAW_KW = dict(max_scale=2.0, max_angle=np.pi, max_shift=(0.5, 2.0, 3.25), max_brightness=0.2, max_contrast=1.5)


@pytest.mark.parametrize('ops', [A.ALL, A.SCALE | A.BRIGHTNESS, A.ROTATE | A.SHIFT | A.CONTRAST], ids=['all', 'scale_brightness', 'rot_shift_contrast'])
def test_draw_equals_the_reference(ops):
    """Gates and identity components exactly; every other entry within 1 f32 ulp (the device's and numpy's exp2 / sincos agree
    to a few float64 ulps, which round to the same or to neighbouring floats)."""
    from saragan_amd import functional as F
    ext = (4, 16, 24)
    ident = A.IDENTITY
    for n, p, offset, seed in ((1, 0.5, 0, 1234), (5, 0.0, 7, 1234), (4096, 0.3, (1 << 40) + 3, 1234), (4096, 1.0, 0, (7 << 32) + 9),
                               (300, 0.8, 11, 99)):
        got = F.augment_affine_draw(n, ops, ext, p, seed, offset=offset, **DRAW_KW).cpu().numpy()
        want, gates = A.draw(n, ops, ext, p, seed, offset, return_gates=True, **DRAW_KW)
        assert got.dtype == np.float32 and got.shape == (n, 16)
        assert _ulps(got, want).max() <= 1, (n, p, offset)
        lin_off = ~gates[:, :2].any(1)                       # neither scale nor rotation: the linear part is the identity's bits
        assert np.array_equal(_bits(got[lin_off][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]), np.tile(_bits(ident[[0, 1, 2, 4, 5, 6, 8, 9, 10]]), (lin_off.sum(), 1)))
        geo_off = ~gates[:, :3].any(1)
        assert np.array_equal(_bits(got[geo_off][:, :12]), np.tile(_bits(ident[:12]), (geo_off.sum(), 1)))
        assert np.array_equal(_bits(got[~gates[:, 3], 13]), _bits(np.zeros((~gates[:, 3]).sum())))
        assert np.array_equal(_bits(got[~gates[:, 4], 12]), _bits(np.ones((~gates[:, 4]).sum())))
        assert np.array_equal(_bits(got[:, [1, 2, 4, 8, 14, 15]]), np.zeros((n, 6), np.uint32))
        # the gates themselves: a gated-on value differs from the identity component (up to the rare exact hit)
        assert ((got[:, 13] != 0) <= gates[:, 3]).all() and ((got[:, 12] != 1) <= gates[:, 4]).all()
        assert ((got[:, 0] != 1) <= gates[:, 0]).all() and ((got[:, 6] != 0) <= gates[:, 1]).all()
        if p == 1.0:
            assert (got[:, 13] != 0).mean() > 0.99 if ops & A.BRIGHTNESS else not got[:, 13].any()


def test_draw_device_offset_and_device_probability():
    from saragan_amd import functional as F
    ext, seed = (2, 8, 8), 99
    for offset in (0, (5 << 40) + 11):
        ctr = torch.tensor([offset], dtype=torch.int64, device='cuda')
        a = F.augment_affine_draw(300, A.ALL, ext, 0.6, seed, offset=ctr, **DRAW_KW)
        assert torch.equal(a, F.augment_affine_draw(300, A.ALL, ext, 0.6, seed, offset=offset, **DRAW_KW))
        assert int(ctr) == offset + (1 << 40)
        b = F.augment_affine_draw(300, A.ALL, ext, 0.6, seed, offset=ctr, bump=0, **DRAW_KW)      # bump 0: the counter stays
        assert int(ctr) == offset + (1 << 40)
        assert torch.equal(b, F.augment_affine_draw(300, A.ALL, ext, 0.6, seed, offset=offset + (1 << 40), **DRAW_KW))
        c = F.augment_affine_draw(300, A.ALL, ext, 0.6, seed, offset=ctr, bump=3, **DRAW_KW)
        assert int(ctr) == offset + (1 << 40) + 3 and torch.equal(b, c)
    for p in (0.0, 0.3, 0.8, 1.0):
        pd = torch.tensor([p], dtype=torch.float32, device='cuda')
        assert torch.equal(F.augment_affine_draw(500, A.ALL, ext, pd, seed, offset=4, **DRAW_KW),
                           F.augment_affine_draw(500, A.ALL, ext, p, seed, offset=4, **DRAW_KW))


def test_refusals():
    from saragan_amd import _lib, functional as F
    x = _to_dev(_data((2, 2, 4, 8, 1), 0))
    prm = _rows(np.stack([A.IDENTITY] * 2))
    lib = _lib.load()
    p = x.data_ptr()
    assert lib.sg_augment_affine_apply(p, p, prm.data_ptr(), 2, 2, 4, 8, 1, 0.0, 0, _lib.SG_F32, None) == -1      # in place
    y = torch.empty_like(x)
    assert lib.sg_augment_affine_apply(p, y.data_ptr(), prm.data_ptr(), 2, 2, 4, 8, 1, 0.0, 4, _lib.SG_F32, None) == -1      # flags
    assert lib.sg_augment_affine_apply(p, y.data_ptr(), prm.data_ptr(), 2, 2, 4, 8, 1, 0.0, 0, 7, None) == -1               # dtype
    with pytest.raises(TypeError, match='float32 and bfloat16'):
        F.augment_affine(x.half(), prm)
    with pytest.raises(ValueError):
        F.augment_affine(x, prm[:1])
    with pytest.raises(ValueError):
        F.augment_affine(x, prm[:, :8].contiguous())
    with pytest.raises(ValueError):
        F.augment_affine(x, prm.double())
    with pytest.raises(ValueError):
        F.augment_affine(x[0], prm)
    with pytest.raises(RuntimeError, match='GPU only'):
        F.augment_affine(x.cpu(), prm)
    ok = dict(max_scale=1.25, max_angle=1.0, max_shift=(1.0, 1.0, 1.0), max_brightness=0.2, max_contrast=1.5)
    for bad in (dict(max_scale=0.5), dict(max_scale=2.5), dict(max_angle=3.2), dict(max_angle=-0.1), dict(max_shift=(0, -1.0, 0)),
                dict(max_brightness=-0.1), dict(max_contrast=0.9), dict(max_contrast=4.5), dict(max_scale=float('nan'))):
        with pytest.raises(_lib.SgError, match='code -1'):
            F.augment_affine_draw(4, A.ALL, (2, 4, 4), 0.5, 1, **{**ok, **bad})
    for ops in (1, 31, 1024, A.ALL | 1):      # blitting bits and unknown bits are not this entry point's
        with pytest.raises(_lib.SgError, match='code -1'):
            F.augment_affine_draw(4, ops, (2, 4, 4), 0.5, 1, **ok)


# ---- the smallest networks: the affine pass inside the loss functions ------------------------------------------------------------
WGAN_P2, LOGISTIC_P3, WGAN_P3 = 'oracle_step_p2_wgan_a060.npz', 'oracle_step_p3_logistic_a025.npz', 'oracle_step_p3_wgan_a000.npz'
STEP_FILL = 0.25


def _step(golden_dir, name, fetch, rnd_extra=None, ops=0, rng_cls=None):
    """One evaluation of the step graph of fixture `name` with injected randomness (as tests/test_augment_gpu.py's).  ops: the
    augmentation mask, 0: augmentation off."""
    import saragan_amd.optimization as opt
    from saragan_amd.networks import loss as L
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
    fx = load_step_fixture(os.path.join(golden_dir, name), torch.float64)
    set_compute_dtype(torch.float32)
    store = VariableStore('cuda', seed=0)
    tensors = {k: v.float() for k, v in fx['rnd'].items()}
    tensors.update(rnd_extra or {})
    L.set_random_source((rng_cls or L.InjectedRandom)(tensors))
    prev = L.set_augment(L.AugmentConfig('fixed', ops=ops, fill=STEP_FILL, p=1.0) if ops else None)
    try:
        alpha = ScalarVariable(fx['alpha'], 'alpha')
        og = opt.AdamOptimizer(ScalarVariable(1e-3, 'g_lr'), 0.0, 0.9)
        od = opt.AdamOptimizer(ScalarVariable(1e-3, 'd_lr'), 0.0, 0.9)
        ph = opt.Placeholder([4, 1, 1, 1, 1])
        freeze = None if fx['freeze'] is None else list(fx['freeze'])
        with use_store(store):
            tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, alpha, fx['phase'], BASE_SHAPE, KERNEL_SPEC,
                                    FILTER_SPEC, 'leaky_relu', 0.2, fx['loss_fn'], fx['cfg']['gp_weight'], 'simultaneous', False,
                                    False, 0.01, freeze)
        store.load_state_dict(dict(fx['p0']), strict=True)
        mixing = freeze is not None
        handles = dict(gen_loss=tup[2], disc_loss=tup[3], gp_loss=tup[4], g_grads=tup[13] if mixing else tup[6],
                       d_grads=tup[17] if mixing else tup[8])
        res = opt.Session('cuda').run([handles[k] for k in fetch], feed_dict={ph: fx['real'].float()})
        out = []
        for r in res:
            out.append([g.detach().clone() for g in r] if isinstance(r, (list, tuple)) else r.detach().clone())
        return out
    finally:
        L.set_augment(prev)
        L.set_random_source(None)


@pytest.mark.parametrize('name', [WGAN_P2, LOGISTIC_P3])
@pytest.mark.parametrize('ops', [A.ALL, A.ALL | R.FLIP_W | R.TRANSLATE], ids=['affine', 'blit_and_affine'])
def test_identity_rows_reproduce_the_unaugmented_step_bit_for_bit(golden_dir, name, ops):
    """The new bits set, identity rows (InjectedRandom without aug_* keys): both batches pass through the resampling kernel,
    G's gradient through its adjoint; losses and every gradient keep their bits (reproducible mode: no float atomics)."""
    import saragan_amd
    fetch = ['gen_loss', 'disc_loss', 'gp_loss', 'g_grads', 'd_grads']
    saragan_amd.set_deterministic(True)
    try:
        gl0, dl0, gp0, gg0, dg0 = _step(golden_dir, name, fetch)
        gl1, dl1, gp1, gg1, dg1 = _step(golden_dir, name, fetch, ops=ops)
    finally:
        saragan_amd.set_deterministic(False)
    assert torch.equal(gl0, gl1) and torch.equal(dl0, dl1) and torch.equal(gp0, gp1)
    assert len(gg0) == len(gg1) > 0 and len(dg0) == len(dg1) > 0
    bad = [i for i, (a, b) in enumerate(zip(gg0 + dg0, gg1 + dg1)) if not torch.equal(a, b)]
    assert not bad, bad


@pytest.mark.parametrize('name', [WGAN_P2, LOGISTIC_P3])
def test_step_with_dyadic_rows_equals_the_step_fed_host_transformed_batches(golden_dir, name):
    """D-side quantities with dyadic rows against the UNAUGMENTED step whose noisy real and noisy generated batches are
    transformed on the host by affref.forward (a random source whose add_noise does it).  The restatement gives the device's
    bits, so D sees the same input in both runs and the three losses are equal exactly; D's weight gradients come out of
    backward passes whose first layer differs in whether it owes a data gradient to the generator, so they are held to the
    project's fp32 gradient tolerance (as tests/test_augment_gpu.py: rtol 1e-3, atol 1e-4 of the largest reference element).
    G's gradient passes through the adjoint in the augmented run; it has no counterpart in the host-fed one and is checked for
    being finite and for differing from the unaugmented step's."""
    import saragan_amd
    from saragan_amd.networks import loss as L
    fx0 = load_step_fixture(os.path.join(golden_dir, name), torch.float64)
    n, _, d, h, w = tuple(fx0['real'].shape)
    dy = DYADIC(d, h, w)
    extra = {'aug_real_affine': torch.from_numpy(np.stack([dy[i] for i in (0, 2, 3, 5)][:n])),
             'aug_fake_affine': torch.from_numpy(np.stack([dy[i] for i in (1, 4, 6, 0)][:n]))}

    class HostAugmented(L.InjectedRandom):
        def add_noise(self, x, stddev, tag):
            y = super().add_noise(x, stddev, tag)
            rows = self.t['aug_real_affine' if tag == 'noise_real' else 'aug_fake_affine'].numpy()
            return _to_dev(A.forward(_to_np(y), rows, STEP_FILL), y.dtype)

    fetch = ['gen_loss', 'disc_loss', 'gp_loss', 'd_grads']
    saragan_amd.set_deterministic(True)
    try:
        gl, dl, gp, dg, gg = _step(golden_dir, name, fetch + ['g_grads'], rnd_extra=extra, ops=A.ALL)
        gl_r, dl_r, gp_r, dg_r = _step(golden_dir, name, fetch, rnd_extra=extra, rng_cls=HostAugmented)
        gl_0, dl_0, _, _, gg_0 = _step(golden_dir, name, fetch + ['g_grads'])
    finally:
        saragan_amd.set_deterministic(False)
    print('losses', float(gl), float(gl_r), float(dl), float(dl_r), 'unaugmented', float(gl_0), float(dl_0))
    assert float(gl) != float(gl_0) and float(dl) != float(dl_0)      # the rows did something
    assert torch.equal(gl, gl_r) and torch.equal(dl, dl_r) and torch.equal(gp, gp_r)
    for a, b in zip(dg, dg_r):
        r = b.double().cpu().numpy()
        np.testing.assert_allclose(a.double().cpu().numpy(), r, rtol=1e-3, atol=1e-4 * np.abs(r).max() + 1e-9)
    assert all(torch.isfinite(g).all() for g in gg)
    assert any(not torch.allclose(a, b, rtol=1e-2, atol=1e-6) for a, b in zip(gg, gg_0))


def _run_steps(golden_dir, steps, captured, ops):
    import saragan_amd.optimization as opt
    from saragan_amd.ExtendedEMA import ExtendedEMA
    from saragan_amd.networks import loss as L
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
    fx = load_step_fixture(os.path.join(golden_dir, WGAN_P3), torch.float64)
    os.environ['SARAGAN_HIPGRAPH'] = '1' if captured else '0'
    set_compute_dtype(torch.float32)
    cfg = L.AugmentConfig('fixed', ops=ops, max_shift=0.25, fill=STEP_FILL, p=0.5, max_scale=1.5, max_angle=90.0)
    prev = L.set_augment(cfg)
    try:
        store = VariableStore('cuda', seed=0)
        L.set_random_source(L.RandomSource(1234, 'cuda'))
        og = opt.AdamOptimizer(ScalarVariable(1e-3, 'g_lr'), 0.0, 0.9)
        od = opt.AdamOptimizer(ScalarVariable(1e-3, 'd_lr'), 0.0, 0.9)
        ph = opt.Placeholder([4, 1, 1, 1, 1])
        with use_store(store):
            tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, ScalarVariable(0.0, 'alpha'), fx['phase'], BASE_SHAPE,
                                    KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, 'wgan', fx['cfg']['gp_weight'], 'simultaneous',
                                    False, False, 0.01, None)
        store.load_state_dict(dict(fx['p0']), strict=True)
        ema = ExtendedEMA(list(store.vars.keys()), 0.99, graph=tup[0].graph)
        ema_op = ema.apply()
        sess = opt.Session('cuda')
        g = torch.Generator().manual_seed(5)
        reals = [(fx['real'].float() + 0.1 * torch.randn(fx['real'].shape, generator=g)).cuda() for _ in range(steps)]
        losses = []
        for real in reals:
            res = sess.run([tup[0], tup[1], tup[2], tup[3]], feed_dict={ph: real})
            sess.run(ema_op)
            losses.append((float(res[2]), float(res[3])))
        ncap = sum(1 for e in tup[0].graph.__dict__.get('_captures', {}).values() if 'graph' in e)
        state = {k: v.detach().clone() for k, v in store.vars.items()}
        return state, losses, ncap, L._rng('cuda').aug_calls
    finally:
        os.environ['SARAGAN_HIPGRAPH'] = '0'
        L.set_augment(prev)
        L.set_random_source(None)


@pytest.mark.parametrize('ops', [A.ALL, A.ALL | R.FLIP_W | R.TRANSLATE], ids=['affine', 'blit_and_affine'])
def test_captured_step_with_the_affine_pass_equals_eager(golden_dir, ops):
    """Four steps (two eager warm-up steps, the capture, a replay) against four eager steps from the same seed, reproducible
    mode, scale,rotate,shift,brightness,contrast at a fixed p: the draws read a device counter that the last draw of a call
    advances, once per call with and without blitting transforms next to the affine ones."""
    import saragan_amd
    saragan_amd.set_deterministic(True)
    try:
        w0, l0, n0, c0 = _run_steps(golden_dir, 4, False, ops)
        w1, l1, n1, c1 = _run_steps(golden_dir, 4, True, ops)
        w2, l2, _, _ = _run_steps(golden_dir, 4, False, 0)
    finally:
        saragan_amd.set_deterministic(False)
    assert (n0, n1) == (0, 1)
    assert c0 == c1 == 8               # two calls per step, counted on the host in both runs
    assert l0 == l1, (l0, l1)
    bad = [k for k in w0 if not torch.equal(w0[k], w1[k])]
    assert not bad, bad
    assert l0 != l2                    # fresh draws did something


# ---- the training loop ------------------------------------------------------------------------------------------------------
def _train_args(data, logdir, extra):
    from saragan_amd.main import build_parser, finalize_args
    argv = ['pgan', str(data) + '/', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 4, 16, 16)',
            '--starting_phase', '1', '--ending_phase', '2', '--base_batch_size', '4', '--latent_dim', '16',
            '--noise_stddev', '0.01', '--mixing_nimg', '16', '--stabilizing_nimg', '16', '--loss_fn', 'logistic',
            '--gp_weight', '10', '--data_mean', '1024', '--data_stddev', '1024', '--logdir', str(logdir),
            '--g_lr', '1e-3', '--d_lr', '1e-3', '--checkpoint_every_nsteps', '1000000', '--dtype', 'f32',
            '--max_steps_per_phase', '8'] + extra
    args = build_parser().parse_args(argv)
    args.kernel_spec = [[[1, 3, 3], [1, 3, 3]], [[1, 3, 3], [3, 3, 3]], [[3, 3, 3], [3, 3, 3]]]
    args.filter_spec = [[16, 16], [16, 8], [8, 8]]
    return finalize_args(args)


def _make_data(root):
    for z, xy in ((1, 4), (2, 8), (4, 16)):
        d = root / f'{xy}x{xy}'
        d.mkdir(parents=True)
        for i in range(12):
            v = np.clip(np.random.default_rng(1234 + i).normal(1024, 512, (z, xy, xy)), 0, 4095).astype(np.int16)
            np.save(d / f'{i:04d}.npy', v)


def test_training_loop_with_the_affine_transforms(tmp_path, capsys):
    """--augment ada --augment_ops flip_w,scale,rotate,brightness through run_training: the run finishes with finite weights
    and reports augment_p per phase."""
    from saragan_amd.train import run_training
    data = tmp_path / 'data'
    _make_data(data)
    args = _train_args(data, tmp_path / 'log', ['--augment', 'ada', '--augment_p', '0.5', '--ada_interval', '2', '--ada_kimg', '0.1',
                                                '--augment_ops', 'flip_w,scale,rotate,brightness'])
    out = run_training(args, max_steps_per_phase=args.max_steps_per_phase)
    st = out['stats']
    assert (st[1]['steps'], st[2]['steps']) == (8, 8)
    for ph in (1, 2):
        assert 0.0 <= st[ph]['augment_p'] <= float(np.float32(args.ada_p_max))      # (p is an f32 on the device)
        assert np.isfinite(st[ph]['d_loss']) and np.isfinite(st[ph]['g_loss'])
    assert all(torch.isfinite(v).all() for v in out['store'].vars.values())
    assert 'Augmentation probability:' in capsys.readouterr().out


def test_training_loop_without_the_new_names_is_what_it_was(tmp_path, monkeypatch):
    """A run with blitting transforms only ends with the same weights, bit for bit, as the same run with the random sources'
    augment methods put back to what they were before the affine family existed (one draw and one apply with the whole
    mask)."""
    import saragan_amd
    from saragan_amd import functional as F
    from saragan_amd.networks import loss as L
    from saragan_amd.train import run_training
    data = tmp_path / 'data'
    _make_data(data)
    extra = ['--augment', 'fixed', '--augment_p', '0.5', '--augment_ops', 'flip_w,flip_h,rot90,translate']

    def eager_before(self, x, tag):
        cfg = L._AUGMENT['cfg']
        self.aug_calls += 1
        params = F.augment_draw(x.shape[0], cfg.ops, cfg.max_shifts(x), cfg.p, self.seed, offset=self.aug_calls << 40, device=x.device)
        return F.augment(x, params, cfg.fill, cfg.ops)

    def static_before(self, x, tag):
        cfg = L._AUGMENT['cfg']
        if self.counting:
            self.aug_calls += 1
        params = F.augment_draw(x.shape[0], cfg.ops, cfg.max_shifts(x), cfg.p, self.base.seed, offset=self.aug_counter, device=x.device)
        return F.augment(x, params, cfg.fill, cfg.ops)

    saragan_amd.set_deterministic(True)
    try:
        now = run_training(_train_args(data, tmp_path / 'log0', extra), max_steps_per_phase=8)
        monkeypatch.setattr(L.RandomSource, 'augment', eager_before)
        monkeypatch.setattr(L.StaticRandom, 'augment', static_before)
        before = run_training(_train_args(data, tmp_path / 'log1', extra), max_steps_per_phase=8)
    finally:
        saragan_amd.set_deterministic(False)
    a, b = now['store'].vars, before['store'].vars
    assert set(a) == set(b)
    assert all(torch.equal(a[k].detach(), b[k].detach()) for k in a)
