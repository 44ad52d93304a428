"""CPU tests of the affine discriminator augmentation's numpy restatement (tests/affref.py) and of its command-line flags.
The restatement is what the device results are compared against bit for bit (tests/test_augment_affine_gpu.py), so its own
properties are checked here: against an independent float64 matrix form on data where every float32 operation is exact,
against the pixel-blitting reference where the two families overlap, and the draw's gates and ranges."""
import numpy as np
import pytest

from tests import affref as A
from tests import augref as R

D, H, W = 2, 4, 4
DYADIC = ([A.shift_row(t) for t in ((0.25, 0, 0), (0, -0.25, 0), (0, 0, 0.75), (-0.5, 1.25, -2.0), (0, 3.0, 0), (0, 0, -4.0))] +
          [A.scale_row(0.5, (D, H, W)), A.scale_row(2.0, (D, H, W))] + [A.quarter_turn_row(k, H) for k in (1, 2, 3)] +
          [A.shear_row(0.25), A.shear_row(-0.25), A.shift_row((0.25, 0.5, -0.25), a=1.5, b=-0.25), A.row_of(a=0.5, b=2.0)])


def _ints(seed, shape):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float32)


@pytest.mark.parametrize('i', range(len(DYADIC)))
def test_restatement_equals_the_float64_dense_form_on_dyadic_rows(i):
    """Dyadic matrix entries and integers in [-8, 8]: every float32 product and sum is exact, so the float32 restatement and
    the float64 matrix form give the same numbers, forward (fill and bias included) and adjoint."""
    row = DYADIC[i]
    x, g = _ints(i, (D, H, W, 2)), _ints(100 + i, (D, H, W, 2))
    M, f = A.dense(row, D, H, W)
    want = M @ x.reshape(-1, 2).astype(np.float64) + f[:, None] * -1.0 + float(row[13])
    assert np.array_equal(A.forward_one(x, row, -1.0).reshape(-1, 2).astype(np.float64), want)
    want_lin = M @ x.reshape(-1, 2).astype(np.float64)
    assert np.array_equal(A.forward_one(x, row, -1.0, linear=True).reshape(-1, 2).astype(np.float64), want_lin)
    assert np.array_equal(A.adjoint_one(g, row).reshape(-1, 2).astype(np.float64), M.T @ g.reshape(-1, 2).astype(np.float64))
    # <A x, y> == <x, A^T y> exactly
    lhs = (A.forward_one(x, row, 0.0, linear=True).astype(np.float64) * g).sum()
    assert lhs == (x.astype(np.float64) * A.adjoint_one(g, row)).sum()


def test_adjoint_order_is_ascending_v_from_the_first_term():
    """The ordered scatter against a literal gather loop in float32 on rows from the draw and non-dyadic data: for each input
    voxel the terms of the output voxels that reach it, in ascending linear order, the first term starting the sum."""
    d, h, w = 2, 5, 5
    rows = A.draw(3, A.ALL, (d, h, w), 0.9, seed=5, offset=2, max_scale=2.0, max_shift=(0.5, 1.0, 1.0))
    g = np.random.default_rng(0).normal(0, 1, (3, d, h, w, 1)).astype(np.float32)
    for i in range(3):
        sup, Wt, tgt, inr = A.geometry(rows[i], d, h, w)
        want = np.zeros(d * h * w, np.float32)
        seen = np.zeros(d * h * w, bool)
        for v in range(d * h * w):
            for k in range(8):
                if sup[v] and inr[v, k] and Wt[v, k] != 0:
                    t = np.float32(Wt[v, k] * g[i].reshape(-1)[v])
                    want[tgt[v, k]] = np.float32(want[tgt[v, k]] + t) if seen[tgt[v, k]] else t
                    seen[tgt[v, k]] = True
        assert np.array_equal(A.adjoint_one(g[i], rows[i]).reshape(-1).view(np.uint32), want.view(np.uint32))
        # one output voxel reaches an input voxel through at most one corner
        for v in range(d * h * w):
            hit = tgt[v][sup[v] & inr[v] & (Wt[v] != 0)]
            assert len(set(hit.tolist())) == len(hit)


def test_identity_rows_return_the_inputs_bits():
    x = np.random.default_rng(1).normal(0, 3, (2, 3, 4, 5, 2)).astype(np.float32)
    x[0, 0, 0, 0, 0], x[1, 2, 3, 4, 1], x[0, 1, 1, 1, 1] = -0.0, 0.0, np.float32(1e-30)
    rows = np.stack([A.IDENTITY, A.IDENTITY])
    for y in (A.forward(x, rows, fill=-1.0), A.adjoint(x, rows)):
        assert np.array_equal(y.view(np.uint32), x.view(np.uint32))
    xb = A.bf16_round(x)
    assert np.array_equal(A.bf16_round(A.forward(xb, rows, -1.0)).view(np.uint32), xb.view(np.uint32))
    # gain and bias on an identity matrix: one product, one sum
    y = A.forward(x, np.stack([A.row_of(a=1.5, b=-0.25)] * 2), 7.0)
    assert np.array_equal(y, np.float32(1.5) * x + np.float32(-0.25))


def test_bf16_rounding_is_to_nearest_even():
    v = np.array([1.0, 1.00390625, 1.01171875, 1.005, -1.00390625, 0.0, -0.0], np.float32)      # two ties, one above a tie
    want = np.array([1.0, 1.0, 1.015625, 1.0078125, -1.0, 0.0, -0.0], np.float32)
    assert np.array_equal(A.bf16_round(v).view(np.uint32), want.view(np.uint32))


def test_quarter_turns_and_integer_shifts_equal_the_blitting_reference():
    x = np.random.default_rng(2).normal(0, 1, (1, 2, 6, 6, 3)).astype(np.float32)
    for k in (1, 2, 3):
        row = A.quarter_turn_row(k, 6)
        assert set(np.unique(row[:3])) <= {0.0, 1.0} and set(np.unique(np.abs(row[:12]))) <= {0.0, 1.0, 5.0}
        want = R.apply(x, [R.params_of(k=k)], -1.0)
        assert np.array_equal(A.forward(x, row[None], -1.0), want)
        assert np.array_equal(A.adjoint(x, row[None]), R.apply(x, [R.params_of(k=k)], 0.0, adjoint=True))
    for t in ((1, 0, 0), (-1, 2, -3), (0, 5, 0), (0, 0, 6), (2, 0, 0), (0, -6, 1)):
        row = A.shift_row(t)
        assert np.array_equal(A.forward(x, row[None], -1.0)[0], R.shift(x[0], t, np.float32(-1.0))), t
        assert np.array_equal(A.adjoint(x, row[None])[0], R.shift(x[0], [-s for s in t], 0)), t
    # a shift far outside: nothing but fill forward, nothing but zeros in the adjoint; NaN and Inf coordinates are out of support
    for row in (A.shift_row((0, 0, 2.0 ** 20)), A.row_of(off=(np.nan, 0, 0)), A.row_of(off=(0, np.inf, 0))):
        assert (A.forward(x, row[None], -1.0) == -1.0).all() and (A.adjoint(x, row[None]) == 0.0).all()


def test_draw_reference():
    ext, ms = (8, 32, 32), (1.0, 4.0, 4.0)
    kw = dict(max_scale=2.0, max_angle=np.pi / 2, max_shift=ms, max_brightness=0.2, max_contrast=1.5)
    n = 4096
    ident = np.tile(A.IDENTITY, (n, 1))
    r0, g0 = A.draw(n, A.ALL, ext, 0.0, 7, 0, return_gates=True, **kw)
    assert not g0.any() and np.array_equal(r0.view(np.uint32), ident.view(np.uint32))      # the identity's BITS (no -0.0)
    r1, g1 = A.draw(n, A.ALL, ext, 1.0, 7, 0, return_gates=True, **kw)
    assert g1.all() and not r1[:, 14:].any() and not r1[:, [1, 2, 4, 8]].any()
    s = 1.0 / r1[:, 0].astype(np.float64)
    assert 0.5 <= s.min() < 0.52 and 1.9 < s.max() <= 2.0
    theta = np.arctan2(r1[:, 6].astype(np.float64), r1[:, 5].astype(np.float64))
    assert -np.pi / 2 - 1e-6 <= theta.min() < -1.5 and 1.5 < theta.max() <= np.pi / 2 + 1e-6
    assert np.allclose(r1[:, 9], -r1[:, 6]) and np.array_equal(r1[:, 10], r1[:, 5])
    assert np.allclose(np.hypot(r1[:, 5], r1[:, 6]), r1[:, 0], rtol=1e-6)            # the rotation block is (1/s) R
    assert np.abs(r1[:, 13]).max() <= np.float32(0.2) and np.abs(r1[:, 13]).max() > 0.19
    assert np.float32(1 / 1.5) <= r1[:, 12].min() < 0.68 and 1.48 < r1[:, 12].max() <= np.float32(1.5)
    # shift alone: u = v - t, |t_a| <= max_shift_a and nearly reached
    rs = A.draw(n, A.SHIFT, ext, 1.0, 7, 0, **kw)
    assert np.array_equal(rs[:, [0, 5, 10]], np.ones((n, 3), np.float32)) and not rs[:, [1, 2, 4, 6, 8, 9]].any()
    for ax in range(3):
        t = -rs[:, 4 * ax + 3]
        assert np.abs(t).max() <= ms[ax] and np.abs(t).max() > 0.98 * ms[ax]
    assert np.array_equal(rs[:, 12:], ident[:, 12:])
    # disabled transforms yield identity components whatever p is
    rb = A.draw(n, A.BRIGHTNESS | A.CONTRAST, ext, 1.0, 7, 0, **kw)
    assert np.array_equal(rb[:, :12].view(np.uint32), ident[:, :12].view(np.uint32)) and rb[:, 13].any() and (rb[:, 12] != 1).any()
    rg = A.draw(n, A.SCALE | A.ROTATE | A.SHIFT, ext, 1.0, 7, 0, **kw)
    assert np.array_equal(rg[:, 12:].view(np.uint32), ident[:, 12:].view(np.uint32))
    # gate frequencies at p = 0.5: within 6 standard deviations of N p; rows with no geometric gate are the identity matrix
    rh, gh = A.draw(n, A.ALL, ext, 0.5, 7, 0, return_gates=True, **kw)
    bound = 6.0 * np.sqrt(n * 0.25)
    for j in range(5):
        assert abs(int(gh[:, j].sum()) - n * 0.5) <= bound, j
    off = ~gh[:, :3].any(1)
    assert off.sum() > n // 16 and np.array_equal(rh[off, :12].view(np.uint32), ident[off, :12].view(np.uint32))
    assert np.array_equal(rh[~gh[:, 3], 13], np.zeros((~gh[:, 3]).sum(), np.float32))
    assert np.array_equal(rh[~gh[:, 4], 12], np.ones((~gh[:, 4]).sum(), np.float32))
    # its own stream: the key differs from the blitting draw's; sample i at offset o is sample 0 at offset o + i
    a = A.draw(8, A.ALL, ext, 0.7, 11, (1 << 40) + 5, **kw)
    assert np.array_equal(a[3], A.draw(1, A.ALL, ext, 0.7, 11, (1 << 40) + 8, **kw)[0])
    assert not np.array_equal(a, A.draw(8, A.ALL, ext, 0.7, 11, 5, **kw))
    assert A.KEY != R.KEY
    # the centre of the volume is the fixed point of scale and rotation
    c = (np.asarray(ext) - 1) / 2
    rr = A.draw(64, A.SCALE | A.ROTATE, ext, 1.0, 3, 0, **kw).astype(np.float64)
    for row in rr:
        m = row[:12].reshape(3, 4)
        assert np.allclose(m[:, :3] @ c + m[:, 3], c, atol=1e-4)


BASE = ['pgan', '/data/', '--start_shape', '(1, 5, 16, 16)', '--final_shape', '(1, 20, 32, 64)', '--starting_phase', '1',
        '--ending_phase', '2', '--latent_dim', '16', '--noise_stddev', '0.01', '--network_size', 'xs']


def _parse(extra):
    from saragan_amd.main import build_parser, finalize_args
    return finalize_args(build_parser().parse_args(BASE + extra))


def test_cli_defaults_and_new_names():
    a = _parse([])
    assert a.augment == 'none' and a.augment_ops == 'flip_w,translate'
    assert (a.augment_max_scale, a.augment_max_angle, a.augment_max_brightness, a.augment_max_contrast) == (1.25, 180.0, 0.2, 1.5)
    # the new names are accepted, and rotate has no square-plane requirement (the final plane here is 32 x 64)
    a = _parse(['--augment', 'fixed', '--augment_p', '0.5', '--augment_ops', 'flip_w,scale,rotate,shift,brightness,contrast',
                '--augment_max_scale', '2', '--augment_max_angle', '30', '--augment_max_brightness', '0.5',
                '--augment_max_contrast', '4'])
    assert a.augment_ops == 'flip_w,scale,rotate,shift,brightness,contrast'
    assert (a.augment_max_scale, a.augment_max_angle, a.augment_max_brightness, a.augment_max_contrast) == (2.0, 30.0, 0.5, 4.0)


@pytest.mark.parametrize('extra, match', [
    (['--augment_max_scale', '0.5'], 'augment_max_scale'),
    (['--augment_max_scale', '3'], 'augment_max_scale'),
    (['--augment_max_angle', '200'], 'augment_max_angle'),
    (['--augment_max_angle', '-1'], 'augment_max_angle'),
    (['--augment_max_brightness', '-0.1'], 'augment_max_brightness'),
    (['--augment_max_contrast', '0.9'], 'augment_max_contrast'),
    (['--augment_max_contrast', '5'], 'augment_max_contrast'),
    (['--augment_ops', 'scale,shear'], 'unknown transform'),
])
def test_cli_refusals(extra, match):
    with pytest.raises(SystemExit, match=match):
        _parse(['--augment', 'fixed'] + extra)


def test_augment_config_from_the_flags():
    from saragan_amd import functional as F
    from saragan_amd.train import augment_config
    cfg = augment_config(_parse(['--augment', 'fixed', '--augment_p', '0.5']), 'cpu')
    assert cfg.ops == R.FLIP_W | R.TRANSLATE and cfg.ops & ~31 == 0            # the old defaults select no affine transform
    assert (cfg.max_scale, cfg.max_angle, cfg.max_brightness, cfg.max_contrast) == (1.25, 180.0, 0.2, 1.5)
    cfg = augment_config(_parse(['--augment', 'fixed', '--augment_ops', 'translate,scale,contrast', '--augment_max_scale', '1.5',
                                 '--augment_max_contrast', '2']), 'cpu')
    assert cfg.ops == R.TRANSLATE | A.SCALE | A.CONTRAST and (cfg.max_scale, cfg.max_contrast) == (1.5, 2.0)
    assert F.augment_ops_mask('flip_w,scale,rotate,shift,brightness,contrast') == 1 | A.ALL
    assert F.AUGF_ALL == A.ALL and F.AUG_ALL == R.ALL
    with pytest.raises(ValueError):
        F.augment_ops_mask('shear')
    assert augment_config(_parse([]), 'cpu') is None
