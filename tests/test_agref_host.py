"""tests/agref.py checked on the host: on small shapes its staged first- and second-order results are the derivatives fp64
autograd finds for a plain composition of oracle.pgan_oracle ops (the composition test_fused_mask_chain_first_and_second_order
uses as ref_chain), and every case of the GPU table (tests/test_autograd_exact_gpu.py) stays inside the exact range at its full
shape, with representable pair intermediates on a copy cropped in H and W."""
import pytest
import torch

from oracle import pgan_oracle as O
from tests import agref as A
from tests import fwdref as R
from tests import wgref as W

SMALL = (2, 4, 8)


def _var(q):
    """The oracle multiplies a filter by its He constant: the fp64 variable whose effective filter is q (to 1 ulp)."""
    coef = O.runtime_coef(q.shape, 'leaky_relu', A.SLOPE)
    return (q.double() / coef).requires_grad_(True), coef


def _stage(x, wv, b):
    return O.act(O.apply_bias(O.conv3d(x, wv, 'leaky_relu', A.SLOPE), b), 'leaky_relu', A.SLOPE)


def _conv(x, wv):
    return O.conv3d(x, wv, 'leaky_relu', A.SLOPE)


def _off_zero(d, key):
    """The oracle's effective filter is q to one fp64 ulp, so a pre-activation that is exactly zero may come out as -1e-16 there
    and flip its LeakyReLU mask: half-integer biases keep every pre-activation at least 1/2 away from zero in this comparison."""
    d[key] = d[key] + 0.5
    return d


def _close(got, ref, what):
    torch.testing.assert_close(got.detach().double(), ref.double(), rtol=1e-12, atol=1e-9, msg=lambda m: f'{what}: {m}')


@pytest.mark.parametrize('variant', ['alone', 'premask', 'mixed'])
def test_conv_bias_act_reference_is_the_fp64_derivative(variant):
    c = A.Case('host', 'cba', A.BF, 2, 8, 16, SMALL, variant=variant, seed=7)
    d = _off_zero(A.cba_data(c), 'b1')
    ref = A.cba_reference(c, d)
    x = d['x'].double().requires_grad_(True)
    w1, c1 = _var(d['q1'])
    b1 = d['b1'].double().requires_grad_(True)
    h = _stage(x, w1, b1)
    _close(h, ref['y'], 'y')
    v = d['v'].double()
    if variant == 'alone':
        gy = d['gy'].double().requires_grad_(True)
        gx, gw1, gb1 = torch.autograd.grad(h, [x, w1, b1], gy, create_graph=True)
        g_gy, g_w1 = torch.autograd.grad((gx * v).sum(), [gy, w1])
    else:
        w2, c2 = _var(d['q2'])
        gy = d['gy'].double().requires_grad_(True)
        outs, gys, ws = [_conv(h, w2)], [gy], [w2]
        if variant == 'mixed':
            w3, c3 = _var(d['q3'])
            gy3 = d['gy3'].double().requires_grad_(True)
            outs.append(_conv(h, w3)), gys.append(gy3), ws.append(w3)
        _close(outs[0], ref['y2'], 'y2')
        gx, gw1, gb1, *gws = torch.autograd.grad(outs, [x, w1, b1] + ws, gys, create_graph=True)
        g_gy, g_w1, *rest = torch.autograd.grad((gx * v).sum(), [gy, w1] + ws + gys[1:])
        _close(gws[0], ref['sw2'] * c2, 'gw2')
        _close(rest[0], ref['s2w2'] * c2, 'second-order gw2')
        if variant == 'mixed':
            _close(gws[1], ref['sw3'] * c3, 'gw3')
            _close(rest[1], ref['s2w3'] * c3, 'second-order gw3')
            _close(rest[2], ref['g_gy3'], 'second-order g_gy3')
    _close(gx, ref['gx'], 'gx')
    _close(gw1, ref['sw1'] * c1, 'gw1')
    _close(gb1, ref['sb1'], 'gb1')
    _close(g_gy, ref['g_gy'], 'second-order g_gy')
    _close(g_w1, ref['s2w1'] * c1, 'second-order gw1')


def test_wgrad_reference_is_the_fp64_derivative():
    c = A.Case('host', 'wgrad', A.BF, 2, 8, 16, SMALL, coef=0.5, seed=8)
    d = A.wgrad_data(c)
    ref = A.wgrad_reference(c, d)
    x = d['x'].double().requires_grad_(True)
    dy = d['dy'].double().requires_grad_(True)
    # dw of conv3d(x, coef * w) for the output gradient dy, as autograd finds it through a dummy filter
    w = torch.zeros_like(d['u']).double().requires_grad_(True)
    coef_o = O.runtime_coef(w.shape, 'leaky_relu', A.SLOPE)
    (dw,) = torch.autograd.grad(_conv(x, w), w, dy, create_graph=True)
    dw = dw / coef_o * c.coef
    _close(dw, ref['sw'] * c.coef, 'dw')
    gx, gdy = torch.autograd.grad((dw * d['u'].double()).sum(), [x, dy])
    _close(gx, ref['gx'], 'gx')
    _close(gdy, ref['gdy'], 'gdy')
    _close(dy.sum((0, 2, 3, 4)), ref['sb'], 'db')


def test_from_rgb_reference_is_the_fp64_derivative():
    c = A.Case('host', 'pw', A.BF, 2, 1, 16, SMALL, seed=9)
    d = _off_zero(A.pw_data(c), 'b1')
    ref = A.pw_reference(c, d)
    x = d['x'].double().requires_grad_(True)
    w1, c1 = _var(d['q1'])
    b1 = d['b1'].double().requires_grad_(True)
    w2, c2 = _var(d['q2'])
    h = _stage(x, w1, b1)
    got = torch.autograd.grad(h, [x, w1, b1], d['gy'].double(), retain_graph=True)
    for a, r, nm in zip(got, (ref['gx'], ref['sw1'] * c1, ref['sb1']), ('gx', 'gw1', 'gb1')):
        _close(a, r, nm)
    y2 = _conv(h, w2)
    _close(y2, ref['y2'], 'y2')
    got = torch.autograd.grad(y2, [x, w1, b1, w2], d['gy2'].double())
    for a, r, nm in zip(got, (ref['pgx'], ref['psw1'] * c1, ref['psb1'], ref['sw2'] * c2), ('gx', 'gw1', 'gb1', 'gw2')):
        _close(a, r, 'pair ' + nm)


@pytest.mark.parametrize('in_mask', [False, True])
def test_pooled_reference_is_the_fp64_derivative(in_mask):
    c = A.Case('host', 'pool', A.BF, 2, 8, 16, (4, 4, 8), density=0.5, seed=11)
    d = _off_zero(A.pool_data(c), 'b')
    ref = A.pool_reference(c, d, in_mask)
    x0 = d['x'].double().requires_grad_(True)
    # a masked input stage: x = leaky_relu(x0) has the derivative M_in for any x0 with the signs of a_in; the layer itself is fed
    # d['x'], so the stage is emulated by multiplying the gradient with M_in -- which is what makes gx = M_in * conv'(...)
    wv, cf = _var(d['q'])
    b = d['b'].double().requires_grad_(True)
    gy = d['gy'].double().requires_grad_(True)
    y = O.downscale3d(_stage(x0, wv, b))
    _close(y, ref['y'], 'y')
    gx, gw, gb = torch.autograd.grad(y, [x0, wv, b], gy, create_graph=True)
    m_in = A.masked(torch.ones_like(gx), ref['in_words'])
    gx = gx * m_in
    _close(gx, ref['gx'], 'gx')
    _close(gw, ref['sw'] * cf, 'gw')
    _close(gb, ref['sb'], 'gb')
    g_gy, g_w = torch.autograd.grad((gx * d['v'].double()).sum(), [gy, wv])
    _close(g_gy, ref['g_gy'], 'second-order g_gy')
    _close(g_w, ref['s2w'] * cf, 'second-order gw')
    # the full-resolution tensor the generic route stores is what g_gy is the block mean of
    _close(R.pool_mean(ref['g_full'], 3), ref['g_gy'], 'g_full')


def test_block_reference_is_the_fp64_derivative():
    c = A.Case('host', 'block', A.BF, 2, 1, 64, (2, 4, 8), seed=13)
    d = A.block_data(c)
    for k in ('b0', 'b1', 'b2'):
        _off_zero(d, k)
    # (half-integer biases: the stored tensors need one more bit than the GPU cases', f32 holds them)
    ref = A.block_reference(A.Case('host', 'block', A.F32, 2, 1, 64, (2, 4, 8), seed=13), d)
    x = d['x'].double().requires_grad_(True)
    ws, cs = zip(*[_var(d[k]) for k in ('q0', 'q1', 'q2')])
    bs = [d[k].double().requires_grad_(True) for k in ('b0', 'b1', 'b2')]
    gy = d['gy'].double().requires_grad_(True)
    h = x
    for wv, b in zip(ws, bs):
        h = _stage(h, wv, b)
    y = O.downscale3d(h)
    _close(y, ref['y'], 'y')
    g1 = torch.autograd.grad(y, [x, *ws, *bs], gy, create_graph=True)
    _close(g1[0], ref['gx'], 'gx')
    for i in range(3):
        _close(g1[1 + i], ref[f'sw{i}'] * cs[i], f'gw{i}')
        _close(g1[4 + i], ref[f'sb{i}'], f'gb{i}')
    g2 = torch.autograd.grad((g1[0] * d['v'].double()).sum(), [gy, *ws])
    _close(g2[0], ref['g_gy'], 'second-order g_gy')
    for i in range(3):
        _close(g2[1 + i], ref[f's2w{i}'] * cs[i], f'second-order gw{i}')


def test_sparse_filters_and_q_over_coef():
    w = A.both_sparse_filter(A.K333, 32, 64, 4)
    assert bool((w.abs().sum((0, 1, 2, 4)) == A.NNZ).all()) and bool((w.abs().sum((0, 1, 2, 3)) == A.NNZ // 2).all())
    for per, dim in (('in', (0, 1, 2, 4)), ('out', (0, 1, 2, 3))):
        w = A.sparse_filter(A.K333, 32, 64, 5, per)
        assert w.shape == (3, 3, 3, 32, 64) and w.is_contiguous()
        assert bool((w.abs().sum(dim) == A.NNZ).all()) and set(w.unique().tolist()) == {-1.0, 0.0, 1.0}
    q = A.dense_filter(A.K333, 32, 64, 6)
    for coef in (A.HE_32, 1.3859292911256331, 0.043):
        A.q_over_coef(q, coef, A.BF)
    assert torch.equal(A.q_over_coef(q, 0.25, A.F32), q)
    with pytest.raises(AssertionError):
        A.q_over_coef(q, 0.3, A.F32)
    x = A.ints((2, 8, 4, 4, 8), 3, A.BF, 0.25)
    frac = float((x != 0).float().mean())
    assert 0.1 < frac < 0.3, frac


def test_range_assertions_fail_when_the_bound_fails():
    x = torch.full((1, 1, 64, 512, 512), 3.0)
    with pytest.raises(AssertionError):
        A.assert_wgrad_range(x, x)
    with pytest.raises(AssertionError):
        A.stored(torch.tensor([257.0], dtype=torch.float64), A.BF)
    A.stored(torch.tensor([256.0, 0.75, 48.0], dtype=torch.float64), A.BF)
    assert A.quantum(torch.tensor([0.75, 2.0], dtype=torch.float64)) == 0.25


@pytest.mark.parametrize('c', A.CASES, ids=repr)
def test_every_gpu_case_is_inside_the_exact_range(c):
    """Small cases: the whole reference on the host (it asserts every bound and every intermediate).  Large ones: the
    weight-gradient bound at the full shape from the data alone (|M| <= 1, so sum |upscale3d(gy)| / 8 bounds the masked
    gradient), and the whole reference on a copy cropped in H and W."""
    if c.kind == 'cba':
        A.cba_reference(c, A.effective(c, A.cba_data(c)))
    elif c.kind == 'wgrad':
        A.wgrad_reference(c, A.wgrad_data(c))
    elif c.kind == 'pw':
        A.pw_reference(c, A.effective(c, A.pw_data(c)))
    elif c.kind == 'pool':
        gy = A.pool_data(c, keys=('gy',))['gy']
        col = float(W.up2(gy.double().abs()).sum((0, 2, 3, 4)).max()) * 0.125
        # x and v are integers in [-3, 3] (agref.ints), v behind a masked input stage a multiple of 1/4; the masked gradient is a
        # multiple of 1/32: units of 1/128
        assert 3.0 * col * 128 < W.LIMIT, f'max|x| * max_co sum_v |dy| in units of 1/128 = {3.0 * col * 128:.3g} passes 2^24'
        dc = A.pool_data(c, crop=(c.sp[0], 8, 32))
        for in_mask in (False, True):
            A.pool_reference(c, dc, in_mask)
    elif c.kind == 'poolfwd':
        d = A.poolfwd_data(c, crop=(c.sp[0], 8, 32))
        A.poolfwd_reference(c, d)
    elif c.kind == 'block':
        if c.sp[1] * c.sp[2] <= 1024:
            A.block_reference(c, A.block_data(c))
        else:
            d = A.block_data(c)
            # |M| <= 1 and |q| <= 1 with NNZ entries per channel: per channel sum_v |gh1| <= NNZ * max_co sum_v |upscale3d(gy)| / 8 and
            # sum_v |gh0| <= NNZ times that again -- bounded here from gy alone; all three sums are in units of 1/512
            g2 = W.up2(d['gy'].double().abs()) * 0.125
            col2 = float(g2.sum((0, 2, 3, 4)).max())
            unit = 1.0 / 512
            for what, mx, col in (('conv_2', 51.0, col2), ('conv_1', 12.0, A.NNZ * col2), ('from_rgb', 3.0, A.NNZ * A.NNZ * col2)):
                assert mx * col / unit < W.LIMIT, (what, mx * col / unit)
            del g2
            A.block_reference(c, A.block_data(c, crop=(c.sp[0], 8, 32)))
    else:
        raise AssertionError(c.kind)
