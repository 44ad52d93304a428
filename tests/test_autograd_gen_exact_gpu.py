"""The generator's autograd routes (saragan_amd/functional.py and the decisions of saragan_amd/networks/ops.py that feed them) pinned
node by node.  tests/gref.py says why there are two tiers and derives every bound; tests/test_gref_host.py shows on the host that
its restatements are the derivatives they claim, that the cases keep their conditions and that the bounds reject wrong kernels.

Tier 1 (torch.equal against the exact value rounded once; integer data as in tests/agref.py):
  test_upsampled_convolution_node     _Conv(ups) and _ConvBiasAct(ups, no pixel_norm): forward through _raw_upconv_subpixel and, under
                                      _NO_SUBPIXEL, the gather kernel; gw / gb through the sub-pixel weight gradient and through
                                      _wgrad_launch with upsample_in; gx through every branch of _upconv_dgrad -- the sub-pixel data
                                      gradient, raw_conv(pool=1) / (pool=2) + _Down(4.0, _POOL_REST[mode]) (mode 1 also where _pool_mode says 3), the generic
                                      _Conv + _Down(1.0) (odd W, f32, _NO_SUBPIXEL, and create_graph=True)
  test_mixing_branch                  lerp(upscale3d(to_rgb(x)), to_rgb(x2), alpha): _ConvBiasAct 1x1x1 to one channel + bias, _Up, _Axpby;
                                      backward _Axpby (twice), _Down(1.0), the pointwise filter / bias gradient with one output channel,
                                      the flipped pointwise data gradient
  test_dense_head                     dense (2-D w) + bias + LeakyReLU reshaped into a 3x3x3 convolution: _ConvBiasAct on [N, F]
Tier 2 (derived bounds on the node's own stored tensors; every route of a test meets ONE reference):
  test_stage_alone                    conv3d(act, pixel_norm) [ups]: _ConvBiasAct.backward's _PnActBwd branch -> _conv_dgrad /
                                      _conv_param_grads; under _NO_SIGN_WORDS its _PixelNormBwd + _BiasActBwd(y) branch
  test_stage_with_a_conv_consumer     ActInfo.pn + pn_bwd_epilogue_available: _dgrad_into's raw_conv(pn_bwd=...) (the producer skips its
                                      pass -- the `fused_pn_act and _masked_in` branch -- and takes gb from the weight-gradient
                                      launch), the same graph under _NO_PN_EPILOGUE, and with the launch declined (_dgrad_into's fallback)
  test_stage_with_to_rgb              _ConvPnActToRgb, only img used: forward with the rgb epilogue / under _NO_RGB_FWD_EPILOGUE / ups (no
                                      epilogue); backward sg_pixel_norm_act_bwd_pw_wg / _pw + separate filter gradient
                                      (_NO_RGB_WG_FUSION, and when the fused launch declines) / the tensor route (_NO_RGB_FUSION);
  test_stage_with_to_rgb_whose_image_is_unused   only g_y present
  test_stage_with_to_rgb_and_a_second_consumer   g_img and g_y both present (the `gy + g_y` branch), at the functional level and through
                                      networks.ops in both orders: rgb first -- _LazyRgbTail.value's one-node branch, the conv reads the
                                      node's second output; conv first -- ops.conv3d's pn_ok sign-up is outvoted by to_rgb's ordinary
                                      _consume (_LazyRgbTail.value's other branch), nobody skips the stage's own backward
  test_wide_stage_through_ops         128 channels > PN_FUSE_MAX_CHANNELS: ops.pixel_norm's unfused branch, _ConvBiasAct(act) + _PixelNorm
  test_gradient_destinations          the conv-consumer and the to_rgb graph inside functional.grads_into (_GradOuts / _f32_out): every
                                      .grad is its slot, bit-identical to the run without, also under _NO_GRAD_DEST
  test_generator_through_ops          generator_in -> generator_block -> to_rgb with the fade-in branch at phase 2, alpha 0 (lerp prunes
                                      the old to_rgb: never launched) and 1/2: every pixel-norm backward and every parameter gradient
                                      checked on the tensors that node read
Second order through these nodes is refused: tests/test_autograd_exact_gpu.py::test_second_order_through_pixel_norm_is_refused."""
import contextlib
import functools
import inspect

import numpy as np
import pytest
import torch

from tests import agref as A
from tests import fwdref as R
from tests import gref as G
from tests import wgref as W
from tests.test_autograd_exact_gpu import Spy, _F, dev, eq, eq_b, eq_w, eq_words, leaf, on_dev, var

pytestmark = pytest.mark.gpu

BF, F32, SLOPE, K333, K111 = G.BF, G.F32, G.SLOPE, G.K333, G.K111


class Tap:
    """Wraps functional.<name>: keeps for every call its bound arguments (tensors included) and its result."""

    def __init__(self, monkeypatch, name):
        F = _F()
        real, self.calls = getattr(F, name), []
        sig = inspect.signature(real)

        def wrapper(*a, **k):
            r = real(*a, **k)
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            self.calls.append((dict(ba.arguments), r))
            return r
        monkeypatch.setattr(F, name, wrapper)

    def clear(self):
        del self.calls[:]


class ApplyTap:
    """Stands in for the autograd Function functional.<name>: .apply forwards to the real one and keeps (arguments, result)."""

    def __init__(self, monkeypatch, name):
        F = _F()
        real, calls = getattr(F, name), []
        self.calls = calls

        class Proxy:
            @staticmethod
            def apply(*a):
                r = real.apply(*a)
                calls.append((a, r))
                return r
        monkeypatch.setattr(F, name, Proxy)

    def clear(self):
        del self.calls[:]


class LibSpy:
    """Counts the calls of one entry point of the library (the return codes)."""

    def __init__(self, monkeypatch, name):
        from saragan_amd import _lib
        lib = _lib.load()
        real, self.codes = getattr(lib, name), []

        def wrapper(*a):
            rc = real(*a)
            self.codes.append(rc)
            return rc
        monkeypatch.setattr(lib, name, wrapper)


def _dz_of(taps, w):
    """The gradient _conv_param_grads was handed for the filter w: the dz of that node, as stored."""
    hits = [c[0]['g'] for c in taps.calls if c[0]['w'].data_ptr() == w.data_ptr()]
    assert len(hits) == 1, f'expected one _conv_param_grads call for the filter, got {len(hits)}'
    return hits[0].detach()


def _check_behind(c, d, q1, dz, gx, gw, gb, gb_form, dz_ref=None, t=None, coef=None, x=None):
    """gx, gw, gb of a stage against the fp64 sums over its captured dz (gb_form 'stored'), or for gb the restated dz
    ('register': summed by the pixel-norm backward pass before the bf16 store)."""
    coef = c.coef if coef is None else coef
    b = G.behind_dz(d['x'] if x is None else x, q1, dz, ups=c.ups)
    if gx is not None:
        assert gx.dtype == BF
        G.check(gx, b['gx'], b['gx_bound'], 'gx')
    G.check_w(gw, b['sw'], b['sw_abs'], b['k'], coef, 'gw')
    if gb_form == 'register':
        G.check_gb_in_register(gb, dz_ref, t, c.c, 'gb (summed in the pixel-norm backward pass)')
    else:
        assert gb is not None and gb.dtype == F32
        G.check(gb, b['sb'], G.sum_bound(b['sb_abs'], b['k']), 'gb (summed over the stored dz)')


def _check_stage_forward(c, d, y, scale, signs):
    a, _, _, words = G.stage_forward(d['x'].double(), d['q1'].double(), d['b1'].double(), ups=c.ups)
    assert y.dtype == BF
    G.pn_check(c.id, y.detach(), scale, a, BF, c.c)
    if signs is not None:
        eq_words(signs, words, 'sign words')
    return words


def _stage_vars(c, dc, d):
    return var(dc['q1'], c.coef, BF), d['b1'].clone().requires_grad_(True)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2, 1: one stage alone
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['fused', 'two_pass'])
@pytest.mark.parametrize('c', [G.S32, G.S_UPS], ids=repr)
def test_stage_alone(c, route, monkeypatch):
    F = _F()
    dc = G.stage_data(c)
    G.stage_conditions(c, dc)
    d = on_dev(dc)
    monkeypatch.setattr(F, '_NO_SIGN_WORDS', route == 'two_pass')
    w1, b1 = _stage_vars(c, dc, d)
    convs, params = Tap(monkeypatch, 'raw_conv'), Tap(monkeypatch, '_conv_param_grads')
    pnact, pnbwd, masks = ApplyTap(monkeypatch, '_PnActBwd'), ApplyTap(monkeypatch, '_PixelNormBwd'), Spy(monkeypatch, 'raw_bias_act_bwd')
    x = leaf(d['x'])
    y = F.conv3d(x, w1, c.coef, bias=b1, act=True, slope=SLOPE, pixel_norm=True, upsample_in=c.ups)
    _, scale, signs = convs.calls[-1][1]
    assert (signs is None) == (route == 'two_pass')
    words = _check_stage_forward(c, d, y, scale, signs)
    gx, gw, gb = torch.autograd.grad(y, [x, w1, b1], d['gy'])
    if route == 'fused':
        assert (len(pnact.calls), len(pnbwd.calls), masks.calls) == (1, 0, []), 'expected the one-pass _PnActBwd'
    else:
        assert (len(pnact.calls), len(pnbwd.calls)) == (0, 1) and masks.args('want_db') == [True], 'expected _PixelNormBwd + _BiasActBwd'
    dz = _dz_of(params, w1)
    dz_ref, t = G.check_dz(dz, d['gy'], y.detach(), scale, words, 'pass', 'dz')
    _check_behind(c, d, d['q1'], dz, gx, gw, gb, 'register' if route == 'fused' else 'stored', dz_ref, t)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2, 2: a stage and the conv that signs up for its backward
# ---------------------------------------------------------------------------------------------------------------------------
def _conv_consumer_graph(c, d, vs, k2):
    """stage -> conv3d + bias, wired as ops.conv3d / ops._consume wire it: (x, h, y2, info, pn_ok)."""
    F = _F()
    w1, b1, w2, b2 = vs
    x = leaf(d['x'])
    info = F.ActInfo(SLOPE)
    h = F.conv3d(x, w1, c.coef, bias=b1, act=True, slope=SLOPE, pixel_norm=True, out_info=info)
    pn_ok = F.pn_bwd_epilogue_available(tuple(h.shape), K333, c.c, BF)
    info.consume(pn_ok)
    y2 = F.conv3d(h, w2, k2, bias=b2, in_info=info if pn_ok else None)
    return x, h, y2, info, pn_ok


def _decline_pn_bwd(monkeypatch):
    """raw_conv answers a pn_bwd request as the library does for a shape it has no such epilogue for: None, nothing written."""
    F = _F()
    real, declined = F.raw_conv, []

    @functools.wraps(real)
    def conv(*a, **k):
        if k.get('pn_bwd') is not None:
            declined.append(True)
            return None
        return real(*a, **k)
    monkeypatch.setattr(F, 'raw_conv', conv)
    return declined


@pytest.mark.parametrize('route', ['epilogue', 'no_epilogue', 'declined'])
def test_stage_with_a_conv_consumer(route, monkeypatch):
    F = _F()
    c = G.S32
    dc = G.stage_data(c)
    G.stage_conditions(c, dc)
    d = on_dev(dc)
    k2 = 0.043
    monkeypatch.setattr(F, '_NO_PN_EPILOGUE', route == 'no_epilogue')
    declined = _decline_pn_bwd(monkeypatch) if route == 'declined' else []
    w1, b1 = _stage_vars(c, dc, d)
    w2, b2 = var(dc['q2'], k2, BF), d['b2'].clone().requires_grad_(True)
    convs, params, wgrads = Tap(monkeypatch, 'raw_conv'), Tap(monkeypatch, '_conv_param_grads'), Spy(monkeypatch, 'raw_wgrad')
    pnact = ApplyTap(monkeypatch, '_PnActBwd')
    x, h, y2, info, pn_ok = _conv_consumer_graph(c, d, (w1, b1, w2, b2), k2)
    assert pn_ok == (route != 'no_epilogue'), 'pn_bwd_epilogue_available at the 32 -> 32, (2, 8, 32) stage'
    _, scale, signs = convs.calls[0][1]
    words = _check_stage_forward(c, d, h, scale, signs)
    assert info.pn is not None and info.pn[1] is scale
    y2_ref, y2_bound = G.conv_of_stored(h.detach(), d['q2'].double(), d['b2'].double())
    G.check(y2, y2_ref, y2_bound, 'y2')
    convs.clear()
    gx, gw1, gb1, gw2, gb2 = torch.autograd.grad(y2, [x, w1, b1, w2, b2], d['gy2'])
    epi = [r is not None for a, r in convs.calls if a['pn_bwd'] is not None]
    stage_db = [a['want_db'] for a, r in wgrads.calls if a['k'] == K333 and a['w_ptr'] == w1.data_ptr()]
    if route == 'epilogue':
        assert epi == [True] and len(pnact.calls) == 0, 'the consumer\'s data gradient did not run the stage\'s backward in its epilogue'
    elif route == 'declined':
        assert declined == [True] and len(pnact.calls) == 1 and pnact.calls[0][0][5] is False, 'expected the fallback inside _dgrad_into'
    else:
        assert epi == [] and len(pnact.calls) == 1 and pnact.calls[0][0][5] is True, 'expected the stage\'s own _PnActBwd'
    assert stage_db == [route != 'no_epilogue'], 'a producer that skips its pass takes gb from the weight-gradient launch'
    # the consumer: integer gy2, stored h
    sw2, sb2 = W.wgrad_ref(h.detach(), d['gy2'], K333)
    sw2_abs, _ = W.wgrad_ref(h.detach().abs(), d['gy2'].abs(), K333)
    G.check_w(gw2, sw2, sw2_abs, c.n * c.sp[0] * c.sp[1] * c.sp[2], k2, 'gw2')
    eq_b(gb2, sb2, 'gb2')
    # the stage: g is the consumer's exact integer data gradient, in registers or stored
    g = A.stored(R.dgrad_ref(d['gy2'].double(), d['q2'].double()), BF)
    dz = _dz_of(params, w1)
    dz_ref, t = G.check_dz(dz, g, h.detach(), scale, words, 'epilogue' if route == 'epilogue' else 'pass', 'dz')
    _check_behind(c, d, d['q1'], dz, gx, gw1, gb1, 'register' if route == 'no_epilogue' else 'stored', dz_ref, t)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2, 3: _ConvPnActToRgb with only the image used
# ---------------------------------------------------------------------------------------------------------------------------
def _rgb_vars(dc, d):
    return var(dc['q_rgb'], G.RGB_COEF, BF), d['b_rgb'].clone().requires_grad_(True)


def _check_rgb(c, d, y, img, gw_rgb, gb_rgb):
    """img from the stored y; to_rgb's own filter gradient (a sum over the voxels of y * g_img) and its exact integer bias gradient."""
    q = d['q_rgb'].reshape(-1)
    ref = G.rgb_forward(y.detach(), q, 2.0)
    assert img.dtype == BF
    G.check(img, ref, G.rgb_bound(y.detach(), q, 2.0, ref), 'img')
    g_y, sw, sw_abs, sb = G.rgb_backward(y.detach(), q, d['g_img'])
    G.check_w(gw_rgb, sw, sw_abs, c.n * c.fine[0] * c.fine[1] * c.fine[2], G.RGB_COEF, 'gw_rgb')
    eq_b(gb_rgb, sb, 'gb_rgb')
    return A.stored(g_y, BF)


RGB_ROUTES = [('s32', 'epilogue', 'pw_wg'), ('s32', 'epilogue', 'pw'), ('s32', 'epilogue', 'pw_wg_declined'), ('s32', 'epilogue', 'tensor'),
              ('s32', 'two_launches', 'pw_wg'), ('ups_64to32', 'ups', 'pw_wg')]


def _decline_pw_wg(monkeypatch):
    """sg_pixel_norm_act_bwd_pw_wg answers as it does for a channel count it has no team for: SG_EUNSUPPORTED, nothing written."""
    from saragan_amd import _lib
    declined = []

    def refuse(*a):
        declined.append(True)
        return _lib.SG_EUNSUPPORTED
    monkeypatch.setattr(_lib.load(), 'sg_pixel_norm_act_bwd_pw_wg', refuse)
    return declined


@pytest.mark.parametrize('cid,fwd,bwd', RGB_ROUTES, ids=['_'.join(r) for r in RGB_ROUTES])
def test_stage_with_to_rgb(cid, fwd, bwd, monkeypatch):
    F = _F()
    c = {s.id: s for s in G.STAGES}[cid]
    dc = G.stage_data(c)
    G.stage_conditions(c, dc)
    d = on_dev(dc)
    monkeypatch.setattr(F, '_NO_RGB_FWD_EPILOGUE', fwd == 'two_launches')
    monkeypatch.setattr(F, '_NO_RGB_WG_FUSION', bwd == 'pw')
    monkeypatch.setattr(F, '_NO_RGB_FUSION', bwd == 'tensor')
    w1, b1 = _stage_vars(c, dc, d)
    w_rgb, b_rgb = _rgb_vars(dc, d)
    convs, params = Tap(monkeypatch, 'raw_conv'), Tap(monkeypatch, '_conv_param_grads')
    pnact = ApplyTap(monkeypatch, '_PnActBwd')
    refused = _decline_pw_wg(monkeypatch) if bwd == 'pw_wg_declined' else []
    pw_wg, pw = LibSpy(monkeypatch, 'sg_pixel_norm_act_bwd_pw_wg'), LibSpy(monkeypatch, 'sg_pixel_norm_act_bwd_pw')
    x = leaf(d['x'])
    img, y = F.conv3d_pn_to_rgb(x, w1, c.coef, b1, c.ups, SLOPE, G.EPS, None, w_rgb, G.RGB_COEF, b_rgb)
    with_rgb = [r is not None for a, r in convs.calls if a['rgb'] is not None]
    if fwd == 'epilogue':
        assert with_rgb == [True] and len(convs.calls) == 1, 'to_rgb did not ride in the stage\'s epilogue'
    else:
        assert with_rgb == [] and len(convs.calls) == 2, 'expected the stage and to_rgb as two launches'
    _, scale, signs = convs.calls[0][1][:3]
    words = _check_stage_forward(c, d, y, scale, signs)
    gx, gw1, gb1, gw_rgb, gb_rgb = torch.autograd.grad(img, [x, w1, b1, w_rgb, b_rgb], d['g_img'])
    took = (pw_wg.codes, pw.codes, len(pnact.calls))
    unsupported = F._lib.SG_EUNSUPPORTED
    assert took == {'pw_wg': ([0], [], 0), 'pw': ([], [0], 0), 'pw_wg_declined': ([unsupported], [0], 0), 'tensor': ([], [], 1)}[bwd], took
    assert refused == ([True] if bwd == 'pw_wg_declined' else [])
    g = _check_rgb(c, d, y, img, gw_rgb, gb_rgb)
    dz = _dz_of(params, w1)
    dz_ref, t = G.check_dz(dz, g, y.detach(), scale, words, 'pass', 'dz')
    _check_behind(c, d, d['q1'], dz, gx, gw1, gb1, 'register', dz_ref, t)


def test_stage_with_to_rgb_whose_image_is_unused(monkeypatch):
    """Only y of the node reaches the loss (g_img is None): no gradient for to_rgb's parameters, the stage's own _PnActBwd on g_y."""
    F = _F()
    c = G.S32
    dc = G.stage_data(c)
    d = on_dev(dc)
    w1, b1 = _stage_vars(c, dc, d)
    w_rgb, b_rgb = _rgb_vars(dc, d)
    convs, params, pnact = Tap(monkeypatch, 'raw_conv'), Tap(monkeypatch, '_conv_param_grads'), ApplyTap(monkeypatch, '_PnActBwd')
    x = leaf(d['x'])
    img, y = F.conv3d_pn_to_rgb(x, w1, c.coef, b1, False, SLOPE, G.EPS, None, w_rgb, G.RGB_COEF, b_rgb)
    _, scale, signs = convs.calls[0][1][:3]
    words = _check_stage_forward(c, d, y, scale, signs)
    gx, gw1, gb1, gw_rgb, gb_rgb = torch.autograd.grad(y, [x, w1, b1, w_rgb, b_rgb], d['gy'], allow_unused=True)
    assert gw_rgb is None and gb_rgb is None and len(pnact.calls) == 1
    dz = _dz_of(params, w1)
    dz_ref, t = G.check_dz(dz, d['gy'], y.detach(), scale, words, 'pass', 'dz')
    _check_behind(c, d, d['q1'], dz, gx, gw1, gb1, 'register', dz_ref, t)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2, 4: the same node with y consumed as well
# ---------------------------------------------------------------------------------------------------------------------------
def _ops_coefs():
    from saragan_amd.networks import ops
    return {'c1': float(ops.calculate_gain('leaky_relu', SLOPE) / np.sqrt(27 * 32)), 'c2': float(1.0 / np.sqrt(27 * 32)), 'rgb': float(1.0 / np.sqrt(32))}


@contextlib.contextmanager
def _bf16_store():
    from saragan_amd import varstore
    store = varstore.VariableStore(dev())
    old = varstore.compute_dtype()
    varstore.set_compute_dtype(BF)
    try:
        with varstore.use_store(store):
            yield store
    finally:
        varstore.set_compute_dtype(old)


@pytest.mark.parametrize('how', ['functional', 'ops_rgb_first', 'ops_conv_first'])
def test_stage_with_to_rgb_and_a_second_consumer(how, monkeypatch):
    F = _F()
    c = G.S32
    dc = G.stage_data(c)
    G.stage_conditions(c, dc)
    d = on_dev(dc)
    params = Tap(monkeypatch, '_conv_param_grads')
    convs = Tap(monkeypatch, 'raw_conv')
    pnact = ApplyTap(monkeypatch, '_PnActBwd')
    pw_wg, pw = LibSpy(monkeypatch, 'sg_pixel_norm_act_bwd_pw_wg'), LibSpy(monkeypatch, 'sg_pixel_norm_act_bwd_pw')
    x = leaf(d['x'])
    if how == 'functional':
        w1, b1 = _stage_vars(c, dc, d)
        w_rgb, b_rgb = _rgb_vars(dc, d)
        k1 = c.coef
        img, y = F.conv3d_pn_to_rgb(x, w1, k1, b1, False, SLOPE, G.EPS, None, w_rgb, G.RGB_COEF, b_rgb)
        scale = convs.calls[0][1][1]
        gx, gw1, gb1, gw_rgb, gb_rgb = torch.autograd.grad([img, y], [x, w1, b1, w_rgb, b_rgb], [d['g_img'], d['gy']])
        g_y = d['gy'].double()
        one_node = True
    else:
        from saragan_amd import varstore
        from saragan_amd.networks import ops
        ks = _ops_coefs()
        k1 = ks['c1']
        state = {'g/c1/weight': A.q_over_coef(dc['q1'], ks['c1'], BF), 'g/c1/bias': dc['b1'], 'g/c2/weight': A.q_over_coef(dc['q2'], ks['c2'], BF),
                 'g/c2/bias': dc['b2'], 'g/rgb/weight': A.q_over_coef(dc['q_rgb'], ks['rgb'], BF), 'g/rgb/bias': dc['b_rgb']}
        assert abs(ks['rgb'] - G.RGB_COEF) < 1e-15

        def net(xin):
            with varstore.variable_scope('g'):
                with varstore.variable_scope('c1'):
                    h1 = ops.pixel_norm(ops.act(ops.apply_bias(ops.conv3d(xin, c.c, K333, 'leaky_relu', SLOPE)), 'leaky_relu', SLOPE))
                if how == 'ops_rgb_first':
                    with varstore.variable_scope('rgb'):
                        im = ops.materialize(ops.to_rgb(h1, 1))
                with varstore.variable_scope('c2'):
                    h2 = ops.materialize(ops.apply_bias(ops.conv3d(h1, c.c, K333, 'linear')))
                if how != 'ops_rgb_first':
                    with varstore.variable_scope('rgb'):
                        im = ops.materialize(ops.to_rgb(h1, 1))
            return h1.value(), h2, im

        with _bf16_store() as store:
            with torch.no_grad():
                net(d['x'])
            store.load_state_dict(state, strict=True)
            w1, b1, w2, b2, w_rgb, b_rgb = (store.vars[k] for k in ('g/c1/weight', 'g/c1/bias', 'g/c2/weight', 'g/c2/bias', 'g/rgb/weight', 'g/rgb/bias'))
            convs.clear(), params.clear(), pnact.clear()
            y, y2, img = net(x)
            stage_call = [r for a, r in convs.calls if a['pixel_norm']]
            assert len(stage_call) == 1
            scale = stage_call[0][1]
            one_node = any(a['rgb'] is not None for a, r in convs.calls)
            assert one_node == (how == 'ops_rgb_first'), 'to_rgb meets the unmaterialised stage only when it comes first'
            convs.clear()
            gx, gw1, gb1, gw_rgb, gb_rgb, gw2, gb2 = torch.autograd.grad([y2, img], [x, w1, b1, w_rgb, b_rgb, w2, b2], [d['gy2'], d['g_img']])
            assert [a for a, r in convs.calls if a['pn_bwd'] is not None] == [], 'a consumer ran the stage\'s backward although it has two consumers'
        y2_ref, y2_bound = G.conv_of_stored(y.detach(), d['q2'].double(), d['b2'].double())
        G.check(y2, y2_ref, y2_bound, 'y2')
        sw2, sb2 = W.wgrad_ref(y.detach(), d['gy2'], K333)
        sw2_abs, _ = W.wgrad_ref(y.detach().abs(), d['gy2'].abs(), K333)
        G.check_w(gw2, sw2, sw2_abs, c.n * c.sp[0] * c.sp[1] * c.sp[2], ks['c2'], 'gw2')
        eq_b(gb2, sb2, 'gb2')
        g_y = A.stored(R.dgrad_ref(d['gy2'].double(), d['q2'].double()), BF)
    assert (pw_wg.codes, pw.codes, len(pnact.calls)) == ([], [], 1), 'two gradients for y: the stage\'s own _PnActBwd on their sum'
    words = _check_stage_forward(c, d, y, scale, None)
    g_rgb = _check_rgb(c, d, y, img, gw_rgb, gb_rgb)
    g = A.stored(g_rgb + g_y, BF)
    if one_node:      # _ConvPnActToRgb.backward formed gy + g_y itself: what _PnActBwd read is that sum, an exact integer tensor
        assert torch.equal(pnact.calls[0][0][0].double(), g), 'gy + g_y'
    dz = _dz_of(params, w1)
    dz_ref, t = G.check_dz(dz, g, y.detach(), scale, words, 'pass', 'dz')
    _check_behind(c, d, d['q1'], dz, gx, gw1, gb1, 'register', dz_ref, t, coef=k1)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2, 5: the wide stage
# ---------------------------------------------------------------------------------------------------------------------------
def test_wide_stage_through_ops(monkeypatch):
    from saragan_amd import varstore
    from saragan_amd.networks import ops
    F = _F()
    c = G.S_WIDE
    assert c.c > F.PN_FUSE_MAX_CHANNELS
    dc = G.stage_data(c)
    G.stage_conditions(c, dc)
    d = on_dev(dc)
    k1 = float(ops.calculate_gain('leaky_relu', SLOPE) / np.sqrt(27 * c.cin))
    params, convs = Tap(monkeypatch, '_conv_param_grads'), Tap(monkeypatch, 'raw_conv')
    pn, pnbwd, pnact = ApplyTap(monkeypatch, '_PixelNorm'), ApplyTap(monkeypatch, '_PixelNormBwd'), ApplyTap(monkeypatch, '_PnActBwd')
    masks = Spy(monkeypatch, 'raw_bias_act_bwd')

    def net(xin):
        with varstore.variable_scope('w'):
            return ops.materialize(ops.pixel_norm(ops.act(ops.apply_bias(ops.conv3d(xin, c.c, K333, 'leaky_relu', SLOPE)), 'leaky_relu', SLOPE)))

    with _bf16_store() as store:
        with torch.no_grad():
            net(d['x'])
        store.load_state_dict({'w/weight': A.q_over_coef(dc['q1'], k1, BF), 'w/bias': dc['b1']}, strict=True)
        w1, b1 = store.vars['w/weight'], store.vars['w/bias']
        convs.clear(), pn.clear()
        x = leaf(d['x'])
        y = net(x)
        assert [a['pixel_norm'] for a, r in convs.calls] == [False] and len(pn.calls) == 1, 'a 128-channel pixel_norm runs as a pass of its own'
        signs = convs.calls[0][1][2]
        gx, gw, gb = torch.autograd.grad(y, [x, w1, b1], d['gy'])
    assert (len(pnbwd.calls), len(pnact.calls)) == (1, 0) and masks.args('want_db') == [True]
    # the conv + bias + LeakyReLU node stores the exact activation rounded once; pixel_norm reads THAT
    pre = R.bias_act(R.conv_ref(d['x'].double(), d['q1'].double()), d['b1'].double())
    a_stored = pn.calls[0][0][0].detach()
    eq(a_stored, R.bias_act(pre, None, SLOPE), BF, 'the stored activation')
    eq_words(signs, R.sign_words(pre), 'sign words')
    g_read, y_read, scale = pnbwd.calls[0][0]
    assert y_read.data_ptr() == y.data_ptr() and torch.equal(g_read, d['gy'])
    G.pn_check(c.id, y.detach(), scale, a_stored.double(), BF, c.c)
    dz = _dz_of(params, w1)
    G.check_dz(dz, d['gy'], y.detach(), scale, R.sign_words(pre), 'pass', 'dz')
    _check_behind(c, d, d['q1'], dz, gx, gw, gb, 'stored', coef=k1)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2, 6: destinations
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', ['conv_consumer', 'to_rgb', 'to_rgb_declined'])
def test_gradient_destinations(graph, monkeypatch):
    """The same backward with and without grads_into, reproducible mode on: every parameter's .grad IS its slot of the flat buffer
    (claimed grows by the number of parameters, nothing is copied), with the bits of the plain run; under _NO_GRAD_DEST the slots stay
    untouched and the bits are the same again.  to_rgb_declined: sg_pixel_norm_act_bwd_pw_wg declines after _GradOuts handed it three
    slots -- they are given back, and the launches that run instead claim them."""
    import saragan_amd
    F = _F()
    if graph == 'to_rgb_declined':
        _decline_pw_wg(monkeypatch)
    c = G.S32_N2
    dc = G.stage_data(c)
    G.stage_conditions(c, dc)
    d = on_dev(dc)
    k2 = 0.043

    def run(dest, no_dest=False):
        monkeypatch.setattr(F, '_NO_GRAD_DEST', no_dest)
        w1, b1 = _stage_vars(c, dc, d)
        if graph == 'conv_consumer':
            ps = [w1, b1, var(dc['q2'], k2, BF), d['b2'].clone().requires_grad_(True)]
        else:
            ps = [w1, b1, *_rgb_vars(dc, d)]
        flat = torch.zeros(sum(p.numel() for p in ps) + 8 * len(ps), device=dev())
        slots, off = {}, 0
        for p in ps:
            slots[p.data_ptr()] = flat[off:off + p.numel()].view(p.shape)
            off += p.numel() + 8
        before = dict(F.GRAD_DEST_STATS)
        with (F.grads_into(slots) if dest else contextlib.nullcontext()):
            if graph == 'conv_consumer':
                x, h, out, info, pn_ok = _conv_consumer_graph(c, d, ps, k2)
                assert pn_ok
                gout = d['gy2']
            else:
                out, _ = F.conv3d_pn_to_rgb(d['x'], ps[0], c.coef, ps[1], False, SLOPE, G.EPS, None, ps[2], G.RGB_COEF, ps[3])
                gout = d['g_img']
            torch.autograd.backward(out, gout, inputs=ps)
        stats = {k: F.GRAD_DEST_STATS[k] - before[k] for k in ('claimed', 'copied')}
        in_slot = [p.grad.data_ptr() == slots[p.data_ptr()].data_ptr() for p in ps]
        return [p.grad.detach().clone() for p in ps], in_slot, stats, flat

    saragan_amd.set_deterministic(True)
    try:
        plain, in_slot, stats, flat = run(False)
        assert not any(in_slot) and stats == {'claimed': 0, 'copied': 0}
        dest, in_slot, stats, flat = run(True)
        assert all(in_slot) and stats == {'claimed': len(plain), 'copied': 0}, (in_slot, stats)
        for i, (a, b) in enumerate(zip(plain, dest)):
            assert torch.equal(a, b), f'parameter {i}: grads_into changed the bits'
        off, in_slot, stats, flat = run(True, no_dest=True)
        assert not any(in_slot) and stats == {'claimed': 0, 'copied': 0} and float(flat.abs().max()) == 0.0
        for i, (a, b) in enumerate(zip(plain, off)):
            assert torch.equal(a, b), f'parameter {i}: _NO_GRAD_DEST changed the bits'
    finally:
        saragan_amd.set_deterministic(False)


# ---------------------------------------------------------------------------------------------------------------------------
# tier 1: the up-sampled convolution node
# ---------------------------------------------------------------------------------------------------------------------------
def _up_variants():
    out = []
    for c in G.UP_CASES:
        big = c.n * c.fine[0] * c.fine[1] * c.fine[2] > 1 << 16
        for act in ((False,) if big else (False, True)):
            out.append((c, act))
    return out


@pytest.mark.parametrize('c,act', _up_variants(), ids=[f'{c.id}_{"cba" if a else "conv"}' for c, a in _up_variants()])
def test_upsampled_convolution_node(c, act, monkeypatch):
    import ctypes as C
    from saragan_amd import _lib
    F = _F()
    dc = G.up_data(c)
    d = on_dev(dc)
    if c.dtype == F32:
        d['q'] = d['q'] * c.coef
    ref = G.up_reference(c, d, act)
    w = var(dc['q'], c.coef, c.dtype)
    b = d['b'].clone().requires_grad_(True)
    low = F._shape(c.n, *c.sp, c.cin, c.cout, K333, False)
    dgrad_ok = bool(_lib.load().sg_upconv3d_subpixel_dgrad_supported(C.byref(low), _lib.SG_BF16)) and c.dtype == BF
    mode = F._pool_mode(torch.empty((c.n, c.cout, *c.fine), dtype=c.dtype, device='meta'), K333, c.cout, c.cin)
    assert (dgrad_ok, mode) == {'subpixel': (True, 0), 'pool1': (False, 1), 'pool2': (False, 2), 'pool3': (False, 3), 'generic': (False, 0)}[c.route], (dgrad_ok, mode)
    subfwd, subdg, launches = Spy(monkeypatch, '_raw_upconv_subpixel'), Spy(monkeypatch, '_upconv_dgrad_subpixel'), Spy(monkeypatch, '_wgrad_launch')
    convs, downs = Tap(monkeypatch, 'raw_conv'), ApplyTap(monkeypatch, '_Down')

    def run(no_subpixel=False, create_graph=False):
        monkeypatch.setattr(F, '_NO_SUBPIXEL', no_subpixel)
        for s in (subfwd, subdg, launches, convs, downs):
            s.clear()
        x = leaf(d['x'])
        y = F.conv3d(x, w, c.coef, bias=b if act else None, act=act, slope=SLOPE, upsample_in=True)
        fwd_sub = subfwd.results()
        eq(y, ref['y'], c.dtype, 'y')
        if act:
            eq_words(convs.calls[0][1][2], ref['words'], 'sign words')
        convs.clear()
        got = torch.autograd.grad(y, [x, w] + ([b] if act else []), d['gy'], create_graph=create_graph)
        eq(got[0], ref['gx'], c.dtype, 'gx')
        eq_w(got[1], ref['sw'], c.coef, 'gw')
        if act:
            eq_b(got[2], ref['sb'], 'gb')
        pools = [(a['pool'], r is not None) for a, r in convs.calls if a['pool']]
        rest = [(a[1], tuple(a[3]) if len(a) > 3 else (2, 2, 2)) for a, r in downs.calls]
        return fwd_sub, subdg.results(), pools, rest, len(launches.calls)

    took = run()
    print(c.id, 'took', took)
    declined = [False] if c.dtype == BF else []      # the sub-pixel data gradient is asked in bf16 only, and has no tile here
    if c.route == 'subpixel' and c.filt == 'dense':
        assert took == ([True], [True], [], [], 0), ('expected the three sub-pixel kernels', took)
    elif c.route == 'subpixel':      # the sub-pixel shape with a sparse filter: the routes behind the switch and behind create_graph
        assert took == ([True], [True], [], [], 0), took
        assert run(no_subpixel=True) == ([], [], [], [(1.0, (2, 2, 2))], 1), 'under _NO_SUBPIXEL: the gather kernels and the generic data gradient'
        assert run(create_graph=True)[1:4] == ([], [], [(1.0, (2, 2, 2))]), 'create_graph: the generic data gradient'
    elif c.route in ('pool1', 'pool2', 'pool3'):
        m = {'pool1': 1, 'pool2': 2, 'pool3': 1}[c.route]      # (the whole mean of mode 3 is no use to a caller that needs the sum: mode 1)
        assert took[1:4] == (declined, [(m, True)], [(4.0, F._POOL_REST[m])]), (f'expected pool mode {m} and the remaining pairs', took)
    else:
        assert took[1:4] == (declined, [], [(1.0, (2, 2, 2))]), ('expected the generic data gradient', took)
    del ref, d
    torch.cuda.empty_cache()


@pytest.mark.parametrize('c', G.MIX_CASES, ids=repr)
def test_mixing_branch(c, monkeypatch):
    F = _F()
    dc = G.mix_data(c)
    d = on_dev(dc)
    ref = G.mix_reference(c, d)
    wa, wb = var(dc['qa'], G.RGB_COEF, BF), var(dc['qb'], G.RGB_COEF, BF)
    ba, bb = d['ba'].clone().requires_grad_(True), d['bb'].clone().requires_grad_(True)
    downs, ups, mixes = ApplyTap(monkeypatch, '_Down'), ApplyTap(monkeypatch, '_Up'), ApplyTap(monkeypatch, '_Axpby')
    wgrads = Spy(monkeypatch, 'raw_wgrad')
    x, x2 = leaf(d['x']), leaf(d['x2'])
    a = F.conv3d(x, wa, G.RGB_COEF, bias=ba)
    b = F.conv3d(x2, wb, G.RGB_COEF, bias=bb)
    y = F.lerp(F.upscale2x(a, 1.0), b, c.alpha, 1.0 - c.alpha)
    eq(a, ref['a'], BF, 'to_rgb(x)')
    eq(b, ref['b'], BF, 'to_rgb(x2)')
    eq(y, ref['y'], BF, 'the mix')
    assert (len(ups.calls), len(mixes.calls)) == (1, 1)
    gx, gx2, gwa, gba, gwb, gbb = torch.autograd.grad(y, [x, x2, wa, ba, wb, bb], d['g'])
    assert len(mixes.calls) == 3 and [(a_[1], tuple(a_[3])) for a_, r in downs.calls] == [(1.0, (2, 2, 2))], 'expected alpha * g, (1 - alpha) * g and one block sum'
    assert sorted(wgrads.args('want_db')) == [True, True] and wgrads.args('k') == [K111, K111]
    eq(gx, ref['gx'], BF, 'gx')
    eq(gx2, ref['gx2'], BF, 'gx2')
    eq_w(gwa, ref['swa'], G.RGB_COEF, 'gw of the old to_rgb')
    eq_b(gba, ref['sba'], 'gb of the old to_rgb')
    eq_w(gwb, ref['swb'], G.RGB_COEF, 'gw of the new to_rgb')
    eq_b(gbb, ref['sbb'], 'gb of the new to_rgb')


def test_dense_head(monkeypatch):
    F = _F()
    c = G.HEAD
    dc = G.head_data(c)
    d = on_dev(dc)
    ref = G.head_reference(c, d)
    k2 = 0.043
    w, b, w2 = var(dc['q'], c.coef, BF), d['b'].clone().requires_grad_(True), var(dc['q2'], k2, BF)
    masks = Spy(monkeypatch, 'raw_bias_act_bwd')
    z = leaf(d['z'])
    info = F.ActInfo(SLOPE)
    h = F.conv3d(z, w, c.coef, bias=b, act=True, slope=SLOPE, out_info=info)
    info.consume(False)      # ops.materialize: a reshape reads it, nobody applies its mask
    assert h.dtype == BF and tuple(h.shape) == (c.n, c.c * 4)
    assert torch.equal(h.detach().double(), ref['h']), 'dense + bias + LeakyReLU'
    y = F.conv3d(h.reshape(c.n, c.c, *c.sp), w2, k2)
    eq(y, ref['y'], BF, 'y')
    gz, gw, gb, gw2 = torch.autograd.grad(y, [z, w, b, w2], d['gy'])
    assert masks.args('want_db') == [True], 'the head\'s own mask pass sums its bias gradient'
    assert gz.dtype == BF and torch.equal(gz.double(), R.expected(ref['gz'], BF).double()), 'gradient for the latents'
    eq_w(gw, ref['sw'], c.coef, 'gw')
    eq_b(gb, ref['sb'], 'gb')
    eq_w(gw2, ref['sw2'], k2, 'gw2')


# ---------------------------------------------------------------------------------------------------------------------------
# tier 2, 7: the generator's graph as networks.ops builds it
# ---------------------------------------------------------------------------------------------------------------------------
def _flat(t):
    """[n, c, d, h, w] (or [n, f]) as [voxels, c]."""
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1]) if t.dim() == 5 else t


@pytest.mark.parametrize('alpha', [0.0, 0.5], ids=['alpha_0', 'alpha_half'])
def test_generator_through_ops(alpha, monkeypatch):
    """Phase 2 at the base shape (1, 2, 2), 32 channels throughout, 4 latents of 32.  ops wires: dense -> reshape -> generator_in's
    stage S0 (materialised by conv_1's up-sampled read, so the old to_rgb is an ordinary second consumer of it), conv_1 (ups) -> S1,
    conv_2 -> S2 (W = 4: no pn_bwd epilogue, S1 runs its own _PnActBwd), to_rgb_2 as _LazyRgbTail on the unmaterialised S2
    (_ConvPnActToRgb, sg_pixel_norm_act_bwd_pw_wg), lerp.  Backward, node by node on what each node read (captured): every
    pixel-norm backward, every stored data gradient (the generic _upconv_dgrad route stores the full-resolution one, then its
    block sum), autograd's one bf16 add where S0 has two consumers, and all twelve parameter gradients."""
    from saragan_amd.networks import ops
    from saragan_amd.networks.pgan.generator import generator
    F = _F()
    c = G.GEN
    dc = G.gen_data(c)
    z, g_out = dc['z'].to(dev()), dc['g'].to(dev()).contiguous(memory_format=torch.channels_last_3d)
    gain = float(ops.calculate_gain('leaky_relu', SLOPE))
    ks = {nm: (1.0 if nm.startswith('to_rgb') else gain) / float(np.sqrt(np.prod(dc['q'][nm].shape[:-1]))) for nm in G.GEN_NAMES}
    state = {}
    for nm in G.GEN_NAMES:
        state[f'generator/{nm}/weight'] = A.q_over_coef(dc['q'][nm], ks[nm], BF)
        state[f'generator/{nm}/bias'] = dc['b'][nm]
    q = {nm: t.to(dev()).double() for nm, t in dc['q'].items()}
    b = {nm: t.to(dev()).double() for nm, t in dc['b'].items()}
    convs, params = Tap(monkeypatch, 'raw_conv'), Tap(monkeypatch, '_conv_param_grads')
    pnact, masks, downs = ApplyTap(monkeypatch, '_PnActBwd'), ApplyTap(monkeypatch, '_BiasActBwd'), ApplyTap(monkeypatch, '_Down')
    pw_wg = LibSpy(monkeypatch, 'sg_pixel_norm_act_bwd_pw_wg')
    mixes = ApplyTap(monkeypatch, '_Axpby')

    def net(zin):
        return generator(zin, alpha, 2, (1, *c.base), 'leaky_relu', c.kernel_spec, c.filter_spec, param=SLOPE, size='xs')

    with _bf16_store() as store:
        with torch.no_grad():
            net(z)
        store.load_state_dict(state, strict=True)
        ws = {nm: store.vars[f'generator/{nm}/weight'] for nm in G.GEN_NAMES}
        bs = {nm: store.vars[f'generator/{nm}/bias'] for nm in G.GEN_NAMES}
        for t in (convs, params, pnact, masks, downs, mixes):
            t.clear()
        zl = leaf(z)
        img = net(zl)
        fwd = list(convs.calls)
        new_img = mixes.calls[0][0][1] if alpha != 0.0 else img      # to_rgb_2's image: the lerp's second operand
        convs.clear()
        leaves = [zl] + [ws[nm] for nm in G.GEN_NAMES] + [bs[nm] for nm in G.GEN_NAMES]
        grads = torch.autograd.grad(img, leaves, g_out, allow_unused=True)
    gz, gw, gb = grads[0], dict(zip(G.GEN_NAMES, grads[1:7])), dict(zip(G.GEN_NAMES, grads[7:]))
    old_rgb = [a for a, r in fwd + convs.calls if a['w'].data_ptr() == ws['to_rgb_1'].data_ptr()]
    if alpha == 0.0:
        assert old_rgb == [] and gw['to_rgb_1'] is None and gb['to_rgb_1'] is None, 'alpha = 0: the pruned to_rgb was launched'
    else:
        assert len(old_rgb) == 2, 'the old to_rgb: one forward and one data-gradient launch'
    stages = [r for a, r in fwd if a['pixel_norm'] and r is not None]      # (a declined rgb epilogue is asked again without)
    assert len(stages) == 3, 'three pixel-norm stages'
    (y0, s0, sg0), (y1, s1, sg1), (y2, s2, sg2) = (st[:3] for st in stages)
    assert (pw_wg.codes, len(pnact.calls)) == ([0], 2), 'S2 through sg_pixel_norm_act_bwd_pw_wg, S1 and S0 through _PnActBwd'
    n_v = c.n * c.fine[0] * c.fine[1] * c.fine[2]

    def dz_for(nm):
        return _dz_of(params, ws[nm])

    # ---- forward: the dense head is exact, S0 reads exact quarter-integers
    pre_d, h0 = G.dense_ref(z, q['generator_in/dense'], b['generator_in/dense'])
    h0 = A.stored(h0, BF).reshape(c.n, c.c, *c.base)
    a0, _, _, words0 = G.stage_forward(h0, q['generator_in/conv'], b['generator_in/conv'])
    G.pn_check('S0', y0.detach(), s0, a0, BF, c.c)
    eq_words(sg0, words0, 'sign words of S0')
    # ---- to_rgb_2 + S2: g = w_b * g_out (x) q_rgb, exact
    g_img = (1.0 - alpha) * g_out.double()
    q2 = q['to_rgb_2'].reshape(-1)
    ref = G.rgb_forward(y2.detach(), q2, float(b['to_rgb_2']))
    G.check(new_img, ref, G.rgb_bound(y2.detach(), q2, float(b['to_rgb_2']), ref), 'to_rgb_2')
    g2, sw, sw_abs, sb = G.rgb_backward(y2.detach(), q2, g_img)
    G.check_w(gw['to_rgb_2'], sw, sw_abs, n_v, ks['to_rgb_2'], 'gw of to_rgb_2')
    eq_b(gb['to_rgb_2'], sb, 'gb of to_rgb_2')
    dz2 = dz_for('generator_block_2/conv_2')
    dz2_ref, t2 = G.check_dz(dz2, A.stored(g2, BF), y2.detach(), s2, sg2, 'pass', 'dz of S2')
    bh = G.behind_dz(y1.detach(), q['generator_block_2/conv_2'], dz2)
    G.check_w(gw['generator_block_2/conv_2'], bh['sw'], bh['sw_abs'], bh['k'], ks['generator_block_2/conv_2'], 'gw of conv_2')
    G.check_gb_in_register(gb['generator_block_2/conv_2'], dz2_ref, t2, c.c, 'gb of conv_2')
    # ---- S1: reads the stored data gradient of conv_2
    g1 = pnact.calls[0][0][0].detach()
    G.check(g1, bh['gx'], bh['gx_bound'], 'data gradient of conv_2')
    assert pnact.calls[0][0][1].data_ptr() == y1.data_ptr() and pnact.calls[0][0][2].data_ptr() == s1.data_ptr()
    dz1 = dz_for('generator_block_2/conv_1')
    assert dz1.data_ptr() == pnact.calls[0][1][0].data_ptr()
    dz1_ref, t1 = G.check_dz(dz1, g1, y1.detach(), s1, sg1, 'pass', 'dz of S1')
    sw, sb_ = W.wgrad_ref(y0.detach(), dz1, K333, ups=True)
    sw_abs, _ = W.wgrad_ref(y0.detach().abs(), dz1.abs(), K333, ups=True)
    G.check_w(gw['generator_block_2/conv_1'], sw, sw_abs, n_v, ks['generator_block_2/conv_1'], 'gw of conv_1')
    G.check_gb_in_register(gb['generator_block_2/conv_1'], dz1_ref, t1, c.c, 'gb of conv_1')
    # the generic route of _upconv_dgrad: the full-resolution data gradient is stored, then its block sum
    up_sums = [(a, r) for a, r in downs.calls if a[1] == 1.0 and a[0].shape[1] == c.c]
    assert len(up_sums) == 1
    full, g0a = up_sums[0][0][0].detach(), up_sums[0][1].detach()
    ref, bound = G.stored_dgrad(dz1, q['generator_block_2/conv_1'])
    G.check(full, ref, bound, 'full-resolution data gradient of conv_1')
    ref, bound = G.stored_block_sum(full)
    G.check(g0a, ref, bound, 'its 2x2x2 block sum')
    # ---- the old to_rgb (alpha = 1/2): its image gradient is the exact block sum of alpha * g_out
    g0 = g0a.double()
    if alpha != 0.0:
        q1 = q['to_rgb_1'].reshape(-1)
        ga = A.stored(R.block_sum(alpha * g_out.double(), (2, 2, 2)), BF)
        g0b, sw, sw_abs, sb = G.rgb_backward(y0.detach(), q1, ga)
        G.check_w(gw['to_rgb_1'], sw, sw_abs, c.n * 4, ks['to_rgb_1'], 'gw of to_rgb_1')
        eq_b(gb['to_rgb_1'], sb, 'gb of to_rgb_1')
        g0 = g0 + A.stored(g0b, BF)      # autograd adds the two shares in bf16: one rounding of the exact sum
    g0_read = pnact.calls[1][0][0].detach()
    assert torch.equal(g0_read.double(), g0.float().to(BF).double()), 'the gradient S0 read is not the (rounded) sum of its consumers\' shares'
    # ---- S0
    dz0 = dz_for('generator_in/conv')
    dz0_ref, t0 = G.check_dz(dz0, g0_read, y0.detach(), s0, sg0, 'pass', 'dz of S0')
    bh = G.behind_dz(h0, q['generator_in/conv'], dz0)
    G.check_w(gw['generator_in/conv'], bh['sw'], bh['sw_abs'], bh['k'], ks['generator_in/conv'], 'gw of generator_in/conv')
    G.check_gb_in_register(gb['generator_in/conv'], dz0_ref, t0, c.c, 'gb of generator_in/conv')
    # ---- the dense head: reads the stored data gradient of generator_in/conv, masks it (exact), then three short sums
    head = [(a, r) for a, r in masks.calls if a[0].dim() == 2]
    assert len(head) == 1, 'the dense layer\'s own mask pass'
    gh = head[0][0][0].detach()
    G.check(gh.reshape(c.n, c.c, *c.base), bh['gx'], bh['gx_bound'], 'data gradient of generator_in/conv')
    dzd = head[0][1][0].detach()
    want = torch.where(pre_d >= 0, gh.double(), gh.double() * SLOPE)
    assert torch.equal(dzd.double(), want), 'the dense layer\'s mask'
    qd, kd = q['generator_in/dense'], ks['generator_in/dense']
    ref = z.double().t() @ want
    G.check(gw['generator_in/dense'], kd * ref, kd * G.matmul_bound(z.double().t(), want, ref) + 2.0 * G.U * (kd * ref).abs(), 'gw of dense')
    G.check(gb['generator_in/dense'], want.sum(0), G.sum_bound(want.abs().sum(0), c.n), 'gb of dense')
    ref = want @ qd.t()
    assert gz.dtype == BF
    G.check(gz, ref, G.sum_bound(want.abs() @ qd.t().abs(), G.nnz_terms(qd.reshape(1, 1, 1, *qd.shape), 'in'), ref, BF), 'gradient for the latents')
