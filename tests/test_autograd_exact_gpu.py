"""The discriminator's autograd routes (saragan_amd/functional.py: which kernel gets which tensor, mask, gain and destination)
pinned node by node and pair by pair to exact sums: every comparison is torch.equal against the fp64 restatement of
tests/agref.py, whose docstring says why integer data make every first- and second-order result exact (one rounding of the
exact value for a stored bf16 tensor, wgref.scaled(sum, coef) for a filter gradient, the exact sum for a bias gradient) and how
the pairs keep their one stored intermediate representable.  tests/test_agref_host.py shows on the host that the restatement is
the derivative it claims to be and that every case stays inside the exact range.

Each case names the route it must take and asserts that it ran, from a spy on the functional helper that route goes through
(raw_conv's pool / mask arguments, raw_bias_act_bwd for a mask pass of its own, _pw_backward, _pw_fused_backward,
_pooled_backward_gather / _planes, _gather_dgrad, _wgrad_launch) or from functional.GRAD_DEST_STATS; every fused route is run
beside its plain counterpart (the matching functional._NO_* switch), and BOTH must equal the reference.

Second order differentiates <gx, v> for a free integer v (never sum(gx^2)): see agref.  Rounding points a route adds by storing a
tensor another route keeps in registers are restated where the stored tensor cannot be representable (the D x W means of pool
mode 1 and the full-resolution tensor of the generic route in the gradient penalty's double backward: dense filters, sums of
hundreds of units); everything else is one rounding of the exact value."""
import contextlib
import inspect

import pytest
import torch

from tests import agref as A
from tests import fwdref as R
from tests import wgref as W

pytestmark = pytest.mark.gpu

BF, F32 = A.BF, A.F32
SLOPE = A.SLOPE


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _F():
    from saragan_amd import functional as F
    return F


def on_dev(d):
    """The CPU tensors of a case on the GPU (5-D ones stay NDHWC)."""
    out = {}
    for k, t in d.items():
        t = t.to(dev())
        out[k] = t.contiguous(memory_format=torch.channels_last_3d) if t.dim() == 5 and k[0] not in 'qu' else t.contiguous()
    return out


def leaf(t):
    return t.detach().clone(memory_format=torch.preserve_format).requires_grad_(True)


def var(q_cpu, coef, dtype):
    """The f32 variable on the GPU whose packed image is exactly q (agref.q_over_coef)."""
    return A.q_over_coef(q_cpu, coef, dtype).to(dev()).requires_grad_(True)


def eq(got, ref, dtype, what):
    """got EQUALS the exact fp64 value rounded once to `dtype`."""
    assert got is not None, what
    assert got.dtype == dtype and tuple(got.shape) == tuple(ref.shape), (what, got.dtype, tuple(got.shape), tuple(ref.shape))
    exp = R.expected(ref, dtype)
    if not torch.equal(got.detach(), exp.to(got.device)):
        bad = (got.detach().double() != exp.to(got.device).double())
        pytest.fail(f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the exact value rounded once '
                    f'(largest difference {float((got.detach().double() - exp.to(got.device).double()).abs().max())})')


def eq_w(got, total, coef, what, prefill=None):
    """A filter gradient EQUALS np.float32(coef) * np.float32(exact sum) [added onto prefill] (wgref.scaled)."""
    assert got is not None, what
    assert got.dtype == F32, (what, got.dtype)
    exp = W.scaled(total, coef, prefill)
    g = got.detach().cpu().reshape(exp.shape)
    if not torch.equal(g, exp):
        bad = g != exp
        pytest.fail(f'{what}: {int(bad.sum())} of {bad.numel()} entries differ from coef * exact sum (largest difference '
                    f'{float((g.double() - exp.double()).abs().max())})')
    return exp


def eq_b(got, total, what):
    assert got is not None, what
    assert got.dtype == F32, (what, got.dtype)
    assert torch.equal(got.detach().double().cpu(), total.cpu()), what


def eq_words(got, ref, what):
    assert got is not None and got.dtype == torch.int32, what
    assert torch.equal(got.reshape(ref.shape), ref.to(got.device)), what


class Spy:
    """Wraps functional.<name>: records for every call its non-tensor arguments (tensors as True, absent ones as None) and
    whether it returned something (the result itself with keep=True)."""

    def __init__(self, monkeypatch, name, keep=False):
        F = _F()
        self.real, self.calls, self.keep = getattr(F, name), [], keep
        sig = inspect.signature(self.real)

        def wrapper(*a, **k):
            r = self.real(*a, **k)
            ba = sig.bind(*a, **k)
            ba.apply_defaults()
            args = {n: (True if isinstance(v, torch.Tensor) else v) for n, v in ba.arguments.items()}
            self.calls.append((args, r if self.keep else (r is not None)))
            return r
        monkeypatch.setattr(F, name, wrapper)

    def clear(self):
        del self.calls[:]

    def args(self, key):
        return [c[0][key] for c in self.calls]

    def results(self):
        return [c[1] for c in self.calls]


def decline_masked_wgrad(monkeypatch):
    """The gathered-dy weight-gradient launch (mask given) declines, as the library does for a shape it has no tile for: nothing
    is written.  Returns the list the declined launches are counted in."""
    F = _F()
    real, declined = F._wgrad_launch, []

    def launch(lib, x, dy, mask, *rest):
        if mask is not None:
            declined.append(True)
            return F._lib.SG_EUNSUPPORTED
        return real(lib, x, dy, mask, *rest)
    monkeypatch.setattr(F, '_wgrad_launch', launch)
    return declined


coefs, effective = A.coefs, A.effective


# ---------------------------------------------------------------------------------------------------------------------------
# a, b: _ConvBiasAct (LeakyReLU), alone and with consumers (ActInfo); the double backward's mask pull-back (BackInfo)
# ---------------------------------------------------------------------------------------------------------------------------
def _cba_graph(c, d, vs, skip=False, create_graph=False):
    """Builds the case's graph on fresh leaves and runs the first backward.  Returns (leaves, forward values, gradients)."""
    F = _F()
    k1, k2, k3 = coefs(c)
    w1, b1, w2, w3 = vs
    x, gy = leaf(d['x']), leaf(d['gy'])
    info = F.ActInfo(SLOPE)
    h = F.conv3d(x, w1, k1, bias=b1, act=True, slope=SLOPE, out_info=info)
    outs, gys, params = [h], [gy], [w1, b1]
    if c.variant != 'alone':
        info.consume(True)          # the consumer's data gradient applies the producer's mask in its epilogue
        outs = [F.conv3d(h, w2, k2, in_info=info)]
        params.append(w2)
        if c.variant == 'mixed':
            info.consume(False)     # a plain consumer: the producer must run its own mask pass
            outs.append(F.conv3d(h, w3, k3))
            gys.append(leaf(d['gy3']))
            params.append(w3)
    else:
        info.consume(False)
    ctx = F.skip_param_grads(params) if skip else contextlib.nullcontext()
    with ctx:
        grads = torch.autograd.grad(outs, [x] + ([] if skip else params), gys, create_graph=create_graph)
    return (x, gys, params, info), (h, outs), grads


@pytest.mark.parametrize('c', A.CBA_CASES, ids=repr)
def test_conv_bias_act_alone_and_with_consumers(c, monkeypatch):
    """alone: one mask pass (which also sums the bias gradient), then the data and the filter gradient.  premask: NO mask pass,
    the consumer's data gradient carries the producer's sign words and the bias gradient comes out of the filter-gradient launch.
    mixed: the producer's own pass, the consumers' data gradients unmasked -- no share masked twice.  Then <gx, v>: with every
    consumer of the masked data gradient a conv (skip_param_grads, the gradient penalty's first backward) the mask pull-back
    rides in that conv's epilogue (BackInfo) -- compared with _NO_BACK_PREMASK -- and with a _Wgrad consumer beside it the
    masked conv keeps its pass."""
    F = _F()
    dc = A.cba_data(c)
    d = effective(c, on_dev(dc))
    ref = A.cba_reference(c, d)
    k1, k2, k3 = coefs(c)
    vs = [var(dc['q1'], k1, c.dtype), d['b1'].clone().requires_grad_(True),
          var(dc['q2'], k2, c.dtype) if 'q2' in dc else None, var(dc['q3'], k3, c.dtype) if 'q3' in dc else None]
    masks = Spy(monkeypatch, 'raw_bias_act_bwd')
    wgrads = Spy(monkeypatch, 'raw_wgrad')
    convs = Spy(monkeypatch, 'raw_conv')

    # ---- forward and first order, nothing differentiates the backward again
    (x, gys, params, info), (h, outs), grads = _cba_graph(c, d, vs)
    eq(h, ref['y'], c.dtype, 'y')
    eq_words(info.bits, ref['words'], 'sign words')
    eq(grads[0], ref['gx'], c.dtype, 'gx')
    eq_w(grads[1], ref['sw1'], k1, 'gw1')
    eq_b(grads[2], ref['sb1'], 'gb1')
    if c.variant != 'alone':
        eq(outs[0], ref['y2'], c.dtype, 'y2')
        eq_w(grads[3], ref['sw2'], k2, 'gw2')
    if c.variant == 'mixed':
        eq(outs[1], ref['y3'], c.dtype, 'y3')
        eq_w(grads[4], ref['sw3'], k3, 'gw3')
    masked_convs = [m for m in convs.args('mask_bits') if m is not None]
    if c.variant == 'premask':
        assert masks.calls == [], 'the producer ran a mask pass although its only consumer pre-masks'
        assert len(masked_convs) == 1, 'the consumer\'s data gradient did not carry the mask'
        assert sorted(wgrads.args('want_db')) == [False, True], 'the bias gradient did not come from the filter-gradient launch'
    else:
        assert masks.args('want_db') == [True] and masks.args('want_dx') == [True], 'expected exactly the producer\'s own mask pass'
        assert masked_convs == [], 'a share of the gradient was masked twice'
        assert not any(wgrads.args('want_db'))

    # ---- <gx, v>: the first backward keeps its graph
    def second(skip, no_back_premask):
        monkeypatch.setattr(F, '_NO_BACK_PREMASK', no_back_premask)
        (x, gys, params, info), _, g1 = _cba_graph(c, d, vs, skip=skip, create_graph=True)
        eq(g1[0], ref['gx'], c.dtype, 'gx (create_graph)')
        if not skip:
            eq_w(g1[1], ref['sw1'], k1, 'gw1 (create_graph)')
            eq_b(g1[2], ref['sb1'], 'gb1 (create_graph)')
        loss = (g1[0].float() * d['v'].float()).sum()
        masks.clear(), convs.clear()
        ws = [p for p in params if p.dim() == 5]
        g2 = torch.autograd.grad(loss, gys + ws)
        what = f'second order (skip={skip}, no_back_premask={no_back_premask}) '
        eq(g2[0], ref['g_gy'], c.dtype, what + 'g_gy')
        if c.variant == 'mixed':
            eq(g2[1], ref['g_gy3'], c.dtype, what + 'g_gy3')
        for g, key, k in zip(g2[len(gys):], ('s2w1', 's2w2', 's2w3'), (k1, k2, k3)):
            eq_w(g, ref[key], k, what + key)
        return len(masks.calls), len([m for m in convs.args('mask_bits') if m is not None])

    try:
        fused = second(True, False)
        plain = second(True, True)
        kept = second(False, False)
    finally:
        monkeypatch.setattr(F, '_NO_BACK_PREMASK', False)
    if c.variant == 'premask':
        assert fused == (0, 1), ('the mask pull-back did not ride in the consumer\'s epilogue', fused)
        assert plain == (1, 0), ('_NO_BACK_PREMASK: expected the separate mask pass', plain)
        assert kept == (1, 0), ('a masked conv with a _Wgrad consumer must keep its own pass', kept)
    else:       # the producer masked in a pass of its own: that pass is its own backward, whatever the switch
        assert fused == plain == kept == (1, 0), (fused, plain, kept)


# ---------------------------------------------------------------------------------------------------------------------------
# c: _Wgrad.backward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', A.WGRAD_CASES, ids=repr)
def test_wgrad_backward_both_outputs(c):
    F = _F()
    d = on_dev(A.wgrad_data(c))
    ref = A.wgrad_reference(c, d)
    x, dy = leaf(d['x']), leaf(d['dy'])
    dw, db = F._Wgrad.apply(x, dy, A.K333, c.coef, False, True, 0, 0)
    eq_w(dw, ref['sw'], c.coef, 'dw')
    eq_b(db, ref['sb'], 'db')
    gx, gdy = torch.autograd.grad((dw * d['u']).sum(), [x, dy])
    eq(gx, ref['gx'], c.dtype, 'gradient for x: the data gradient of dy with the filter coef * u')
    eq(gdy, ref['gdy'], c.dtype, 'gradient for dy: conv3d(x, coef * u)')
    # through a fused up-sample the third order is refused, not mis-computed
    xh = leaf(d['x'][:, :, :c.sp[0] // 2, :c.sp[1] // 2, :c.sp[2] // 2].contiguous(memory_format=torch.channels_last_3d))
    dwu, _ = F._Wgrad.apply(xh, dy, A.K333, c.coef, True, False, 0, 0)
    eq_w(dwu, W.wgrad_ref(xh.detach(), d['dy'], A.K333, ups=True)[0], c.coef, 'dw (fused up-sample)')
    with pytest.raises(NotImplementedError):
        torch.autograd.grad((dwu * d['u']).sum(), [xh])


# ---------------------------------------------------------------------------------------------------------------------------
# d: from_rgb
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', A.PW_CASES, ids=repr)
def test_from_rgb_backward_routes(c, monkeypatch):
    """_pw_backward: gx, gw and gb in one pass over the output gradient; _pw_fused_backward: the whole backward in the epilogue of
    the consumer's data gradient (bf16; the consumer's (4, 8, 32) volume engages it, W a multiple of 32), the placeholder gy is
    never read; beside each its plain counterpart, and the declined variants."""
    F = _F()
    dc = A.pw_data(c)
    d = effective(c, on_dev(dc))
    ref = A.pw_reference(c, d)
    k1, k2, _ = coefs(c)
    w1, b1, w2 = var(dc['q1'], k1, c.dtype), d['b1'].clone().requires_grad_(True), var(dc['q2'], k2, c.dtype)
    one_pass = Spy(monkeypatch, '_pw_backward')
    fused = Spy(monkeypatch, '_pw_fused_backward')
    bf = c.dtype == BF

    def alone():
        x = leaf(d['x'])
        y = F.conv3d(x, w1, k1, bias=b1, act=True, slope=SLOPE, out_info=F.ActInfo(SLOPE))
        eq(y, ref['y'], c.dtype, 'y')
        gx, gw, gb = torch.autograd.grad(y, [x, w1, b1], d['gy'])
        eq(gx, ref['gx'], c.dtype, 'gx')
        eq_w(gw, ref['sw1'], k1, 'gw')
        eq_b(gb, ref['sb1'], 'gb')

    alone()
    assert one_pass.results() == [True], 'the one-pass backward was not used'
    monkeypatch.setattr(F, '_NO_RGB_FUSION', True)
    alone()
    assert one_pass.results() == [True], 'the plain counterpart ran the one-pass backward'
    monkeypatch.setattr(F, '_NO_RGB_FUSION', False)

    def pair(x_req=True, skip=False):
        x = leaf(d['x']) if x_req else d['x']
        info = F.ActInfo(SLOPE)
        h = F.conv3d(x, w1, k1, bias=b1, act=True, slope=SLOPE, out_info=info)
        info.consume(True)
        y2 = F.conv3d(h, w2, k2, in_info=info)
        eq(y2, ref['y2'], c.dtype, 'y2')
        eq_words(info.bits, ref['words'], 'sign words')
        wanted = ([x] if x_req else []) + ([] if skip else [w1, b1]) + [w2]
        with F.skip_param_grads([w1, b1]) if skip else contextlib.nullcontext():
            got = list(torch.autograd.grad(y2, wanted, d['gy2']))
        if x_req:
            eq(got.pop(0), ref['pgx'], c.dtype, 'gx (pair)')
        if not skip:
            eq_w(got.pop(0), ref['psw1'], k1, 'gw1 (pair)')
            eq_b(got.pop(0), ref['psb1'], 'gb1 (pair)')
        eq_w(got.pop(0), ref['sw2'], k2, 'gw2 (pair)')
        return info

    fused.clear()
    pair()
    assert fused.results() == ([True] if bf else []), 'bf16 runs from_rgb\'s backward in the consumer\'s epilogue, f32 takes the plain path'
    fused.clear()
    info = pair(x_req=False)      # no image gradient: the epilogue still reduces gw and gb, gx is None
    assert fused.results() == ([True] if bf else [])
    assert info.pw_result is None, 'from_rgb\'s backward did not pick its result up'
    fused.clear()
    pair(x_req=False, skip=True)      # nothing of from_rgb's is wanted: declined, the plain masked data gradient runs
    assert fused.results() == ([False] if bf else [])
    monkeypatch.setattr(F, '_NO_PW_EPILOGUE', True)
    fused.clear()
    pair()
    assert fused.results() == [], 'the plain counterpart ran the fused epilogue'


# ---------------------------------------------------------------------------------------------------------------------------
# e: _ConvBiasActPool forward
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', A.POOLFWD_CASES, ids=repr)
def test_conv_bias_act_pool_forward_modes(c, monkeypatch):
    """Pool mode 3 (32 input channels, 2^20 voxels: functional._pool_mode), mode 1 (by _NO_POOL3 and for a 16-channel input) and
    mode 2 (64 -> 64 at 2^18 voxels): y is the exact 2x2x2 mean rounded once (the 4-voxel means modes 1 and 2 store are bf16
    values by construction, agref.poolfwd_data), the sign words are those of the pre-pool activation."""
    F = _F()
    mode, switch = c.variant
    dc = A.poolfwd_data(c)
    d = on_dev(dc)
    ref = A.poolfwd_reference(c, d)
    if switch:
        monkeypatch.setattr(F, switch, True)
    w = var(dc['q'], c.coef, c.dtype)
    convs = Spy(monkeypatch, 'raw_conv', keep=True)
    with torch.no_grad():
        y = F.conv3d_act_pool(d['x'], w, c.coef, d['b'], SLOPE)
    torch.cuda.synchronize()
    took = [(a['pool'], r is not None) for a, r in convs.calls]
    assert took == [(mode, True)], f'expected one launch with sg_conv_epilogue.pool = {mode}, got {took}'
    signs = convs.calls[0][1][2]
    eq(y, ref['y'], c.dtype, 'y')
    eq_words(signs, ref['words'], 'sign words')
    del convs, ref, d, y, signs
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------
# f, g, h: the 32 -> 64 layer with downscale3d
# ---------------------------------------------------------------------------------------------------------------------------
_POOL_REFS = {}


@pytest.fixture(scope='module')
def pool_refs():
    """The references of the pooled cases, computed once per (case, masked input) on the GPU and shared; released at the end."""
    def get(c, in_mask):
        key = (c.id, in_mask)
        if key not in _POOL_REFS:
            for other in [k for k in _POOL_REFS if k[0] != c.id]:      # (the cases come grouped: only one case's references are alive)
                del _POOL_REFS[other]
            torch.cuda.empty_cache()
            dc = A.pool_data(c)
            d = on_dev(dc)
            ref = A.pool_reference(c, d, in_mask)
            del ref['pre']
            _POOL_REFS[key] = (dc, d, ref)
        return _POOL_REFS[key]
    yield get
    _POOL_REFS.clear()
    torch.cuda.empty_cache()


POOL = {c.id: c for c in A.POOL_CASES}


def _pool_layer(c, d, ref, in_mask, w, b):
    """conv3d_act_pool on a fresh leaf x [whose producer's mask this layer's data gradient applies]: (x, y, sign words)."""
    F = _F()
    info = None
    if in_mask:
        info = F.ActInfo(SLOPE)
        info.bits = F.sign_words(d['a_in'])
        eq_words(info.bits, ref['in_words'], 'sg_sign_words of the input stage')
        info.consume(True)
    x = leaf(d['x'])
    y = F.conv3d_act_pool(x, w, c.coef, b, SLOPE, info)
    return x, y


@pytest.mark.parametrize('route', ['gather', 'planes', 'generic'])
@pytest.mark.parametrize('in_mask', [False, True], ids=['plain_input', 'masked_input'])
def test_pooled_backward_routes(route, in_mask, monkeypatch, pool_refs):
    """_ConvBiasActPool.backward when nothing differentiates it again, on the ragged volume (H = 126 no multiple of the 4-row tile, D / 2
    = 3 odd): the fused gather, the two-tensor planes (_NO_GATHER_BWD) and the generic masked up-scale + plain kernels (_NO_GATHER_BWD
    and _NO_PLANES) must each EQUAL the reference -- gx one rounding of the exact value [masked by the input stage], gw and gb
    the exact sums."""
    F = _F()
    c = POOL['pool_ragged']
    dc, d, ref = pool_refs(c, in_mask)
    w, b = var(dc['q'], c.coef, c.dtype), d['b'].clone().requires_grad_(True)
    monkeypatch.setattr(F, '_NO_GATHER_BWD', route != 'gather')
    monkeypatch.setattr(F, '_NO_PLANES', route == 'generic')
    gather, planes = Spy(monkeypatch, '_pooled_backward_gather'), Spy(monkeypatch, '_pooled_backward_planes')
    convs = Spy(monkeypatch, 'raw_conv', keep=True)
    x, y = _pool_layer(c, d, ref, in_mask, w, b)
    eq_words(convs.calls[-1][1][2], ref['words'], 'sign words')
    convs.keep = False
    convs.clear()
    gx, gw, gb = torch.autograd.grad(y, [x, w, b], d['gy'])
    assert (gather.results(), planes.results()) == {'gather': ([True], []), 'planes': ([], [True]), 'generic': ([], [])}[route]
    eq(gx, ref['gx'], c.dtype, 'gx')
    eq_w(gw, ref['sw'], c.coef, 'gw')
    eq_b(gb, ref['sb'], 'gb')


PENALTY = [('pool_ragged', False, 'gather', 'generic'), ('pool_ragged', True, 'gather', 'generic'), ('pool_ragged', True, 'up', 'generic'),
           ('pool_2p20', True, 'gather', 'pool3'), ('pool_2p20', True, 'gather', 'pool1')]


@pytest.mark.parametrize('cid,in_mask,first,second', PENALTY, ids=[f'{p[0]}_{"masked" if p[1] else "plain"}_{p[2]}_{p[3]}' for p in PENALTY])
def test_gradient_penalty_routes(cid, in_mask, first, second, monkeypatch, pool_refs):
    """The gradient penalty's first backward (skip_param_grads on w and b, create_graph): _PooledDgradGather ('gather') or, with
    _NO_GATHER_BWD, the generic _Up + data-gradient conv ('up').  Then <gx, v>: the gradient for gy is the layer's forward map on
    [M_in *] v -- through pool mode 3 (2^20 voxels: one rounding), mode 1 (_NO_POOL3: the D x W means are stored, then the H
    pairs) or the generic _Down(_Conv(.), mask) below 2^20 voxels (the full-resolution tensor is stored, then the masked block
    mean) -- and the gradient for w the weight sum of ([M_in *] v, M * upscale3d(gy) / 8) as a fresh tensor."""
    F = _F()
    c = POOL[cid]
    dc, d, ref = pool_refs(c, in_mask)
    w, b = var(dc['q'], c.coef, c.dtype), d['b'].clone().requires_grad_(True)
    monkeypatch.setattr(F, '_NO_GATHER_BWD', first != 'gather')
    monkeypatch.setattr(F, '_NO_POOL3', second == 'pool1')
    gathers = Spy(monkeypatch, '_gather_dgrad')
    x, y = _pool_layer(c, d, ref, in_mask, w, b)
    gy = leaf(d['gy'])
    with F.skip_param_grads([w, b]):
        (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
    assert gathers.results() == ([True] if first == 'gather' else []), 'the first backward took another route'
    eq(gx, ref['gx'], c.dtype, 'gx')
    loss = (gx.float() * d['v'].float()).sum()
    convs = Spy(monkeypatch, 'raw_conv')
    launches = Spy(monkeypatch, '_wgrad_launch')
    g_gy, g_w = torch.autograd.grad(loss, [gy, w])
    pools = [p for p in convs.args('pool') if p]
    full = ref['g_full']
    if second == 'pool3':
        assert pools == [3] and convs.results()[convs.args('pool').index(3)], pools
        exact = ref['g_gy']
    elif second == 'pool1':
        assert pools == [1], pools
        exact = 0.5 * R.block_sum(R.expected(R.pool_mean(full, 1), c.dtype).double(), (1, 2, 1))
    else:
        assert pools == [], pools
        exact = R.pool_mean(R.expected(full, c.dtype).double(), 3)
    eq(g_gy, exact, c.dtype, 'second-order g_gy')
    if first == 'gather':
        assert launches.args('mask') == [True] and launches.args('accumulate') == [False], 'expected one gathered-dy launch into a fresh tensor'
    eq_w(g_w, ref['s2w'], c.coef, 'second-order gw')


def test_grads_into_accumulates_the_second_order_term_in_place(monkeypatch, pool_refs):
    """A first-order backward of the 32 -> 64 layer and the gradient penalty's second-order term inside one grads_into: the first
    claims the filter's and the bias' slot of the flat buffer, the second is ADDED to the filter's slot in place
    (SG_WGRAD_ACCUMULATE) -- the slot holds exactly scaled(s2, coef, prefill=scaled(s1, coef)).  _NO_GRAD_DEST gives the same sum
    through autograd; a declined launch gives its slot back (and the second-order term then takes the materialised fallback); a
    slot whose numel does not match is left alone."""
    F = _F()
    c = POOL['pool_ragged']
    dc, d, ref = pool_refs(c, False)
    nw = dc['q'].numel()

    def run(wrong_numel=False):
        w, b = var(dc['q'], c.coef, c.dtype), d['b'].clone().requires_grad_(True)
        flat = torch.zeros(nw + 64 + 8, device=dev())
        slots = {w.data_ptr(): flat[:nw + 8] if wrong_numel else flat[:nw].view(w.shape), b.data_ptr(): flat[nw + 8:nw + 72]}
        before = dict(F.GRAD_DEST_STATS)
        with F.grads_into(slots):
            x, y = _pool_layer(c, d, ref, False, w, b)
            torch.autograd.backward(y, d['gy'], inputs=[w, b])
            first = (w.grad.data_ptr() == flat.data_ptr(), b.grad.data_ptr() == slots[b.data_ptr()].data_ptr())
            claimed_1 = {k: v[1] for k, v in F._GRAD_DEST.items()}
            x2, y2 = _pool_layer(c, d, ref, False, w, b)
            gy = leaf(d['gy'])
            with F.skip_param_grads([w, b]):
                (gx,) = torch.autograd.grad(y2, x2, gy, create_graph=True)
            torch.autograd.backward((gx.float() * d['v'].float()).sum(), inputs=[w])
            in_place = w.data_ptr() in F.ACCUMULATED_IN_PLACE
        stats = {k: F.GRAD_DEST_STATS[k] - before[k] for k in ('claimed', 'accumulated')}
        return w, b, flat, first, claimed_1, in_place, stats

    s1 = W.scaled(ref['sw'], c.coef)
    # the route: claimed, then accumulated in place
    w, b, flat, first, claimed_1, in_place, stats = run()
    assert first == (True, True) and all(claimed_1.values()), 'the first-order gradients were not written into their slots'
    assert in_place and stats == {'claimed': 2, 'accumulated': 1}, (in_place, stats)
    total = eq_w(flat[:nw], ref['s2w'], c.coef, 'the filter\'s slot', prefill=s1)
    assert torch.equal(w.grad.cpu().reshape(total.shape), total), '.grad is not the slot\'s sum'
    eq_b(flat[nw + 8:nw + 72], ref['sb'], 'the bias\' slot')
    # the plain counterpart: tensors of their own, added by autograd
    monkeypatch.setattr(F, '_NO_GRAD_DEST', True)
    w, b, flat, first, claimed_1, in_place, stats = run()
    monkeypatch.setattr(F, '_NO_GRAD_DEST', False)
    assert first == (False, False) and not in_place and stats == {'claimed': 0, 'accumulated': 0}, (first, in_place, stats)
    assert torch.equal(w.grad.cpu().reshape(total.shape), total), '_NO_GRAD_DEST: another sum'
    eq_b(b.grad, ref['sb'], '_NO_GRAD_DEST: gb')
    assert float(flat.abs().max()) == 0.0
    # a slot of another numel is left alone (the bias' slot is used as before)
    w, b, flat, first, claimed_1, in_place, stats = run(wrong_numel=True)
    assert first == (False, True) and not in_place and stats == {'claimed': 1, 'accumulated': 0}, (first, in_place, stats)
    assert torch.equal(w.grad.cpu().reshape(total.shape), total), 'mismatched slot: another sum'
    assert float(flat[:nw + 8].abs().max()) == 0.0, 'a slot whose numel does not match was written'
    eq_b(flat[nw + 8:nw + 72], ref['sb'], 'the bias\' slot')
    # the gathered launch declines: the claims are given back, the planes route and the materialised fallback compute the same
    declined = decline_masked_wgrad(monkeypatch)
    w, b, flat, first, claimed_1, in_place, stats = run()
    assert len(declined) == 2, declined
    assert first == (False, False) and not any(claimed_1.values()), 'a declined launch kept its slot'
    assert not in_place and stats == {'claimed': 1, 'accumulated': 0}, (in_place, stats)      # (the fallback's plain launch claims the free slot)
    assert torch.equal(w.grad.cpu().reshape(total.shape), total), 'declined launch: another sum'
    eq_w(flat[:nw], ref['s2w'], c.coef, 'the fallback\'s gradient in the slot it claimed')
    eq_b(b.grad, ref['sb'], 'declined launch: gb')


# ---------------------------------------------------------------------------------------------------------------------------
# i: one real pair through networks.ops
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', A.BLOCK_CASES, ids=repr)
def test_from_rgb_and_discriminator_block_through_ops(c, monkeypatch):
    """from_rgb -> discriminator_block (conv_1 32 -> 32, conv_2 32 -> 64, downscale3d) built by networks.ops under a
    VariableStore with q / he_std weights: the ActInfo wiring of ops._consume(premask=...), not only functional.py.  First order
    for the image and all six parameters, then <gx, v> for the pooled gradient and the three filters.  block_fused (2^20 voxels,
    W a multiple of 32) must run pool mode 3 forward and in the double backward, _PooledDgradGather and from_rgb's backward in
    conv_1's data-gradient epilogue; block_tiny must fuse none of them (its stored full-resolution tensors are restated)."""
    import numpy as np
    from saragan_amd import varstore
    from saragan_amd.networks import ops
    from saragan_amd.networks.pgan.discriminator import discriminator_block
    F = _F()
    big = c.id == 'block_fused'
    dc = A.block_data(c)
    d = on_dev(dc)
    ref = A.block_reference(c, d)
    y_exact = ref['y'] if big else R.pool_mean(R.expected(ref.pop('a2'), c.dtype).double(), 3)
    ref.pop('a2', None)
    g_gy_exact = ref['g_gy'] if big else R.pool_mean(R.expected(ref['g_full'], c.dtype).double(), 3)
    del ref['g_full']
    gain = ops.calculate_gain('leaky_relu', SLOPE)
    names = ['from_rgb', 'block/conv_1', 'block/conv_2']
    ks = [float(gain / np.sqrt(np.prod(dc[q].shape[:-1]))) for q in ('q0', 'q1', 'q2')]      # he_std, as ops.get_weight forms it
    state = {}
    for i, nm in enumerate(names):
        state[nm + '/weight'] = A.q_over_coef(dc[f'q{i}'], ks[i], c.dtype)
        state[nm + '/bias'] = dc[f'b{i}']
    kspec = [[(3, 3, 3), (3, 3, 3)], [(3, 3, 3), (3, 3, 3)]]
    fspec = [[0, 64], [32, 0]]

    def net(img):
        with varstore.variable_scope('from_rgb'):
            h = ops.from_rgb(img, 32, 'leaky_relu', param=SLOPE)
        with varstore.variable_scope('block'):
            return ops.materialize(discriminator_block(h, 'leaky_relu', kspec, fspec, 2, param=SLOPE))

    store = varstore.VariableStore(dev())
    old_dt = varstore.compute_dtype()
    varstore.set_compute_dtype(c.dtype)
    fused = Spy(monkeypatch, '_pw_fused_backward')
    gathers = Spy(monkeypatch, '_gather_dgrad')
    convs = Spy(monkeypatch, 'raw_conv')
    try:
        with varstore.use_store(store):
            with torch.no_grad():
                net(d['x'])         # creates the variables
            store.load_state_dict(state, strict=True)
            assert sorted(store.vars) == sorted(state), sorted(store.vars)
            ws = [store.vars[nm + '/weight'] for nm in names]
            bs = [store.vars[nm + '/bias'] for nm in names]
            # ---- first order
            convs.clear()
            x = leaf(d['x'])
            y = net(x)
            assert [p for p in convs.args('pool') if p] == ([3] if big else []), 'forward pool mode'
            eq(y, y_exact, c.dtype, 'y')
            g1 = torch.autograd.grad(y, [x, *ws, *bs], d['gy'])
            assert fused.results() == [big], 'from_rgb\'s backward in conv_1\'s epilogue: expected ' + ('engaged' if big else 'declined')
            assert gathers.results() == ([True] if big else []), 'the pooled backward\'s gather'
            eq(g1[0], ref['gx'], c.dtype, 'gx')
            for i in range(3):
                eq_w(g1[1 + i], ref[f'sw{i}'], ks[i], f'gw of {names[i]}')
                eq_b(g1[4 + i], ref[f'sb{i}'], f'gb of {names[i]}')
            del g1, y, x
            # ---- <gx, v>
            x, gy = leaf(d['x']), leaf(d['gy'])
            y = net(x)
            gathers.clear()
            with F.skip_param_grads(ws + bs):
                (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
            assert gathers.results() == ([True] if big else []), 'the gradient penalty\'s first backward'
            eq(gx, ref['gx'], c.dtype, 'gx (create_graph)')
            convs.clear()
            g2 = torch.autograd.grad((gx.float() * d['v'].float()).sum(), [gy, *ws])
            assert [p for p in convs.args('pool') if p] == ([3] if big else []), 'pool mode of the double backward'
            eq(g2[0], g_gy_exact, c.dtype, 'second-order g_gy')
            for i in range(3):
                eq_w(g2[1 + i], ref[f's2w{i}'], ks[i], f'second-order gw of {names[i]}')
    finally:
        varstore.set_compute_dtype(old_dt)
    del ref, d, g2, gx, y
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------
# j: refusals
# ---------------------------------------------------------------------------------------------------------------------------
def test_second_order_through_pixel_norm_is_refused():
    """_PixelNormBwd, _PnActBwd, _dgrad_into and _ConvPnActToRgb raise NotImplementedError where a second-order gradient would
    have to pass a pixel-norm stage; none returns a value."""
    F = _F()
    n, ch, sp = 2, 32, (2, 8, 32)
    x0 = A.ints((n, ch, *sp), 901, BF).to(dev()).contiguous(memory_format=torch.channels_last_3d)
    w = A.dense_filter(A.K333, ch, ch, 902).to(dev()).requires_grad_(True)
    w2 = A.dense_filter(A.K333, ch, ch, 903).to(dev()).requires_grad_(True)
    w_rgb = A.dense_filter(A.K111, ch, 1, 904).to(dev()).requires_grad_(True)
    b = W.int_data((ch,), 905, F32).to(dev()).requires_grad_(True)
    b_rgb = torch.zeros(1, device=dev()).requires_grad_(True)

    def twice(y, x):
        gy = leaf(torch.ones_like(y))
        (gx,) = torch.autograd.grad(y, x, gy, create_graph=True)
        return torch.autograd.grad(gx.float().sum(), [gy, w], allow_unused=True)

    x = leaf(x0)
    with pytest.raises(NotImplementedError):      # _PixelNormBwd: the stage as passes of its own
        twice(F.conv3d(x, w, 0.05, bias=b, act=True, slope=SLOPE, pixel_norm=True, fuse=False), x)
    x = leaf(x0)
    with pytest.raises(NotImplementedError):      # _PnActBwd: the stage fused into the conv epilogue
        twice(F.conv3d(x, w, 0.05, bias=b, act=True, slope=SLOPE, pixel_norm=True), x)
    x = leaf(x0)
    info = F.ActInfo(SLOPE)
    h = F.conv3d(x, w, 0.05, bias=b, act=True, slope=SLOPE, pixel_norm=True, out_info=info)
    info.consume(True)
    assert info.pn is not None
    y = F.conv3d(h, w2, 0.05, in_info=info)
    with pytest.raises(NotImplementedError):      # _dgrad_into: the stage's backward in the consumer's epilogue
        torch.autograd.grad(y.float().sum(), x, create_graph=True)
    x = leaf(x0)
    img, y = F.conv3d_pn_to_rgb(x, w, 0.05, b, False, SLOPE, 1e-8, None, w_rgb, 0.1, b_rgb)
    with pytest.raises(NotImplementedError):      # _ConvPnActToRgb
        torch.autograd.grad(img.float().sum(), x, create_graph=True)
