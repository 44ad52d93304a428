"""csrc/optim.hip at kernel level: sg_adam_ema, sg_optim_step (SGD, Momentum, Nesterov, Adadelta), their `_dev` entry
points and sg_segment_sumsq(_flag) against the fp64 rules of include/saragan_hip.h (tests/ewref.py; O.TFAdam and
O.ema_update where the oracle has them).  Three steps with fresh gradients, gscale = 0.5, ema_decay = 0.99; parameters and
every state tensor are compared at rtol 1e-5 / atol 1e-6 (tests/test_kernels_gpu.py: test_adam_ema_matches_tf_rule).
Sizes: numel < 4 (scalar tail only), numel % 4 in {0, 1, 2, 3}, and 2048 * 256 * 4 + 6 -- one f32x4 more than the
2048-block cap holds in one trip, plus a tail of two."""
import numpy as np
import pytest
import torch

from oracle import pgan_oracle as O
from tests import ewref as R
from tests.ewref import dev

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 4, 5, 1003, 2048 * 256 * 4 + 6]
STEPS, GSCALE, DECAY, LR = 3, 0.5, 0.99, 1e-3
B1, B2 = 0.5, 0.9


def _same(got, ref, what):
    np.testing.assert_allclose(got.double().cpu().numpy(), ref.numpy(), rtol=1e-5, atol=1e-6, err_msg=what)


def _gpu(t):
    return t.float().to(dev())


def _grads(numel):
    return [R.f32_vec(numel, 200 + s) for s in range(STEPS)]


@pytest.mark.parametrize('numel', SIZES)
def test_adam_ema_every_form(numel):
    from saragan_amd import functional as F
    p0, gs = R.f32_vec(numel, 199), _grads(numel)
    # reference: the oracle's Adam and EMA on the scaled gradients, fp64
    params, shadow, opt = {'w': p0.clone()}, {'w': p0.clone()}, O.TFAdam(B1, B2)
    for g in gs:
        opt.apply(params, {'w': g * GSCALE}, LR)
        O.ema_update(shadow, params, DECAY)
    # with EMA, host step size
    p, m, v, ema = _gpu(p0), torch.zeros(numel, device=dev()), torch.zeros(numel, device=dev()), _gpu(p0)
    # with EMA, step size on the device: the same f32 value, the same arithmetic
    pd, md, vd, emad = p.clone(), m.clone(), v.clone(), ema.clone()
    # without EMA
    pn, mn, vn = p.clone(), m.clone(), v.clone()
    for step, g in enumerate(gs, 1):
        gd = _gpu(g)
        F.adam_ema_(p, gd, m, v, ema, LR, B1, B2, step, gscale=GSCALE, ema_decay=DECAY)
        lr_t = torch.tensor([np.float32(F.adam_step_size(LR, B1, B2, step))], device=dev())
        F.adam_ema_(pd, gd, md, vd, emad, 0.0, B1, B2, 0, gscale=GSCALE, ema_decay=DECAY, lr_dev=lr_t)
        F.adam_ema_(pn, gd, mn, vn, None, LR, B1, B2, step, gscale=GSCALE, ema_decay=DECAY)
    for got, ref, what in ((p, params['w'], 'p'), (m, opt.m['w'], 'm'), (v, opt.v['w'], 'v'), (ema, shadow['w'], 'ema')):
        _same(got, ref, what)
    for a, b, what in ((pd, p, 'p'), (md, m, 'm'), (vd, v, 'v'), (emad, ema, 'ema')):
        assert torch.equal(a, b), f'sg_adam_ema_dev differs from sg_adam_ema in {what}'
    for a, b, what in ((pn, p, 'p'), (mn, m, 'm'), (vn, v, 'v')):
        assert torch.equal(a, b), f'ema = NULL changes {what}'
    # EMA-only launch (g = NULL): parameters untouched, the shadow moves
    pe, eme = p.clone(), _gpu(p0)
    F.adam_ema_(pe, None, None, None, eme, LR, B1, B2, 1, ema_decay=DECAY)
    assert torch.equal(pe, p)
    _same(eme, R.ema_rule(p0, p.double().cpu(), DECAY), 'EMA-only')


OPT_CASES = [
    # name, kind, h, eps, nesterov
    ('sgd', 0, 0.0, 0.0, False),
    ('momentum', 1, 0.9, 0.0, False),
    ('nesterov', 1, 0.9, 0.0, True),
    ('adadelta', 2, 0.95, 1e-6, False),
]


@pytest.mark.parametrize('case', OPT_CASES, ids=[c[0] for c in OPT_CASES])
@pytest.mark.parametrize('numel', SIZES)
def test_optim_step_every_rule(numel, case):
    from saragan_amd import functional as F
    name, kind, h, eps, nesterov = case
    lr = 1.0 if name == 'adadelta' else LR * 10      # (Adadelta's own step is ~ sqrt(eps): lr = 1 as its callers use it)
    p0, gs = R.f32_vec(numel, 198), _grads(numel)
    pr, a, a2, sh = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0), p0.clone()
    for g in gs:
        g = g * GSCALE
        if name == 'sgd':
            pr = R.sgd_rule(pr, g, lr)
        elif name == 'adadelta':
            pr, a, a2 = R.adadelta_rule(pr, g, a, a2, lr, h, eps)
        else:
            pr, a = R.momentum_rule(pr, g, a, lr, h, nesterov)
        sh = R.ema_rule(sh, pr, DECAY)

    def state():
        return [_gpu(p0), torch.zeros(numel, device=dev()) if kind >= 1 else None,
                torch.zeros(numel, device=dev()) if kind == 2 else None]
    (p, s1, s2), (pd, s1d, s2d), (pn, s1n, s2n) = state(), state(), state()
    ema, emad = _gpu(p0), _gpu(p0)
    lr_dev = torch.tensor([np.float32(lr)], device=dev())
    for g in gs:
        gd = _gpu(g)
        F.optim_step_(kind, p, gd, s1, s2, ema, lr, h, eps, nesterov, GSCALE, DECAY)
        F.optim_step_(kind, pd, gd, s1d, s2d, emad, 0.0, h, eps, nesterov, GSCALE, DECAY, lr_dev=lr_dev)
        F.optim_step_(kind, pn, gd, s1n, s2n, None, lr, h, eps, nesterov, GSCALE, DECAY)
    _same(p, pr, 'p')
    _same(ema, sh, 'ema')
    if kind >= 1:
        _same(s1, a, 's1')
    if kind == 2:
        _same(s2, a2, 's2')
    for x, y, what in ((pd, p, 'p'), (s1d, s1, 's1'), (s2d, s2, 's2'), (emad, ema, 'ema')):
        assert x is None or torch.equal(x, y), f'sg_optim_step_dev differs from sg_optim_step in {what}'
    for x, y, what in ((pn, p, 'p'), (s1n, s1, 's1'), (s2n, s2, 's2')):
        assert x is None or torch.equal(x, y), f'ema = NULL changes {what}'


def test_optimisers_refuse_unaligned_buffers_without_a_write():
    """SG_EALIGN (-3, not another error) from the host-scalar and the `_dev` entry points when any one of g, p, m / s1,
    v / s2 or ema starts one element past a 16-byte boundary; parameters and state keep their values."""
    from saragan_amd import _lib
    from saragan_amd import functional as F
    n = 1003
    ealign = r'\(code -3\)'
    gu = R.unaligned(R.f32_vec(n, 197).reshape(1, n), torch.float32).reshape(n)
    g = gu.clone()
    assert gu.data_ptr() % 16 != 0 and gu.is_contiguous() and g.data_ptr() % 16 == 0
    bufs = [torch.full((n,), 7.0, device=dev()) for _ in range(4)]
    odd = torch.full((n + 4,), 7.0, device=dev())
    u = odd[1:1 + n]
    assert u.data_ptr() % 16 != 0
    lr_dev = torch.tensor([LR], dtype=torch.float32, device=dev())
    for which in range(5):      # the misaligned argument: g, p, m / s1, v / s2, ema
        p, m, v, ema = [u if which == i + 1 else t for i, t in enumerate(bufs)]
        gg = gu if which == 0 else g
        for dev_form in (None, lr_dev):
            with pytest.raises(_lib.SgError, match=ealign):
                F.adam_ema_(p, gg, m, v, ema, LR, B1, B2, 1, lr_dev=dev_form)
            for kind in (0, 1, 2):
                if (which == 2 and kind == 0) or (which == 3 and kind != 2):
                    continue        # a state tensor the rule does not take is passed as NULL below, not misaligned
                s1, s2 = (m if kind >= 1 else None), (v if kind == 2 else None)
                with pytest.raises(_lib.SgError, match=ealign):
                    F.optim_step_(kind, p, gg, s1, s2, ema, LR, 0.9, 1e-6, lr_dev=dev_form)
    with pytest.raises(_lib.SgError, match=ealign):     # the EMA-only launch
        F.adam_ema_(bufs[0], None, None, None, u, LR, B1, B2, 1)
    torch.cuda.synchronize()
    for b in bufs + [odd]:
        assert bool((b == 7.0).all()), 'a refused call wrote'


# ---------------------------------------------------------------------------------------------------
# sg_segment_sumsq(_flag)
# ---------------------------------------------------------------------------------------------------
OFFSETS = [0, 0, 1, 256, 257, 1000, 70000]      # an empty segment, one element, 255, one element behind a full trip, 743, 69,000


def _seg_ref(flat):
    ref = [float((flat[a:b] ** 2).sum()) for a, b in zip(OFFSETS[:-1], OFFSETS[1:])]
    return np.asarray(ref), [b - a for a, b in zip(OFFSETS[:-1], OFFSETS[1:])]


def _check_segments(got, flat):
    ref, lens = _seg_ref(flat)
    got = got.double().cpu().numpy()
    assert got[0] == 0.0, 'empty segment'
    for i, k in enumerate(lens):
        assert abs(got[i] - ref[i]) <= R.sum_rtol(k) * ref[i], (i, got[i], ref[i])


def test_segment_sumsq_against_fp64():
    from saragan_amd import functional as F
    flat = R.f32_vec(OFFSETS[-1], 196)
    offs = torch.tensor(OFFSETS, dtype=torch.int64, device=dev())
    nseg = len(OFFSETS) - 1
    _check_segments(F.segment_sumsq(_gpu(flat), offs, nseg), flat)
    flag = torch.ones(1, dtype=torch.int32, device=dev())
    _check_segments(F.segment_sumsq(_gpu(flat), offs, nseg, flag=flag), flat)
    assert int(flag.item()) == 0, 'accumulate = 0 clears an earlier flag on finite data'
    flag.fill_(1)
    _check_segments(F.segment_sumsq(_gpu(flat), offs, nseg, flag=flag, accumulate=True), flat)
    assert int(flag.item()) == 1, 'accumulate = 1 keeps an earlier flag'


@pytest.mark.parametrize('bad', [float('nan'), float('-inf')], ids=['nan', 'neginf'])
@pytest.mark.parametrize('seg', [1, 2, 4, 5])
def test_segment_sumsq_flag_sees_the_last_element(seg, bad):
    """A non-finite value in the LAST element of a segment (one-element segment included) sets the flag."""
    from saragan_amd import functional as F
    flat = R.f32_vec(OFFSETS[-1], 195)
    flat[OFFSETS[seg + 1] - 1] = bad
    offs = torch.tensor(OFFSETS, dtype=torch.int64, device=dev())
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    out = F.segment_sumsq(_gpu(flat), offs, len(OFFSETS) - 1, flag=flag).cpu()
    assert int(flag.item()) == 1
    assert not np.isfinite(float(out[seg]))
    others = [i for i in range(len(OFFSETS) - 1) if i != seg]
    assert np.isfinite(out[others].numpy()).all()
    ref, _ = _seg_ref(torch.where(torch.isfinite(flat), flat, 0.0))
    np.testing.assert_allclose(out[others].double().numpy(), ref[others], rtol=R.sum_rtol(69000))


def test_segment_sumsq_overflow_is_not_flagged():
    """Finite values whose squares overflow give an infinite sum and a clear flag (csrc/optim.hip, include/saragan_hip.h)."""
    from saragan_amd import functional as F
    flat = R.f32_vec(OFFSETS[-1], 194)
    flat[257:1000] = 3e38
    offs = torch.tensor(OFFSETS, dtype=torch.int64, device=dev())
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    out = F.segment_sumsq(_gpu(flat), offs, len(OFFSETS) - 1, flag=flag).cpu()
    assert float(out[4]) == float('inf') and int(flag.item()) == 0
