"""LAMBOptimizer / AdamWOptimizer at kernel level (sg_lamb_moments / sg_lamb_ratios / sg_lamb_update, sg_adamw_ema): one flat
buffer of six segments with sentinels in the alignment padding, three steps against the fp64 rules of tests/lamb_rules.py,
frozen-style subsets, run-to-run bits, the device-scalar learning rate and the non-finite guard's three cases."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests.lamb_rules import RULES

pytestmark = pytest.mark.gpu

CHUNK = 4096                      # _lib.SG_SEG_CHUNK (asserted below)
LR, B1, B2, LAM, EMA, GSCALE = 1e-3, 0.5, 0.9, 0.01, 0.99, 0.5
SENTINEL = 7.5
SEGMENTS = OrderedDict([
    ('net/one/weight', 1),                    # smallest segment
    ('net/ragged/weight', 1003),              # numel % 4 == 3
    ('net/zero_w/weight', 37),                # w = 0, g != 0: r = 1 by the |w| = 0 branch (then a normal ratio)
    ('net/zero_u/bias', 20),                  # g = 0, zero moments, no decay: |u| = 0, r = 1, nothing moves
    ('net/live/bias', 130),                   # not decayed, but adapted
    ('net/big/weight', 3 * CHUNK + 5),        # four blocks, the last one ragged: a multi-block norm
])
KINDS = ['LAMB', 'AdamW']
STEPS = 3


def _layout():
    offs, total = OrderedDict(), 0
    for k, n in SEGMENTS.items():
        offs[k] = (total, n)
        total += (n + 3) // 4 * 4
    return offs, total


def _host_state():
    """{p, ema, g[step]} as float32 CPU tensors over the whole flat buffer, sentinels in the padding."""
    offs, total = _layout()
    gen = torch.Generator().manual_seed(11)
    st = {k: torch.full((total,), SENTINEL) for k in ('p', 'ema', 'm', 'v')}
    st['g'] = [torch.full((total,), SENTINEL) for _ in range(STEPS)]
    for name, (o, n) in offs.items():
        st['p'][o:o + n] = 0.0 if 'zero_w' in name else torch.randn(n, generator=gen)
        st['ema'][o:o + n] = torch.randn(n, generator=gen)
        st['m'][o:o + n] = 0.0
        st['v'][o:o + n] = 0.0
        for g in st['g']:
            g[o:o + n] = 0.0 if 'zero_u' in name else torch.randn(n, generator=gen)
    return st


def _pad_mask():
    offs, total = _layout()
    mask = torch.ones(total, dtype=torch.bool)
    for o, n in offs.values():
        mask[o:o + n] = False
    return mask


_REF = {}


def _reference(kind, gscale=GSCALE):
    """Per step {name: (w, m, v, shadow)} in fp64, computed once per rule and gradient scale and shared (never modified)."""
    if (kind, gscale) not in _REF:
        offs, _ = _layout()
        st = _host_state()
        rule = RULES[kind](B1, B2, LAM, 1e-6)
        p = {k: st['p'][o:o + n].double() for k, (o, n) in offs.items()}
        sh = {k: st['ema'][o:o + n].double() for k, (o, n) in offs.items()}
        out = []
        for s in range(STEPS):
            rule.apply(p, {k: st['g'][s][o:o + n].double() * gscale for k, (o, n) in offs.items()}, LR)
            for k in p:
                sh[k] = sh[k] - (1 - EMA) * (sh[k] - p[k])
            out.append({k: (p[k].clone(), rule.m[k].clone(), rule.v[k].clone(), sh[k].clone()) for k in p})
        if kind == 'LAMB':      # the cases the segments are there for
            assert rule.ratios['net/zero_u/bias'] == 1.0 and rule.ratios['net/live/bias'] != 1.0
        _REF[kind, gscale] = out
    return _REF[kind, gscale]


def _make(kind, names=None):
    """(optimizer, flat, ema, ranges) on the device from the seeded host state; ranges cover `names` (default: all) the way
    StepGraph._ranges builds them."""
    import saragan_amd.optimization as opt
    from saragan_amd import _lib
    assert _lib.SG_SEG_CHUNK == CHUNK
    offs, total = _layout()
    st = _host_state()
    o = {'LAMB': opt.LAMBOptimizer, 'AdamW': opt.AdamWOptimizer}[kind](LR, B1, B2, weight_decay_rate=LAM)
    flat = dict(param=st['p'].cuda(), grad=st['g'][0].cuda(), offsets=offs, total=total)
    o._slots('net/', flat, ('m', 'v'))
    o.state['net/']['m'].copy_(st['m'])      # (zero in the segments, sentinels in the padding)
    o.state['net/']['v'].copy_(st['v'])
    runs = []
    for k, (s, n) in offs.items():
        if names is None or k in names:
            npad = (n + 3) // 4 * 4
            if runs and runs[-1][0] + runs[-1][1] == s:
                runs[-1][1] += npad
            else:
                runs.append([s, npad])
    return o, flat, st['ema'].cuda(), [tuple(r) for r in runs], [g.cuda() for g in st['g']]


def _snap(o, flat, ema):
    return dict(p=flat['param'].clone(), m=o.state['net/']['m'].clone(), v=o.state['net/']['v'].clone(), ema=ema.clone())


def _run(kind, steps=STEPS, lr_dev=False, names=None, gscale=GSCALE):
    o, flat, ema, ranges, gs = _make(kind, names)
    lr_t = torch.tensor([LR], device='cuda') if lr_dev else None
    snaps = []
    for s in range(steps):
        flat['grad'].copy_(gs[s])
        o.apply('net/', flat, ranges, gscale, ema, EMA, lr_dev=lr_t)
        snaps.append(_snap(o, flat, ema))
    return o, snaps


def _guard(lr=LR):
    z = lambda n, dt: torch.zeros(n, dtype=dt, device='cuda')
    return dict(flag=z(1, torch.int32), lr_t=z(1, torch.float32), counters=z(3, torch.int64), lr=lr, lr_dev=None)


def _equal(a, b, keys=('p', 'm', 'v', 'ema')):
    for k in keys:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize('kind', KINDS)
def test_three_steps_match_the_fp64_rule_and_leave_the_padding(kind):
    offs, _ = _layout()
    ref = _reference(kind)
    o, snaps = _run(kind)
    pad = _pad_mask().cuda()
    for s, snap in enumerate(snaps):
        for k in ('p', 'm', 'v', 'ema'):
            assert bool((snap[k][pad] == SENTINEL).all()), (s, k)          # bit-unchanged
        for name, (b, n) in offs.items():
            for key, want in zip(('p', 'm', 'v', 'ema'), ref[s][name]):
                np.testing.assert_allclose(snap[key][b:b + n].double().cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-6,
                                           err_msg=f'{kind} step {s} {name} {key}')
    b, n = offs['net/zero_u/bias']
    assert torch.equal(snaps[-1]['p'][b:b + n].cpu(), _host_state()['p'][b:b + n])      # |u| = 0: r = 1, w stays
    assert o.t == STEPS
    if kind == 'LAMB':
        assert o.sync_step_count() == STEPS                                # the device advanced its own count
        tab = next(iter(o.tables.values()))
        assert (tab.nseg, tab.nblocks) == (len(SEGMENTS), len(SEGMENTS) + 3)
    else:
        assert o.t_dev is None                                             # AdamW reads only lr


@pytest.mark.parametrize('gscale', [0.5, 1.0 / 3.0])
@pytest.mark.parametrize('kind', KINDS)
def test_the_gradient_scale_of_n_ranks_enters_as_g_times_gscale(kind, gscale):
    """gscale = 1 / world (the data-parallel average folded into the update): sg_adamw_ema and the sg_lamb_moments /
    sg_lamb_ratios / sg_lamb_update chain against the fp64 rule fed g * gscale formed in fp64 -- 1/3 is no power of two, so a
    kernel that scaled anything but the gradient (m, v and, through u, LAMB's trust-ratio norms) would not round its way back.
    Same segments (vector body, scalar tail, multi-block norm) and tolerances as the test above; and the gscale = 1 rule is
    NOT within them, so the comparison can tell."""
    offs, _ = _layout()
    ref, unscaled = _reference(kind, gscale), _reference(kind, 1.0)
    _, snaps = _run(kind, gscale=gscale)
    pad = _pad_mask().cuda()
    for s, snap in enumerate(snaps):
        for k in ('p', 'm', 'v', 'ema'):
            assert bool((snap[k][pad] == SENTINEL).all()), (s, k)
        for name, (b, n) in offs.items():
            for key, want in zip(('p', 'm', 'v', 'ema'), ref[s][name]):
                np.testing.assert_allclose(snap[key][b:b + n].double().cpu().numpy(), want.numpy(), rtol=1e-5, atol=1e-6,
                                           err_msg=f'{kind} gscale {gscale} step {s} {name} {key}')
    b, n = offs['net/big/weight']
    for key, j in (('m', 1), ('v', 2)):
        got, other = snaps[0][key][b:b + n].double().cpu(), unscaled[0]['net/big/weight'][j]
        assert bool(((got - other).abs() > 1e-6 + 1e-5 * other.abs()).any()), key


@pytest.mark.parametrize('kind', KINDS)
def test_a_subset_of_ranges_updates_only_its_segments(kind):
    """The frozen case: the train op of the new variables only.  Their result is the full run's, bit for bit (a variable's
    arithmetic does not depend on which others share the launch); everything else keeps its bits."""
    offs, _ = _layout()
    names = ['net/ragged/weight', 'net/live/bias', 'net/big/weight']
    _, full = _run(kind, steps=1)
    o, part = _run(kind, steps=1, names=names)
    o0, flat0, ema0, _, _ = _make(kind)
    before = _snap(o0, flat0, ema0)
    for name, (b, n) in offs.items():
        want = full[0] if name in names else before
        for k in ('p', 'm', 'v', 'ema'):
            assert torch.equal(part[0][k][b:b + n], want[k][b:b + n]), (name, k)
    pad = _pad_mask().cuda()
    for k in ('p', 'm', 'v', 'ema'):
        assert bool((part[0][k][pad] == SENTINEL).all()), k
    assert len(o.tables) == 1 and next(iter(o.tables.values())).nseg == len(names)


@pytest.mark.parametrize('kind', KINDS)
def test_two_runs_give_identical_bits(kind):
    _, a = _run(kind)
    _, b = _run(kind)
    for x, y in zip(a, b):
        _equal(x, y)


@pytest.mark.parametrize('kind', KINDS)
def test_device_learning_rate_equals_the_value_form(kind):
    o, a = _run(kind)
    od, b = _run(kind, lr_dev=True)
    for x, y in zip(a, b):
        _equal(x, y)
    assert od.t == 0                       # the captured step's caller counts (next_step_size) ...
    if kind == 'LAMB':
        assert int(od.t_dev) == STEPS      # ... the device counts for itself


@pytest.mark.parametrize('kind', KINDS)
def test_guarded_flag_set_is_ema_only(kind):
    from saragan_amd import functional as F
    offs, _ = _layout()
    o, flat, ema, ranges, gs = _make(kind)
    o.device_step_count('cuda')
    flat['grad'].copy_(gs[0])
    flat['grad'][offs['net/big/weight'][0] + CHUNK + 1] = float('nan')
    before = _snap(o, flat, ema)
    guard = _guard()
    F.nonfinite_flag_(guard['flag'], flat['grad'])
    o.apply('net/', flat, ranges, GSCALE, ema, EMA, guard=guard)
    after = _snap(o, flat, ema)
    _equal(after, before, ('p', 'm', 'v'))
    assert int(o.t_dev) == 0 and guard['counters'].tolist() == [1, 1, 1]
    want = before['ema'].clone()
    for b, n in offs.values():             # the existing EMA-only launch, per segment (it would write the padding)
        F.adam_ema_(before['p'][b:b + n], None, None, None, want[b:b + n], 0.0, 0.0, 0.9, 1, ema_decay=EMA)
    assert torch.equal(after['ema'], want)
    assert not torch.equal(after['ema'], before['ema'])


@pytest.mark.parametrize('kind', KINDS)
def test_guarded_flag_clear_equals_the_unguarded_launch(kind):
    from saragan_amd import functional as F
    _, plain = _run(kind, steps=2)
    o, flat, ema, ranges, gs = _make(kind)
    o.device_step_count('cuda')
    guard = _guard()
    for s in range(2):
        flat['grad'].copy_(gs[s])
        F.nonfinite_flag_(guard['flag'], flat['grad'])
        assert int(guard['flag']) == 0
        o.apply('net/', flat, ranges, GSCALE, ema, EMA, guard=guard)
        _equal(_snap(o, flat, ema), plain[s])
    assert int(o.t_dev) == 2 and guard['counters'].tolist() == [0, 0, 0]


@pytest.mark.parametrize('kind', KINDS)
def test_guarded_ok_skip_ok_equals_two_unguarded_steps(kind):
    """t counts APPLIED updates: [ok, skip, ok] is the unguarded updates at t = 1, 2 with the skipped step's EMA between."""
    from saragan_amd import functional as F
    offs, _ = _layout()
    o, flat, ema, ranges, gs = _make(kind)
    o.device_step_count('cuda')
    guard = _guard()
    for s, bad in ((0, False), (1, True), (2, False)):
        flat['grad'].copy_(gs[s])
        guard['flag'].fill_(1 if bad else 0)      # (what sg_nonfinite_flag would leave)
        o.apply('net/', flat, ranges, GSCALE, ema, EMA, guard=guard)
    got = _snap(o, flat, ema)
    assert int(o.t_dev) == 2 and guard['counters'].tolist() == [1, 0, 1]
    assert o.sync_step_count() == 2
    r, rflat, rema, _, _ = _make(kind)
    for s in (0, 1, 2):
        if s == 1:
            for b, n in offs.values():
                F.adam_ema_(rflat['param'][b:b + n], None, None, None, rema[b:b + n], 0.0, 0.0, 0.9, 1, ema_decay=EMA)
            continue
        rflat['grad'].copy_(gs[s])
        r.apply('net/', rflat, ranges, GSCALE, rema, EMA)
    _equal(got, _snap(r, rflat, rema))


@pytest.mark.parametrize('kind', KINDS)
def test_no_ema_form_moves_the_weights_only(kind):
    """The Adasum delta form calls apply with no shadow."""
    o, flat, ema, ranges, gs = _make(kind)
    _, want = _run(kind, steps=1)
    o.apply('net/', flat, ranges, GSCALE, None, 0.0)
    _equal(_snap(o, flat, ema), want[0], ('p', 'm', 'v'))


def test_launch_count_does_not_depend_on_the_number_of_variables(monkeypatch):
    """LAMB: three launches per train op (+ the guard's bookkeeping thread), AdamW: one -- for six variables or three."""
    from saragan_amd import functional as F
    lib = F._lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith('sg_') or name == 'sg_prof_enabled':
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    for kind, want in (('LAMB', ['sg_lamb_moments', 'sg_lamb_ratios', 'sg_lamb_update']), ('AdamW', ['sg_adamw_ema'])):
        for names in (None, ['net/ragged/weight', 'net/live/bias', 'net/big/weight']):
            o, flat, ema, ranges, gs = _make(kind, names)
            o.device_step_count('cuda')
            guard = _guard()
            o.apply('net/', flat, ranges, GSCALE, ema, EMA)            # (tables and step count exist from here on)
            with monkeypatch.context() as mp:
                mp.setattr(F._lib, 'load', lambda: Counting())
                o.apply('net/', flat, ranges, GSCALE, ema, EMA)
                assert calls == want, (kind, names, calls)
                del calls[:]
                o.apply('net/', flat, ranges, GSCALE, ema, EMA, guard=guard)
                assert calls == ['sg_guard_step'] + want, (kind, names, calls)
                del calls[:]
