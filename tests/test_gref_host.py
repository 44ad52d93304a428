"""tests/gref.py checked on the host.  (1) Each restatement is the derivative it claims: against fp64 autograd through a plain
composition of oracle.pgan_oracle ops.  (2) Every tier-1 case of tests/test_autograd_gen_exact_gpu.py stays inside the exact range
with representable stored intermediates, every tier-2 case has exact integer incoming gradients and K <= 2048 in every toleranced
sum.  (3) The bounds have teeth: a correct route emulated in f32 (another order of summation, one bf16 rounding) passes, and each
of a list of subtly wrong kernels is rejected."""
import pytest
import torch

from oracle import pgan_oracle as O
from tests import agref as A
from tests import fwdref as R
from tests import gref as G
from tests import wgref as W

BF, F32, SLOPE = G.BF, G.F32, G.SLOPE


def _var(q, act='leaky_relu'):
    """The fp64 variable whose effective filter under the oracle's He constant is q (to 1 ulp)."""
    coef = O.runtime_coef(q.shape, act, SLOPE if act == 'leaky_relu' else None)
    return (q.double() / coef).requires_grad_(True), coef


def _close(got, ref, what):
    torch.testing.assert_close(got.detach().double().reshape(ref.shape), ref.double(), rtol=1e-11, atol=1e-9, msg=lambda m: f'{what}: {m}')


def _oracle_stage(x, wv, b, ups):
    h = O.upscale3d(x) if ups else x
    return O.pixel_norm(O.act(O.apply_bias(O.conv3d(h, wv, 'leaky_relu', SLOPE), b), 'leaky_relu', SLOPE))


# ---------------------------------------------------------------------------------------------------------------------------
# 1. the restatements are the derivatives
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ups', [False, True], ids=['plain', 'ups'])
@pytest.mark.parametrize('consumers', ['gy', 'conv', 'rgb', 'rgb+gy'])
def test_stage_restatement_is_the_fp64_derivative(ups, consumers):
    """One pixel-norm stage with (a) a direct output gradient, (b) a plain conv consumer, (c) to_rgb, (d) to_rgb and a direct
    gradient: pn_act_bwd on the EXACT y and scale, then behind_dz / rgb_backward, are what autograd finds."""
    c = G.Stage('host', 2, 8, 16, (2, 4, 8), ups=ups, seed=77)
    d = G.stage_data(c)
    d['b1'] = d['b1'] + 0.5          # (keeps every pre-activation off zero: the oracle's filter is q to one fp64 ulp)
    x = d['x'].double().requires_grad_(True)
    w1, c1 = _var(d['q1'])
    b1 = d['b1'].double().requires_grad_(True)
    y = _oracle_stage(x, w1, b1, ups)
    a, y_ref, s, words = G.stage_forward(d['x'].double(), d['q1'].double(), d['b1'].double(), ups=ups)
    _close(y, y_ref, 'y')
    leaves, outs, gouts = [x, w1, b1], [], []
    g = torch.zeros_like(y_ref)
    if consumers == 'conv':
        w2, c2 = _var(d['q2'], 'linear')
        b2 = d['b2'].double().requires_grad_(True)
        outs.append(O.apply_bias(O.conv3d(y, w2, 'linear'), b2)), gouts.append(d['gy2'].double()), leaves.extend([w2, b2])
        g = g + R.dgrad_ref(d['gy2'].double(), d['q2'].double())
    if consumers in ('rgb', 'rgb+gy'):
        wr, cr = _var(d['q_rgb'], 'linear')
        br = d['b_rgb'].double().requires_grad_(True)
        outs.append(O.apply_bias(O.conv3d(y, wr, 'linear'), br)), gouts.append(d['g_img'].double()), leaves.extend([wr, br])
        gy_rgb, sw_rgb, _, sb_rgb = G.rgb_backward(y_ref, d['q_rgb'].reshape(-1), d['g_img'])
        _close(outs[-1], G.rgb_forward(y_ref, d['q_rgb'].reshape(-1), 2.0), 'img')
        g = g + gy_rgb
    if consumers in ('gy', 'rgb+gy'):
        outs.append(y), gouts.append(d['gy'].double())
        g = g + d['gy'].double()
    got = torch.autograd.grad(outs, leaves, gouts)
    dz, _ = G.pn_act_bwd(g, y_ref, s, words)
    b = G.behind_dz(d['x'], d['q1'], dz, ups=ups)
    _close(got[0], b['gx'], 'gx')
    _close(got[1], b['sw'] * c1, 'gw')
    _close(got[2], b['sb'], 'gb')
    if consumers == 'conv':
        sw2, sb2 = W.wgrad_ref(y_ref, d['gy2'].double(), G.K333)
        _close(got[3], sw2 * c2, 'gw2')
        _close(got[4], sb2, 'gb2')
    if consumers in ('rgb', 'rgb+gy'):
        _close(got[3], sw_rgb * cr, 'gw_rgb')
        _close(got[4], sb_rgb, 'gb_rgb')


def test_pixel_norm_alone_restatement_is_the_fp64_derivative():
    """words None: the backward of pixel_norm as its own pass (the wide stage)."""
    x = A.ints((2, 16, 2, 4, 8), 7801, F32).double().requires_grad_(True)
    y = O.pixel_norm(x)
    g = A.ints((2, 16, 2, 4, 8), 7802, F32).double()
    (gx,) = torch.autograd.grad(y, x, g)
    yr, s = R.pixel_norm(x.detach(), G.EPS)
    _close(gx, G.pn_act_bwd(g, yr, s, None)[0], 'pixel_norm backward')


@pytest.mark.parametrize('act', [False, True], ids=['conv', 'conv_bias_act'])
def test_upsampled_node_reference_is_the_fp64_derivative(act):
    c = G.Up('host', 'generic', BF, 2, 8, 16, (2, 4, 8), 'in', 0.25, seed=78)
    d = G.up_data(c)
    d['b'] = d['b'] + 0.5
    ref = G.up_reference(c, d, act)
    x = d['x'].double().requires_grad_(True)
    wv, coef = _var(d['q'])
    b = d['b'].double().requires_grad_(True)
    y = O.conv3d(O.upscale3d(x), wv, 'leaky_relu', SLOPE)
    if act:
        y = O.act(O.apply_bias(y, b), 'leaky_relu', SLOPE)
    _close(y, ref['y'], 'y')
    got = torch.autograd.grad(y, [x, wv] + ([b] if act else []), d['gy'].double())
    _close(got[0], ref['gx'], 'gx')
    _close(got[1], ref['sw'] * coef, 'gw')
    if act:
        _close(got[2], ref['sb'], 'gb')


@pytest.mark.parametrize('c', G.MIX_CASES, ids=repr)
def test_mixing_branch_reference_is_the_fp64_derivative(c):
    d = G.mix_data(c)
    ref = G.mix_reference(c, d)
    x, x2 = d['x'].double().requires_grad_(True), d['x2'].double().requires_grad_(True)
    wa, ca = _var(d['qa'], 'linear')
    wb, cb = _var(d['qb'], 'linear')
    ba, bb = d['ba'].double().requires_grad_(True), d['bb'].double().requires_grad_(True)
    a = O.apply_bias(O.conv3d(x, wa, 'linear'), ba)
    b = O.apply_bias(O.conv3d(x2, wb, 'linear'), bb)
    y = c.alpha * O.upscale3d(a) + (1 - c.alpha) * b
    _close(y, ref['y'], 'y')
    got = torch.autograd.grad(y, [x, x2, wa, ba, wb, bb], d['g'].double())
    for t, r, nm in zip(got, (ref['gx'], ref['gx2'], ref['swa'] * ca, ref['sba'], ref['swb'] * cb, ref['sbb']), ('gx', 'gx2', 'gwa', 'gba', 'gwb', 'gbb')):
        _close(t, r, nm)


def test_dense_head_reference_is_the_fp64_derivative():
    c = G.HEAD
    d = G.head_data(c)
    d['b'] = d['b'] + 0.5
    ref = G.head_reference(c, d)
    z = d['z'].double().requires_grad_(True)
    wv, coef = _var(d['q'])
    b = d['b'].double().requires_grad_(True)
    w2, c2 = _var(d['q2'], 'linear')
    h = O.act(O.apply_bias(O.dense(z, wv, 'leaky_relu', SLOPE), b), 'leaky_relu', SLOPE)
    _close(h, ref['h'], 'h')
    y = O.conv3d(h.reshape(c.n, c.c, *c.sp), w2, 'linear')
    _close(y, ref['y'], 'y')
    gz, gw, gb, gw2 = torch.autograd.grad(y, [z, wv, b, w2], d['gy'].double())
    _close(gz, ref['gz'], 'gz')
    _close(gw, ref['sw'] * coef, 'gw')
    _close(gb, ref['sb'], 'gb')
    _close(gw2, ref['sw2'] * c2, 'gw2')


# ---------------------------------------------------------------------------------------------------------------------------
# 2. the cases keep their conditions
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', G.STAGES, ids=repr)
def test_tier2_cases_have_integer_gradients_and_short_sums(c):
    ks = G.stage_conditions(c, G.stage_data(c))
    assert max(ks.values()) <= G.KMAX


@pytest.mark.parametrize('c', G.UP_CASES, ids=repr)
def test_tier1_upsampled_cases_stay_exact(c):
    """The full shape where it is small; for the 2^18 .. 2^20-voxel shapes of the pooled routes the voxel sums' range at the
    full shape (it depends on the gradient's density alone) and everything else on the leading (2, 8, 32) low-resolution corner."""
    d = G.up_data(c)
    big = c.n * c.fine[0] * c.fine[1] * c.fine[2] > 1 << 16
    if big:
        A.assert_wgrad_range(d['x'], d['gy'])
        lo = (min(c.sp[0], 2), 8, 32)
        d['x'] = d['x'][:1, :, :lo[0], :lo[1], :lo[2]].contiguous(memory_format=torch.channels_last_3d)
        d['gy'] = d['gy'][:1, :, :2 * lo[0], :2 * lo[1], :2 * lo[2]].contiguous(memory_format=torch.channels_last_3d)
    for act in ((False,) if big else (False, True)):
        ref = G.up_reference(c, d, act)
        R.expected(ref['gx'], c.dtype), W.scaled(ref['sw'], c.coef)
    A.q_over_coef(d['q'], c.coef, c.dtype)


def test_tier1_mixing_and_head_cases_stay_exact():
    for c in G.MIX_CASES:
        d = G.mix_data(c)
        ref = G.mix_reference(c, d)
        for k in ('gx', 'gx2'):
            R.expected(ref[k], BF)
        A.q_over_coef(d['qa'], G.RGB_COEF, BF), A.q_over_coef(d['qb'], G.RGB_COEF, BF)
    d = G.head_data(G.HEAD)
    ref = G.head_reference(G.HEAD, d)
    R.expected(ref['gz'], BF), R.expected(ref['y'], BF)
    A.q_over_coef(d['q'], G.HEAD.coef, BF)


# ---------------------------------------------------------------------------------------------------------------------------
# 3. the bounds have teeth
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def stored_stage():
    """The 32 -> 32 stage as a GPU run leaves it: y rounded to bf16, scale to f32, the sign words; g = g_img (x) q_rgb + gy."""
    c = G.S32
    d = G.stage_data(c)
    a, y, s, words = G.stage_forward(d['x'].double(), d['q1'].double(), d['b1'].double())
    ys, ss = y.float().to(BF), s.float().reshape(-1)
    g_rgb = G.rgb_backward(ys, d['q_rgb'].reshape(-1), d['g_img'])[0]
    return c, d, ys, ss, words, g_rgb


def _dz_bound(g, ys, ss, words, c):
    ref, t = G.pn_act_bwd(g, ys, ss, words)
    return ref, t, G.pn_bwd_bound(ref, t, G.PN_BWD_ROUNDINGS['pass'](c.c))


def test_emulated_correct_routes_pass(stored_stage):
    c, d, ys, ss, words, g_rgb = stored_stage
    g = g_rgb + d['gy'].double()
    ref, t, bound = _dz_bound(g, ys, ss, words, c)
    dz = G.emulate_pn_act_bwd(g, ys, ss, words)
    assert G.within(dz, ref, bound), G.excess(dz, ref, bound)
    # the two-pass route: pixel_norm backward stored in bf16, then the mask (a power of two)
    two = R.apply_mask(G.emulate_pn_act_bwd(g, ys, ss, R.sign_words(torch.ones_like(ref))).float(), words, SLOPE).to(BF)
    assert G.within(two, ref, bound)
    assert G.excess(dz, ref, G.pn_bwd_bound(ref, t, G.PN_BWD_ROUNDINGS['epilogue'](c.c))) <= 1.0
    # behind the stored dz: filter and bias gradient, summed in f32 in another order
    b = G.behind_dz(d['x'], d['q1'], dz)
    sw32 = G.emulate_voxel_sum(d['x'], dz, G.K333)
    G.check_w(W.scaled(sw32.double(), c.coef), b['sw'], b['sw_abs'], b['k'], c.coef, 'gw')
    sb32 = dz.float().permute(0, 2, 3, 4, 1).reshape(-1, c.c).flip(0).sum(0)
    G.check(sb32, b['sb'], G.sum_bound(b['sb_abs'], b['k']), 'gb over the stored dz')
    unrounded = G.emulate_pn_act_bwd(g, ys, ss, words, round_to=None)
    G.check_gb_in_register(unrounded.permute(0, 2, 3, 4, 1).reshape(-1, c.c).flip(0).sum(0), ref, t, c.c, 'gb in registers')
    gx32 = R.dgrad_ref(dz.double(), d['q1'].double()).float().to(BF)
    G.check(gx32, b['gx'], b['gx_bound'], 'gx')


def test_wrong_kernels_are_rejected(stored_stage):
    c, d, ys, ss, words, g_rgb = stored_stage
    g = g_rgb + d['gy'].double()
    ref, t, bound = _dz_bound(g, ys, ss, words, c)

    def rejected(dz, what):
        assert not G.within(dz, ref, bound), f'{what}: not rejected'

    rejected(G.emulate_pn_act_bwd(g, ys, ss, words, channels=c.c - 1), 'mean_c over C - 1 channels')
    rejected(G.emulate_pn_act_bwd(g, ys, ss.roll(1), words), 'the neighbouring voxel\'s scale')
    # slope 0.2 instead of 1/4 on ONE voxel (the first one with a masked, non-zero element)
    good = G.emulate_pn_act_bwd(g, ys, ss, words)
    bits = R.word_bits(words, c.n, c.c, c.sp)
    hit = (bits & (good.double() != 0)).permute(0, 2, 3, 4, 1).reshape(-1, c.c).any(1).nonzero()[0, 0]
    raw = G.emulate_pn_act_bwd(g, ys, ss, R.sign_words(torch.ones_like(ref)), round_to=None)
    one = good.clone().permute(0, 2, 3, 4, 1).reshape(-1, c.c)
    one[hit] = torch.where(bits.permute(0, 2, 3, 4, 1).reshape(-1, c.c)[hit], raw.permute(0, 2, 3, 4, 1).reshape(-1, c.c)[hit] * 0.2,
                           raw.permute(0, 2, 3, 4, 1).reshape(-1, c.c)[hit]).to(BF)
    rejected(one.reshape(c.n, *c.sp, c.c).permute(0, 4, 1, 2, 3), 'slope 0.2 on one voxel')
    rejected(G.emulate_pn_act_bwd(g, ys, ss, words, mask_words=R.sign_words(g)), 'the mask of gy instead of y')
    # g_y dropped where both consumers send a gradient
    rejected(G.emulate_pn_act_bwd(g_rgb, ys, ss, words), 'g_y dropped')
    # behind dz
    b = G.behind_dz(d['x'], d['q1'], good)
    missing = W.scaled(G.emulate_voxel_sum(d['x'], good, G.K333, skip=137).double(), c.coef)
    assert not G.within(missing, c.coef * b['sw'], G.wgrad_bound(b['sw'], b['sw_abs'], b['k'], c.coef)), 'one voxel missing from a filter gradient'
    unmasked = G.emulate_pn_act_bwd(g, ys, ss, R.sign_words(torch.ones_like(ref)))
    early = unmasked.float().permute(0, 2, 3, 4, 1).reshape(-1, c.c).sum(0)
    assert not G.within(early, b['sb'], G.sum_bound(b['sb_abs'], b['k'])), 'the bias gradient summed before the mask (stored dz)'
    bound_reg = (G.PN_BWD_ROUNDINGS['pass'](c.c) * G.U * t).sum((0, 2, 3, 4)) + G.sum_bound(ref.abs().sum((0, 2, 3, 4)), b['k'])
    assert not G.within(early, ref.sum((0, 2, 3, 4)), bound_reg), 'the bias gradient summed before the mask (in registers)'


def test_forward_and_rgb_bounds_have_teeth(stored_stage):
    """The shared forward bound accepts the stored y and rejects a pixel norm over 31 of 32 channels; the rgb bound accepts an f32
    head in another order and rejects one that drops a channel."""
    c, d, ys, ss, words, _ = stored_stage
    a = G.stage_forward(d['x'].double(), d['q1'].double(), d['b1'].double())[0]
    G.pn_check('stored', ys, ss, a, BF, c.c)
    wrong = (a * torch.rsqrt((a[:, :-1] ** 2).sum(1, keepdim=True) / c.c + G.EPS)).float().to(BF)
    with pytest.raises(AssertionError):
        G.pn_check('31 channels', wrong, None, a, BF, c.c)
    q = d['q_rgb'].reshape(-1)
    ref = G.rgb_forward(ys, q, 2.0)
    img = ((ys.float() * q.reshape(1, -1, 1, 1, 1)).flip(1).sum(1, keepdim=True) + 2.0).to(BF)
    assert G.within(img, ref, G.rgb_bound(ys, q, 2.0, ref))
    nz = int(q.nonzero()[0, 0])
    q_bad = q.clone()
    q_bad[nz] = 0
    bad = ((ys.float() * q_bad.reshape(1, -1, 1, 1, 1)).sum(1, keepdim=True) + 2.0).to(BF)
    assert not G.within(bad, ref, G.rgb_bound(ys, q, 2.0, ref))
