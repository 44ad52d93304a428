"""Minibatch standard deviation on the device (csrc/mbstd.hip through functional.mbstd_stat / mbstd_term / mbstd_plane) against the
fp64 statements of tests/mbstdref.py, and the 3-D pgan discriminator with the layer on (networks.ops.set_minibatch_stddev) against
the oracle architecture that helper registers: logits, losses, penalty and every D gradient of a step, the batched D pass against
separate passes, a captured step against eager ones, the default-off path, the combination with spectral normalisation and the
training loop's hand-over and restore.

Inputs are drawn in fp64 and rounded to the storage type first (tests/ewref.py).  Tolerances: ewref.tol for stored tensors,
ewref.assert_sum_close for the f32 sums with k = the number of terms of the sum (P for the statistic, P * G for ggstat, the plane
for the term's dot product, n for its outer product, positions * n for the filter gradient)."""
import os

import numpy as np
import pytest
import torch

from tests import ewref as R
from tests import mbstdref as M

pytestmark = pytest.mark.gpu

# n, c, (d, h, w), group, nseg, seed, why
KERNEL_CASES = [
    (8, 16, (1, 4, 4), 4, 1, 11, 'base case'),
    (8, 16, (2, 4, 4), 4, 2, 12, 'two segments'),
    (2, 8, (1, 4, 4), 4, 1, 55, 'G = 2, M = 1: the batch is smaller than the group'),
    (12, 24, (1, 4, 4), 4, 1, 14, 'M = 3: the members of a group are three samples apart'),
    (4, 20, (1, 3, 5), 4, 1, 15, 'P = 300: a ragged last block, c is not a multiple of a 16-byte piece'),
    (4, 512, (2, 4, 4), 4, 1, 16, 'P = 16384: 64 blocks of partial sums per group'),
]
KERNEL_IDS = ['base', 'segments', 'g2m1', 'm3', 'ragged-p300', 'p16384']
MIN_SIGMA = 0.02
_REF = {}


def _case(i, dtype):
    """Inputs (fp64 values representable in dtype) and the fp64 results of case i, computed once and never modified."""
    key = (i, dtype)
    if key not in _REF:
        n, c, ext, group, nseg, seed, _ = KERNEL_CASES[i]
        x = R.rnd((n, c, *ext), seed, dtype)
        gstat = R.rnd((n,), seed + 100, torch.float32)
        h = R.rnd((n, c, *ext), seed + 200, dtype)
        stat, stat_abs = M.stat(x, group, nseg)
        gg, gg_abs, gx = M.stat_bwd2(h, x, gstat, group, nseg)
        _REF[key] = dict(x=x, gstat=gstat, h=h, stat=stat, stat_abs=stat_abs, dx=M.stat_bwd(gstat, x, group, nseg), gg=gg,
                         gg_abs=gg_abs, gx=gx, min_sigma=M.min_sigma(x, group, nseg))
    return _REF[key]


def _run_stat(x, gstat, h, group, nseg, dtype):
    """(stat, dx, ggstat, gx) from the device through autograd: forward, backward, backward of the backward."""
    from saragan_amd import functional as F
    xg = R.cl(x, dtype).requires_grad_(True)
    gs = gstat.float().to(R.dev()).requires_grad_(True)
    s = F.mbstd_stat(xg, group, nseg)
    (dx,) = torch.autograd.grad(s, xg, gs, create_graph=True)
    ggstat, gx = torch.autograd.grad(dx, [gs, xg], R.cl(h, dtype))
    return s.detach(), dx.detach(), ggstat, gx


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
@pytest.mark.parametrize('i', range(len(KERNEL_CASES)), ids=KERNEL_IDS)
def test_statistic_and_both_gradients_match_the_closed_forms(i, dtype):
    n, c, ext, group, nseg, _, why = KERNEL_CASES[i]
    ref = _case(i, dtype)
    assert ref['min_sigma'] >= MIN_SIGMA, (why, ref['min_sigma'])      # 1 / sigma amplification is not what is measured here
    P, G = c * int(np.prod(ext)), min(group, n // nseg)
    s, dx, ggstat, gx = _run_stat(ref['x'], ref['gstat'], ref['h'], group, nseg, dtype)
    assert s.dtype == torch.float32 and tuple(s.shape) == (n,) and ggstat.dtype == torch.float32 and dx.dtype == dtype
    R.assert_sum_close(s, ref['stat'], ref['stat_abs'], P, why + ': stat')
    R.close(dx, ref['dx'], dtype, why + ': dx')
    R.assert_sum_close(ggstat, ref['gg'], ref['gg_abs'], P * G, why + ': ggstat')
    R.close(gx, ref['gx'], dtype, why + ': gx')


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
def test_two_segments_are_bit_equal_to_two_calls_on_the_halves(dtype):
    n, c, ext, group, nseg, _, _ = KERNEL_CASES[1]
    ref = _case(1, dtype)
    both = _run_stat(ref['x'], ref['gstat'], ref['h'], group, 2, dtype)
    half = n // 2
    lo = _run_stat(ref['x'][:half], ref['gstat'][:half], ref['h'][:half], group, 1, dtype)
    hi = _run_stat(ref['x'][half:], ref['gstat'][half:], ref['h'][half:], group, 1, dtype)
    for name, b, l, h_ in zip(('stat', 'dx', 'ggstat', 'gx'), both, lo, hi):
        assert torch.equal(b, torch.cat([l, h_], dim=0)), name
    one = _run_stat(ref['x'], ref['gstat'], ref['h'], group, 1, dtype)      # one segment groups the samples m, m + 2, ... instead
    assert not torch.equal(one[0], both[0])


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
def test_a_group_of_one_has_the_floor_statistic_and_no_gradient(dtype):
    """1,8,(1,4,4),4,1: G = 1, every deviation is zero: stat = sqrt(1e-8) = 1e-4, dx = 0, and so are both second-order outputs."""
    x, gstat, h = R.rnd((1, 8, 1, 4, 4), 21, dtype), R.rnd((1,), 22, torch.float32), R.rnd((1, 8, 1, 4, 4), 23, dtype)
    s, dx, ggstat, gx = _run_stat(x, gstat, h, 4, 1, dtype)
    R.assert_sum_close(s, torch.full((1,), 1e-4, dtype=torch.float64), torch.full((1,), 1e-4, dtype=torch.float64), 128, 'stat')
    assert torch.count_nonzero(dx) == 0 and torch.count_nonzero(gx) == 0 and torch.count_nonzero(ggstat) == 0


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
@pytest.mark.parametrize('copies', [4, 2])
def test_identical_samples_have_zero_variance_exactly(copies, dtype):
    """A group of four identical samples, and one of two: a + a and (a + a) + (a + a) are exact in f32, so the mean is a, every
    deviation 0 and dx exactly 0; the second-order outputs are finite and equal the closed form (sigma = 1e-4 everywhere)."""
    a = R.rnd((1, 8, 1, 4, 4), 31, dtype)
    x = a.expand(copies, -1, -1, -1, -1).contiguous()
    gstat, h = R.rnd((copies,), 32, torch.float32), R.rnd(tuple(x.shape), 33, dtype)
    s, dx, ggstat, gx = _run_stat(x, gstat, h, 4, 1, dtype)
    assert torch.count_nonzero(dx) == 0
    want_gg, gg_abs, want_gx = M.stat_bwd2(h, x, gstat, 4)
    assert float(want_gg.abs().max()) == 0 and float(gg_abs.abs().max()) == 0
    assert torch.count_nonzero(ggstat) == 0
    assert torch.isfinite(gx).all() and float(want_gx.abs().max()) > 0
    R.close(gx, want_gx, dtype, 'gx at zero variance')
    R.assert_sum_close(s, torch.full((copies,), 1e-4, dtype=torch.float64), torch.full((copies,), 1e-4, dtype=torch.float64), 128)


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
def test_bad_arguments_are_refused_before_any_launch(dtype):
    """6,8,(1,4,4),4,1: the group does not divide the batch.  Also n not divisible by nseg and null pointers: SG_EINVAL from
    every entry point, the outputs untouched."""
    import ctypes as C
    from saragan_amd import _lib
    from saragan_amd import functional as F
    lib = _lib.load()
    x = R.cl(R.rnd((6, 8, 1, 4, 4), 41, dtype), dtype)
    with pytest.raises(_lib.SgError):
        F.mbstd_stat(x, 4, 1)
    with pytest.raises(_lib.SgError):
        F.mbstd_stat(R.cl(R.rnd((8, 8, 1, 4, 4), 42, dtype), dtype), 4, 3)
    dt = _lib.SG_F32 if dtype == torch.float32 else _lib.SG_BF16
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    SENT = 7.5
    stat = torch.full((8,), SENT, device='cuda')
    ws = torch.full((64,), SENT, device='cuda')
    out = torch.full_like(x, SENT)
    p = lambda t: C.c_void_p(t.data_ptr())
    for n, group, nseg in ((6, 4, 1), (8, 4, 3), (6, 2, 4)):
        assert lib.sg_mbstd_stat_workspace(n, 16, 8, group, nseg) == 0
        assert lib.sg_mbstd_stat_fwd(p(x), p(stat), p(ws), 256, n, 16, 8, group, nseg, dt, st) == -1
        assert lib.sg_mbstd_stat_bwd(p(stat), p(x), p(out), n, 16, 8, group, nseg, dt, st) == -1
        assert lib.sg_mbstd_stat_bwd2(p(x), p(x), p(stat), p(out), p(stat), p(ws), 256, n, 16, 8, group, nseg, dt, st) == -1
    assert lib.sg_mbstd_stat_fwd(None, p(stat), p(ws), 256, 4, 16, 8, 4, 1, dt, st) == -1
    assert lib.sg_mbstd_stat_fwd(p(x), None, p(ws), 256, 4, 16, 8, 4, 1, dt, st) == -1
    assert lib.sg_mbstd_stat_fwd(p(x), p(stat), p(ws), 0, 4, 16, 8, 4, 1, dt, st) == -1          # workspace too small
    assert lib.sg_mbstd_stat_bwd(None, p(x), p(out), 4, 16, 8, 4, 1, dt, st) == -1
    assert lib.sg_mbstd_stat_bwd2(p(x), p(x), p(stat), None, None, p(ws), 256, 4, 16, 8, 4, 1, dt, st) == -1
    assert lib.sg_mbstd_term_fwd(p(x), None, p(ws), p(out), 4, 16, dt, st) == -1
    assert lib.sg_mbstd_term_dot(p(x), p(ws), None, 4, 16, dt, st) == -1
    assert lib.sg_mbstd_term_outer(p(stat), p(x), None, 4, 16, dt, st) == -1
    assert lib.sg_mbstd_term_fwd(p(x), p(stat), p(ws), p(out), 0, 16, dt, st) == -1
    torch.cuda.synchronize()
    for t in (stat, ws, out):
        assert bool((t == SENT).all())


# ---- the term kernels ------------------------------------------------------------------------------------------------------------
TERM_N, TERM_EXT, TERM_COEF = 3, (2, 4, 4), 0.0625


def _term_inputs(cout, k, dtype):
    shape = (TERM_N, cout, *TERM_EXT)
    return dict(y=R.rnd(shape, 51, dtype), s=R.rnd((TERM_N,), 52, torch.float32), w=R.rnd((*k, 1, cout), 53, torch.float32),
                gout=R.rnd(shape, 54, dtype), a=R.rnd((TERM_N,), 55, torch.float32), b=R.rnd((*k, 1, cout), 56, torch.float32))


def _run_term(t, dtype):
    """The device's first- and second-order results: out, (gy, gs, gw) for the cotangent gout of out, and the gradients of
    L = <gs, a> + <gw, b> for gout, s and w -- every one of the six Function edges runs."""
    from saragan_amd import functional as F
    dev = R.dev()
    y, gout = R.cl(t['y'], dtype).requires_grad_(True), R.cl(t['gout'], dtype).requires_grad_(True)
    s, w = t['s'].float().to(dev).requires_grad_(True), t['w'].float().to(dev).requires_grad_(True)
    B = F.mbstd_plane(w, TERM_COEF, TERM_EXT)
    out = F.mbstd_term(y, s, B)
    gy, gs, gw = torch.autograd.grad(out, [y, s, w], gout, create_graph=True)
    L = (gs * t['a'].float().to(dev)).sum() + (gw * t['b'].float().to(dev)).sum()
    l_gout, l_s, l_w = torch.autograd.grad(L, [gout, s, w])
    return dict(B=B.detach(), out=out.detach(), gy=gy.detach(), gs=gs.detach(), gw=gw.detach(), l_gout=l_gout, l_s=l_s, l_w=l_w,
                gout=gout.detach())


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
@pytest.mark.parametrize('k', [(3, 3, 3), (1, 3, 3)], ids=['k333', 'k133'])
@pytest.mark.parametrize('cout', [24, 512])
def test_term_kernels_match_the_helper_at_every_order(cout, k, dtype):
    t = _term_inputs(cout, k, dtype)
    got = _run_term(t, dtype)
    plane_n, pos, taps = cout * int(np.prod(TERM_EXT)), int(np.prod(TERM_EXT)), int(np.prod(k))
    B = M.plane(t['w'], TERM_COEF, TERM_EXT)
    R.assert_sum_close(got['B'], B, M.plane(t['w'].abs(), TERM_COEF, TERM_EXT), taps, 'B')
    R.close(got['out'], M.term(t['y'], t['s'], B), dtype, 'out')
    assert torch.equal(got['gy'], got['gout'])                                      # the term passes y's gradient through
    gs, gs_abs = M.dot(t['gout'], B)
    R.assert_sum_close(got['gs'], gs, gs_abs, plane_n, 'gs')
    Bg, Bg_abs = M.outer(t['s'], t['gout'])
    R.assert_sum_close(got['gw'], M.plane_t(Bg, TERM_COEF, k), M.plane_t(Bg_abs, TERM_COEF, k), pos * TERM_N, 'gw')
    # second order, L = <gs, a> + <gw, b>:  gs = <gout, B(w)>,  gw = plane_t(sum_n s_n gout[n])
    Bb = M.plane(t['b'], TERM_COEF, TERM_EXT)
    want = t['a'].reshape(-1, 1, 1, 1, 1) * B.permute(3, 0, 1, 2).unsqueeze(0) + \
        t['s'].reshape(-1, 1, 1, 1, 1) * Bb.permute(3, 0, 1, 2).unsqueeze(0)
    R.close(got['l_gout'], want, dtype, 'dL/dgout')
    ls, ls_abs = M.dot(t['gout'], Bb)
    R.assert_sum_close(got['l_s'], ls, ls_abs, plane_n, 'dL/ds')
    Ba, Ba_abs = M.outer(t['a'], t['gout'])
    R.assert_sum_close(got['l_w'], M.plane_t(Ba, TERM_COEF, k), M.plane_t(Ba_abs, TERM_COEF, k), pos * TERM_N, 'dL/dw')


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
def test_two_runs_of_every_kernel_give_identical_bits(dtype):
    """No float atomics: the statistic's three kernels at the multi-block case and at two segments, the term's at cout = 512, twice
    each, whether or not the reproducible mode is set (it is not here)."""
    for i in (5, 1):
        n, c, ext, group, nseg, _, _ = KERNEL_CASES[i]
        ref = _case(i, dtype)
        a = _run_stat(ref['x'], ref['gstat'], ref['h'], group, nseg, dtype)
        b = _run_stat(ref['x'], ref['gstat'], ref['h'], group, nseg, dtype)
        assert all(torch.equal(p, q) for p, q in zip(a, b)), KERNEL_IDS[i]
    t = _term_inputs(512, (3, 3, 3), dtype)
    a, b = _run_term(t, dtype), _run_term(t, dtype)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_each_pass_is_one_entry_point_call(monkeypatch):
    """The launch budget (forward 2, backward 1, backward of the backward 2, each term kernel 1) is what the entry points of
    csrc/mbstd.hip launch; here: every pass through autograd is ONE call of its entry point and nothing else of the library."""
    from saragan_amd import functional as F
    lib = F._lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith('sg_') or name.endswith('_workspace'):
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    monkeypatch.setattr(F._lib, 'load', lambda: Counting())
    ref = _case(0, torch.float32)
    _run_stat(ref['x'], ref['gstat'], ref['h'], 4, 1, torch.float32)
    assert calls == ['sg_mbstd_stat_fwd', 'sg_mbstd_stat_bwd', 'sg_mbstd_stat_bwd2'], calls
    del calls[:]
    _run_term(_term_inputs(24, (1, 3, 3), torch.float32), torch.float32)
    first = ['sg_mbstd_term_fwd', 'sg_mbstd_term_dot', 'sg_mbstd_term_outer']      # out; gs and gB for its cotangent
    # L's gradients: the dot's backward is an outer product and a term, the outer product's a dot and a term
    assert calls[:3] == first and sorted(calls[3:]) == sorted(first + ['sg_mbstd_term_fwd']), calls


# ---- D and the step: the toy pgan of the step fixtures with the layer on ---------------------------------------------------------
P2, P3 = 'oracle_step_p2_wgan_a060.npz', 'oracle_step_p3_wgan_a000.npz'      # phase 2 while mixing, phase 3 stabilising
GROUP = 4


@pytest.fixture
def deterministic(sg_env):
    from saragan_amd import functional as F
    F.clear_kept_workspaces()
    sg_env(SG_DETERMINISTIC=1)
    yield
    F.clear_kept_workspaces()


@pytest.fixture
def mbstd_on():
    """The module switch at group 4 for the whole test (the discriminator reads it at every call), restored afterwards; the helper's
    oracle architecture registered."""
    from saragan_amd import functional as F
    from saragan_amd.networks import loss as L
    from saragan_amd.networks import ops as nops
    from saragan_amd.varstore import set_compute_dtype
    prev = nops.set_minibatch_stddev(GROUP)
    M.register()
    try:
        with M.configured(GROUP):
            yield
    finally:
        nops.set_minibatch_stddev(prev)
        set_compute_dtype(torch.float32)
        L.set_random_source(None)
        F.clear_pack_cache()
        F.clear_kept_workspaces()


def _step(golden_dir, name, dtype, loss_fn='wgan', strategy='simultaneous', **kw):
    """tests.test_spectral_gpu._Step over the fixture's weights and randomness (spectral normalisation off unless asked for); the
    statistic channel's filter is the store's own seeded draw (the fixture has none)."""
    from tests.test_spectral_gpu import _Step
    kw.setdefault('spectral', False)
    st = _Step(golden_dir, name, dtype, loss_fn, strategy, **kw)
    assert M.MBSTD_WEIGHT in st.store.vars
    return st


def _oracle_step(st, loss_fn, strategy, dtype=torch.float64):
    """The registered oracle architecture's step on the product's initial weights (read before any update), in `dtype`."""
    from oracle import pgan_oracle as O
    fx = st.fx
    p = {k: v.detach().cpu().to(dtype).clone() for k, v in st.store.vars.items()}
    rnd = {k: v.to(dtype) for k, v in fx['rnd'].items()}
    cfg = dict(fx['cfg'], loss_fn=loss_fn, arch=M.ARCH)
    fn = O.step_simultaneous if strategy == 'simultaneous' else O.step_alternate
    ref = fn(p, O.TFAdam(0.0, 0.9), O.TFAdam(0.0, 0.9), None, rnd, fx['real'].to(dtype), fx['alpha'], cfg, 1e-3, 1e-3,
             freeze=fx['freeze'])
    return ref, p


STEP_CASES = [(name, loss, strat) for name in (P2, P3) for loss in ('wgan', 'logistic') for strat in ('simultaneous', 'alternate')]
STEP_IDS = [f"{'p2' if n == P2 else 'p3'}-{l}-{s}" for n, l, s in STEP_CASES]


@pytest.mark.parametrize('name,loss_fn,strategy', STEP_CASES, ids=STEP_IDS)
def test_step_with_the_layer_matches_the_oracle_architecture(golden_dir, mbstd_on, name, loss_fn, strategy):
    """f32 compute, group 4, both fixtures, both losses, `simultaneous` (wgan: the batched pass, nseg = 2) and `alternate`: logits
    of D(real), both losses, the penalty and every D gradient against the registered oracle architecture in fp64, at
    tests/test_step_gpu.py's comparisons (1e-4 / 1e-5 on logits and losses, rtol 1e-3 with atol 1e-4 of the maximum on gradients).
    Whether those tolerances can be relied on for this architecture was measured on the CPU with the oracle itself in float32
    against float64 on the same inputs (store seed 0; tests/test_mbstd_host.py asserts it stays below one half).  The largest
    share of a tolerance it uses: 0.27 with the phase-3 fixture under the wgan loss (dense_2/bias' gradient), below 0.01 in the
    other cases (logits)."""
    from saragan_amd.varstore import use_store
    st = _step(golden_dir, name, torch.float32, loss_fn, strategy)
    ref, _ = _oracle_step(st, loss_fn, strategy)
    p0 = {k: v.detach().double().cpu().clone() for k, v in st.store.vars.items()}
    fx = st.fx
    with use_store(st.store), torch.no_grad():
        real = st.real.contiguous(memory_format=torch.channels_last_3d)
        logits = st.discriminator(real, st.net_args[1], fx['phase'], st.net_args[0], 'leaky_relu', st.net_args[4], st.net_args[5],
                                  param=0.2)
    want = M.discriminator(p0, fx['real'], fx['alpha'], fx['phase'], st.net_args[0], 'leaky_relu', st.net_args[4], st.net_args[5],
                           param=0.2)
    np.testing.assert_allclose(logits.double().cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5)
    mixing = fx['freeze'] is not None
    dg_h, dv = (st.tup[17], st.tup[18]) if mixing else (st.tup[8], st.tup[9])
    # (with the train ops, as tests/test_step_gpu.py fetches: an `alternate` step builds the generator loss on the UPDATED D)
    _, _, gl, dl, gpl, dg = st.sess.run(st.train + [st.tup[2], st.tup[3], st.tup[4], dg_h], feed_dict={st.ph: st.real})
    print(name, loss_fn, strategy, 'gen_loss', float(gl), float(ref['gen_loss']), 'disc_loss', float(dl), float(ref['disc_loss']))
    np.testing.assert_allclose(float(gl), float(ref['gen_loss']), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(float(dl), float(ref['disc_loss']), rtol=1e-4, atol=1e-5)
    gp = ref['gp_loss'].numpy()
    np.testing.assert_allclose(gpl.double().cpu().numpy().reshape(gp.shape), gp, rtol=1e-3, atol=1e-5 * max(1.0, np.abs(gp).max()))
    assert [v.key for v in dv] == list(ref['d_grads'].keys()) and M.MBSTD_WEIGHT in ref['d_grads']
    assert float(ref['d_grads'][M.MBSTD_WEIGHT].abs().max()) > 0
    for v, g in zip(dv, dg):
        r = ref['d_grads'][v.key].numpy()
        np.testing.assert_allclose(g.double().cpu().numpy(), r, rtol=1e-3, atol=1e-4 * np.abs(r).max() + 1e-9, err_msg=v.key)


@pytest.mark.parametrize('name', [P2, P3], ids=['p2', 'p3'])
def test_step_bf16_close_to_the_oracle_architecture(golden_dir, mbstd_on, name):
    """bf16 storage against the fp64 oracle architecture at test_step_bf16_close_to_oracle's tolerances (3e-2 on losses and sample)."""
    st = _step(golden_dir, name, torch.bfloat16)
    ref, _ = _oracle_step(st, 'wgan', 'simultaneous')
    res = st.sess.run(st.train + [st.tup[2], st.tup[3], st.tup[5]], feed_dict={st.ph: st.real})
    gl, dl, gs = res[2], res[3], res[4]
    np.testing.assert_allclose(float(gl), float(ref['gen_loss']), rtol=3e-2, atol=3e-2)
    np.testing.assert_allclose(float(dl), float(ref['disc_loss']), rtol=3e-2, atol=3e-2)
    want = ref['gen_sample'].numpy()
    np.testing.assert_allclose(gs.double().cpu().numpy(), want, rtol=3e-2, atol=3e-2 * np.abs(want).max())


@pytest.mark.parametrize('dtype', R.DT, ids=['f32', 'bf16'])
@pytest.mark.parametrize('name', [P2, P3], ids=['p2', 'p3'])
def test_batched_pass_equals_separate_passes(golden_dir, deterministic, mbstd_on, monkeypatch, name, dtype):
    """The wgan step's one D pass over [real, generated] under mbstd_segments(2) against SARAGAN_NO_BATCHED_D=1: every logit in
    every bit, hence both losses."""
    from saragan_amd.networks import loss as L
    from saragan_amd.varstore import use_store
    seen = {}
    for batched in (True, False):
        monkeypatch.setattr(L, '_NO_BATCHED_D', not batched)
        st = _step(golden_dir, name, dtype)
        calls = []

        def disc(x, *a, **k):
            out = st.discriminator(x, *a, **k)
            calls.append(out.detach().float().clone())
            return out
        with use_store(st.store), L.linear_generator_link():
            gen_loss, disc_loss, _, _ = L.forward_simultaneous(st.generator, disc, st.real, *st.net_args, st.fx['cfg']['gp_weight'],
                                                               0.01)
        n = st.real.shape[0]
        if batched:
            assert [c.shape[0] for c in calls] == [2 * n, n]
            real, fake = calls[0][:n], calls[0][n:]
        else:
            assert [c.shape[0] for c in calls] == [n, n, n]
            fake, real = calls[0], calls[1]
        seen[batched] = (real, fake, calls[-1], gen_loss.detach().clone(), disc_loss.detach().clone())
    for a, b, what in zip(seen[True], seen[False], ('D(real)', 'D(fake)', 'D(interpolates)', 'gen_loss', 'disc_loss')):
        assert torch.equal(a, b), what
    assert not torch.equal(seen[True][0], seen[True][1])


@pytest.mark.parametrize('name,loss_fn,strategy,dtype', [(P3, 'wgan', 'simultaneous', torch.float32),
                                                         (P3, 'wgan', 'alternate', torch.bfloat16),
                                                         (P2, 'logistic', 'simultaneous', torch.bfloat16)],
                         ids=['p3-wgan-sim-f32', 'p3-wgan-alt-bf16', 'p2-mixing-logistic-sim-bf16'])
def test_captured_step_equals_eager_steps_bit_for_bit(golden_dir, deterministic, mbstd_on, monkeypatch, name, loss_fn, strategy, dtype):
    """Two eager warm-up steps, a capture, two replays against five eager steps: weights and losses in every bit (the statistic's
    kernels and the term's take no host decision and allocate through torch)."""
    runs = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('SARAGAN_HIPGRAPH', mode)
        st = _step(golden_dir, name, dtype, loss_fn, strategy, rnd='device')
        gen = torch.Generator().manual_seed(5)
        losses = []
        for i in range(5):
            real = (st.fx['real'].float() + 0.1 * torch.randn(st.fx['real'].shape, generator=gen)).cuda()
            res = st.step(real)
            losses.append((float(res[2]), float(res[3])))
        ncap = sum(1 for e in st.graph.__dict__.get('_captures', {}).values() if 'graph' in e)
        runs[mode] = (st.snapshot(), losses, ncap)
        st = None
    monkeypatch.setenv('SARAGAN_HIPGRAPH', '0')
    (w0, l0, n0), (w1, l1, n1) = runs['0'], runs['1']
    assert (n0, n1) == (0, 1)
    assert l0 == l1, (l0, l1)
    assert M.MBSTD_WEIGHT in w0
    bad = [k for k in w0 if not torch.equal(w0[k], w1[k])]
    assert not bad, bad


def test_default_off_calls_no_new_entry_point(golden_dir, monkeypatch):
    from oracle import pgan_oracle as O
    from saragan_amd import functional as F
    from saragan_amd.networks import loss as L
    from saragan_amd.networks import ops as nops
    from saragan_amd.varstore import set_compute_dtype
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT
    from tests.test_spectral_gpu import _Step
    calls = []
    for fn in ('mbstd_stat', 'mbstd_term', 'mbstd_plane', 'mbstd_tap_mask'):
        monkeypatch.setattr(F, fn, lambda *a, _fn=fn, **k: calls.append(_fn))
    for cls in ('_MbstdStat', '_MbstdStatBwd', '_MbstdTerm', '_MbstdDot', '_MbstdOuter', '_MbstdPlane'):
        monkeypatch.setattr(getattr(F, cls), 'apply', lambda *a, _c=cls, **k: calls.append(_c))
    assert nops.minibatch_stddev_settings() == 0
    try:
        st = _Step(golden_dir, P3, torch.float32, 'wgan', spectral=False)
        st.step()
        st.step()
        assert not calls
        assert list(st.store.vars) == list(O.variable_shapes(3, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC))
    finally:
        set_compute_dtype(torch.float32)
        L.set_random_source(None)
        F.clear_pack_cache()
        F.clear_kept_workspaces()


def test_spectral_normalisation_and_the_layer_together(golden_dir, mbstd_on):
    st = _step(golden_dir, P3, torch.float32, spectral=True)
    res = st.step()
    assert np.isfinite(float(res[2])) and np.isfinite(float(res[3]))
    assert 'discriminator/discriminator_out/mbstd/u' in st.store.state and M.MBSTD_WEIGHT in st.store.effective
    for k, v in st.snapshot().items():
        assert torch.isfinite(v).all(), k


def test_training_run_hands_the_weight_over_and_restores_without_it(tmp_path, capsys):
    """--d_mbstd_group through the training loop: two phases, the end-of-phase checkpoints hold the statistic channel's filter and
    the switch is off again when the run returns; a run continued from a checkpoint written without the flag prints the notice and
    starts the filter from zeros (one Adam step of 1e-3 later it is still below 2e-3 everywhere, where a drawn one is N(0, 1))."""
    from saragan_amd.networks import ops as nops
    from saragan_amd.train import run_training
    from saragan_amd.utils import load_checkpoint
    from tests.test_train_gpu import _args, _make_data
    data, logdir = tmp_path / 'data', tmp_path / 'log'
    _make_data(data)
    out = run_training(_args(data, logdir, d_mbstd_group=4), max_steps_per_phase=1)
    assert nops.minibatch_stddev_settings() == 0
    assert all(np.isfinite(out['stats'][p]['d_loss']) and np.isfinite(out['stats'][p]['g_loss']) for p in (1, 2))
    ck1, ck2 = (load_checkpoint(os.path.join(str(logdir), f'model_{p}')) for p in (1, 2))
    assert M.MBSTD_WEIGHT in ck1 and M.MBSTD_WEIGHT in ck2 and ck1[M.MBSTD_WEIGHT].shape == (1, 3, 3, 1, 16)
    assert np.abs(ck1[M.MBSTD_WEIGHT]).max() > 0.5                     # a drawn filter, trained for one step
    assert np.abs(ck2[M.MBSTD_WEIGHT] - ck1[M.MBSTD_WEIGHT]).max() < 5e-3      # phase 2 started from phase 1's, not from a fresh draw
    assert 'written without --d_mbstd_group' not in capsys.readouterr().out
    plain = run_training(_args(data, tmp_path / 'log2', ending_phase=1), max_steps_per_phase=1)
    assert M.MBSTD_WEIGHT not in plain['store'].vars
    args = _args(data, tmp_path / 'log3', starting_phase=2, continue_path=os.path.join(str(tmp_path / 'log2'), 'model_1'),
                 d_mbstd_group=4)
    out3 = run_training(args, max_steps_per_phase=1)
    assert 'written without --d_mbstd_group' in capsys.readouterr().out
    w = out3['store'].vars[M.MBSTD_WEIGHT].detach()
    assert torch.isfinite(w).all() and float(w.abs().max()) < 2e-3
    with pytest.raises(ValueError, match='--d_mbstd_group'):           # the checkpoint has the filter, the run does not
        run_training(_args(data, tmp_path / 'log4', starting_phase=2, continue_path=os.path.join(str(logdir), 'model_1')),
                     max_steps_per_phase=1)
