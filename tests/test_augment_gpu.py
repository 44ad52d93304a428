"""Discriminator augmentation on the device (saragan_amd/csrc/augment.hip) against its numpy definition (tests/augref.py).
The transforms are index gathers and the draw is integer arithmetic on Philox words, so every kernel comparison here is
bit for bit; the network-level tests state their own tolerances where two different kernel routes are compared."""
import os

import numpy as np
import pytest
import torch

from tests import augref as R
from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]


def _to_dev(a, dtype=torch.float32):
    """numpy [n, d, h, w, c] -> device tensor of logical shape [n, c, d, h, w] stored NDHWC."""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    return t.permute(0, 4, 1, 2, 3).contiguous(memory_format=torch.channels_last_3d)


def _to_np(t):
    return t.detach().float().permute(0, 2, 3, 4, 1).contiguous().cpu().numpy()


def _prm(rows):
    return torch.as_tensor(np.asarray(rows, np.int32).reshape(-1, 8)).cuda()


def _data(shape, dtype, seed):
    """Values every format holds exactly: distinct integers in f32, small random integers in bf16."""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        return (np.random.default_rng(seed).permutation(n).astype(np.float32) - n // 2).reshape(shape)
    return np.random.default_rng(seed).integers(-120, 121, shape).astype(np.float32)


def _cases(shape, ops):
    """Lists of n parameter rows, a different row per sample: every flip alone, every k alone, translations of +-1 and +-m
    per axis (m = half the extent, so that rows move across 16-byte pieces), the whole extent shifted out along each axis
    (all fill), the identity and 8 compositions drawn from the reference."""
    n, d, h, w, c = shape
    rows = [R.IDENTITY, R.params_of(flip_d=1), R.params_of(flip_h=1), R.params_of(flip_w=1)]
    if ops & R.ROT90:
        rows += [R.params_of(k=k) for k in (1, 2, 3)]
    for ax, e in enumerate((d, h, w)):
        for s in sorted({1, -1, max(1, e // 2), -max(1, e // 2), e - 1, e, -e}):
            t = [0, 0, 0]
            t[ax] = s
            rows.append(R.params_of(t=t))
    rows += [tuple(r) for r in R.draw(8, ops, (d, (h + 1) // 2, (w + 1) // 2), 0.8, seed=d * 100 + w, offset=5)]
    while len(rows) % n:
        rows.append(rows[len(rows) % 7 + 1])
    return [rows[i:i + n] for i in range(0, len(rows), n)]


SHAPES = [(3, 2, 8, 8, 1),      # c = 1, one piece per row in bf16
          (2, 1, 6, 6, 3),      # D = 1; rows of 18 elements: no multiple of the piece, the scalar path with its short last piece
          (2, 3, 4, 4, 32),     # pieces within the channels
          (3, 4, 64, 64, 1),    # several blocks, two trips of the grid-stride loop
          (2, 2, 4, 8, 1)]      # h != w: every transform but rot90


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_apply_is_bit_exact_forward_and_adjoint(shape, dtype):
    from saragan_amd import functional as F
    ops = R.ALL if shape[2] == shape[3] else R.ALL & ~R.ROT90
    x = _data(shape, dtype, seed=shape[3])
    xd = _to_dev(x, dtype)
    for rows in _cases(shape, ops):
        prm = _prm(rows)
        y = _to_np(F.augment(xd, prm, fill=-1.0, ops=ops))
        assert np.array_equal(y, R.apply(x, rows, -1.0)), rows
        ya = _to_np(F.augment(xd, prm, fill=-1.0, ops=ops, adjoint=True))      # the adjoint fills with 0 whatever `fill` is
        assert np.array_equal(ya, R.apply(x, rows, 0.0, adjoint=True)), rows
    # whole extent shifted out: nothing but fill forward, nothing but zeros in the adjoint
    gone = [R.params_of(t=(0, 0, shape[3]))] * shape[0]
    assert (_to_np(F.augment(xd, _prm(gone), fill=-1.0, ops=ops)) == -1.0).all()
    assert (_to_np(F.augment(xd, _prm(gone), fill=-1.0, ops=ops, adjoint=True)) == 0.0).all()
    # identity and pure permutations reproduce the input's bits
    ident = F.augment(xd, _prm([R.IDENTITY] * shape[0]), fill=-1.0, ops=ops)
    assert torch.equal(ident.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       xd.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))
    perm = _prm([R.params_of(flip_d=1, flip_w=1, k=2 if ops & R.ROT90 else 0)] * shape[0])
    back = F.augment(F.augment(xd, perm, ops=ops), perm, ops=ops, adjoint=True)
    assert torch.equal(back, xd)


def test_apply_refuses_rot90_on_a_non_square_plane_and_in_place():
    from saragan_amd import _lib, functional as F
    x = _to_dev(_data((2, 2, 4, 8, 1), torch.float32, 0))
    prm = _prm([R.params_of(k=1)] * 2)
    with pytest.raises(_lib.SgError, match='code -1'):
        F.augment(x, prm, ops=R.ALL)
    y = F.augment(x, prm, ops=R.ALL & ~R.ROT90)          # the rotation is not among the enabled transforms: ignored
    assert torch.equal(y, x)
    lib = _lib.load()
    p = x.data_ptr()
    assert lib.sg_augment_apply(p, p, prm.data_ptr(), 2, 2, 4, 8, 1, R.FLIP_W, 0.0, 0, _lib.SG_F32, None) == -1
    with pytest.raises(ValueError):
        F.augment(x, prm[:1], ops=R.FLIP_W)
    with pytest.raises(RuntimeError, match='GPU only'):
        F.augment(x.cpu(), prm, ops=R.FLIP_W)


def test_adjoint_identity_on_the_device():
    """<A x, y> == <x, A^T y> exactly: integer-valued f32 data, the sums taken in float64 on the host."""
    from saragan_amd import functional as F
    shape = (4, 3, 8, 8, 2)
    rng = np.random.default_rng(3)
    x, y = (rng.integers(-8, 9, shape).astype(np.float32) for _ in range(2))
    xd, yd = _to_dev(x), _to_dev(y)
    for trial in range(6):
        rows = R.draw(shape[0], R.ALL, (2, 4, 4), 0.8, seed=trial, offset=trial)
        ax = _to_np(F.augment(xd, _prm(rows), fill=0.0)).astype(np.float64)
        aty = _to_np(F.augment(yd, _prm(rows), adjoint=True)).astype(np.float64)
        assert (ax * y).sum() == (x * aty).sum()


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'bf16'])
def test_autograd_first_and_second_order(dtype):
    from saragan_amd import functional as F
    shape = (3, 2, 6, 6, 2)
    x, y, v = (_data(shape, torch.bfloat16, s) for s in (1, 2, 3))      # (small integers: exact in both formats)
    rows = [R.params_of(flip_w=1, k=1, t=(0, 1, -2)), R.params_of(flip_d=1, flip_h=1, t=(1, 0, 0)), R.params_of(k=3, t=(0, -2, 3))]
    prm = _prm(rows)
    xd, yd, vd = _to_dev(x, dtype).requires_grad_(True), _to_dev(y, dtype).requires_grad_(True), _to_dev(v, dtype)
    out = F.augment(xd, prm, fill=-1.0)
    assert np.array_equal(_to_np(out), R.apply(x, rows, -1.0))
    (g,) = torch.autograd.grad((out * yd).sum(), xd, create_graph=True)
    assert np.array_equal(_to_np(g), R.apply(y, rows, 0.0, adjoint=True))
    # g = A^T y: its derivative with respect to y, contracted with v, is A v (the forward, fill 0)
    (gg,) = torch.autograd.grad((g * vd).sum(), yd)
    assert np.array_equal(_to_np(gg), R.apply(v, rows, 0.0))


@pytest.mark.parametrize('ops', [R.ALL, R.FLIP_W | R.TRANSLATE], ids=['all', 'flipw_translate'])
def test_draw_equals_the_reference(ops):
    from saragan_amd import functional as F
    m = (2, 5, 7)
    for n in (1, 5, 4096):
        for p in (0.0, 0.3, 1.0):
            for offset in (0, 7, (1 << 40) + 3):
                got = F.augment_draw(n, ops, m, p, seed=1234, offset=offset).cpu().numpy()
                want = R.draw(n, ops, m, p, seed=1234, offset=offset)
                assert got.dtype == np.int32 and np.array_equal(got, want), (n, p, offset)
    # a seed above 2^32 uses both key words
    got = F.augment_draw(64, ops, m, 0.5, seed=(7 << 32) + 9, offset=1).cpu().numpy()
    assert np.array_equal(got, R.draw(64, ops, m, 0.5, seed=(7 << 32) + 9, offset=1))


def test_draw_device_offset_and_device_probability():
    from saragan_amd import functional as F
    m, seed = (1, 3, 3), 99
    for offset in (0, (5 << 40) + 11):
        ctr = torch.tensor([offset], dtype=torch.int64, device='cuda')
        a = F.augment_draw(300, R.ALL, m, 0.6, seed, offset=ctr)
        assert torch.equal(a, F.augment_draw(300, R.ALL, m, 0.6, seed, offset=offset))
        assert int(ctr) == offset + (1 << 40)
        b = F.augment_draw(300, R.ALL, m, 0.6, seed, offset=ctr)          # the next draw continues from the advanced counter
        assert np.array_equal(b.cpu().numpy(), R.draw(300, R.ALL, m, 0.6, seed, offset + (1 << 40)))
        assert int(ctr) == offset + (2 << 40)
    for p in (0.0, 0.3, 0.8, 1.0):
        pd = torch.tensor([p], dtype=torch.float32, device='cuda')
        assert torch.equal(F.augment_draw(500, R.ALL, m, pd, seed, offset=4), F.augment_draw(500, R.ALL, m, p, seed, offset=4))
        assert np.array_equal(F.augment_draw(500, R.ALL, m, pd, seed, offset=4).cpu().numpy(), R.draw(500, R.ALL, m, p, seed, 4))


def test_controller_follows_the_reference_after_every_call():
    from saragan_amd import functional as F
    rng = np.random.default_rng(8)
    batches = []
    for i in range(12):      # mixed signs, exact zeros of both signs, one NaN; the first six batches mostly positive, the rest negative
        b = rng.normal(2.0 if i < 6 else -2.0, 1.0, 7).astype(np.float32)
        b[i % 7] = 0.0
        if i % 4 == 1:
            b[(i + 2) % 7] = -0.0
        if i == 6:
            b[0] = np.nan
        batches.append(b)
    interval, target, delta, p_max = 2, (600000, 1000000), 0.3, 0.8
    state = torch.zeros(4, dtype=torch.int64, device='cuda')
    p = torch.tensor([0.5], dtype=torch.float32, device='cuda')
    rs, rp = (0, 0, 0, 0), np.float32(0.5)
    seen = set()
    for b in batches:
        F.ada_update_(torch.from_numpy(b).cuda().reshape(-1, 1), state, p, interval, target, delta, p_max)
        rs, rp = R.ada_update(rs, rp, b, interval, target[0], target[1], np.float32(delta), np.float32(p_max))
        assert tuple(state.tolist()) == rs
        assert p.cpu().numpy()[0] == rp
        seen.add(float(rp))
    assert rs[2:] == (12, 6) and {0.0, float(np.float32(0.8))} <= seen      # both clamps were reached on the way


# ---- the smallest networks: augmentation inside the loss functions --------------------------------------------------------
WGAN_P2, LOGISTIC_P3, WGAN_P3 = 'oracle_step_p2_wgan_a060.npz', 'oracle_step_p3_logistic_a025.npz', 'oracle_step_p3_wgan_a000.npz'
FILL = 0.25


def _aug_rows(shape, seed):
    """Non-identity parameters, a different row per sample ([N, C, D, H, W] batch)."""
    n, _, d, h, w = shape
    rows = R.draw(n, R.ALL, (d // 2, h // 4, w // 4), 1.0, seed=seed, offset=0)
    assert all(np.any(r != 0) for r in rows)
    return rows


def _step(golden_dir, name, fetch, rnd_extra=None, augment=False, rng_cls=None):
    """One evaluation of the step graph of fixture `name` with injected randomness.  fetch: names from
    {'gen_loss', 'disc_loss', 'gp_loss', 'g_grads', 'd_grads'}; returns the fetched values in that order."""
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
    prev = L.set_augment(L.AugmentConfig('fixed', ops=R.ALL, fill=FILL, p=1.0) if augment else None)
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
        return out, fx
    finally:
        L.set_augment(prev)
        L.set_random_source(None)


@pytest.mark.parametrize('name', [WGAN_P2, LOGISTIC_P3])
def test_identity_parameters_reproduce_the_unaugmented_step_bit_for_bit(golden_dir, name):
    """Augmentation ON with identity parameters (InjectedRandom without aug_* keys): both batches pass through the apply
    kernel, G's gradient through its adjoint; losses and every gradient keep their bits (reproducible mode: no float atomics)."""
    import saragan_amd
    fetch = ['gen_loss', 'disc_loss', 'gp_loss', 'g_grads', 'd_grads']
    saragan_amd.set_deterministic(True)
    try:
        (gl0, dl0, gp0, gg0, dg0), _ = _step(golden_dir, name, fetch)
        (gl1, dl1, gp1, gg1, dg1), _ = _step(golden_dir, name, fetch, augment=True)
    finally:
        saragan_amd.set_deterministic(False)
    print('losses', float(gl0), float(gl1), float(dl0), float(dl1))
    assert torch.equal(gl0, gl1) and torch.equal(dl0, dl1) and torch.equal(gp0, gp1)
    assert len(gg0) == len(gg1) > 0 and len(dg0) == len(dg1) > 0
    bad = [i for i, (a, b) in enumerate(zip(gg0 + dg0, gg1 + dg1)) if not torch.equal(a, b)]
    assert not bad, bad


@pytest.mark.parametrize('name', [WGAN_P2, LOGISTIC_P3])
def test_augmented_step_equals_the_step_fed_host_transformed_batches(golden_dir, name):
    """D-side quantities with non-identity parameters against the UNAUGMENTED step whose noisy real and noisy generated
    batches are transformed on the host by augref.apply (a random source whose add_noise does it).  D sees the same bits in
    both runs and its forward passes launch the same kernels (reproducible mode), so the three losses are equal exactly; D's
    weight gradients come out of backward passes whose first layer differs in whether it owes a data gradient to the
    generator, so they are held to the project's fp32 gradient tolerance (as tests/test_step_gpu.py:
    rtol 1e-3, atol 1e-4 of the largest reference element)."""
    import saragan_amd
    from saragan_amd.networks import loss as L
    fx0 = load_step_fixture(os.path.join(golden_dir, name), torch.float64)
    shape = tuple(fx0['real'].shape)
    extra = {'aug_real': torch.as_tensor(_aug_rows(shape, 21)), 'aug_fake': torch.as_tensor(_aug_rows(shape, 22))}

    class HostAugmented(L.InjectedRandom):
        def add_noise(self, x, stddev, tag):
            y = super().add_noise(x, stddev, tag)
            rows = self.t['aug_real' if tag == 'noise_real' else 'aug_fake'].numpy()
            return _to_dev(R.apply(_to_np(y), rows, FILL), y.dtype)

    fetch = ['gen_loss', 'disc_loss', 'gp_loss', 'd_grads']
    saragan_amd.set_deterministic(True)
    try:
        (gl, dl, gp, dg), _ = _step(golden_dir, name, fetch, rnd_extra=extra, augment=True)
        (gl_r, dl_r, gp_r, dg_r), _ = _step(golden_dir, name, fetch, rnd_extra=extra, rng_cls=HostAugmented)
        (gl_0, dl_0, _, _), _ = _step(golden_dir, name, fetch)
    finally:
        saragan_amd.set_deterministic(False)
    print('losses', float(gl), float(gl_r), float(dl), float(dl_r), 'unaugmented', float(gl_0), float(dl_0))
    assert float(gl) != float(gl_0) and float(dl) != float(dl_0)      # the parameters did something
    assert torch.equal(gl, gl_r) and torch.equal(dl, dl_r) and torch.equal(gp, gp_r)
    for a, b in zip(dg, dg_r):
        r = b.double().cpu().numpy()
        np.testing.assert_allclose(a.double().cpu().numpy(), r, rtol=1e-3, atol=1e-4 * np.abs(r).max() + 1e-9)


def test_generator_gradients_agree_with_and_without_the_link(golden_dir):
    """wgan: with both networks' gradients asked for, G's gradient arrives through linear_generator_link (the AUGMENTED fake is
    the detached leaf, G's backward starts at the augment node); with G's alone, through the general path.  Tolerance: the one
    tests/test_step_gpu.py holds the linked path's gradients to against the oracle (rtol 1e-3, atol 1e-4 of the largest
    reference element)."""
    fx0 = load_step_fixture(os.path.join(golden_dir, WGAN_P2), torch.float64)
    shape = tuple(fx0['real'].shape)
    extra = {'aug_real': torch.as_tensor(_aug_rows(shape, 31)), 'aug_fake': torch.as_tensor(_aug_rows(shape, 32))}
    (g_link, _), _ = _step(golden_dir, WGAN_P2, ['g_grads', 'd_grads'], rnd_extra=extra, augment=True)
    (g_plain,), _ = _step(golden_dir, WGAN_P2, ['g_grads'], rnd_extra=extra, augment=True)
    (g_noaug,), _ = _step(golden_dir, WGAN_P2, ['g_grads'])
    assert len(g_link) == len(g_plain) > 0
    for a, b in zip(g_link, g_plain):
        r = b.double().cpu().numpy()
        np.testing.assert_allclose(a.double().cpu().numpy(), r, rtol=1e-3, atol=1e-4 * np.abs(r).max() + 1e-9)
    assert any(not torch.allclose(a, b, rtol=1e-2, atol=1e-6) for a, b in zip(g_plain, g_noaug))      # the adjoint matters


# ---- the captured step ------------------------------------------------------------------------------------------------------
def _run_steps(golden_dir, steps, captured, mode, loss_fn, interval):
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
    cfg = L.AugmentConfig(mode, ops=R.ALL, max_shift=0.25, fill=FILL, p=0.5, interval=interval, target=0.6, delta=0.05, p_max=0.8)
    prev = L.set_augment(cfg)
    try:
        store = VariableStore('cuda', seed=0)
        L.set_random_source(L.RandomSource(1234, 'cuda'))
        og = opt.AdamOptimizer(ScalarVariable(1e-3, 'g_lr'), 0.0, 0.9)
        od = opt.AdamOptimizer(ScalarVariable(1e-3, 'd_lr'), 0.0, 0.9)
        ph = opt.Placeholder([4, 1, 1, 1, 1])
        with use_store(store):
            tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, ScalarVariable(0.0, 'alpha'), fx['phase'], BASE_SHAPE,
                                    KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, loss_fn, fx['cfg']['gp_weight'], 'simultaneous',
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
        p = float(cfg.p)
        st = None if cfg.state is None else tuple(cfg.state.tolist())
        return state, losses, ncap, p, st, L._rng('cuda').aug_calls
    finally:
        os.environ['SARAGAN_HIPGRAPH'] = '0'
        L.set_augment(prev)
        L.set_random_source(None)


@pytest.mark.parametrize('mode, loss_fn, steps', [('fixed', 'wgan', 4), ('ada', 'logistic', 5)])
def test_captured_step_with_augmentation_equals_eager(golden_dir, mode, loss_fn, steps):
    """Four steps (two eager warm-up steps, the capture, replays) against four eager steps from the same seed, reproducible
    mode: the draws read a device counter the captured launches advance, p and the controller's sums live on the device.
    'ada' runs five steps with an adjustment of 0.05 after each: an odd number of equal moves cannot return to 0.5, and
    0.5 +- 5 * 0.05 stays inside (0, p_max), so p has moved whichever way D's logits sent it."""
    import saragan_amd
    saragan_amd.set_deterministic(True)
    try:
        w0, l0, n0, p0, s0, c0 = _run_steps(golden_dir, steps, False, mode, loss_fn, 1)
        w1, l1, n1, p1, s1, c1 = _run_steps(golden_dir, steps, True, mode, loss_fn, 1)
    finally:
        saragan_amd.set_deterministic(False)
    print('p', p0, p1, 'state', s0, s1, 'losses', l0, l1)
    assert (n0, n1) == (0, 1)
    assert c0 == c1 == 2 * steps               # two draws per step, counted on the host in both runs
    assert l0 == l1, (l0, l1)
    bad = [k for k in w0 if not torch.equal(w0[k], w1[k])]
    assert not bad, bad
    assert p0 == p1 and s0 == s1
    if mode == 'ada':
        assert s0[2:] == (5, 5) and p0 != 0.5


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


def test_training_loop_with_adaptive_augmentation(tmp_path, capsys):
    """--augment ada through run_training: the run finishes, p is reported per phase, lies in [0, p_max] and has left its
    initial value.  --ada_target 1.0 makes the direction certain (mean sign(D(real)) never exceeds 1, so every one of the four
    adjustments per phase lowers p): 0.3 - 4 * 0.08 clamps at 0 in phase 1 whatever D's logits are."""
    from saragan_amd.networks import loss as L
    from saragan_amd.train import run_training
    data = tmp_path / 'data'
    _make_data(data)
    args = _train_args(data, tmp_path / 'log', ['--augment', 'ada', '--augment_p', '0.3', '--ada_interval', '2', '--ada_kimg', '0.1',
                                                '--ada_target', '1.0', '--augment_ops', 'flip_w,flip_h,rot90,translate'])
    out = run_training(args, max_steps_per_phase=args.max_steps_per_phase)
    st = out['stats']
    assert (st[1]['steps'], st[2]['steps']) == (8, 8)
    for ph in (1, 2):
        assert 0.0 <= st[ph]['augment_p'] <= args.ada_p_max
        assert np.isfinite(st[ph]['d_loss']) and np.isfinite(st[ph]['g_loss'])
    assert st[1]['augment_p'] != 0.3 and st[1]['augment_p'] == 0.0
    assert 'Augmentation probability:' in capsys.readouterr().out
    assert not L._AUGMENT['cfg'].on          # the run's configuration does not outlive it


def test_training_loop_without_augmentation_is_reproducible(tmp_path):
    """--augment none (the default): two identical runs in reproducible mode end with the same weights, and no augmentation
    statistic is reported."""
    import saragan_amd
    from saragan_amd.train import run_training
    data = tmp_path / 'data'
    _make_data(data)
    saragan_amd.set_deterministic(True)
    try:
        outs = [run_training(_train_args(data, tmp_path / f'log{i}', []), max_steps_per_phase=8) for i in range(2)]
    finally:
        saragan_amd.set_deterministic(False)
    assert 'augment_p' not in outs[0]['stats'][1]
    a, b = (o['store'].vars for o in outs)
    assert set(a) == set(b)
    assert all(torch.equal(a[k].detach(), b[k].detach()) for k in a)
