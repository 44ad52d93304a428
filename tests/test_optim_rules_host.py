"""CPU-only self-checks of the references in tests/ewref.py that the GPU kernel tests (test_elementwise_gpu.py,
test_optim_kernels_gpu.py) compare with: the numpy sign-word packing against a bit-by-bit restatement, the optimiser rules
against the oracle's TF optimisers, and every other fp64 helper against an independent formulation."""
import numpy as np
import pytest
import torch

from oracle import pgan_oracle as O
from tests import ewref as R


@pytest.mark.parametrize('c', [1, 31, 32, 33, 72])
def test_sign_word_packing(c):
    t = R.rnd((2, c, 1, 3, 5), 1, torch.bfloat16)
    t[0, :, 0, 0, 0] = -0.0
    t[1, 0] = -(2.0 ** -133)
    w = R.sign_words_np(t)
    nw = (c + 31) // 32
    assert w.dtype == np.int32 and w.shape == (2, 1, 3, 5, nw)
    u = w.view(np.uint32)
    for n in range(2):
        for h in range(3):
            for x in range(5):
                for k in range(nw):
                    word = 0
                    for j in range(32):
                        ch = 32 * k + j
                        if ch < c and float(t[n, ch, 0, h, x]) < 0:
                            word |= 1 << j
                    assert int(u[n, 0, h, x, k]) == word
    assert not (u[0, 0, 0, 0] != 0).any(), '-0.0 is not negative'
    assert (u[1, ..., 0] & 1).all(), 'the smallest negative subnormal is negative'
    assert np.array_equal(R.sign_words_np(t[:, :, 0, 0, 0]), w[:, 0, 0, 0][:, None, None, None])     # [N, F] form
    assert np.array_equal(torch.where(t < 0, R.SLOPE, 1.0).numpy(), R.lrelu_mask(t).numpy())


def test_optimiser_rules_match_the_oracle():
    n, lr = 37, 1e-2
    p0 = R.f32_vec(n, 2)
    grads = [R.f32_vec(n, 3 + s) for s in range(3)]
    # Adam + EMA
    params, shadow, opt = {'w': p0.clone()}, {'w': p0.clone()}, O.TFAdam(0.5, 0.9)
    p, m, v, sh = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p0.clone()
    for t, g in enumerate(grads, 1):
        opt.apply(params, {'w': g}, lr)
        O.ema_update(shadow, params, 0.99)
        p, m, v = R.adam_rule(p, g, m, v, lr * np.sqrt(1 - 0.9 ** t) / (1 - 0.5 ** t), 0.5, 0.9)
        sh = R.ema_rule(sh, p, 0.99)
    for a, b in ((p, params['w']), (m, opt.m['w']), (v, opt.v['w']), (sh, shadow['w'])):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-13, atol=0)
    # SGD, Momentum (plain and Nesterov), Adadelta
    for mk, rule in ((lambda: O.TFSGD(), lambda p_, g_, s_: (R.sgd_rule(p_, g_, lr), s_)),
                     (lambda: O.TFMomentum(0.9, False), lambda p_, g_, s_: R.momentum_rule(p_, g_, s_, lr, 0.9, False)),
                     (lambda: O.TFMomentum(0.9, True), lambda p_, g_, s_: R.momentum_rule(p_, g_, s_, lr, 0.9, True))):
        params, opt = {'w': p0.clone()}, mk()
        p, s = p0.clone(), torch.zeros(n, dtype=torch.float64)
        for g in grads:
            opt.apply(params, {'w': g}, lr)
            p, s = rule(p, g, s)
        np.testing.assert_allclose(p.numpy(), params['w'].numpy(), rtol=1e-13, atol=0)
    params, opt = {'w': p0.clone()}, O.TFAdadelta(0.95, 1e-6)
    p, a, a2 = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for g in grads:
        opt.apply(params, {'w': g}, 1.0)
        p, a, a2 = R.adadelta_rule(p, g, a, a2, 1.0, 0.95, 1e-6)
    for x, y in ((p, params['w']), (a, opt.accum['w']), (a2, opt.accum_update['w'])):
        np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=1e-13, atol=0)


def test_elementwise_references():
    x = R.rnd((2, 6, 2, 4, 6), 11, torch.bfloat16)
    assert torch.equal(x.to(torch.bfloat16).double(), x)
    # pixel norm: scale and backward against the oracle's forward and autograd
    xr = x.clone().requires_grad_(True)
    y = O.pixel_norm(xr)
    np.testing.assert_allclose((x * R.pn_scale(x)).numpy(), y.detach().numpy(), rtol=1e-13)
    gy = R.rnd(tuple(x.shape), 12, torch.bfloat16)
    (gx,) = torch.autograd.grad(y, xr, gy)
    np.testing.assert_allclose(R.pn_bwd(gy, y.detach(), R.pn_scale(x)).numpy(), gx.numpy(), rtol=1e-9, atol=1e-12)
    # nearest up / block sum: the oracle's ops at (2, 2, 2), each other's adjoint at other factors
    assert torch.equal(R.up_nn(x, (2, 2, 2)), O.upscale3d(x))
    np.testing.assert_allclose(R.down_sum(x, (2, 2, 2)).numpy() / 8, O.downscale3d(x).numpy(), rtol=1e-13)
    for f in ((2, 1, 2), (1, 2, 2), (1, 1, 2)):
        u = R.up_nn(x, f)
        g = R.rnd(tuple(u.shape), 13, torch.float32)
        np.testing.assert_allclose(float((u * g).sum()), float((x * R.down_sum(g, f)).sum()), rtol=1e-12)
    # trilinear and its adjoint
    u = R.tri_up(x)
    g = R.rnd(tuple(u.shape), 14, torch.float32)
    np.testing.assert_allclose(float((u * g).sum()), float((x * R.tri_up_adj(g)).sum()), rtol=1e-12)
    # sums: the bound grows with the number of terms and never drops below the f32 tolerance
    assert R.sum_rtol(1) == 1e-4 and R.sum_rtol(1 << 20) == 0.25
    R.assert_sum_close(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0]), 4)
    with pytest.raises(AssertionError):
        R.assert_sum_close(torch.tensor([1.0, 2.001]), torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0]), 4)
    # the statistic channel of the minibatch-stddev gradient is boosted and of one sign; values stay representable
    gm = R.mbstd_grad_input((4, 7, 1, 4, 4), 15, torch.bfloat16)
    assert float(gm[:, -1].min()) >= 0 and torch.equal(gm.to(torch.bfloat16).double(), gm)
    assert R.elems16(torch.bfloat16) == 8 and R.elems16(torch.float32) == 4


def test_gpu_test_modules_import_and_name_every_case():
    """The two kernel-test modules import without a GPU, and every case table states its dispatch condition."""
    from tests import test_elementwise_gpu as E
    from tests import test_optim_kernels_gpu as K
    for table in (E.PN_CASES, E.BA_CASES, E.UP_CASES, E.DOWN_CASES, E.TRI_CASES, E.MBSTD_CASES):
        assert all(isinstance(c[-1], str) and c[-1] for c in table)
    assert K.SIZES[-1] == 2048 * 256 * 4 + 6 and E.BIG % 8 == 5
    for dtype, shape, factors, _ in E.UP_CASES + E.DOWN_CASES:      # no tensor above 64 MB
        n, c, d, h, w = shape
        up = n * c * d * h * w * (factors[0] * factors[1] * factors[2] if (dtype, shape, factors, _) in E.UP_CASES else 1)
        assert up * (2 if dtype == torch.bfloat16 else 4) <= 64 << 20, (shape, factors)
