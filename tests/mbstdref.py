"""fp64 statements shared by tests/test_mbstd_host.py and tests/test_mbstd_gpu.py: the closed forms of the minibatch-stddev
statistic, its gradient and the gradient of that gradient (include/saragan_hip.h, sg_mbstd_stat_*), the rank-1 plane B of the
statistic channel's share of a SAME-padded convolution, and a discriminator assembled from oracle.pgan_oracle's own blocks with
minibatch_stddev_layer in front of discriminator_out's convolution, registered under O.ARCHS['pgan_mbstd'] so that the oracle's
loss functions and steps run with it.  Nothing here touches the GPU."""
import contextlib

import numpy as np
import torch

from oracle import pgan_oracle as O

ARCH = 'pgan_mbstd'
MBSTD_WEIGHT = 'discriminator/discriminator_out/mbstd/weight'
EPS = 1e-8
_CFG = {'group': 4}


# ---- closed forms, fp64, x [N, C, D, H, W] -----------------------------------------------------------------------------------
def _grouped(x, group, nseg):
    """x [N, ...] -> [nseg, G, M, P] (the reference's reshape [G, M, ...] inside each of the nseg consecutive sub-batches)."""
    n = x.shape[0]
    assert n % nseg == 0
    sub = n // nseg
    g = min(group, sub)
    assert sub % g == 0
    return x.reshape(nseg, g, sub // g, -1), g


def parts(x, group, nseg=1):
    xg, g = _grouped(x.double(), group, nseg)
    mu = xg.mean(dim=1, keepdim=True)
    d = xg - mu
    sigma = torch.sqrt((d * d).mean(dim=1, keepdim=True) + EPS)
    return xg, d, sigma, g


def stat(x, group, nseg=1):
    """(stat [N], abs_terms [N]): the statistic per sample and the sum of the absolute values of the terms of its sum."""
    xg, d, sigma, g = parts(x, group, nseg)
    p = xg.shape[-1]
    s = sigma.sum(dim=-1, keepdim=True) / p                          # [nseg, 1, M, 1]
    out = s.expand(-1, g, -1, -1).reshape(x.shape[0])
    return out, out.clone()                                          # (every term is positive)


def min_sigma(x, group, nseg=1):
    return float(parts(x, group, nseg)[2].min())


def stat_bwd(gstat, x, group, nseg=1):
    xg, d, sigma, g = parts(x, group, nseg)
    p = xg.shape[-1]
    S = gstat.double().reshape(nseg, g, -1, 1).sum(dim=1, keepdim=True)
    return (S / (p * g) * d / sigma).reshape(x.shape)


def stat_bwd2(h, x, gstat, group, nseg=1):
    """(ggstat [N], abs_terms [N], gx like x)."""
    xg, d, sigma, g = parts(x, group, nseg)
    p = xg.shape[-1]
    hg = h.double().reshape(xg.shape)
    S = gstat.double().reshape(nseg, g, -1, 1).sum(dim=1, keepdim=True)
    terms = hg * d / sigma
    gg = terms.sum(dim=(1, 3), keepdim=True) / (p * g)
    ab = terms.abs().sum(dim=(1, 3), keepdim=True) / (p * g)
    q = (hg * d).sum(dim=1, keepdim=True)
    gx = S / (p * g) * ((hg - hg.mean(dim=1, keepdim=True)) / sigma - d * q / (g * sigma ** 3))
    exp = lambda t: t.expand(-1, g, -1, -1).reshape(x.shape[0])
    return exp(gg), exp(ab), gx.reshape(x.shape)


def stat_torch(x, group, nseg=1):
    """The statistic as plain differentiable torch ops (for torch's own double backward)."""
    xg, g = _grouped(x, group, nseg)
    d = xg - xg.mean(dim=1, keepdim=True)
    s = torch.sqrt((d * d).mean(dim=1, keepdim=True) + EPS).mean(dim=-1, keepdim=True)
    return s.expand(-1, g, -1, -1).reshape(x.shape[0])


# ---- the rank-1 term ---------------------------------------------------------------------------------------------------------
def tap_mask(extent, kernel):
    """[positions, taps] 0/1 (fp64): tap (kd, kh, kw order) of a SAME-padded convolution reads inside the volume at pos."""
    axes = []
    for e, k in zip(extent, kernel):
        pos = np.arange(e)[:, None] + np.arange(k)[None, :] - (k - 1) // 2
        axes.append(((pos >= 0) & (pos < e)).astype(np.float64))
    md, mh, mw = axes
    full = md[:, None, None, :, None, None] * mh[None, :, None, None, :, None] * mw[None, None, :, None, None, :]
    return torch.from_numpy(full.reshape(int(np.prod(extent)), int(np.prod(kernel))))


def plane_t(Bg, coef, kernel):
    """The filter gradient [kd, kh, kw, 1, cout] that plane() hands a gradient Bg [D, H, W, cout] of B back to."""
    m = tap_mask(Bg.shape[:3], kernel)
    return (coef * (m.t() @ Bg.double().reshape(m.shape[0], -1))).reshape(*kernel, 1, Bg.shape[-1])


def plane(w, coef, extent):
    """B [D, H, W, cout] (fp64) from the statistic channel's filter w [kd, kh, kw, 1, cout]."""
    m = tap_mask(extent, w.shape[:3])
    return (coef * (m @ w.double().reshape(m.shape[1], -1))).reshape(*extent, w.shape[-1])


def ndhwc(t):
    return t.permute(0, 2, 3, 4, 1)


def term(y, s, B):
    """y [N, C, D, H, W] + s (x) B, fp64."""
    return y.double() + (s.double().reshape(-1, 1, 1, 1, 1) * B.double().unsqueeze(0)).permute(0, 4, 1, 2, 3)


def dot(g, B):
    """(r [N], abs_terms [N])."""
    t = ndhwc(g.double()) * B.double().unsqueeze(0)
    return t.sum(dim=(1, 2, 3, 4)), t.abs().sum(dim=(1, 2, 3, 4))


def outer(s, g):
    """(Bg [D, H, W, C], abs_terms)."""
    t = s.double().reshape(-1, 1, 1, 1, 1) * ndhwc(g.double())
    return t.sum(dim=0), t.abs().sum(dim=0)


# ---- the oracle's discriminator with the layer ---------------------------------------------------------------------------------
@contextlib.contextmanager
def configured(group=4):
    """The layer's group size for the registered architecture (the oracle's network signature has no room for it)."""
    prev = dict(_CFG)
    _CFG.update(group=group)
    try:
        yield
    finally:
        _CFG.update(prev)


def full_weight(p):
    """The reference layer's filter [k, k, k, C + 1, cout]: the C real channels' variable and the statistic channel's."""
    d = 'discriminator/discriminator_out/'
    return torch.cat([p[d + 'weight'], p[d + 'mbstd/weight']], dim=3)


def discriminator(p, x, alpha, phase, latent_dim, activation, kernel_spec, filter_spec, param=None, conditioning=None):
    """oracle.pgan_oracle.discriminator block for block, with minibatch_stddev_layer in front of discriminator_out's
    convolution (the reference's commented-out line pgan/discriminator.py:50 put back)."""
    if conditioning is not None:
        raise NotImplementedError()
    q, d = O._q, 'discriminator/'
    x_downscale = x
    x = O.conv3d(x, p[d + f'from_rgb_{phase}/weight'], activation, param)
    x = q(O.act(O.apply_bias(x, p[d + f'from_rgb_{phase}/bias']), activation, param))
    for i in reversed(range(2, phase + 1)):
        b = d + f'discriminator_block_{i}/'
        x = O.conv3d(x, p[b + 'conv_1/weight'], activation, param)
        x = q(O.act(O.apply_bias(x, p[b + 'conv_1/bias']), activation, param))
        cin = x.shape[1]
        x = O.conv3d(x, p[b + 'conv_2/weight'], activation, param)
        x = O.act(O.apply_bias(x, p[b + 'conv_2/bias']), activation, param)
        x = O._downscale_stored(x, cin, p[b + 'conv_2/weight'].shape[:3])
        if i == phase:
            if O._EMU['on'] and float(alpha) == 0.0:
                continue
            t = O.conv3d(q(O.downscale3d(x_downscale)), p[d + f'from_rgb_{phase - 1}/weight'], activation, param)
            t = q(O.act(O.apply_bias(t, p[d + f'from_rgb_{phase - 1}/bias']), activation, param))
            x = t if (O._EMU['on'] and float(alpha) == 1.0) else q(alpha * t + (1 - alpha) * x)
    x = O.conv3d(O.minibatch_stddev_layer(x, _CFG['group']), full_weight(p), activation, param)
    x = q(O.act(O.apply_bias(x, p[d + 'discriminator_out/bias']), activation, param))
    x = O.dense(x, p[d + 'discriminator_out/dense_1/weight'], activation, param)
    x = q(O.act(O.apply_bias(x, p[d + 'discriminator_out/dense_1/bias']), activation, param))
    x = O.dense(x, p[d + 'discriminator_out/dense_2/weight'], 'linear')
    return O.apply_bias(x, p[d + 'discriminator_out/dense_2/bias'])


def variable_shapes(phase, base_shape, latent_dim, kernel_spec, filter_spec):
    out = O.variable_shapes(phase, base_shape, latent_dim, kernel_spec, filter_spec)
    k = tuple(kernel_spec[0][1])
    out[MBSTD_WEIGHT] = (*k, 1, filter_spec[0][0])
    return out


def register():
    """Puts the architecture under O.ARCHS[ARCH] (at run time: nothing under oracle/ changes) and returns its key."""
    O.ARCHS.setdefault(ARCH, (O.generator, discriminator, variable_shapes))
    return ARCH


def mbstd_weight(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(tuple(shape), generator=g, dtype=torch.float32).double()
