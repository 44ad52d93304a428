"""The loss's own elementwise passes: instance noise on D's inputs, the gradient penalty's interpolates and its per-row sums of
squares.  Re-exported by functional."""
import torch

from . import _lib
from ._consumers import _note_all
from ._launch import _dims, _dt, _ptr, _req_cuda, _stream, ndhwc
from ._lib import check


class _AddNoise(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, stddev, seed, offset):
        """offset: a Python int, or a one-element int64 DEVICE tensor holding the Philox offset (read by the kernel and then
        advanced by 1 << 40 on the device: the form a captured step uses, sg_add_noise_dev)."""
        _note_all(x, stddev, seed, offset)
        lib = _lib.load()
        _req_cuda(x)
        x = ndhwc(x)
        out = torch.empty_like(x)
        if torch.is_tensor(offset):
            check(lib.sg_add_noise_dev(_ptr(x), _ptr(out), float(stddev), int(seed), _ptr(offset), 1 << 40, x.numel(), _dt(x),
                                       _stream()), 'sg_add_noise_dev')
        else:
            check(lib.sg_add_noise(_ptr(x), _ptr(out), float(stddev), int(seed), int(offset), x.numel(), _dt(x),
                                   _stream()), 'sg_add_noise')
        return out

    @staticmethod
    def backward(ctx, g):
        return g, None, None, None


def add_noise(x, stddev, seed, offset=0):
    return _AddNoise.apply(x, stddev, seed, offset)


def interpolate_rows(gamma, a, b):
    """gamma * a + (1 - gamma) * b with one weight per batch sample (gamma: [N, 1, 1, 1, 1] or [N], f32): the gradient
    penalty's interpolates (networks/loss.py:70-71, :133-134) in ONE launch with one rounding (sg_lerp_rows).  No gradient:
    every caller detaches the result (the penalty differentiates with respect to the interpolates, not through them)."""
    lib = _lib.load()
    _req_cuda(a, b, gamma)
    a, b = ndhwc(a.detach()), ndhwc(b.detach())
    if a.shape != b.shape or a.dtype != b.dtype:
        raise ValueError('interpolate_rows: operands differ in shape or dtype')
    g = gamma.detach().reshape(-1).float().contiguous()
    if g.numel() != a.shape[0]:
        raise ValueError('interpolate_rows: one weight per batch sample')
    out = torch.empty_like(a)
    check(lib.sg_lerp_rows(_ptr(a), _ptr(b), _ptr(g), _ptr(out), a.shape[0], a.numel() // a.shape[0], _dt(a), _stream()),
          'sg_lerp_rows')
    return out


class _SumsqKeepW(torch.autograd.Function):
    """out[n, w] = sum_{c,d,h} g^2: tf.reduce_sum(tf.square(g), (1,2,3)) on NCDHW (networks/loss.py:140)."""

    @staticmethod
    def forward(ctx, g):
        _note_all(g)
        lib = _lib.load()
        _req_cuda(g)
        g = ndhwc(g)
        n, c, d, h, w = _dims(g)
        out = torch.empty((n, w), device=g.device, dtype=torch.float32)
        check(lib.sg_sumsq_ndhwc_keep_w(_ptr(g), _ptr(out), n, d, h, w, c, _dt(g), _stream()),
              'sg_sumsq_ndhwc_keep_w')
        ctx.save_for_backward(g)
        return out

    @staticmethod
    def backward(ctx, gout):
        (g,) = ctx.saved_tensors
        n, w = gout.shape
        return (2.0 * gout.reshape(n, 1, 1, 1, w)).to(g.dtype) * g


def sumsq_keep_w(g):
    return _SumsqKeepW.apply(g)
