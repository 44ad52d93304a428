"""Minibatch standard deviation: the reference's concatenating layer, and the form the discriminator uses -- the
statistic as N floats, twice differentiable, and the rank-1 term it adds to the convolution that follows.  Re-exported by
functional."""
import math

import torch

from . import _lib
from ._consumers import _note_all
from ._grad_dest import _f32_out, _wants
from ._launch import _DT, _dims, _dt, _empty_like_shape, _ptr, _req_cuda, _stream, ndhwc
from ._lib import check


class _MinibatchStddev(torch.autograd.Function):
    """networks/ops.py:313-325: concat(x, per-group mean stddev).  Once-differentiable (the layer is disabled in
    pgan, pgan/discriminator.py:50, so it never sits under the gradient penalty)."""

    @staticmethod
    def forward(ctx, x, group_size):
        _note_all(x, group_size)
        lib = _lib.load()
        _req_cuda(x)
        x = ndhwc(x)
        n, c, d, h, w = _dims(x)
        g = min(group_size, n)
        if n % g != 0:
            raise ValueError(f'minibatch_stddev_layer: batch {n} not divisible by group {g}')
        y = _empty_like_shape(x, c + 1)
        ws = torch.empty(n // g, device=x.device, dtype=torch.float32)
        check(lib.sg_minibatch_stddev_fwd(_ptr(x), _ptr(y), _ptr(ws), n, d * h * w, c, group_size, _dt(x), _stream()),
              'sg_minibatch_stddev_fwd')
        ctx.save_for_backward(x)
        ctx.group_size = group_size
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        lib = _lib.load()
        (x,) = ctx.saved_tensors
        gy = ndhwc(gy)
        n, c, d, h, w = _dims(x)
        g = min(ctx.group_size, n)
        dx = torch.empty_like(x)
        ws = torch.empty(n // g, device=x.device, dtype=torch.float32)
        check(lib.sg_minibatch_stddev_bwd(_ptr(gy), _ptr(x), _ptr(dx), _ptr(ws), n, d * h * w, c, ctx.group_size, _dt(x),
                                          _stream()), 'sg_minibatch_stddev_bwd')
        return dx, None


def minibatch_stddev(x, group_size=4):
    """networks/ops.py:313-325 (the layer is disabled in pgan, pgan/discriminator.py:50)."""
    return _MinibatchStddev.apply(x, group_size)


# ---- without the concatenation.  Every backward is a Function of this group again.
def _mbstd_ws(lib, x, n, vox, c, group, nseg):
    nbytes = int(lib.sg_mbstd_stat_workspace(n, vox, c, group, nseg))      # (0: a batch the groups do not divide -- the launch refuses)
    return torch.empty(nbytes // 4, device=x.device, dtype=torch.float32), nbytes


class _MbstdStat(torch.autograd.Function):
    """stat[n] (f32): the mean over a sample's positions of the standard deviation over its group (sg_mbstd_stat_fwd)."""

    @staticmethod
    def forward(ctx, x, group, nseg):
        _note_all(x)
        lib = _lib.load()
        _req_cuda(x)
        ctx.save_for_backward(x)      # (the inputs themselves are saved throughout this group: the backward Functions take them as
        x = ndhwc(x)                  # inputs again, and a converted copy would cut the second-order graph)
        n, c, d, h, w = _dims(x)
        stat = torch.empty(n, device=x.device, dtype=torch.float32)
        ws, nbytes = _mbstd_ws(lib, x, n, d * h * w, c, group, nseg)
        check(lib.sg_mbstd_stat_fwd(_ptr(x), _ptr(stat), _ptr(ws), nbytes, n, d * h * w, c, group, nseg, _dt(x), _stream()),
              'sg_mbstd_stat_fwd')
        ctx.group, ctx.nseg = group, nseg
        return stat

    @staticmethod
    def backward(ctx, gstat):
        (x,) = ctx.saved_tensors
        return _MbstdStatBwd.apply(gstat, x, ctx.group, ctx.nseg), None, None


class _MbstdStatBwd(torch.autograd.Function):
    """dx of _MbstdStat (sg_mbstd_stat_bwd); its own backward is sg_mbstd_stat_bwd2, which ends the chain: nothing in the step
    differentiates a third time."""

    @staticmethod
    def forward(ctx, gstat, x, group, nseg):
        _note_all(gstat, x)
        lib = _lib.load()
        ctx.save_for_backward(gstat, x)
        gstat, x = gstat.contiguous().float(), ndhwc(x)
        n, c, d, h, w = _dims(x)
        dx = torch.empty_like(x)
        check(lib.sg_mbstd_stat_bwd(_ptr(gstat), _ptr(x), _ptr(dx), n, d * h * w, c, group, nseg, _dt(x), _stream()),
              'sg_mbstd_stat_bwd')
        ctx.group, ctx.nseg = group, nseg
        return dx

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, hh):
        lib = _lib.load()
        gstat, x = ctx.saved_tensors
        want_gg, want_gx = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_gg or want_gx):
            return None, None, None, None
        gstat, x = gstat.contiguous().float(), ndhwc(x)
        hh = ndhwc(hh.to(x.dtype))
        n, c, d, h, w = _dims(x)
        gx = torch.empty_like(x) if want_gx else None
        ggstat = torch.empty(n, device=x.device, dtype=torch.float32) if want_gg else None
        ws, nbytes = _mbstd_ws(lib, x, n, d * h * w, c, ctx.group, ctx.nseg) if want_gg else (None, 0)
        check(lib.sg_mbstd_stat_bwd2(_ptr(hh), _ptr(x), _ptr(gstat), _ptr(gx), _ptr(ggstat), _ptr(ws), nbytes, n, d * h * w, c,
                                     ctx.group, ctx.nseg, _dt(x), _stream()), 'sg_mbstd_stat_bwd2')
        return ggstat, gx, None, None


def _plane_numel(shape):
    return math.prod(shape[1:])


class _MbstdTerm(torch.autograd.Function):
    """out = y + s (x) B (sg_mbstd_term_fwd): y [N,C,D,H,W] (None: the outer product alone, shaped `shape`, of `dtype`),
    s f32 [N], B f32 [D,H,W,C].  w_ptr: the data_ptr of the weight B was made from (0: none), for skip_param_grads."""

    @staticmethod
    def forward(ctx, y, s, B, w_ptr, shape, dtype):
        _note_all(y, s, B)
        lib = _lib.load()
        _req_cuda(s, B)
        ctx.save_for_backward(s, B)
        if y is not None:
            y = ndhwc(y)
            shape, dtype = tuple(y.shape), y.dtype
        s, B = s.contiguous().float(), B.contiguous().float()
        if B.numel() != _plane_numel(shape) or s.numel() != shape[0]:
            raise ValueError(f'mbstd_term: s {tuple(s.shape)} / B {tuple(B.shape)} do not fit the tensor {tuple(shape)}')
        out = torch.empty(shape, device=s.device, dtype=dtype, memory_format=torch.channels_last_3d)
        check(lib.sg_mbstd_term_fwd(_ptr(y), _ptr(s), _ptr(B), _ptr(out), shape[0], B.numel(), _DT[dtype], _stream()),
              'sg_mbstd_term_fwd')
        ctx.w_ptr = w_ptr
        return out

    @staticmethod
    def backward(ctx, gout):
        s, B = ctx.saved_tensors
        gy = gout if ctx.needs_input_grad[0] else None
        gs = _MbstdDot.apply(gout, B, ctx.w_ptr) if ctx.needs_input_grad[1] else None
        gB = _MbstdOuter.apply(s, gout) if _wants(ctx, 2, ctx.w_ptr) else None
        return gy, gs, gB, None, None, None


class _MbstdDot(torch.autograd.Function):
    """r[n] = <g[n], B> (sg_mbstd_term_dot), f32 [N]."""

    @staticmethod
    def forward(ctx, g, B, w_ptr):
        _note_all(g, B)
        lib = _lib.load()
        _req_cuda(g, B)
        ctx.save_for_backward(g, B)
        g, B = ndhwc(g), B.contiguous().float()
        if B.numel() != _plane_numel(g.shape):
            raise ValueError(f'mbstd: B {tuple(B.shape)} does not fit the tensor {tuple(g.shape)}')
        r = torch.empty(g.shape[0], device=g.device, dtype=torch.float32)
        check(lib.sg_mbstd_term_dot(_ptr(g), _ptr(B), _ptr(r), g.shape[0], B.numel(), _dt(g), _stream()), 'sg_mbstd_term_dot')
        ctx.w_ptr = w_ptr
        return r

    @staticmethod
    def backward(ctx, gr):
        g, B = ctx.saved_tensors
        gg = _MbstdTerm.apply(None, gr, B, ctx.w_ptr, tuple(g.shape), g.dtype) if ctx.needs_input_grad[0] else None
        gB = _MbstdOuter.apply(gr, g) if _wants(ctx, 1, ctx.w_ptr) else None
        return gg, gB, None


class _MbstdOuter(torch.autograd.Function):
    """Bg = sum_n s_n g[n] (sg_mbstd_term_outer), f32 [D,H,W,C], n ascending."""

    @staticmethod
    def forward(ctx, s, g):
        _note_all(s, g)
        lib = _lib.load()
        _req_cuda(s, g)
        ctx.save_for_backward(s, g)
        s, g = s.contiguous().float(), ndhwc(g)
        n, c, d, h, w = _dims(g)
        if s.numel() != n:
            raise ValueError(f'mbstd: s {tuple(s.shape)} does not fit the tensor {tuple(g.shape)}')
        Bg = torch.empty((d, h, w, c), device=g.device, dtype=torch.float32)
        check(lib.sg_mbstd_term_outer(_ptr(s), _ptr(g), _ptr(Bg), n, Bg.numel(), _dt(g), _stream()), 'sg_mbstd_term_outer')
        return Bg

    @staticmethod
    def backward(ctx, gBg):
        s, g = ctx.saved_tensors
        gs = _MbstdDot.apply(g, gBg, 0) if ctx.needs_input_grad[0] else None
        gg = _MbstdTerm.apply(None, s, gBg, 0, tuple(g.shape), g.dtype) if ctx.needs_input_grad[1] else None
        return gs, gg


_MBSTD_MASKS = {}


def mbstd_tap_mask(extent, kernel, coef, device):
    """coef * Mask, f32 [positions, taps] on `device`: Mask[pos, tap] = 1 where tap (kd, kh, kw order) of a SAME-padded
    `kernel` convolution over `extent` = (d, h, w) reads inside the volume at output position pos.  Built on the host once per
    (extent, kernel, coef, device) and kept: a captured step finds it ready."""
    key = (tuple(int(e) for e in extent), tuple(int(k) for k in kernel), float(coef), str(device))
    m = _MBSTD_MASKS.get(key)
    if m is None:
        axes = []
        for e, k in zip(key[0], key[1]):
            pos = torch.arange(e).reshape(e, 1) + torch.arange(k).reshape(1, k) - (k - 1) // 2
            axes.append(((pos >= 0) & (pos < e)).to(torch.float32))                      # [extent, taps] of one axis
        md, mh, mw = axes
        full = md[:, None, None, :, None, None] * mh[None, :, None, None, :, None] * mw[None, None, :, None, None, :]
        m = _MBSTD_MASKS[key] = (full.reshape(math.prod(key[0]), math.prod(key[1])) * float(coef)).to(device)
    return m


class _MbstdPlane(torch.autograd.Function):
    """B[pos, :] = coef * sum over the taps in bounds at pos of w[tap, 0, :]: maskc [positions, taps] (mbstd_tap_mask) times
    w [kd, kh, kw, 1, cout] as [taps, cout].  A few thousand products: torch element-wise ops (multiply, then a sum over the
    taps, whose order is fixed).  The weight's gradient honours skip_param_grads and grads_into like a convolution's."""

    @staticmethod
    def forward(ctx, w, maskc):
        ctx.save_for_backward(maskc)
        ctx.w_shape, ctx.w_ptr = tuple(w.shape), w.data_ptr()
        w2 = w.detach().reshape(maskc.shape[1], -1)
        return (maskc.unsqueeze(-1) * w2.unsqueeze(0)).sum(dim=1)

    @staticmethod
    def backward(ctx, gB):
        (maskc,) = ctx.saved_tensors
        if not _wants(ctx, 0, ctx.w_ptr):
            return None, None
        prod = maskc.t().unsqueeze(-1) * gB.reshape(maskc.shape[0], -1).unsqueeze(0)      # [taps, positions, cout]
        if torch.is_grad_enabled():
            return prod.sum(dim=1).reshape(ctx.w_shape), None
        out = _f32_out(ctx.w_ptr, ctx.w_shape, gB.device)
        torch.sum(prod, dim=1, out=out.view(maskc.shape[1], -1))
        return out, None


def mbstd_stat(x, group, nseg=1):
    """The minibatch-stddev statistic of x [N,C,D,H,W] as f32 [N] (networks/ops.py:313-325 without the concatenation): the batch
    is `nseg` consecutive sub-batches, each grouped on its own (G = min(group, N / nseg), group m = samples g * M + m).  Twice
    differentiable."""
    return _MbstdStat.apply(x, int(group), int(nseg))


def mbstd_plane(w, coef, extent):
    """B f32 [D,H,W,cout] for mbstd_term from the statistic channel's filter w [kd,kh,kw,1,cout] and its runtime coefficient."""
    if w.dim() != 5 or w.shape[3] != 1:
        raise ValueError(f'mbstd_plane: expected a [kd, kh, kw, 1, cout] filter, got {tuple(w.shape)}')
    B = _MbstdPlane.apply(w, mbstd_tap_mask(extent, w.shape[:3], coef, w.device)).reshape(*extent, w.shape[-1])
    B._sg_w_ptr = w.data_ptr()
    return B


def mbstd_term(y, s, B):
    """conv(concat(x, stat), W) = conv(x, W[..., :C, :]) + s (x) B: adds the statistic channel's share to y = the convolution of
    the C real channels.  One f32 add per element, one rounding to y's type."""
    return _MbstdTerm.apply(y, s, B, getattr(B, '_sg_w_ptr', 0), None, None)
