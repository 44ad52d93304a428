"""On-device discriminator augmentation: per-sample pixel-blitting and affine transforms, their parameter draws and the adaptive
probability's controller (ADA).  Re-exported by functional."""
import math

import torch

from . import _lib
from ._consumers import _note_all
from ._launch import _dims, _dt, _ptr, _req_cuda, _stream, ndhwc
from ._lib import check


class _Augment(torch.autograd.Function):
    """sg_augment_apply: per-sample flips / rot90 / integer translation of an NDHWC batch (forward), or its exact adjoint.
    The derivative of either with respect to x is the other one with fill 0, so the backward is this Function again with the
    flag flipped: differentiable to any order (the gradient penalty differentiates through D's data gradient)."""

    @staticmethod
    def forward(ctx, x, params, fill, ops, adjoint):
        _note_all(x, params)
        lib = _lib.load()
        _req_cuda(x, params)
        if x.dim() != 5:
            raise ValueError(f'augment takes a [N,C,D,H,W] tensor, got shape {tuple(x.shape)}')
        x = ndhwc(x)
        n, c, d, h, w = _dims(x)
        if params.dtype != torch.int32 or tuple(params.shape) != (n, 8) or not params.is_contiguous():
            raise ValueError(f'augment parameters are a contiguous int32 [{n}, 8] tensor, got {params.dtype} {tuple(params.shape)}')
        y = torch.empty_like(x)
        check(lib.sg_augment_apply(_ptr(x), _ptr(y), _ptr(params), n, d, h, w, c, int(ops), float(fill), 1 if adjoint else 0,
                                   _dt(x), _stream()), 'sg_augment_apply')
        ctx.save_for_backward(params)
        ctx.ops, ctx.adjoint = int(ops), bool(adjoint)
        return y

    @staticmethod
    def backward(ctx, g):
        (params,) = ctx.saved_tensors
        return _Augment.apply(g, params, 0.0, ctx.ops, not ctx.adjoint), None, None, None, None


class _AugmentAffine(torch.autograd.Function):
    """sg_augment_affine_apply: per-sample trilinear resampling of an NDHWC batch by a 3 x 4 matrix with gain and bias (forward),
    or the exact adjoint of its linear part.  The derivative of either direction with respect to x is the other one with the
    LINEAR flag (fill and bias read as 0), so the backward is this Function again: differentiable to any order."""

    @staticmethod
    def forward(ctx, x, params, fill, adjoint, linear):
        _note_all(x, params)
        lib = _lib.load()
        _req_cuda(x, params)
        if x.dim() != 5:
            raise ValueError(f'augment_affine takes a [N,C,D,H,W] tensor, got shape {tuple(x.shape)}')
        x = ndhwc(x)
        n, c, d, h, w = _dims(x)
        if params.dtype != torch.float32 or tuple(params.shape) != (n, 16) or not params.is_contiguous():
            raise ValueError(f'augment_affine parameters are a contiguous float32 [{n}, 16] tensor, got {params.dtype} '
                             f'{tuple(params.shape)}')
        y = torch.empty_like(x)
        flags = (_lib.SG_AUGF_ADJOINT if adjoint else 0) | (_lib.SG_AUGF_LINEAR if linear else 0)
        check(lib.sg_augment_affine_apply(_ptr(x), _ptr(y), _ptr(params), n, d, h, w, c, float(fill), flags, _dt(x), _stream()),
              'sg_augment_affine_apply')
        ctx.save_for_backward(params)
        ctx.adjoint = bool(adjoint)
        return y

    @staticmethod
    def backward(ctx, g):
        (params,) = ctx.saved_tensors
        return _AugmentAffine.apply(g, params, 0.0, not ctx.adjoint, True), None, None, None, None


AUG_OPS = {'flip_w': _lib.SG_AUG_FLIP_W, 'flip_h': _lib.SG_AUG_FLIP_H, 'flip_d': _lib.SG_AUG_FLIP_D, 'rot90': _lib.SG_AUG_ROT90,
           'translate': _lib.SG_AUG_TRANSLATE, 'scale': _lib.SG_AUGF_SCALE, 'rotate': _lib.SG_AUGF_ROTATE,
           'shift': _lib.SG_AUGF_SHIFT, 'brightness': _lib.SG_AUGF_BRIGHTNESS, 'contrast': _lib.SG_AUGF_CONTRAST}
AUG_ALL = _lib.SG_AUG_ALL            # the pixel-blitting transforms (sg_augment_draw / sg_augment_apply)
AUGF_ALL = _lib.SG_AUGF_ALL          # the intensity and fractional-geometry transforms (sg_augment_affine_*)


def augment_ops_mask(names):
    """'flip_w,translate' (or a list of names) -> the combined SG_AUG_* | SG_AUGF_* bit mask (mask & AUG_ALL goes to the blitting
    entry points, mask & AUGF_ALL to the affine ones)."""
    if isinstance(names, str):
        names = [s for s in names.split(',') if s]
    mask = 0
    for name in names:
        if name not in AUG_OPS:
            raise ValueError(f'unknown augmentation {name!r}: choose from {", ".join(AUG_OPS)}')
        mask |= AUG_OPS[name]
    return mask


def augment_draw(n, ops, max_shift, p, seed, offset=0, device=None):
    """Per-sample augmentation parameters, int32 [n, 8] = {flip_d, flip_h, flip_w, rot_k, t_d, t_h, t_w, 0}, drawn on the device
    (sg_augment_draw; the rule is in include/saragan_hip.h).  ops: SG_AUG_* mask; max_shift: (m_d, m_h, m_w).  p: a Python
    float, or a one-element f32 DEVICE tensor the kernel reads.  offset: a Python int, or a one-element int64 DEVICE tensor
    read by the kernel and then advanced by 1 << 40 on the device (the forms a captured step uses)."""
    lib = _lib.load()
    for t in (p, offset):
        if torch.is_tensor(t):
            _req_cuda(t)
            device = device or t.device
    out = torch.empty((int(n), 8), dtype=torch.int32, device=device or 'cuda')
    _req_cuda(out)
    m_d, m_h, m_w = (int(m) for m in max_shift)
    p_dev = torch.is_tensor(p)
    if p_dev and (p.dtype != torch.float32 or p.numel() != 1):
        raise ValueError('a device-side probability is a one-element float32 tensor')
    off_dev = torch.is_tensor(offset)
    if off_dev and (offset.dtype != torch.int64 or offset.numel() != 1):
        raise ValueError('a device-side Philox offset is a one-element int64 tensor')
    check(lib.sg_augment_draw(_ptr(out), int(n), int(ops), m_d, m_h, m_w, 0.0 if p_dev else float(p), _ptr(p) if p_dev else None,
                              int(seed) & (2 ** 64 - 1), 0 if off_dev else int(offset) & (2 ** 64 - 1),
                              _ptr(offset) if off_dev else None, (1 << 40) if off_dev else 0, _stream()), 'sg_augment_draw')
    return out


def augment(x, params, fill=0.0, ops=AUG_ALL, adjoint=False):
    """y[i] = shift(rot90(flip(x[i], axes), k, plane (h, w)), t, fill) with sample i's `params` row (augment_draw's layout);
    adjoint=True: the exact transpose of its linear part.  Only the transforms in `ops` are read from params; rot90 needs
    h == w.  Values are copied: a permutation reproduces x's bits."""
    return _Augment.apply(x, params, fill, ops, adjoint)


def augment_affine_draw(n, ops, extent, p, seed, offset=0, max_scale=1.25, max_angle=math.pi, max_shift=(0.0, 0.0, 0.0),
                        max_brightness=0.2, max_contrast=1.5, device=None, bump=1 << 40):
    """Per-sample affine augmentation parameters, float32 [n, 16] = {row-major 3 x 4 source matrix, gain, bias, 0, 0}, drawn on
    the device (sg_augment_affine_draw; the rule is in include/saragan_hip.h).  ops: SG_AUGF_* mask; extent: (d, h, w) of the
    volumes the rows are for; max_angle in radians; max_shift: (m_d, m_h, m_w) in voxels, fractions allowed.  p and offset as
    augment_draw; a device offset is advanced by `bump` after it is read (0: a blitting draw that follows reads the same offset
    and advances it)."""
    lib = _lib.load()
    for t in (p, offset):
        if torch.is_tensor(t):
            _req_cuda(t)
            device = device or t.device
    out = torch.empty((int(n), 16), dtype=torch.float32, device=device or 'cuda')
    _req_cuda(out)
    d, h, w = (int(e) for e in extent)
    m_d, m_h, m_w = (float(m) for m in max_shift)
    p_dev = torch.is_tensor(p)
    if p_dev and (p.dtype != torch.float32 or p.numel() != 1):
        raise ValueError('a device-side probability is a one-element float32 tensor')
    off_dev = torch.is_tensor(offset)
    if off_dev and (offset.dtype != torch.int64 or offset.numel() != 1):
        raise ValueError('a device-side Philox offset is a one-element int64 tensor')
    check(lib.sg_augment_affine_draw(_ptr(out), int(n), int(ops), d, h, w, float(max_scale), float(max_angle), m_d, m_h, m_w,
                                     float(max_brightness), float(max_contrast), 0.0 if p_dev else float(p),
                                     _ptr(p) if p_dev else None, int(seed) & (2 ** 64 - 1),
                                     0 if off_dev else int(offset) & (2 ** 64 - 1), _ptr(offset) if off_dev else None,
                                     int(bump) if off_dev else 0, _stream()), 'sg_augment_affine_draw')
    return out


def augment_affine(x, params, fill=0.0, adjoint=False):
    """y[i] = trilinear resampling of x[i] at u = A v + t with gain and bias, sample i's `params` row (augment_affine_draw's
    layout; source voxels outside the volume read `fill`); adjoint=True: the exact transpose of its linear part, a gather in a
    fixed order (no atomics).  An identity row reproduces x's bits."""
    return _AugmentAffine.apply(x, params, fill, adjoint, bool(adjoint))


def ada_update_(logits, state, p, interval, target, delta, p_max):
    """The adaptive augmentation probability's controller (sg_ada_update, one thread; rule in include/saragan_hip.h).
    logits: D's outputs on the real batch; state: int64 [4] {sum_sign, count, steps, adjustments}; p: f32 [1] (device tensors,
    updated in place).  target: (numerator, denominator) of the sign statistic's set point."""
    lib = _lib.load()
    _req_cuda(logits, state, p)
    lg = logits.detach().reshape(-1)
    if lg.dtype != torch.float32 or not lg.is_contiguous():
        lg = lg.float().contiguous()
    if state.dtype != torch.int64 or state.numel() != 4 or p.dtype != torch.float32 or p.numel() != 1:
        raise ValueError('ada_update_: state is int64 [4], p is float32 [1]')
    check(lib.sg_ada_update(_ptr(lg), lg.numel(), _ptr(state), _ptr(p), int(interval), int(target[0]), int(target[1]),
                            float(delta), float(p_max), _stream()), 'sg_ada_update')
