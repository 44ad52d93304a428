"""The non-finite step guard's launches and the per-segment norms, all decided on the device.  Re-exported by functional."""
import torch

from . import _lib
from ._launch import _ptr, _req_cuda, _stream
from ._lib import check
from ._scalars import _dev_ptr


def segment_sumsq(flat, offsets_dev, nseg, flag=None, accumulate=False):
    """Per-segment sums of squares; flag (a one-element int32 device tensor): also the all-finite test of nonfinite_flag_
    on the values read (sg_segment_sumsq_flag)."""
    lib = _lib.load()
    out = torch.empty(nseg, device=flat.device, dtype=torch.float32)
    if flag is not None:
        check(lib.sg_segment_sumsq_flag(_ptr(flat), _ptr(offsets_dev), _ptr(out), nseg, _ptr(flag), 1 if accumulate else 0,
                                        _stream()), 'sg_segment_sumsq_flag')
        return out
    check(lib.sg_segment_sumsq(_ptr(flat), _ptr(offsets_dev), _ptr(out), nseg, _stream()), 'sg_segment_sumsq')
    return out


def nonfinite_flag_(flag, x, accumulate=False):
    """flag (one-element int32 device tensor) = 1 if any entry of the flat f32 tensor x is NaN or +-Inf, else 0
    (sg_nonfinite_flag; accumulate=True ORs into the flag instead of clearing it first).  No host sync."""
    lib = _lib.load()
    _req_cuda(flag, x)
    if flag.dtype != torch.int32 or x.dtype != torch.float32 or not x.is_contiguous():
        raise TypeError('nonfinite_flag_: an int32 flag and a contiguous float32 buffer')
    check(lib.sg_nonfinite_flag(_ptr(x), x.numel(), _ptr(flag), 1 if accumulate else 0, _stream()), 'sg_nonfinite_flag')
    return flag


def guard_step_(flag, t, counters, lr, lr_t, adam=None, lr_dev=None):
    """Bookkeeping of a guarded train op (sg_guard_step, one thread): flag clear -> t += 1 and lr_t = the step size at the
    new t (adam=(beta1, beta2): Adam's bias-corrected lr, in double as adam_step_size; None: lr); flag set -> counters
    [skipped, consecutive, longest run] advance.  t: int64 [1], counters: int64 [3], lr_t: f32 [1] (device tensors);
    lr_dev: a float64 DevCoef read instead of `lr` (captured step)."""
    lib = _lib.load()
    _req_cuda(flag, t, counters, lr_t)
    b1, b2 = adam if adam is not None else (0.0, 0.0)
    check(lib.sg_guard_step(_ptr(flag), _ptr(t), _ptr(counters), float(lr), None if lr_dev is None else _dev_ptr(lr_dev),
                            _ptr(lr_t), 1 if adam is not None else 0, float(b1), float(b2), _stream()), 'sg_guard_step')
