"""The optimiser kernels' launches over flat f32 buffers: fused Adam / SGD-family (+ EMA), and the segmented AdamW / LAMB with
their device table.  Each one rewrites parameters behind torch's version counters and says so to the weight-image cache.
Re-exported by functional."""
import math

import torch

from . import _lib
from ._launch import _ptr, _req_cuda, _stream
from ._lib import check
from ._scalars import _dev_ptr
from ._weight_images import IMAGES


def adam_step_size(lr, beta1, beta2, step):
    """lr_t = lr * sqrt(1 - b2^t) / (1 - b1^t) (tf.train.AdamOptimizer), in host doubles."""
    return lr * math.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step)


def adam_ema_(p, g, m, v, ema, lr, beta1, beta2, step, eps=1e-8, gscale=1.0, ema_decay=0.99, lr_dev=None, skip=None):
    """In-place fused TF-Adam + EMA over flat f32 buffers.  lr_dev: a DevCoef (or one-element f32
    device tensor) holding lr_t on the device (captured step): `lr` and `step` are then not used.  skip: a one-element int32
    device flag (non-finite step guard, sg_adam_ema_guarded): set, the launch is the EMA-only update; clear, it computes
    what the lr_dev launch computes.  Needs lr_dev."""
    lib = _lib.load()
    _req_cuda(p, g, m, v, ema)
    if g is not None:
        IMAGES.params_rewritten()
    if skip is not None:
        if lr_dev is None or g is None:
            raise ValueError('adam_ema_: a guarded launch needs the gradient and the step size on the device (lr_dev)')
        check(lib.sg_adam_ema_guarded(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), p.numel(), _dev_ptr(lr_dev), _ptr(skip),
                                      float(beta1), float(beta2), float(eps), float(gscale), float(ema_decay), _stream()),
              'sg_adam_ema_guarded')
        return
    if lr_dev is not None and g is not None:
        check(lib.sg_adam_ema_dev(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), p.numel(), _dev_ptr(lr_dev), float(beta1),
                                  float(beta2), float(eps), float(gscale), float(ema_decay), _stream()), 'sg_adam_ema_dev')
        return
    lr_t = adam_step_size(lr, beta1, beta2, step) if g is not None else 0.0
    check(lib.sg_adam_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), p.numel(), float(lr_t), float(beta1),
                          float(beta2), float(eps), float(gscale), float(ema_decay), _stream()), 'sg_adam_ema')


def optim_step_(kind, p, g, s1, s2, ema, lr, h=0.0, eps=0.0, nesterov=False, gscale=1.0, ema_decay=0.99, lr_dev=None,
                skip=None):
    """In-place fused SGD / Momentum / Adadelta (+ EMA) over flat f32 buffers (sg_optim_step; lr_dev: the learning rate as
    a DevCoef or one-element f32 tensor on the device, captured step; skip: the guard's int32 device flag, as in adam_ema_)."""
    lib = _lib.load()
    _req_cuda(p, g, s1, s2, ema)
    IMAGES.params_rewritten()
    if skip is not None:
        if lr_dev is None:
            raise ValueError('optim_step_: a guarded launch needs the step size on the device (lr_dev)')
        check(lib.sg_optim_step_guarded(int(kind), _ptr(p), _ptr(g), _ptr(s1), _ptr(s2), _ptr(ema), p.numel(), _dev_ptr(lr_dev),
                                        _ptr(skip), float(h), float(eps), 1 if nesterov else 0, float(gscale),
                                        float(ema_decay), _stream()), 'sg_optim_step_guarded')
        return
    if lr_dev is not None:
        check(lib.sg_optim_step_dev(int(kind), _ptr(p), _ptr(g), _ptr(s1), _ptr(s2), _ptr(ema), p.numel(), _dev_ptr(lr_dev), float(h),
                                    float(eps), 1 if nesterov else 0, float(gscale), float(ema_decay), _stream()),
              'sg_optim_step_dev')
        return
    check(lib.sg_optim_step(int(kind), _ptr(p), _ptr(g), _ptr(s1), _ptr(s2), _ptr(ema), p.numel(), float(lr), float(h),
                            float(eps), 1 if nesterov else 0, float(gscale), float(ema_decay), _stream()),
          'sg_optim_step')


def segment_table_arrays(segments, total, chunk=_lib.SG_SEG_CHUNK):
    """Host half of SegmentTable: segments [(start, count, decay flag)] of a flat buffer of `total` elements ->
    (segs [[start, count, flag, first block]], blocks [[segment, chunk]]) as include/saragan_hip.h lays them out."""
    segs, blocks, end = [], [], 0
    for s, (start, count, flag) in enumerate(sorted((int(a), int(b), int(bool(c))) for a, b, c in segments)):
        if start % 4 or count < 1 or start < end or start + count > total:
            raise ValueError(f'segment [{start}, {start + count}) of a flat buffer of {total}: starts must be multiples of 4 and '
                             f'segments disjoint and inside the buffer')
        end = start + count
        segs.append([start, count, flag, len(blocks)])
        blocks.extend([s, c] for c in range((count + chunk - 1) // chunk))
    if not segs:
        raise ValueError('a segment table needs at least one segment')
    return segs, blocks


class SegmentTable:
    """Device table of a train op's variables for the segmented optimiser launches (sg_adamw_ema, sg_lamb_*), with LAMB's
    workspace: per-block partial sums and per-segment trust ratios.  Built once per train op (it copies to the device);
    a step only launches with it."""

    def __init__(self, segments, total, device):
        segs, blocks = segment_table_arrays(segments, total)
        self.total, self.nseg, self.nblocks = int(total), len(segs), len(blocks)
        self.segs = torch.tensor(segs, dtype=torch.int64).to(device)
        self.blocks = torch.tensor(blocks, dtype=torch.int32).to(device)
        self.partials = torch.zeros(2 * self.nblocks, dtype=torch.float32, device=device)
        self.ratios = torch.ones(self.nseg, dtype=torch.float32, device=device)

    def check(self, *bufs):
        _req_cuda(*bufs)
        for b in bufs:
            if b is not None and (b.dtype != torch.float32 or not b.is_contiguous() or b.numel() != self.total):
                raise ValueError(f'the segment table describes contiguous float32 buffers of {self.total} elements')


def adamw_ema_(table, p, g, m, v, ema, lr, beta1, beta2, eps=1e-6, decay=0.0, gscale=1.0, ema_decay=0.99, lr_dev=None,
               skip=None):
    """In-place AdamW (no bias correction; decay on the table's flagged segments) + EMA over the segments of whole flat f32
    buffers: ONE launch (sg_adamw_ema).  lr_dev / skip as in adam_ema_."""
    lib = _lib.load()
    table.check(p, g, m, v, ema)
    if skip is not None and lr_dev is None:
        raise ValueError('adamw_ema_: a guarded launch needs the step size on the device (lr_dev)')
    IMAGES.params_rewritten()
    check(lib.sg_adamw_ema(_ptr(p), _ptr(g), _ptr(m), _ptr(v), _ptr(ema), table.total, _ptr(table.segs), _ptr(table.blocks),
                           table.nseg, table.nblocks, float(lr), None if lr_dev is None else _dev_ptr(lr_dev), _ptr(skip),
                           float(beta1), float(beta2), float(eps), float(decay), float(gscale), float(ema_decay), _stream()),
          'sg_adamw_ema')


def lamb_ema_(table, p, g, m, v, ema, t, lr, beta1, beta2, eps=1e-6, decay=0.0, gscale=1.0, ema_decay=0.99, lr_dev=None,
              skip=None):
    """In-place LAMB + EMA over the segments of whole flat f32 buffers: moments and per-block norms (sg_lamb_moments), one
    trust ratio per segment (sg_lamb_ratios), update (sg_lamb_update) -- three launches whatever the number of segments.
    t: the int64 [1] device count of applied updates.  Unguarded, the launches advance it; with skip (the guard's flag;
    needs lr_dev) sg_guard_step has advanced it already, and a set flag leaves everything but the EMA as it was."""
    lib = _lib.load()
    table.check(p, g, m, v, ema)
    _req_cuda(t)
    if t.dtype != torch.int64:
        raise TypeError('lamb_ema_: the step count is an int64 device tensor')
    if skip is not None and lr_dev is None:
        raise ValueError('lamb_ema_: a guarded launch needs the step size on the device (lr_dev)')
    IMAGES.params_rewritten()
    advance = 0 if skip is not None else 1
    tab = (_ptr(table.segs), _ptr(table.blocks), table.nseg, table.nblocks)
    check(lib.sg_lamb_moments(_ptr(p), _ptr(g), _ptr(m), _ptr(v), table.total, *tab, _ptr(table.partials), _ptr(t), advance,
                              _ptr(skip), float(beta1), float(beta2), float(eps), float(decay), float(gscale), _stream()),
          'sg_lamb_moments')
    check(lib.sg_lamb_ratios(_ptr(table.segs), table.nseg, table.nblocks, _ptr(table.partials), _ptr(table.ratios), _ptr(t),
                             advance, _ptr(skip), _stream()), 'sg_lamb_ratios')
    check(lib.sg_lamb_update(_ptr(p), _ptr(m), _ptr(v), _ptr(ema), table.total, *tab, _ptr(table.ratios), _ptr(t), float(lr),
                             None if lr_dev is None else _dev_ptr(lr_dev), _ptr(skip), float(beta1), float(beta2), float(eps),
                             float(decay), float(ema_decay), _stream()), 'sg_lamb_update')
