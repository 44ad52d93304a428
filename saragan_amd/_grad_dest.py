"""Where a backward Function's parameter gradients go: the slots of the step's flat gradient buffer (grads_into), the parameters
whose gradients are not wanted at all (skip_param_grads), and the shared placeholder for 'no bias gradient'.  State is mutated in
place only, so functional's re-exported references are the live ones."""
import contextlib
import math

import torch

from . import _lib

_ZERO = {}


def _zero_scalar(like):
    """A shared 0-d placeholder for 'no bias gradient' outputs (a fresh new_zeros(()) is one fill launch each,
    ~60 per step)."""
    z = _ZERO.get(like.device)
    if z is None:
        z = _ZERO[like.device] = torch.zeros((), device=like.device, dtype=torch.float32)
    return z.detach()    # a new tensor object over the same storage: autograd may tag it per Function


_SKIP = {'ptrs': frozenset()}
_GRAD_DEST = {}      # parameter data_ptr -> [f32 view of the step's flat gradient buffer, claimed]
ACCUMULATED_IN_PLACE = set()   # data_ptr of the parameters whose slot took a later contribution in place during this backward
GRAD_DEST_STATS = {'claimed': 0, 'accumulated': 0, 'adopted': 0, 'copied': 0, 'unreached': 0}   # counters for the tests (host side only)


@contextlib.contextmanager
def grads_into(dest, enabled=True):
    """dest: {parameter data_ptr: view of the flat gradient buffer shaped like the parameter}.  Inside this context (the
    torch.autograd.backward of one training step, optimization.StepGraph._backward) the FIRST weight / bias gradient a
    backward Function computes for a registered parameter is written by its kernel straight into that view and handed to
    autograd as such: AccumulateGrad keeps a gradient tensor nobody else holds as .grad, so the parameter's gradient is
    in the optimiser's buffer without the zero-fill + `add` launch per parameter (71 per step at the benchmarked
    configuration, 0.37 ms).  Further contributions to the same parameter (the gradient penalty's second-order term of the
    discriminator's weights) are tensors of their own, summed by autograd; a sum that ended up outside the buffer is
    copied in by the caller (StepGraph._land).  enabled=False (functional passes its NO_GRAD_DEST switch): no slot is
    registered, every gradient is a tensor of its own."""
    prev = dict(_GRAD_DEST)
    _GRAD_DEST.clear()
    ACCUMULATED_IN_PLACE.clear()
    if enabled:
        _GRAD_DEST.update({k: [v, False] for k, v in dest.items()})
    try:
        yield
    finally:
        _GRAD_DEST.clear()
        _GRAD_DEST.update(prev)


def _grad_out(ptr, shape):
    """A fresh alias (f32, `shape`) of the flat-buffer slot registered for parameter `ptr` if no gradient has been written
    to it in this backward, else None.  Never while a graph of the backward is being recorded (create_graph)."""
    if not ptr or not _GRAD_DEST or torch.is_grad_enabled():
        return None
    ent = _GRAD_DEST.get(ptr)
    if ent is None or ent[1] or ent[0].numel() != math.prod(shape):
        return None
    ent[1] = True
    GRAD_DEST_STATS['claimed'] += 1
    return ent[0].view(shape)


def _grad_acc(ptr, shape):
    """The slot registered for parameter `ptr` when a gradient HAS been written to it in this backward (by a kernel of this
    package: the alias is with autograd, waiting for the parameter's other contributions) -- a kernel that accumulates
    (sg_conv3d_wgrad_bias_ex, SG_WGRAD_ACCUMULATE) adds the next contribution in place and the Function returns None for it."""
    if not ptr or not _GRAD_DEST or torch.is_grad_enabled():
        return None
    ent = _GRAD_DEST.get(ptr)
    if ent is None or not ent[1] or ent[0].numel() != math.prod(shape):
        return None
    return ent[0].view(shape)


def _note_accumulated(ptr):
    """A kernel HAS added a contribution in place to the slot of parameter `ptr` (the launch was not declined).  From here on the
    slot holds more than what autograd was handed: sound only while every later contribution is made in place too -- one that
    arrives as a tensor of its own makes the engine sum OUT of place (V1 + T2 elsewhere), and copying that sum over the slot would
    drop what was added here.  StepGraph._land refuses that case."""
    ACCUMULATED_IN_PLACE.add(ptr)
    GRAD_DEST_STATS['accumulated'] += 1


def _unclaim(ptr, t):
    """The launch that was to write `t` declined (SG_EUNSUPPORTED: nothing was written) and the caller takes another path: if
    `t` is the slot of parameter `ptr`, the slot is free again.  (A slot that stayed claimed without being handed to autograd
    would take later contributions in place -- _grad_acc -- while the parameter's .grad is built from other tensors.)"""
    ent = _GRAD_DEST.get(ptr) if (ptr and t is not None) else None
    if ent is not None and ent[1] and t.data_ptr() == ent[0].data_ptr():
        ent[1] = False
        GRAD_DEST_STATS['claimed'] -= 1


def _f32_out(ptr, shape, device):
    out = _grad_out(ptr, shape)
    return out if out is not None else torch.empty(shape, device=device, dtype=torch.float32)


class _GradOuts:
    """The f32 outputs of ONE launch that may decline (SG_EUNSUPPORTED: nothing was written, the caller takes another path).
    take() hands each one out like _f32_out -- the parameter's slot when it is free, else a fresh tensor; declined(rc) / release()
    frees exactly the slots that were claimed here (_unclaim says why none may be forgotten), fresh tensors are nobody's business."""

    def __init__(self, device):
        self.device, self.claimed = device, []

    def take(self, ptr, shape, want=True):
        if not want:
            return None
        out = _grad_out(ptr, shape)
        if out is None:
            return torch.empty(shape, device=self.device, dtype=torch.float32)
        self.claimed.append((ptr, out))
        return out

    def release(self):
        for ptr, out in self.claimed:
            _unclaim(ptr, out)
        self.claimed = []

    def declined(self, rc):
        if rc != _lib.SG_EUNSUPPORTED:
            return False
        self.release()
        return True


@contextlib.contextmanager
def skip_param_grads(params):
    """Inside this context the backward Functions do not compute gradients of the given parameters.
    `ctx.needs_input_grad` is True for every weight that requires grad, also when the caller asked autograd for other
    inputs only (the gradient-penalty d D/d x pass, networks/loss.py:136-139; the generator loss flowing through the
    discriminator, optimization.py:128-163): the weight/bias-gradient kernels would run and their results be dropped."""
    prev = _SKIP['ptrs']
    _SKIP['ptrs'] = prev | frozenset(p.data_ptr() for p in params)
    try:
        yield
    finally:
        _SKIP['ptrs'] = prev


def _wants(ctx, i, ptr):
    return ctx.needs_input_grad[i] and ptr not in _SKIP['ptrs']
