"""Step scalars that live on the device as well as on the host: what the kernels of a captured step read (the lerp weights, the
optimisers' step sizes, the guard's learning rate).  Shared by functional's lerp and the optimiser and guard launches."""
import ctypes as C

import torch

from ._launch import _ptr


class DevCoef(float):
    """A step scalar that ALSO lives in device memory (element `idx` of `buf`, f32): the value a kernel of a captured step
    reads (sg_axpby_dev, sg_adam_ema_dev).  Behaves as its host value everywhere else."""

    def __new__(cls, value, buf, idx):
        o = float.__new__(cls, value)
        o.buf, o.idx = buf, int(idx)
        return o

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.buf.element_size() * self.idx)


def _dev_ptr(x):
    """Device address of a one-element step scalar: a DevCoef, or a tensor (its first element)."""
    return x.ptr() if isinstance(x, DevCoef) else _ptr(x)


class DevScalars:
    """The per-step scalars of a captured step (optimization.StepGraph): fade-in weights [alpha, 1 - alpha] and the step size
    of each optimiser.  The host writes them into a pinned mirror (`set`) and `flush()` sends all of them with one
    asynchronous copy before the graph is replayed; the captured kernels read the device copy.  The values are the f32
    roundings of the doubles the eager path hands to ctypes: the same bits reach the same arithmetic.
    A replayed step costs the host next to nothing, so it runs ahead of the device: the pinned source of a copy that has not
    executed yet must not be rewritten (with ONE mirror a replay could read the alpha / step size of a later
    step).  The mirror is a ring of pinned slots, each with the event recorded behind its last copy; a slot is rewritten only
    after that event (the host waits only if it is RING flushes ahead)."""
    RING = 8

    def __init__(self, device, n=8, dtype=torch.float32):
        cuda = torch.device(device).type == 'cuda'
        self._ring = [torch.zeros(n, dtype=dtype).pin_memory() if cuda else torch.zeros(n, dtype=dtype)
                      for _ in range(self.RING if cuda else 1)]
        self._events = [None] * len(self._ring)
        self._cur = 0
        self.host = self._ring[0]
        self.dev = torch.zeros(n, dtype=dtype, device=device)
        self.waits = 0            # times the host had to wait for a slot (tests)

    def set(self, idx, value):
        self.host[idx] = float(value)

    def coef(self, idx, value):
        self.set(idx, value)
        return DevCoef(value, self.dev, idx)

    def flush(self):
        self.dev.copy_(self.host, non_blocking=True)
        if len(self._ring) == 1:
            return
        ev = self._events[self._cur]
        if ev is None:
            ev = self._events[self._cur] = torch.cuda.Event()
        ev.record()
        nxt = (self._cur + 1) % len(self._ring)
        if self._events[nxt] is not None and not self._events[nxt].query():
            self._events[nxt].synchronize()
            self.waits += 1
        self._ring[nxt].copy_(self.host)      # values not set again keep theirs
        self._cur, self.host = nxt, self._ring[nxt]
