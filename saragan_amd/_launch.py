"""What every launch needs and nothing else: dtype codes, the current stream, layout and shape helpers.  No state; imports only
_lib.  (Layer 0 of the map in functional.py's docstring.)"""
import ctypes as C

import torch

from . import _lib

_DT = {torch.float32: _lib.SG_F32, torch.bfloat16: _lib.SG_BF16}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f'saragan_amd supports float32 and bfloat16 activations, got {t.dtype}')


def _req_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('saragan_amd ops run on the GPU only (no CPU fallback); got a CPU tensor')


def ndhwc(x):
    """Returns x stored as NDHWC (5-D: channels_last_3d; 2-D: row-major)."""
    if x.dim() == 5:
        return x.contiguous(memory_format=torch.channels_last_3d)
    if x.dim() == 2:
        return x.contiguous()
    raise ValueError(f'expected a [N,C,D,H,W] or [N,F] tensor, got shape {tuple(x.shape)}')


def _dims(x):
    """-> (n, c, d, h, w) of an NCDHW / [N,F] tensor."""
    if x.dim() == 5:
        n, c, d, h, w = x.shape
        return n, c, d, h, w
    n, c = x.shape
    return n, c, 1, 1, 1


def _empty_like_shape(x, c_out, spatial=None, dtype=None):
    n, _, d, h, w = _dims(x)
    if spatial is not None:
        d, h, w = spatial
    dtype = dtype or x.dtype
    if x.dim() == 5:
        return torch.empty((n, c_out, d, h, w), device=x.device, dtype=dtype, memory_format=torch.channels_last_3d)
    return torch.empty((n, c_out), device=x.device, dtype=dtype)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None
