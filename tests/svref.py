"""Inputs for the store_volumes tests: values that sit on every edge of the definition, and a set on which a fused
multiply-add would round differently from the two operations the definition asks for."""
import numpy as np
import torch

T_OUT = {'i16': torch.int16, 'u16': torch.uint16, 'u8': torch.uint8, 'f32': torch.float32}
T_SRC = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}
# (scale, shift, clip) per output type: the reference's int16 recipe, prepare_data's uint16 default, a narrow uint8 window, and
# float32 with bounds that are no integers
CONFIG = {'i16': (1024.0, 0.0, (-1024, 2048)), 'u16': (1024.0, 1024.0, None), 'u8': (64.0, 100.0, (3, 250)),
          'f32': (1024.0, 1024.0, (-1.5, 3000.25))}


def neighbours(values, dtype):
    """Every value with the representable numbers one step below and above it, in dtype."""
    t = torch.tensor(values, dtype=dtype)
    bits = t.view(torch.int32 if dtype == torch.float32 else torch.int16)
    return torch.cat([t, (bits + 1).view(dtype), (bits - 1).view(dtype)])


def edge_values(dtype, scale, shift, lo, hi):
    """Source values x (1-D, dtype) whose t = x * scale + shift lands on ties k + 0.5 of both signs, on lo and hi and next to them,
    plus +-0, +-inf, NaN and +-1e10."""
    lo = -8.0 if np.isinf(lo) else float(lo)
    hi = 8.0 if np.isinf(hi) else float(hi)
    ties = [k + 0.5 for k in range(-6, 7)] + [lo + 0.5, lo + 1.5, hi - 0.5, hi - 1.5, (lo + hi) // 2 + 0.5, (lo + hi) // 2 + 1.5]
    targets = ties + [lo, hi, lo - 1.0, hi + 1.0, lo + 0.75, hi - 0.25, -0.75, -0.25, 0.25, 0.75]
    x = [(t - shift) / scale for t in targets]
    return torch.cat([neighbours(x, dtype), torch.tensor([0.0, -0.0, np.inf, -np.inf, np.nan, 1e10, -1e10, 1.0, -1.0], dtype=dtype)])


def make_input(name, shape, scale, shift, lo, hi, seed=0):
    """A CPU tensor of `shape` in the source type `name`: normal draws that reach past both clip bounds, the edge values in
    front (as many as fit)."""
    dtype = T_SRC[name]
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    lo_ = -8.0 if np.isinf(lo) else float(lo)
    hi_ = 8.0 if np.isinf(hi) else float(hi)
    mid, half = ((lo_ + hi_) / 2 - shift) / scale, (hi_ - lo_) / 2 / scale
    x = (torch.randn(n, generator=g) * (0.7 * half) + mid).to(dtype)
    e = edge_values(dtype, scale, shift, lo, hi)[:n]
    x[:e.numel()] = e
    return x.reshape(shape)


def fma_sensitive(count=4096, seed=5):
    """(x f32 [count], scale, shift): |x| in [0.5, 2), so that x * scale + shift is EXACT in float64 (50 significant bits at most)
    and one rounding of it to float32 is what a fused multiply-add gives.  Returns also the two float32 results: (x, scale, shift,
    two_ops, fused)."""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(0.5, 2.0, count) * rng.choice([-1.0, 1.0], count)).astype(np.float32)
    scale, shift = np.float32(1023.7), np.float32(1024.3)
    two = x * scale + shift
    fused = (x.astype(np.float64) * np.float64(scale) + np.float64(shift)).astype(np.float32)
    return x, float(scale), float(shift), two, fused


def recompute_stats(stored, below, above, nan):
    """int64 [n, 7] from the stored array and the three boolean masks, directly."""
    n = stored.shape[0]
    st = np.zeros((n, 7), np.int64)
    for i in range(n):
        if stored.dtype.kind in 'iu' and stored[i].size:
            s = [int(v) for v in stored[i].reshape(-1)]
            st[i, :4] = [sum(s), sum(v * v for v in s), min(s), max(s)]
        st[i, 4:] = [int(below[i].sum()), int(above[i].sum()), int(nan[i].sum())]
    return st
