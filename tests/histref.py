"""numpy restatement of sg_intensity_hist (csrc/hist.hip) and loop versions of the three histogram distances of
saragan_amd/metrics/intensity_metrics.py, written from the definition and not from the code under test:

  t      = x * scale + shift in float32, a product and then a sum, each rounded on its own (numpy's float32 arithmetic)
  column = bins                          where t is NaN
           bins - 1                      where t >= lo + bins  (+inf too): saturated, and the top edge is closed
           0                             where t <  lo         (-inf too)
           min(floor(t) - lo, bins - 1)  otherwise
The comparisons are made on the float (in float64, which holds every float32 and every 32-bit integer exactly)."""
from fractions import Fraction

import numpy as np


def to_f32(x):
    """x as float32: every input type of the kernel converts exactly (bf16 has no numpy type: the caller passes the values
    of bf16_bits_to_f32)."""
    return np.asarray(x).astype(np.float32)


def bf16_bits_to_f32(bits):
    return (np.asarray(bits).astype(np.uint32) << 16).view(np.float32)


def mapped(x, scale, shift):
    with np.errstate(all='ignore'):
        return to_f32(x) * np.float32(scale) + np.float32(shift)


def columns(x, lo, hi, scale=1.0, shift=0.0):
    t = mapped(x, scale, shift).astype(np.float64)
    bins = hi - lo
    nan = np.isnan(t)
    safe = np.where(nan, lo, t)
    with np.errstate(all='ignore'):
        q = np.floor(np.clip(safe, lo, hi))        # saturation decided on the float, before the conversion
    col = np.minimum(q.astype(np.int64) - lo, bins - 1)
    col[safe >= hi] = bins - 1
    col[safe < lo] = 0
    col[nan] = bins
    return col


def hist(x, lo, hi, scale=1.0, shift=0.0, pooled=False):
    """int64 [rows, hi - lo + 1] of x [n, ...]."""
    x = np.asarray(x)
    col = columns(x, lo, hi, scale, shift).reshape(1 if pooled else x.shape[0], -1)
    return np.stack([np.bincount(r, minlength=hi - lo + 1) for r in col]).astype(np.int64)


def distances(h_real, h_fake):
    """ks, w1, max_density_gap of two count vectors [bins + 1] in exact rationals, by the textbook loops."""
    r = [int(v) for v in np.asarray(h_real).reshape(-1)[:-1]]
    f = [int(v) for v in np.asarray(h_fake).reshape(-1)[:-1]]
    tr, tf = sum(r), sum(f)
    ks = w1 = gap = Fraction(0)
    for k in range(len(r)):
        cdf_r, cdf_f = Fraction(sum(r[:k + 1]), tr), Fraction(sum(f[:k + 1]), tf)
        ks = max(ks, abs(cdf_r - cdf_f))
        w1 += abs(cdf_r - cdf_f)
        gap = max(gap, abs(Fraction(r[k], tr) - Fraction(f[k], tf)))
    return {'ks': float(ks), 'w1': float(w1), 'max_density_gap': float(gap)}
