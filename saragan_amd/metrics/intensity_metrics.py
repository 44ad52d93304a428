"""Voxel-intensity histogram metrics of a set of real and a set of generated volumes, in data units (CT: Hounsfield units).
The reference's metrics/kms.py builds a unit-wide histogram per image with np.histogram on the host, averages the densities
and reports the largest gap between the real and the generated one; it notes "To Do: across the laplacian pyramid".  Here the
histograms are counted on the device (`sg_intensity_hist`, csrc/hist.hip, through functional.intensity_hist) over the volumes
AND over the detail levels of the Laplacian pyramid the SWD code builds, and three distances are read off the counts:

  * ks               max_k |CDF_r(k) - CDF_f(k)|: the Kolmogorov-Smirnov distance of the binned distributions;
  * w1               sum_k |CDF_r(k) - CDF_f(k)|: their Wasserstein-1 distance in data units (bins are one unit wide);
  * max_density_gap  max_k |p_r(k) - p_f(k)|: the reference's statistic.

Histograms of sets add, so nothing but two count vectors per level is kept: an evaluation accumulates batch by batch
(IntensityAccumulator) and the command line streams directories of any size.

    python -m saragan_amd.metrics.intensity_metrics REAL_DIR FAKE_DIR --range LO,HI [--levels N] [--max_samples N]
                                                    [--scale S --shift T] [--batch 16]

evaluates two directories of .npy volumes; the files' own dtype goes to the kernel where it reads that dtype."""
import numpy as np
import torch

from .. import functional as F
from ..table_ops import HIST_DT
from . import swd as SWD


def _counts(h):
    if torch.is_tensor(h):
        h = h.cpu().numpy()
    h = np.asarray(h).reshape(-1)
    if h.size < 2 or not np.issubdtype(h.dtype, np.integer):
        raise ValueError(f'expected an integer count vector [bins + 1], got {h.dtype} {h.shape}')
    return [int(v) for v in h]


def histogram_distances(h_real, h_fake):
    """The three distances of two count vectors [bins + 1] (the last column counts NaN: it is left out of the distributions
    and reported as nan_real / nan_fake).  The differences are formed in exact integers, |C_r T_f - C_f T_r| with the totals
    T and one division at the end: equal inputs give exactly 0, a shift by d bins gives w1 == d exactly."""
    r, f = _counts(h_real), _counts(h_fake)
    if len(r) != len(f):
        raise ValueError(f'count vectors of {len(r)} and {len(f)} columns')
    nan_r, nan_f = r.pop(), f.pop()
    tr, tf = sum(r), sum(f)
    if tr == 0 or tf == 0:
        raise ValueError(f'a side without finite elements: {tr} real, {tf} generated')
    ks = w1 = gap = cr = cf = 0
    for a, b in zip(r, f):
        cr += a
        cf += b
        d = abs(cr * tf - cf * tr)
        ks = max(ks, d)
        w1 += d
        gap = max(gap, abs(a * tf - b * tr))
    den = tr * tf
    return {'ks': ks / den, 'w1': w1 / den, 'max_density_gap': gap / den, 'nan_real': nan_r, 'nan_fake': nan_f}


def usable_levels(shape, levels):
    """How many of `levels` exist for volumes of this shape: level k >= 1 halves the extents of level k - 1, which must all be
    even (the pyramid's minimum: pyr_up(pyr_down(x)) has x's shape only then)."""
    if levels <= 1:
        return max(levels, 0)
    if len(shape) != 5:
        raise ValueError(f'pyramid levels need [n, c, d, h, w] volumes, got {tuple(shape)}')
    ext, k = list(shape[2:]), 1
    while k < levels and all(e >= 2 and e % 2 == 0 for e in ext):
        ext = [e // 2 for e in ext]
        k += 1
    return k


class IntensityAccumulator:
    """Pooled histograms of everything passed to add(), per level, for reals and fakes: two int64 [levels][1][bins + 1] device
    buffers, no volume is kept.  Level 0 is the volumes themselves over [lo, hi] after x * scale + shift.  Level k >= 1 is
    detail level k - 1 of swd.generate_laplacian_pyramid(x, levels) (full resolution first; the low-pass residual is not
    used): detail coefficients are signed, so they are counted over the symmetric range [-(hi - lo) // 2, (hi - lo) // 2]
    after x * scale, without the shift."""

    def __init__(self, lo, hi, scale=1.0, shift=0.0, levels=1):
        lo, hi, levels = int(lo), int(hi), int(levels)
        if hi <= lo:
            raise ValueError(f'the range [{lo}, {hi}] is empty')
        if levels < 1:
            raise ValueError(f'levels must be >= 1, got {levels}')
        if levels > 1 and (hi - lo) // 2 < 1:
            raise ValueError(f'the range [{lo}, {hi}] leaves no bins for the detail levels')
        self.lo, self.hi, self.scale, self.shift, self.levels = lo, hi, float(scale), float(shift), levels
        self.real = self.fake = None
        self.samples = 0

    def level_range(self, level):
        half = (self.hi - self.lo) // 2
        return (self.lo, self.hi) if level == 0 else (-half, half)

    def _start(self, x):
        got = usable_levels(x.shape, self.levels)
        if got < self.levels:
            print(f'Intensity histograms stop at level {got}: volumes of {"x".join(map(str, x.shape[2:]))} leave an odd or '
                  f'empty extent there ({self.levels} levels were asked for)')
            self.levels = got
        shape = (self.levels, 1, self.hi - self.lo + 1)
        self.real = torch.zeros(shape, dtype=torch.int64, device=x.device)
        self.fake = torch.zeros(shape, dtype=torch.int64, device=x.device)

    def _row(self, buf, level):
        """The [1, bins of the level + 1] counts of a level: with an odd hi - lo a detail level is one column narrower than the
        buffer (a view of one row, so still contiguous)."""
        lo, hi = self.level_range(level)
        return buf[level][:, :hi - lo + 1]

    def _add_side(self, x, buf, keep):
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError('saragan_amd.metrics run on the GPU only (no CPU fallback)')
        if x.dtype not in HIST_DT:
            x = x.to(torch.float32)
        x = x.contiguous()
        F.intensity_hist(x, self.lo, self.hi, self.scale, self.shift, pooled=True, out=self._row(buf, 0), accumulate=True)
        if self.levels > 1:
            pyramid = SWD.generate_laplacian_pyramid(x, self.levels)
            if keep is not None:
                keep.append([p.cpu().numpy() for p in pyramid])
            lo, hi = self.level_range(1)
            for k in range(1, self.levels):
                F.intensity_hist(pyramid[k - 1], lo, hi, self.scale, 0.0, pooled=True, out=self._row(buf, k), accumulate=True)

    def add(self, real_batch, fake_batch, keep=None):
        """Counts one batch of each side into the buffers (launches only: no copy to the host, no synchronisation).  `keep`: a
        list that receives the two pyramids as lists of numpy arrays, the reals' first (tests; levels > 1 only)."""
        if self.real is None:
            self._start(real_batch)
        self._add_side(real_batch, self.real, keep)
        self._add_side(fake_batch, self.fake, keep)
        self.samples += int(real_batch.shape[0])

    def counts(self):
        """Per level, the (real, fake) count vectors as numpy int64 [bins of the level + 1]."""
        if self.real is None:
            raise ValueError('nothing was added')
        real, fake = self.real.cpu().numpy(), self.fake.cpu().numpy()
        out = []
        for k in range(self.levels):
            lo, hi = self.level_range(k)
            out.append((real[k, 0, :hi - lo + 1], fake[k, 0, :hi - lo + 1]))
        return out

    def result(self):
        """{'intensity_ks': [...], 'intensity_w1': [...], 'intensity_gap': [...]}, one entry per level."""
        m = {'intensity_ks': [], 'intensity_w1': [], 'intensity_gap': []}
        for r, f in self.counts():
            d = histogram_distances(r, f)
            m['intensity_ks'].append(d['ks'])
            m['intensity_w1'].append(d['w1'])
            m['intensity_gap'].append(d['max_density_gap'])
        return m


def get_intensity_metrics(real, fake, lo, hi, scale=1.0, shift=0.0, levels=1):
    """real, fake: device tensors [n, ...] ([n, c, d, h, w] for levels > 1).  Keys intensity_ks, intensity_w1, intensity_gap,
    each a list with one value per level (see IntensityAccumulator for the levels)."""
    acc = IntensityAccumulator(lo, hi, scale, shift, levels)
    acc.add(real, fake)
    return acc.result()


def format_lines(m):
    """The stdout lines of the metrics in `m` (save_metrics and the command line print the same text)."""
    fmt = lambda vs: ' '.join(f'{v:.6g}' for v in vs)
    lines = []
    if 'intensity_ks' in m:
        lines.append(f"Intensity KS (per level): {fmt(m['intensity_ks'])}")
    if 'intensity_w1' in m:
        lines.append(f"Intensity W1 (per level, data units): {fmt(m['intensity_w1'])}")
    if 'intensity_gap' in m:
        lines.append(f"Intensity max density gap (per level): {fmt(m['intensity_gap'])}")
    return lines


def parse_range(text):
    """'LO,HI' -> (lo, hi), integers in data units with hi > lo; ValueError otherwise."""
    parts = str(text).split(',')
    if len(parts) != 2:
        raise ValueError(f'expected LO,HI, got {text!r}')
    lo, hi = int(parts[0]), int(parts[1])
    if hi <= lo:
        raise ValueError(f'the range {lo},{hi} is empty')
    return lo, hi


def _names(path, max_samples):
    import os
    names = sorted(f for f in os.listdir(path) if f.endswith('.npy'))
    if max_samples is not None:
        names = names[:max_samples]
    if not names:
        raise SystemExit(f'{path}: no .npy files')
    return [os.path.join(path, f) for f in names]


_NUMPY_NATIVE = ('uint8', 'int8', 'int16', 'uint16', 'float16', 'float32')


def _load_batch(files, shape):
    vols = [np.load(f) for f in files]
    for f, v in zip(files, vols):
        if v.shape != shape:
            raise SystemExit(f'{f}: shape {v.shape}, the first volume has {shape}')
    x = np.stack(vols)
    if x.dtype.name not in _NUMPY_NATIVE:
        x = x.astype(np.float32)
    if x.ndim == 4:      # [n, d, h, w] -> one channel
        x = x[:, None]
    return torch.from_numpy(np.ascontiguousarray(x)).to('cuda')


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog='python -m saragan_amd.metrics.intensity_metrics', description=__doc__.split('\n\n')[0])
    p.add_argument('real_dir')
    p.add_argument('fake_dir')
    p.add_argument('--range', required=True, help='LO,HI in data units: unit-wide bins over [LO, HI] (a negative LO: --range=LO,HI)')
    p.add_argument('--levels', type=int, default=1, help='1: the volumes; N: plus N - 1 detail levels of the Laplacian pyramid')
    p.add_argument('--max_samples', type=int, default=None)
    p.add_argument('--scale', type=float, default=1.0, help='with --shift: the files hold (data - shift) / scale')
    p.add_argument('--shift', type=float, default=0.0)
    p.add_argument('--batch', type=int, default=16, help='volumes per launch: only this many are held at a time')
    args = p.parse_args(argv)
    try:
        lo, hi = parse_range(args.range)
    except ValueError as e:
        raise SystemExit(f'--range: {e}')
    if args.batch < 1 or args.levels < 1:
        raise SystemExit('--batch and --levels must be >= 1')
    real, fake = _names(args.real_dir, args.max_samples), _names(args.fake_dir, args.max_samples)
    n = min(len(real), len(fake))
    shape = np.load(real[0], mmap_mode='r').shape
    if not torch.cuda.is_available():
        raise RuntimeError('saragan_amd.metrics run on the GPU only (no CPU fallback)')
    acc = IntensityAccumulator(lo, hi, args.scale, args.shift, args.levels)
    for at in range(0, n, args.batch):
        acc.add(_load_batch(real[at:at + args.batch], shape), _load_batch(fake[at:at + args.batch], shape))
    print(f'{n} real and {n} generated volumes of shape {tuple(shape)}')
    m = acc.result()
    for line in format_lines(m):
        print(line)
    return m


if __name__ == '__main__':
    main()
