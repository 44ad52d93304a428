"""Power-spectrum metrics of a set of real and a set of generated volumes.  Both generators up-sample by
nearest-neighbour repetition followed by a convolution, the construction known to leave a fingerprint in the high-frequency
tail of the spectrum (Durall et al. 2020; Dzanic et al. 2020), and for CT the noise power spectrum is the standard description of
noise texture.  Per volume the device computes the shell-binned power spectrum (`sg_power_spectrum`, csrc/spectrum.hip, through
table_ops.power_spectrum: a direct 3-D DFT on f64 MFMAs): sums of g |F|^2 per radial column of |f| in cycles / mm and per |k|
along each axis.  Spectra of sets add, so nothing but two f64 sum vectors is kept (SpectrumAccumulator), and the distances are
read off the means P[c] = sum over samples / (n * coefficients in c):

  * spectrum_lsd            sqrt(mean_c (10 log10(P_real[c] / P_fake[c]))^2) in dB: the log-spectral distance over the radial
                            columns c >= 1 that are non-empty and positive on both sides (the number skipped is reported);
  * spectrum_lsd_d|h|w      the same over the axis profiles, q >= 1 (an axis of extent 1 has none and is left out);
  * spectrum_hf_excess      10 log10(sum_{c > 3 B / 4} fake / sum_{c > 3 B / 4} real) in dB of the per-sample means: positive
                            means too much fine grain or checkerboard, negative means blur.

Equal sets give exactly 0.0 everywhere.  With --window hann the mean is not removed: DC leaks into |k| <= 1 per axis, equally
for both sets.

    python -m saragan_amd.metrics.spectrum_metrics REAL_DIR FAKE_DIR [--spacing d,h,w] [--bins B] [--window none|hann]
                                                   [--max_samples N] [--scale S --shift T] [--batch 8] [--device cuda|cpu]
                                                   [--report JSON]

evaluates two directories of .npy volumes in the files' own dtype and writes a report (default FAKE_DIR/spectrum.json)."""
import math

import numpy as np
import torch

from .. import _lib
from ..table_ops import HIST_DT, SPECTRUM_WINDOWS, SpectrumPlan, power_spectrum

DEFINITION = ('t = f64(x) * scale + shift; F = the 3-D DFT of t (kw = 0 .. W // 2, weight g = 1 at kw = 0 and kw = W / 2, else 2); '
              'radial[c] = sum g |F|^2 over r2 = (f2_d + f2_h) + f2_w in column c, f2 = (min(k, n - k) / (n * spacing))^2, '
              'column 0 = DC, else min(1 + #{b >= 1: (b sqrt(top) / B)^2 <= r2}, B); axis profiles: the same sums over '
              'min(k, n - k) = q per axis; means divide by samples * weighted coefficients')


def _db(ratio):
    return 10.0 * math.log10(ratio)


def _lsd(real, fake, counts, n_real, n_fake):
    """(log-spectral distance in dB over the bins 1 .., bins skipped): Python floats on the accumulated sums."""
    sq, used, skipped = 0.0, 0, 0
    for r, f, c in zip(real[1:], fake[1:], counts[1:]):
        r, f, c = float(r), float(f), float(c)
        if c > 0 and r > 0 and f > 0 and math.isfinite(r) and math.isfinite(f):
            pr, pf = r / (n_real * c), f / (n_fake * c)
            sq += _db(pr / pf) ** 2
            used += 1
        else:
            skipped += 1
    return (math.sqrt(sq / used) if used else float('nan')), skipped


def hf_first_column(bins):
    """The first radial column of the high-frequency band c > 3 B / 4."""
    return (3 * bins) // 4 + 1


def hf_excess(real_radial, fake_radial, n_real, n_fake, bins):
    """10 log10 of the ratio of the per-sample mean energies above 3 B / 4 (fake over real); nan where a side has none."""
    c0 = hf_first_column(bins)
    r = math.fsum(float(v) for v in real_radial[c0:]) / n_real
    f = math.fsum(float(v) for v in fake_radial[c0:]) / n_fake
    return _db(f / r) if r > 0 and f > 0 and math.isfinite(r) and math.isfinite(f) else float('nan')


def spectrum_distances(plan, real_sums, fake_sums, n_real, n_fake):
    """The distances of two accumulated rows [radial | axis_d | axis_h | axis_w] over n_real and n_fake samples."""
    nrad = plan.bins + 1
    m = {}
    m['spectrum_lsd'], m['spectrum_skipped_columns'] = _lsd(real_sums[:nrad], fake_sums[:nrad], plan.counts, n_real, n_fake)
    at = nrad
    for name, extent, length, counts in zip('dhw', plan.shape, plan.axis_len, plan.axis_counts):
        if extent > 1:
            m[f'spectrum_lsd_{name}'] = _lsd(real_sums[at:at + length], fake_sums[at:at + length], counts, n_real, n_fake)[0]
        at += length
    m['spectrum_hf_excess'] = hf_excess(real_sums[:nrad], fake_sums[:nrad], n_real, n_fake, plan.bins)
    return m


class SpectrumAccumulator:
    """Sums of the per-sample spectrum rows of everything passed to add(), for reals and fakes: two f64 vectors
    [radial | axis_d | axis_h | axis_w], added sample by sample in the order given (so two batches and their concatenation
    leave the same bits); no volume is kept.  Volumes are [n, d, h, w] or [n, 1, d, h, w] (one channel) of `shape`."""

    def __init__(self, shape, spacing=(1.0, 1.0, 1.0), bins=None, window='none', scale=1.0, shift=0.0, workspace_mib=512):
        self.plan = SpectrumPlan(shape, spacing, bins, window)
        self.scale, self.shift, self.workspace_mib = float(scale), float(shift), workspace_mib
        if not (math.isfinite(self.scale) and math.isfinite(self.shift)):
            raise ValueError(f'scale {scale} and shift {shift} must be finite')
        length = self.plan.bins + 1 + sum(self.plan.axis_len)
        self.real, self.fake = np.zeros(length), np.zeros(length)
        self.n_real = self.n_fake = 0

    def rows(self, x):
        """The per-sample rows [n, radial | axis_d | axis_h | axis_w] of a batch as numpy f64."""
        if torch.is_tensor(x) and x.dtype not in HIST_DT:
            x = x.to(torch.float32)
        radial, axes = power_spectrum(x.contiguous(), self.plan, self.scale, self.shift, self.workspace_mib)
        return torch.cat((radial,) + tuple(axes), dim=1).cpu().numpy()

    def add_rows(self, rows, fake):
        dest = self.fake if fake else self.real
        for row in rows:
            dest += row
        if fake:
            self.n_fake += len(rows)
        else:
            self.n_real += len(rows)

    def add(self, real_batch, fake_batch):
        self.add_rows(self.rows(real_batch), False)
        self.add_rows(self.rows(fake_batch), True)

    def means(self):
        """(real, fake): per side the mean radial spectrum [bins + 1] and the three mean profiles (nan in empty columns)."""
        if not self.n_real or not self.n_fake:
            raise ValueError('nothing was added')
        out = []
        for sums, n in ((self.real, self.n_real), (self.fake, self.n_fake)):
            parts, at = [], 0
            for counts in (self.plan.counts,) + tuple(self.plan.axis_counts):
                with np.errstate(divide='ignore', invalid='ignore'):
                    parts.append(np.where(counts > 0, sums[at:at + len(counts)] / (n * counts), np.nan))
                at += len(counts)
            out.append(parts)
        return out

    def result(self):
        if not self.n_real or not self.n_fake:
            raise ValueError('nothing was added')
        return spectrum_distances(self.plan, self.real, self.fake, self.n_real, self.n_fake)


def get_spectrum_metrics(real, fake, spacing=(1.0, 1.0, 1.0), bins=None, window='none', scale=1.0, shift=0.0):
    """real, fake: tensors [n, d, h, w] or [n, 1, d, h, w] (device tensors: the kernel; CPU tensors: the numpy twin)."""
    acc = SpectrumAccumulator(tuple(real.shape[-3:]), spacing, bins, window, scale, shift)
    acc.add(real, fake)
    return acc.result()


def format_lines(m):
    """The stdout lines of the metrics in `m` (save_metrics and the command line print the same text)."""
    lines = []
    if 'spectrum_lsd' in m:
        skipped = m.get('spectrum_skipped_columns', 0)
        lines.append(f"Spectrum LSD (dB): {m['spectrum_lsd']:.6g}" + (f' ({skipped} columns skipped)' if skipped else ''))
    per_axis = [f"{a} {m['spectrum_lsd_' + a]:.6g}" for a in 'dhw' if 'spectrum_lsd_' + a in m]
    if per_axis:
        lines.append('Spectrum LSD per axis (dB): ' + ' '.join(per_axis))
    if 'spectrum_hf_excess' in m:
        lines.append(f"Spectrum high-frequency excess (dB, fake over real above 3/4 of the band): {m['spectrum_hf_excess']:.6g}")
    return lines


def parse_spacing(text):
    """'d,h,w' -> three positive floats (mm); ValueError otherwise."""
    parts = str(text).split(',')
    if len(parts) != 3:
        raise ValueError(f'expected d,h,w, got {text!r}')
    sp = tuple(float(v) for v in parts)
    if not all(math.isfinite(v) and v > 0 for v in sp):
        raise ValueError(f'the spacing must be positive, got {text!r}')
    return sp


def check_bins(bins):
    if bins is not None and not 1 <= int(bins) <= _lib.POWER_SPECTRUM_MAX_BINS:
        raise ValueError(f'bins lie in 1 .. {_lib.POWER_SPECTRUM_MAX_BINS}, got {bins}')
    return bins


def _names(path, max_samples):
    import os
    names = sorted(f for f in os.listdir(path) if f.endswith('.npy'))
    if max_samples is not None:
        names = names[:max_samples]
    if not names:
        raise SystemExit(f'{path}: no .npy files')
    return [os.path.join(path, f) for f in names]


_NUMPY_NATIVE = ('uint8', 'int8', 'int16', 'uint16', 'float16', 'float32')


def _volume_shape(shape):
    """The (d, h, w) of a file's array: [d, h, w], [h, w] (d = 1) or either with a leading channel axis of 1."""
    shape = tuple(shape)
    if len(shape) == 4 and shape[0] == 1:
        shape = shape[1:]
    if len(shape) == 2:
        shape = (1,) + shape
    return shape if len(shape) == 3 else None


def _load_batch(files, vol, device):
    x = np.stack([np.load(f).reshape(vol) for f in files])
    if x.dtype.name not in _NUMPY_NATIVE:
        x = x.astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(x)).to(device)


def main(argv=None):
    import argparse
    import json
    import os
    p = argparse.ArgumentParser(prog='python -m saragan_amd.metrics.spectrum_metrics', description=__doc__.split('\n\n')[0])
    p.add_argument('real_dir')
    p.add_argument('fake_dir')
    p.add_argument('--spacing', default='1,1,1', help='voxel spacing d,h,w in mm: frequencies are in cycles / mm')
    p.add_argument('--bins', type=int, default=None, help='radial columns next to DC (default: the largest extent // 2)')
    p.add_argument('--window', default='none', choices=SPECTRUM_WINDOWS)
    p.add_argument('--max_samples', type=int, default=None)
    p.add_argument('--scale', type=float, default=1.0, help='with --shift: the files hold (data - shift) / scale')
    p.add_argument('--shift', type=float, default=0.0)
    p.add_argument('--batch', type=int, default=8, help='volumes per launch: only this many are held at a time')
    p.add_argument('--device', default='cuda', choices=['cuda', 'cpu'], help='cpu: the numpy twin (np.fft.rfftn)')
    p.add_argument('--report', default=None, help='the JSON report (default: FAKE_DIR/spectrum.json)')
    args = p.parse_args(argv)
    # every refusal comes before any work: nothing is read in full, launched or written
    try:
        spacing = parse_spacing(args.spacing)
        check_bins(args.bins)
    except ValueError as e:
        raise SystemExit(f'--spacing / --bins: {e}')
    if args.batch < 1 or (args.max_samples is not None and args.max_samples < 1):
        raise SystemExit('--batch and --max_samples must be >= 1')
    if not (math.isfinite(args.scale) and math.isfinite(args.shift)):
        raise SystemExit('--scale and --shift must be finite')
    real, fake = _names(args.real_dir, args.max_samples), _names(args.fake_dir, args.max_samples)
    first = np.load(real[0], mmap_mode='r')
    vol = _volume_shape(first.shape)
    if vol is None:
        raise SystemExit(f'{real[0]}: expected a [d, h, w] or [h, w] volume of one channel, got shape {tuple(first.shape)}')
    for f in real + fake:
        v = np.load(f, mmap_mode='r')
        if v.shape != first.shape:
            raise SystemExit(f'{f}: shape {tuple(v.shape)}, the first volume has {tuple(first.shape)}')
        if v.dtype != first.dtype:
            raise SystemExit(f'{f}: dtype {v.dtype}, the first volume has {first.dtype}')
    if max(vol) > _lib.POWER_SPECTRUM_MAX_EXTENT:
        raise SystemExit(f'volumes of {vol}: extents above {_lib.POWER_SPECTRUM_MAX_EXTENT} are not supported')
    if args.device == 'cuda' and not torch.cuda.is_available():
        raise RuntimeError('no GPU is available (--device cpu runs the numpy twin)')
    acc = SpectrumAccumulator(vol, spacing, args.bins, args.window, args.scale, args.shift)
    plan = acc.plan
    c0 = hf_first_column(plan.bins)
    fake_hf = []      # per generated file, its own energy above 3 B / 4
    for at in range(0, len(real), args.batch):
        acc.add_rows(acc.rows(_load_batch(real[at:at + args.batch], vol, args.device)), False)
    for at in range(0, len(fake), args.batch):
        rows = acc.rows(_load_batch(fake[at:at + args.batch], vol, args.device))
        acc.add_rows(rows, True)
        fake_hf.extend(math.fsum(float(v) for v in row[c0:plan.bins + 1]) for row in rows)
    print(f'{len(real)} real and {len(fake)} generated volumes of shape {vol}, spacing {spacing} mm, {plan.bins} radial columns, '
          f'window {args.window}')
    m = acc.result()
    for line in format_lines(m):
        print(line)
    (real_rad, *real_axes), (fake_rad, *fake_axes) = acc.means()
    centres = plan.centres()
    print('  cycles/mm    coefficients       real mean       fake mean    real/fake dB')
    for c in range(plan.bins + 1):
        ok = plan.counts[c] > 0 and real_rad[c] > 0 and fake_rad[c] > 0
        print(f'{centres[c]:11.5g} {plan.counts[c]:15.0f} {real_rad[c]:15.6g} {fake_rad[c]:15.6g} '
              + (f'{_db(float(real_rad[c]) / float(fake_rad[c])):15.4f}' if ok else f'{"-":>15}'))
    real_hf = math.fsum(float(v) for v in acc.real[c0:plan.bins + 1]) / acc.n_real
    per_file = {os.path.basename(f): (_db(v / real_hf) if v > 0 and real_hf > 0 else None) for f, v in zip(fake, fake_hf)}
    listed = lambda a: [None if not math.isfinite(float(v)) else float(v) for v in a]
    report = {
        'arguments': {'real_dir': args.real_dir, 'fake_dir': args.fake_dir, 'spacing': list(spacing), 'bins': plan.bins,
                      'window': args.window, 'scale': args.scale, 'shift': args.shift, 'max_samples': args.max_samples,
                      'device': args.device},
        'definition': DEFINITION, 'shape': list(vol), 'dtype': str(first.dtype), 'n_real': len(real), 'n_fake': len(fake),
        'frequencies': listed(centres), 'counts': listed(plan.counts),
        'axis_frequencies': {a: listed(v) for a, v in zip('dhw', plan.axis_frequencies())},
        'axis_counts': {a: listed(v) for a, v in zip('dhw', plan.axis_counts)},
        'real': {'radial': listed(real_rad), **{f'axis_{a}': listed(v) for a, v in zip('dhw', real_axes)}},
        'fake': {'radial': listed(fake_rad), **{f'axis_{a}': listed(v) for a, v in zip('dhw', fake_axes)}},
        'distances': {k: (v if isinstance(v, int) or math.isfinite(v) else None) for k, v in m.items()},
        'hf_excess_per_file': per_file,
    }
    path = args.report or os.path.join(args.fake_dir, 'spectrum.json')
    with open(path, 'w') as f:
        json.dump(report, f, indent=1)
    print(f'Report: {path}')
    return m


if __name__ == '__main__':
    main()
