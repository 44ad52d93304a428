"""python -m saragan_amd.prepare_data SRC_DIR DST_DIR --final_shape D,H,W (--start_shape d,h,w | --levels L)

Builds the per-phase dataset the training loop reads (train.get_numpy_dataset: DST_DIR/{size}x{size}/*.npy) from a directory of
full-size `.npy` volumes, as the original's data_scripts/convert_nrrd_to_numpy_pgan.py does on a CPU pool: every volume is padded
or cropped to the final shape, the intercept is subtracted, and level i is the block mean (or maximum) over 2^i cubes, clipped and
cast.  Here one sg_block_pyramid launch per batch of volumes reads them once and writes every level (functional.block_pyramid;
DESIGN.md 4.9); `--device cpu` takes the same integer definition in numpy and writes the same bytes.  Sources are `.npy` only:
NRRD / DICOM reading, resampling by voxel spacing and filtering are not part of this tool.

DST_DIR/stats.json holds, per level, the file count, shape, dtype, min, max, mean and standard deviation over all voxels of all
files; the two flags to hand to the training command (--data_mean / --data_stddev of level 0) are printed."""
import argparse
import json
import math
import os
import sys
import time
from fractions import Fraction

import numpy as np

DEFINITION = ('per level, over all voxels of all files: mean = S / N and stddev = sqrt(SS / N - (S / N)^2) (population), with N the '
              'voxel count, S the sum and SS the sum of squares of the stored values; for integer dtypes S and SS are exact integers '
              '(summed by the pyramid kernel per volume, pooled as Python integers), for float32 they are float64 reductions')
OUT_DTYPES = ('uint16', 'int16', 'float32')
SRC_KINDS = ('uint8', 'int8', 'int16', 'uint16', 'float16', 'float32')


def _triple(text, what):
    """'D,H,W', '(D, H, W)' or the training command's '(1, D, H, W)' -> (D, H, W)."""
    parts = [p for p in text.replace('(', ' ').replace(')', ' ').replace(',', ' ').split() if p]
    try:
        vals = [int(p) for p in parts]
    except ValueError:
        raise SystemExit(f'prepare_data: {what} {text!r}: expected three integers D,H,W')
    if len(vals) == 4 and vals[0] == 1:
        vals = vals[1:]
    if len(vals) != 3 or min(vals) < 1:
        raise SystemExit(f'prepare_data: {what} {text!r}: expected three positive integers D,H,W')
    return tuple(vals)


def levels_between(final, start):
    """L with final = start * 2^(L-1) on every axis; ValueError names the axis that disagrees."""
    count = None
    for name, f, s in zip('DHW', final, start):
        ratio, rem = divmod(f, s)
        if rem or ratio < 1 or ratio & (ratio - 1):
            raise ValueError(f'axis {name}: final {f} is not start {s} times a power of two')
        lv = ratio.bit_length()
        if count is not None and lv != count:
            raise ValueError(f'axis {name}: final {f} = start {s} * 2^{lv - 1}, the axes before it give 2^{count - 1}')
        count = lv
    return count


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog='python -m saragan_amd.prepare_data', description=__doc__.split('\n\n')[1])
    ap.add_argument('src_dir')
    ap.add_argument('dst_dir')
    ap.add_argument('--final_shape', required=True, help='D,H,W: the target of level 0')
    ap.add_argument('--start_shape', help='d,h,w: the coarsest level; gives the number of levels')
    ap.add_argument('--levels', type=int, help='the number of levels (instead of --start_shape)')
    ap.add_argument('--reduce', choices=('mean', 'max'), default='mean')
    ap.add_argument('--intercept', default='0')
    ap.add_argument('--pad_value', default=None, help='default: the intercept')
    ap.add_argument('--clip', default=None, help='LO,HI (a negative LO as --clip=LO,HI); default: the output type\'s range')
    ap.add_argument('--out_dtype', choices=OUT_DTYPES, default='uint16')
    ap.add_argument('--anchor', default='center,center,center', help='center|start|end per axis')
    ap.add_argument('--batch', type=int, default=4, help='volumes per launch')
    ap.add_argument('--max_samples', type=int, default=None)
    ap.add_argument('--device', choices=('cuda', 'cpu'), default='cuda')
    ap.add_argument('--overwrite', action='store_true')
    a = ap.parse_args(argv)
    a.final_shape = _triple(a.final_shape, '--final_shape')
    if (a.start_shape is None) == (a.levels is None):
        raise SystemExit('prepare_data: give --start_shape or --levels (one of them)')
    if a.start_shape is not None:
        a.start_shape = _triple(a.start_shape, '--start_shape')
        try:
            a.levels = levels_between(a.final_shape, a.start_shape)
        except ValueError as e:
            raise SystemExit(f'prepare_data: --start_shape {a.start_shape} does not lead to --final_shape {a.final_shape}: {e}')
    if not 1 <= a.levels <= 6:
        raise SystemExit(f'prepare_data: {a.levels} levels; a pyramid has 1 to 6 (final = start * 2^(levels-1), at most start * 32)')
    for name, f in zip('DHW', a.final_shape):
        if f % (1 << (a.levels - 1)):
            raise SystemExit(f'prepare_data: --final_shape axis {name} = {f} is not a multiple of 2^{a.levels - 1} ({a.levels} levels)')
    a.anchor = tuple(a.anchor.split(','))
    if len(a.anchor) != 3 or any(x not in ('center', 'start', 'end') for x in a.anchor):
        raise SystemExit(f'prepare_data: --anchor is center|start|end per axis, got {a.anchor}')
    if a.clip is not None:
        parts = a.clip.split(',')
        if len(parts) != 2:
            raise SystemExit(f'prepare_data: --clip {a.clip!r}: expected LO,HI')
        a.clip = tuple(parts)
    if a.batch < 1:
        raise SystemExit(f'prepare_data: --batch {a.batch} < 1')
    return a


def _number(text, is_int, what):
    try:
        return int(text) if is_int else float(text)
    except ValueError:
        raise SystemExit(f'prepare_data: {what} {text!r} is not {"an integer (the sources are integers)" if is_int else "a number"}')


def scan_sources(src_dir, max_samples=None):
    """[(name, path, shape)] of the sorted 3-D `.npy` volumes and their common dtype (headers only: the files are memory-mapped)."""
    names = sorted(f for f in os.listdir(src_dir) if f.endswith('.npy'))
    if max_samples is not None:
        names = names[:max_samples]
    if not names:
        raise SystemExit(f'prepare_data: no .npy files in {src_dir}')
    found, dtype = [], None
    for f in names:
        path = os.path.join(src_dir, f)
        head = np.load(path, mmap_mode='r')
        if head.ndim != 3:
            raise SystemExit(f'prepare_data: {path} is {head.ndim}-D {head.shape}; sources are 3-D volumes [d, h, w]')
        if dtype is None:
            dtype = head.dtype
        elif head.dtype != dtype:
            raise SystemExit(f'prepare_data: {path} is {head.dtype}, the files before it {dtype}: one dtype per directory')
        found.append((f, path, tuple(head.shape)))
    if dtype.name not in SRC_KINDS:
        raise SystemExit(f'prepare_data: sources are {", ".join(SRC_KINDS)}, got {dtype}')
    return found, dtype


def level_dirs(dst_dir, final_shape, levels):
    return [os.path.join(dst_dir, f'{final_shape[2] >> i}x{final_shape[2] >> i}') for i in range(levels)]


def run(a, out=sys.stdout):
    import torch
    from .table_ops import block_pyramid
    files, dtype = scan_sources(a.src_dir, a.max_samples)
    is_int = dtype.kind in 'iu'
    if not is_int and a.out_dtype != 'float32':
        raise SystemExit(f'prepare_data: {dtype} sources take --out_dtype float32')
    intercept = _number(a.intercept, is_int, '--intercept')
    pad_value = None if a.pad_value is None else _number(a.pad_value, is_int, '--pad_value')
    clip = None if a.clip is None else (_number(a.clip[0], is_int, '--clip'), _number(a.clip[1], is_int, '--clip'))
    dirs = level_dirs(a.dst_dir, a.final_shape, a.levels)
    # every destination is checked before any work is done
    if not a.overwrite:
        for d in dirs:
            for name, _, _ in files:
                if os.path.exists(os.path.join(d, name)):
                    raise SystemExit(f'prepare_data: {os.path.join(d, name)} exists (--overwrite replaces it); nothing was written')
    if a.device == 'cuda' and not torch.cuda.is_available():
        raise SystemExit('prepare_data: --device cuda, and no GPU is visible (--device cpu takes the numpy path)')
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    out_dtype = getattr(torch, a.out_dtype)
    integer_out = a.out_dtype != 'float32'
    padded = sum(any(s < t for s, t in zip(shape, a.final_shape)) for _, _, shape in files)
    cropped = sum(any(s > t for s, t in zip(shape, a.final_shape)) for _, _, shape in files)
    by_shape = {}
    for item in files:      # files of one shape are batched together (sorted order within a shape)
        by_shape.setdefault(item[2], []).append(item)
    pooled = [{'n': 0, 's': 0, 'ss': 0, 'min': None, 'max': None} for _ in range(a.levels)]
    spent = dict.fromkeys(('load', 'upload', 'kernel', 'download', 'save'), 0.0)

    def tick(key, t0):
        if a.device == 'cuda':
            torch.cuda.synchronize()
        spent[key] += time.perf_counter() - t0

    for shape, items in by_shape.items():
        for at in range(0, len(items), a.batch):
            group = items[at:at + a.batch]
            t0 = time.perf_counter()
            host = torch.from_numpy(np.stack([np.load(path) for _, path, _ in group]))
            tick('load', t0)
            t0 = time.perf_counter()
            x = host.to(a.device)
            tick('upload', t0)
            t0 = time.perf_counter()
            res = block_pyramid(x, a.final_shape, a.levels, reduce=a.reduce, intercept=intercept, pad_value=pad_value, clip=clip,
                                out_dtype=out_dtype, anchor=a.anchor, stats=integer_out)
            lvls, st = res if integer_out else (res, None)
            if not integer_out:      # float64 reductions of the level tensors
                st = torch.stack([torch.stack([v.double().sum(dim=(1, 2, 3)), (v.double() ** 2).sum(dim=(1, 2, 3)),
                                               v.double().amin(dim=(1, 2, 3)), v.double().amax(dim=(1, 2, 3))], dim=1)
                                  for v in lvls], dim=1)
            tick('kernel', t0)
            t0 = time.perf_counter()
            arrays = [v.cpu().numpy() for v in lvls]
            st = st.cpu().tolist()
            tick('download', t0)
            t0 = time.perf_counter()
            for i, (d, arr) in enumerate(zip(dirs, arrays)):
                for k, (name, _, _) in enumerate(group):
                    np.save(os.path.join(d, name), arr[k])
                    p, (s, ss, mn, mx) = pooled[i], st[k][i]
                    p['n'] += arr[k].size
                    p['s'] += s
                    p['ss'] += ss
                    p['min'] = mn if p['min'] is None else min(p['min'], mn)
                    p['max'] = mx if p['max'] is None else max(p['max'], mx)
            tick('save', t0)

    levels = []
    for i, p in enumerate(pooled):
        if integer_out:
            mean = Fraction(p['s'], p['n'])
            var = Fraction(p['ss'], p['n']) - mean * mean
            mean, std = float(mean), math.sqrt(var)
        else:
            mean = p['s'] / p['n']
            std = math.sqrt(max(p['ss'] / p['n'] - mean * mean, 0.0))
        levels.append({'level': i, 'directory': os.path.basename(dirs[i]), 'files': len(files),
                       'shape': [t >> i for t in a.final_shape], 'dtype': a.out_dtype, 'min': p['min'], 'max': p['max'],
                       'mean': mean, 'stddev': std})
    with open(os.path.join(a.dst_dir, 'stats.json'), 'w') as f:
        json.dump({'definition': DEFINITION, 'reduce': a.reduce, 'intercept': intercept,
                   'pad_value': intercept if pad_value is None else pad_value, 'clip': clip, 'anchor': list(a.anchor),
                   'levels': levels}, f, indent=1)
        f.write('\n')
    print(f'padded {padded} / cropped {cropped} / files {len(files)}', file=out)
    per = len(files)
    print('seconds per volume: ' + ', '.join(f'{k} {v / per:.4f}' for k, v in spent.items()) + f' ({a.device})', file=out)
    print(f'--data_mean {levels[0]["mean"]!r} --data_stddev {levels[0]["stddev"]!r}', file=out)
    return levels, spent


def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
