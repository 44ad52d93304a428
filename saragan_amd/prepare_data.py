"""python -m saragan_amd.prepare_data SRC_DIR DST_DIR --final_shape D,H,W (--start_shape d,h,w | --levels L)

Builds the per-phase dataset the training loop reads (train.get_numpy_dataset: DST_DIR/{size}x{size}/*.npy) from a directory of
full-size volumes, as the original's data_scripts/convert_nrrd_to_numpy_pgan.py does on a CPU pool: every volume is padded
or cropped to the final shape, the intercept is subtracted, and level i is the block mean (or maximum) over 2^i cubes, clipped and
cast.  Here one sg_block_pyramid launch per batch of volumes reads them once and writes every level (functional.block_pyramid;
DESIGN.md 4.9); `--device cpu` takes the same integer definition in numpy and writes the same bytes.

Sources are `.npy`, `.nrrd` and `.nhdr` files (nrrd_io: the array as [z, y, x], nothing re-oriented).  `--spacing d,h,w` (mm)
resamples every volume to one voxel spacing first, on the device too (functional.resample_volume, one sg_resample_axes launch per
batch): `--interp linear|nearest|antialias`, `--grid itk` (the original's resample_sitk_image: ceil(S * old / new)
voxels from source voxel 0) or `edges` (the volume's faces aligned, round(S * old / new) voxels), voxels outside the source
taking --pad_value.  NRRD files carry their spacing; `.npy` files take it from --src_spacing or --spacing_table.  `--orient
positive` permutes and flips NRRD volumes so that z, y, x increase along the array's axes; oblique directions are an error, or,
with --skip_unsupported, a skipped and counted file.  DICOM reading and filtering are not part of this tool.

DST_DIR/stats.json holds, per level, the file count, shape, dtype, min, max, mean and standard deviation over all voxels of all
files; the two flags to hand to the training command (--data_mean / --data_stddev of level 0) are printed."""
import argparse
import collections
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


def _spacing(text, what):
    parts = [p for p in text.replace(',', ' ').split() if p]
    try:
        vals = tuple(float(p) for p in parts)
    except ValueError:
        vals = ()
    if len(vals) != 3 or not all(math.isfinite(v) and v > 0 for v in vals):
        raise SystemExit(f'prepare_data: {what} {text!r}: expected three positive numbers d,h,w (mm)')
    return vals


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
    ap.add_argument('--spacing', default=None, help='d,h,w in mm: resample every volume to this voxel spacing first')
    ap.add_argument('--interp', choices=('linear', 'nearest', 'antialias'), default='linear')
    ap.add_argument('--grid', choices=('itk', 'edges'), default='itk')
    ap.add_argument('--src_spacing', default=None, help='d,h,w in mm: the spacing of every .npy source')
    ap.add_argument('--spacing_table', default=None, help='a CSV of lines name,sd,sh,sw: the spacing of each .npy source')
    ap.add_argument('--orient', choices=('keep', 'positive'), default='keep')
    ap.add_argument('--skip_unsupported', action='store_true', help='skip (and count) files with oblique directions')
    a = ap.parse_args(argv)
    a.spacing = None if a.spacing is None else _spacing(a.spacing, '--spacing')
    a.src_spacing = None if a.src_spacing is None else _spacing(a.src_spacing, '--src_spacing')
    if a.spacing is None:
        for flag, on in (('--interp', a.interp != 'linear'), ('--grid', a.grid != 'itk'), ('--src_spacing', a.src_spacing is not None),
                         ('--spacing_table', a.spacing_table is not None), ('--orient', a.orient != 'keep')):
            if on:
                raise SystemExit(f'prepare_data: {flag} goes with --spacing (nothing is resampled without it)')
    elif a.src_spacing is not None and a.spacing_table is not None:
        raise SystemExit('prepare_data: give --src_spacing or --spacing_table (one of them)')
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


SOURCE_EXTS = ('.npy', '.nrrd', '.nhdr')
OBLIQUE = 1e-6      # a direction is oblique when a second component exceeds this fraction of its length

# one source volume: header facts only (spacing, directions: per array axis, None where the file has none)
Source = collections.namedtuple('Source', 'name path shape spacing directions')


def scan_sources(src_dir, max_samples=None):
    """[Source] of the sorted 3-D `.npy` / `.nrrd` / `.nhdr` volumes and their common dtype (headers only); name: the output file
    name, the source's stem + `.npy`.  Two sources with one stem are an error."""
    from . import nrrd_io
    names = sorted(f for f in os.listdir(src_dir) if f.endswith(SOURCE_EXTS))
    if max_samples is not None:
        names = names[:max_samples]
    if not names:
        raise SystemExit(f'prepare_data: no .npy files in {src_dir}')
    stems = {}
    for f in names:
        stem = os.path.splitext(f)[0]
        if stem in stems:
            raise SystemExit(f'prepare_data: {stems[stem]} and {f} in {src_dir} would both be written as {stem}.npy; nothing was written')
        stems[stem] = f
    found, dtype = [], None
    for f in names:
        path = os.path.join(src_dir, f)
        if f.endswith('.npy'):
            head = np.load(path, mmap_mode='r')
            this, shape, spacing, directions = head.dtype, tuple(head.shape), None, None
            if head.ndim != 3:
                raise SystemExit(f'prepare_data: {path} is {head.ndim}-D {head.shape}; sources are 3-D volumes [d, h, w]')
        else:
            try:
                h = nrrd_io.read_header(path)
            except ValueError as e:
                raise SystemExit(f'prepare_data: {e}')
            this, shape, spacing, directions = np.dtype(h.dtype), h.shape, h.spacing, h.directions
        if dtype is None:
            dtype = this
        elif this != dtype:
            raise SystemExit(f'prepare_data: {path} is {this}, the files before it {dtype}: one dtype per directory')
        found.append(Source(os.path.splitext(f)[0] + '.npy', path, shape, spacing, directions))
    if dtype.name not in SRC_KINDS:
        raise SystemExit(f'prepare_data: sources are {", ".join(SRC_KINDS)}, got {dtype}')
    return found, dtype


def load_source(src):
    if src.path.endswith('.npy'):
        return np.load(src.path)
    from . import nrrd_io
    return nrrd_io.read(src.path)[0]


def level_dirs(dst_dir, final_shape, levels):
    return [os.path.join(dst_dir, f'{final_shape[2] >> i}x{final_shape[2] >> i}') for i in range(levels)]


def read_spacing_table(path):
    """{name: (sd, sh, sw)} of a CSV of lines name,sd,sh,sw (blank lines, # comments and a `name,...` heading are passed over); a
    source is looked up by its file name, then by its stem."""
    table = {}
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            text = line.strip()
            if not text or text.startswith('#') or text.lower().startswith('name,'):
                continue
            parts = [p.strip() for p in text.split(',')]
            if len(parts) != 4:
                raise SystemExit(f'prepare_data: {path} line {ln}: expected name,sd,sh,sw, got {text!r}')
            table[parts[0]] = _spacing(','.join(parts[1:]), f'{path} line {ln}:')
    return table


class Unsupported(ValueError):
    """A source this tool cannot resample (oblique directions): an error, or a skipped file with --skip_unsupported."""


def plan_resample(src, a, table):
    """How one source reaches the target spacing: dict(perm, source_shape, source_spacing, out_shape, step, start), the last five
    along the array's axes AFTER the permutation perm.  --orient positive: perm puts the world's z, y, x on the array's axes and
    an axis that runs against its world axis gets a negative step; keep: the file's axes as they are, |spacing|."""
    spacing = src.spacing
    if src.path.endswith('.npy'):
        spacing = a.src_spacing
        if table is not None:
            base = os.path.basename(src.path)
            spacing = table.get(base, table.get(os.path.splitext(base)[0]))
    if spacing is None:
        raise SystemExit(f'prepare_data: {src.path} has no voxel spacing (--src_spacing, --spacing_table, or a spacing in the NRRD header)')
    perm, flip = (0, 1, 2), (False, False, False)
    if src.directions is not None:
        world = []
        for v, length in zip(src.directions, spacing):
            big = [k for k in range(3) if abs(v[k]) > OBLIQUE * length]
            if len(big) != 1:
                raise Unsupported(f'{src.path}: oblique space directions {v}')
            world.append(big[0])
        if sorted(world) != [0, 1, 2]:
            raise Unsupported(f'{src.path}: the space directions do not span three axes')
        if a.orient == 'positive':
            perm = tuple(world.index(2 - t) for t in range(3))      # array axis t becomes the world's z, y, x
            flip = tuple(src.directions[p][2 - t] < 0 for t, p in enumerate(perm))
    shape = tuple(src.shape[p] for p in perm)
    spacing = tuple(abs(spacing[p]) for p in perm)
    out_shape, step, start = [], [], []
    for S, old, new, fl in zip(shape, spacing, a.spacing, flip):
        st = new / old
        if a.grid == 'itk':
            O, s0 = int(math.ceil(S * (old / new))), 0.0
        else:
            O, s0 = int(math.floor(S * (old / new) + 0.5)), 0.5 * st - 0.5
        out_shape.append(max(O, 1))
        step.append(-st if fl else st)
        start.append((S - 1) - s0 if fl else s0)
    return dict(perm=perm, source_shape=shape, source_spacing=spacing, out_shape=tuple(out_shape), step=tuple(step), start=tuple(start))


def run(a, out=sys.stdout):
    import torch
    from .table_ops import block_pyramid, resample_volume
    files, dtype = scan_sources(a.src_dir, a.max_samples)
    is_int = dtype.kind in 'iu'
    if not is_int and a.out_dtype != 'float32':
        raise SystemExit(f'prepare_data: {dtype} sources take --out_dtype float32')
    intercept = _number(a.intercept, is_int, '--intercept')
    pad_value = None if a.pad_value is None else _number(a.pad_value, is_int, '--pad_value')
    clip = None if a.clip is None else (_number(a.clip[0], is_int, '--clip'), _number(a.clip[1], is_int, '--clip'))
    resampling = a.spacing is not None
    plans, discarded = {}, 0
    if resampling:
        table = None if a.spacing_table is None else read_spacing_table(a.spacing_table)
        kept = []
        for src in files:
            try:
                plans[src.name] = plan_resample(src, a, table)
                kept.append(src)
            except Unsupported as e:
                if not a.skip_unsupported:
                    raise SystemExit(f'prepare_data: {e} (--skip_unsupported passes such files over); nothing was written')
                print(f'skipped {e}', file=out)
                discarded += 1
        files = kept
        if not files:
            raise SystemExit(f'prepare_data: every source in {a.src_dir} was skipped; nothing was written')
    dirs = level_dirs(a.dst_dir, a.final_shape, a.levels)
    # every destination is checked before any work is done
    if not a.overwrite:
        for d in dirs:
            for src in files:
                if os.path.exists(os.path.join(d, src.name)):
                    raise SystemExit(f'prepare_data: {os.path.join(d, src.name)} exists (--overwrite replaces it); nothing was written')
    if a.device == 'cuda' and not torch.cuda.is_available():
        raise SystemExit('prepare_data: --device cuda, and no GPU is visible (--device cpu takes the numpy path)')
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    out_dtype = getattr(torch, a.out_dtype)
    integer_out = a.out_dtype != 'float32'
    placed = {src.name: plans[src.name]['out_shape'] if resampling else src.shape for src in files}      # what is padded / cropped
    padded = sum(any(s < t for s, t in zip(placed[src.name], a.final_shape)) for src in files)
    cropped = sum(any(s > t for s, t in zip(placed[src.name], a.final_shape)) for src in files)
    groups = {}
    for item in files:      # files of one shape (resampling: of one shape, spacing and orientation) are batched together, in sorted order
        key = (item.shape,) + (tuple(sorted(plans[item.name].items())) if resampling else ())
        groups.setdefault(key, []).append(item)
    pooled = [{'n': 0, 's': 0, 'ss': 0, 'min': None, 'max': None} for _ in range(a.levels)]
    spent = dict.fromkeys(('load', 'upload') + (('resample',) if resampling else ()) + ('kernel', 'download', 'save'), 0.0)

    def tick(key, t0):
        if a.device == 'cuda':
            torch.cuda.synchronize()
        spent[key] += time.perf_counter() - t0

    for items in groups.values():
        for at in range(0, len(items), a.batch):
            group = items[at:at + a.batch]
            t0 = time.perf_counter()
            host = torch.from_numpy(np.stack([load_source(src) for src in group]))
            tick('load', t0)
            t0 = time.perf_counter()
            x = host.to(a.device)
            tick('upload', t0)
            if resampling:
                t0 = time.perf_counter()
                plan = plans[group[0].name]
                if plan['perm'] != (0, 1, 2):
                    x = x.permute(0, *(1 + p for p in plan['perm'])).contiguous()
                x = resample_volume(x, plan['out_shape'], plan['step'], plan['start'], mode=a.interp,
                                    fill=intercept if pad_value is None else pad_value)
                tick('resample', t0)
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
                for k, src in enumerate(group):
                    np.save(os.path.join(d, src.name), arr[k])
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
    record = {'definition': DEFINITION, 'reduce': a.reduce, 'intercept': intercept,
              'pad_value': intercept if pad_value is None else pad_value, 'clip': clip, 'anchor': list(a.anchor), 'levels': levels}
    if resampling:
        record['resample'] = {'spacing': list(a.spacing), 'interp': a.interp, 'grid': a.grid, 'orient': a.orient, 'discarded': discarded,
                              'files': [{'name': src.name, 'source_shape': list(plans[src.name]['source_shape']),
                                         'source_spacing': list(plans[src.name]['source_spacing']),
                                         'resampled_shape': list(plans[src.name]['out_shape'])} for src in files]}
    with open(os.path.join(a.dst_dir, 'stats.json'), 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    print(f'padded {padded} / cropped {cropped} / files {len(files)}' + (f' / discarded {discarded}' if resampling else ''), file=out)
    per = len(files)
    print('seconds per volume: ' + ', '.join(f'{k} {v / per:.4f}' for k, v in spent.items()) + f' ({a.device})', file=out)
    print(f'--data_mean {levels[0]["mean"]!r} --data_stddev {levels[0]["stddev"]!r}', file=out)
    return levels, spent

def main(argv=None):
    run(parse_args(argv))


if __name__ == '__main__':
    main()
