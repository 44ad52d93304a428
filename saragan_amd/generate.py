"""python -m saragan_amd.generate ARCH ...: a checkpoint turned into a synthetic dataset (the reference's
generate.py:136-175 without its metrics).  One typed file per sample, `OUT/generated_{phase}/{prefix}{index:07d}.npy` ([d, h, w]
when the model has one channel, as prepare_data writes training volumes, else [c, d, h, w]) or `.nrrd`, in the training data's
layout and dtype: the directory is read unchanged by metrics.sample_metrics, metrics.intensity_metrics, preview and the training
loader.  Takes generate_minimal's flags and:

  --out_dtype uint16|int16|uint8|float32, --clip LO,HI (data units), --rounding trunc|rint: what functional.store_volumes stores,
      scale / shift = --data_stddev / --data_mean (1 / 0 when neither is given).  `--out_dtype int16 --data_stddev 1024 --data_mean 0
      --clip=-1024,2048` gives the bytes of the reference's (np.clip(x, -1, 2) * 1024).astype(np.int16).
  --format npy|nrrd, --spacing d,h,w (NRRD, one channel), --name_prefix, --overwrite, --resume, --first_index I
  --shard R/W (default: RANK / WORLD_SIZE of the launcher, else 0/1): this process makes the indices i in [I, num_samples) with
      i % W == R; shards do not communicate, W independent processes do as well as one launcher.
  --inflight, --writers: the pipeline below.  --warn_clipped: the share of clipped voxels that draws a warning.
  --png, --preview_samples: the contact sheet of the shard's first samples.

Sample i's latent row is np.random.default_rng([seed, i]).standard_normal(latent_dim, dtype=np.float32) -- or, with
--latents_path FILE.npy (float32 [N, latent_dim], e.g. the latents.npy of saragan_amd.project; --num_samples then defaults to N and
the manifest records the path instead of the rule), row i of that table -- and its label row is row i of the label table: a sample depends on the seed and its index only, not on the batch size, the shard or where a run resumed.

The pipeline: per batch G's forward pass, one store_volumes pass into a typed device buffer (with every sample's statistics), an
asynchronous copy into one of --inflight pinned host buffers behind an event; while the next batch is generated the event is
awaited and a pool of --writers threads saves the files straight from the pinned buffer (to a temporary name, then renamed: a
file that exists is whole).  Host memory holds --inflight batches and nothing else.  A writer's exception ends the run.

`manifest_{R}of{W}.json` records the arguments, the definition, per file the index, name, min, max, mean, stddev (exact, from the
kernel's integer sums) and the numbers of voxels clipped from below, from above and NaN, the pooled totals and the seconds spent."""
import argparse
import json
import math
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction

import numpy as np
import torch

from .generation import RestoredGenerator, add_model_arguments, add_preview_arguments, label_rows, optional_num_samples

OUT_DTYPES = ('uint16', 'int16', 'uint8', 'float32')
LATENT_RULE = 'np.random.default_rng([seed, index]).standard_normal(latent_dim, dtype=np.float32)'


def build_parser():
    p = add_model_arguments(argparse.ArgumentParser(prog='python -m saragan_amd.generate', description=__doc__.split('\n\n')[0]))
    optional_num_samples(p)      # (required still, unless --latents_path says how many there are: plan())
    add_preview_arguments(p, 'preview_{R}of{W}.png')
    p.add_argument('--latents_path', type=str, default=None,
                   help='a float32 [N, latent_dim] .npy (project\'s latents.npy): row i is sample i\'s latent instead of the seeded rule')
    p.add_argument('--preview_samples', type=int, default=8, help='with --png: the sheet shows the first so many samples of this shard')
    p.add_argument('--out_dtype', default='uint16', choices=OUT_DTYPES)
    p.add_argument('--clip', type=str, default=None, help='LO,HI in data units (negative LO: --clip=LO,HI); default: the range of --out_dtype')
    p.add_argument('--rounding', default='trunc', choices=['trunc', 'rint'])
    p.add_argument('--format', default='npy', choices=['npy', 'nrrd'])
    p.add_argument('--spacing', type=str, default='1,1,1', help='d,h,w voxel spacing written into NRRD headers')
    p.add_argument('--name_prefix', type=str, default='')
    p.add_argument('--shard', type=str, default=None, help='R/W: this process makes the indices i with i %% W == R')
    p.add_argument('--first_index', type=int, default=0)
    p.add_argument('--resume', default=False, action='store_true', help='skip the indices whose file exists')
    p.add_argument('--overwrite', default=False, action='store_true')
    p.add_argument('--inflight', type=int, default=3, help='batches in host memory at any time')
    p.add_argument('--writers', type=int, default=4, help='threads that save files')
    p.add_argument('--warn_clipped', type=float, default=0.01)
    return p


def latent_rows(seed, indices, latent_dim):
    """float32 [len(indices), latent_dim]: row k belongs to sample indices[k], whatever else is in the batch."""
    return np.stack([np.random.default_rng([seed, int(i)]).standard_normal(latent_dim, dtype=np.float32) for i in indices])


def parse_shard(text, env=os.environ):
    if text is None:
        r, w = int(env.get('RANK', 0)), int(env.get('WORLD_SIZE', 1))
    else:
        try:
            r, w = (int(v) for v in text.split('/'))
        except ValueError:
            raise ValueError(f'--shard is R/W, got {text!r}') from None
    if w < 1 or not 0 <= r < w:
        raise ValueError(f'--shard {r}/{w}: expected 0 <= R < W')
    return r, w


def _numbers(text, count, what, kind=float):
    try:
        vals = tuple(kind(v) for v in text.split(','))
    except ValueError:
        vals = ()
    if len(vals) != count:
        raise ValueError(f'{what} is {count} numbers separated by commas, got {text!r}')
    return vals


def plan(args, env=os.environ):
    """The checked settings of a run: shard, indices, names, scale / shift / clip.  ValueError on a bad flag; nothing is written."""
    if (args.data_mean is None) != (args.data_stddev is None):
        raise ValueError('give both --data_mean and --data_stddev, or neither')
    latents = None
    if getattr(args, 'latents_path', None):
        latents = np.load(args.latents_path)
        if latents.ndim != 2 or latents.shape[1] != args.latent_dim or latents.dtype != np.float32:
            raise ValueError(f'--latents_path {args.latents_path}: expected float32 [N, latent_dim = {args.latent_dim}], got '
                             f'{latents.dtype} {latents.shape}')
        if args.num_samples is None:
            args.num_samples = latents.shape[0]
        if args.num_samples > latents.shape[0]:
            raise ValueError(f'--num_samples {args.num_samples} exceeds the {latents.shape[0]} rows of --latents_path')
    if args.num_samples is None:
        raise ValueError('--num_samples is required (or --latents_path, whose rows are counted)')
    if args.num_samples < 0 or not 0 <= args.first_index or args.batch_size < 1:
        raise ValueError('--num_samples and --first_index are >= 0, --batch_size >= 1')
    if args.inflight < 1 or args.writers < 1 or args.preview_samples < 1:
        raise ValueError('--inflight, --writers and --preview_samples are at least 1')
    if args.resume and args.overwrite:
        raise ValueError('give --resume or --overwrite, not both')
    r, w = parse_shard(args.shard, env)
    clip = None
    if args.clip is not None:
        clip = _numbers(args.clip, 2, '--clip')
        if args.out_dtype != 'float32':
            if any(not math.isfinite(v) or int(v) != v for v in clip):
                raise ValueError(f'--clip for --out_dtype {args.out_dtype} is two integers, got {args.clip!r}')
            clip = tuple(int(v) for v in clip)
    spacing = _numbers(args.spacing, 3, '--spacing')
    if any(not (math.isfinite(s) and s > 0) for s in spacing):
        raise ValueError(f'--spacing is three positive numbers, got {args.spacing!r}')
    scale, shift = (1.0, 0.0) if args.data_mean is None else (float(args.data_stddev), float(args.data_mean))
    directory = os.path.join(args.output_dir or '.', f'generated_{args.phase}')
    indices = [i for i in range(args.first_index, args.num_samples) if i % w == r]
    names = {i: f'{args.name_prefix}{i:07d}.{args.format}' for i in indices}
    return dict(rank=r, world=w, clip=clip, spacing=spacing, scale=scale, shift=shift, directory=directory, indices=indices, names=names, latents=latents,
                manifest=os.path.join(directory, f'manifest_{r}of{w}.json'), sheet=os.path.join(directory, f'preview_{r}of{w}.png'))


def file_stats(voxels, row):
    """min, max, mean, stddev of one file or of a pool from the exact integer sums: (n, sum, sum of squares, min, max)."""
    s, ss, mn, mx = row
    mean = Fraction(s, voxels)
    var = Fraction(ss, voxels) - mean * mean
    return dict(min=mn, max=mx, mean=float(mean), stddev=math.sqrt(var))


def _float_stats(arr):
    a = arr.astype(np.float64)
    return dict(min=float(np.nanmin(a)) if a.size else None, max=float(np.nanmax(a)) if a.size else None, mean=float(np.nanmean(a)),
                stddev=float(np.nanstd(a)))


def _save(path, arr, fmt, spacing):
    """Runs in a writer thread.  The file appears under its name only when it is whole.  Returns (seconds, float statistics or None)."""
    t0 = time.perf_counter()
    tmp = path + '.part'
    if fmt == 'nrrd':
        from . import nrrd_io
        nrrd_io.write(tmp, arr, spacing)
    else:
        with open(tmp, 'wb') as f:
            np.save(f, arr)
    os.replace(tmp, path)
    extra = _float_stats(arr) if arr.dtype == np.float32 else None
    return time.perf_counter() - t0, extra


class _Slot:
    """One batch in flight: the typed device buffer, its pinned host twin, the events around the three device stages."""

    def __init__(self, shape, dtype, device):
        self.dev = torch.empty(shape, device=device, dtype=dtype)
        self.host = torch.empty(shape, dtype=dtype, pin_memory=True)
        self.host_stats = torch.empty((shape[0], 7), dtype=torch.int64, pin_memory=True)
        self.events = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        self.batch, self.futures = None, []

    def drain(self, spent, records):
        """Waits for the slot's writers (a writer's exception is raised here) and files their results."""
        for fut, rec in self.futures:
            seconds, extra = fut.result()
            spent['save'] += seconds
            if extra is not None:
                rec.update(extra)
            records.append(rec)
        self.futures = []


def run(args, device=None, out=sys.stdout, env=os.environ):
    """Generates this shard's files.  Returns the manifest (also written next to the files)."""
    from . import functional as F
    p = plan(args, env)
    directory, names = p['directory'], p['names']
    if args.format == 'nrrd' and _channels(args) != 1:
        raise ValueError('--format nrrd holds one channel per file')
    existing = [i for i in p['indices'] if os.path.exists(os.path.join(directory, names[i]))]
    if existing and not (args.resume or args.overwrite):
        raise FileExistsError(f'{os.path.join(directory, names[existing[0]])} exists ({len(existing)} of this shard\'s files do): '
                              f'give --resume to keep them or --overwrite to replace them')
    kept = set(existing) if args.resume else set()
    todo = [i for i in p['indices'] if i not in kept]
    labels = label_rows(args)
    if not torch.cuda.is_available():
        raise RuntimeError('saragan_amd generates on MI355X only: no CPU fallback')
    if device is None:
        local = env.get('LOCAL_RANK')
        device = f'cuda:{int(local) % torch.cuda.device_count()}' if local is not None else 'cuda'
    if torch.device(device).index is not None:
        torch.cuda.set_device(torch.device(device))      # (the events and pinned copies below belong to the current device)
    t_start = time.perf_counter()
    g = RestoredGenerator(args, device)
    B = args.batch_size
    warm = g(torch.zeros(B, args.latent_dim, device=device),
             None if labels is None else torch.zeros(B, labels.shape[1], device=device))      # creates the variables
    g.restore(labels is not None)
    n, c, d, h, w = warm.shape
    del warm
    os.makedirs(directory, exist_ok=True)
    out_dtype = getattr(torch, args.out_dtype)
    integer = args.out_dtype != 'float32'
    voxels = c * d * h * w
    slots = [_Slot((B, c, d, h, w), out_dtype, device) for _ in range(min(args.inflight, max(1, -(-len(todo) // B))))]
    spent = dict.fromkeys(('generation', 'store', 'download', 'save'), 0.0)
    records, keep = [], []
    pool = ThreadPoolExecutor(max_workers=args.writers)

    def finish(slot):
        """The batch of `slot` has been launched: wait for its copy, then hand its samples to the writers."""
        ev = slot.events
        ev[3].synchronize()
        for key, a, b in (('generation', 0, 1), ('store', 1, 2), ('download', 2, 3)):
            spent[key] += ev[a].elapsed_time(ev[b]) * 1e-3
        vols, st = slot.host.numpy(), slot.host_stats.tolist()
        for k, i in enumerate(slot.batch):
            s, ss, mn, mx, below, above, nan = st[k]
            rec = dict(index=i, name=names[i], below=below, above=above, nan=nan)
            if integer:
                rec.update(file_stats(voxels, (s, ss, mn, mx)), sum=s, sum_squares=ss)
            arr = vols[k, 0] if c == 1 else vols[k]
            slot.futures.append((pool.submit(_save, os.path.join(directory, names[i]), arr, args.format, p['spacing']), rec))

    try:
        prev = None
        for k, at in enumerate(range(0, len(todo), B)):
            batch = todo[at:at + B]
            padded = batch + [batch[-1]] * (B - len(batch))      # a last short batch is padded; the padding is dropped
            slot = slots[k % len(slots)]
            if prev is slot:                                     # (one slot: nothing overlaps)
                finish(prev)
                prev = None
            slot.drain(spent, records)
            rows = latent_rows(args.seed, padded, args.latent_dim) if p['latents'] is None else np.ascontiguousarray(p['latents'][padded])
            z = torch.from_numpy(rows).to(device, non_blocking=True)
            cond = None if labels is None else torch.from_numpy(labels[padded]).to(device, non_blocking=True)
            ev = slot.events
            ev[0].record()
            x = g(z, cond)
            ev[1].record()
            _, st = F.store_volumes(x, out_dtype, scale=p['scale'], shift=p['shift'], clip=p['clip'], rounding=args.rounding, stats=True,
                                    out=slot.dev)
            ev[2].record()
            slot.host.copy_(slot.dev, non_blocking=True)
            slot.host_stats.copy_(st, non_blocking=True)
            ev[3].record()
            slot.batch = batch
            if args.png and sum(t.shape[0] for t in keep) < args.preview_samples:
                keep.append(x[:min(len(batch), args.preview_samples - sum(t.shape[0] for t in keep))].float())
            if prev is not None:
                finish(prev)                                     # the previous batch is saved while this one is generated
            prev = slot
        if prev is not None:
            finish(prev)
        for slot in slots:
            slot.drain(spent, records)
    finally:
        pool.shutdown(wait=True, cancel_futures=True)
    records.sort(key=lambda r: r['index'])
    if args.png and keep:
        _write_sheet(args, p, keep)
    manifest = _manifest(args, p, records, existing if args.resume else [], spent, time.perf_counter() - t_start, (c, d, h, w), integer)
    with open(p['manifest'], 'w') as f:
        json.dump(manifest, f, indent=1)
        f.write('\n')
    pooled = manifest['pooled']
    print(f'Wrote {len(records)} files of shape {manifest["shape"]} {args.out_dtype} to {directory} (shard {p["rank"]}/{p["world"]}, '
          f'{len(manifest["skipped"])} kept), {manifest["volumes_per_second"]:.2f} volumes/s', file=out)
    if pooled['voxels'] and pooled['clipped_share'] > args.warn_clipped:
        lo, hi = manifest['clip'] or ('-inf', 'inf')
        print(f'warning: {pooled["clipped_share"]:.2%} of the voxels lay outside [{lo}, {hi}] and were clipped ({pooled["below"]} below, '
              f'{pooled["above"]} above, {pooled["nan"]} NaN; --warn_clipped {args.warn_clipped}): widen --clip, or choose an --out_dtype '
              f'that holds the data', file=out)
    return manifest


def _channels(args):
    from .utils import get_num_channels
    return get_num_channels(args.start_shape)


def _write_sheet(args, p, keep):
    from . import preview
    window = (preview.default_window(args.data_mean, args.data_stddev) if args.preview_window is None
              else preview.parse_window(args.preview_window))
    # (render_view reads a second axis of size > 1 as NDHWC's d: several channels go channels-last)
    chunks = [t if t.shape[1] == 1 else t.permute(0, 2, 3, 4, 1).contiguous() for t in keep]
    img = preview.sheet(chunks, args.preview_views, window, p['scale'], p['shift'], args.preview_zoom_d)
    return preview.write_png(p['sheet'], img, dict(phase=args.phase, views=args.preview_views, window=f'{window[0]},{window[1]}',
                                                   seed=args.seed, model=args.model_path))


def _manifest(args, p, records, skipped, spent, wall, shape, integer):
    c, d, h, w = shape
    voxels = c * d * h * w
    pooled = dict(files=len(records), voxels=voxels * len(records), below=sum(r['below'] for r in records),
                  above=sum(r['above'] for r in records), nan=sum(r['nan'] for r in records))
    pooled['clipped_share'] = (pooled['below'] + pooled['above'] + pooled['nan']) / pooled['voxels'] if records else 0.0
    if records and integer:
        pooled.update(file_stats(pooled['voxels'], (sum(r['sum'] for r in records), sum(r['sum_squares'] for r in records),
                                                    min(r['min'] for r in records), max(r['max'] for r in records))))
    elif records:
        pooled.update(min=min(r['min'] for r in records), max=max(r['max'] for r in records))
    from .table_ops import STORE_DEFINITION, _STORE_RANGE
    clip = list(p['clip']) if p['clip'] is not None else (list(_STORE_RANGE[getattr(torch, args.out_dtype)]) if integer else None)
    arguments = {k: v for k, v in vars(args).items()}
    return dict(arguments=arguments, definition=STORE_DEFINITION, scale=p['scale'], shift=p['shift'], clip=clip,
                rounding=args.rounding, dtype=args.out_dtype, shape=[d, h, w] if c == 1 else [c, d, h, w], format=args.format,
                shard=[p['rank'], p['world']], seed=args.seed, latent_dim=args.latent_dim,
                latent=LATENT_RULE if p['latents'] is None else f'row index of {args.latents_path}',
                files=records, skipped=[p['names'][i] for i in skipped], pooled=pooled,
                seconds=dict(spent, wall=wall), volumes_per_second=len(records) / wall if wall > 0 else 0.0,
                seconds_note='generation, store, download: device time between events, summed over batches; save: summed over the '
                             'writer threads (they overlap each other and the device); wall: the whole run, restore included')


def main(argv=None, device=None):
    args = build_parser().parse_args(argv)
    try:
        return run(args, device)
    except (ValueError, FileExistsError) as e:
        raise SystemExit(f'generate: {e}') from None


if __name__ == '__main__':
    main()
