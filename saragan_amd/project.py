"""python -m saragan_amd.project ARCH --model_path CKPT --phase P TARGET_DIR --output_dir OUT: volumes inverted to latents
(DESIGN.md 4.13).  For every `.npy` volume of TARGET_DIR (the training data's layout: [d, h, w] with one channel, else [c, d, h, w];
one shape and one of gather_rows' six dtypes for the whole directory) the latent z* is sought whose image G(z*) is nearest in the
multi-scale residual loss (functional.multiscale_residual: block means over cubes of edge 1, 2, 4, ..., weighted).  The answer per
file is a reconstruction, its error and where it sits -- sample-level recall, the AnoGAN anomaly map |x - G(z*)|, and latents that
generate --latents_path regenerates or edits.  Takes the model flags of generate (conditioning rows are given and held fixed) and:

  --data_mean, --data_stddev: the normalisation the generator was trained under (0 / 1 when neither is given)
  --steps (200), --lr (0.05), --lr_rampup (0.05), --lr_rampdown (0.25): Adam on the latents; iteration i of S runs at
      lr * min(1, (i + 1) / (rampup S)) * (0.5 - 0.5 cos(pi min(1, (1 - i / S) / rampdown))): linear up, cosine down
  --levels (3), --level_weights w0,w1,...: the loss; every extent must be a multiple of 2^(levels - 1)
  --restarts R (1): R initial latents per file, the best one is kept
  --latent_norm none|sphere: with sphere every step ends by rescaling the latent to norm sqrt(latent_dim)
  --batch_size (files per batch; the generator runs batch_size * R rows), --max_samples, --seed
  --out_dtype, --clip, --rounding: how reconstructions are stored, as in generate
  --residual_dir DIR: also |x - reconstruction| per file, in data units and the output type
  --png, --preview_views, --window LO,HI: one sheet per batch, per view three row bands (target, reconstruction, residual)
  --overwrite; --device cpu: the numpy twins of the two kernels, for small cases with a generator handed to run()

The initial latent of file i (its place in the sorted listing), restart r is np.random.default_rng([seed, i, r]).standard_normal(
latent_dim, dtype=np.float32): the result does not depend on the batch size.

The loop: a batch's targets are uploaded once in their stored type; per iteration the generator's forward pass, one
multiscale_residual pass (loss and d loss / d y), the backward pass to z -- the generator's variables take no gradient: no
weight-gradient kernel runs -- and one latent_step_ launch, which keeps every row's best latent so far on the device.  Nothing is
read back inside the loop; a last forward pass and a latent_step_ with lr = 0 score the final latents, then the losses come back
once.  Written under OUT/projected_{phase}/: NAME.npy (the reconstruction from the best restart's best latent, through
store_volumes), latents.npy ([N, latent_dim] float32, sorted file order) and projection.json (arguments, definitions, per file the
best loss, its per-level terms, the RMS difference in data units, the best step, the chosen restart and `failed` when no finite
loss was seen; pooled quartiles of the RMS; seconds per stage)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

from .generate import OUT_DTYPES, _numbers
from .generation import RestoredGenerator, add_model_arguments, label_rows, optional_num_samples
from .utils import get_current_input_shape

TARGET_DTYPES = ('uint8', 'int8', 'int16', 'uint16', 'float16', 'float32')
LATENT_RULE = 'np.random.default_rng([seed, index, restart]).standard_normal(latent_dim, dtype=np.float32)'
SCHEDULE = 'lr * min(1, (i + 1) / (lr_rampup * steps)) * (0.5 - 0.5 * cos(pi * min(1, (1 - i / steps) / lr_rampdown))), i = 0 .. steps - 1'


def build_parser():
    p = add_model_arguments(argparse.ArgumentParser(prog='python -m saragan_amd.project', description=__doc__.split('\n\n')[0]))
    optional_num_samples(p)      # (the directory says how many there are; --max_samples cuts it)
    p.add_argument('target_dir', type=str)
    p.add_argument('--steps', type=int, default=200)
    p.add_argument('--lr', type=float, default=0.05)
    p.add_argument('--lr_rampup', type=float, default=0.05)
    p.add_argument('--lr_rampdown', type=float, default=0.25)
    p.add_argument('--levels', type=int, default=3)
    p.add_argument('--level_weights', type=str, default=None, help='w0,w1,...: one weight per level (default: ones)')
    p.add_argument('--restarts', type=int, default=1)
    p.add_argument('--latent_norm', default='none', choices=['none', 'sphere'])
    p.add_argument('--max_samples', type=int, default=None)
    p.add_argument('--out_dtype', default='uint16', choices=OUT_DTYPES)
    p.add_argument('--clip', type=str, default=None, help='LO,HI in data units (negative LO: --clip=LO,HI); default: the range of --out_dtype')
    p.add_argument('--rounding', default='trunc', choices=['trunc', 'rint'])
    p.add_argument('--residual_dir', type=str, default=None)
    p.add_argument('--png', default=False, action='store_true')
    p.add_argument('--preview_views', type=str, default='slice_d,slice_h,max_h')
    p.add_argument('--window', type=str, default=None, help='with --png: LO,HI in data units; default data_mean - data_stddev,data_mean + 2 data_stddev')
    p.add_argument('--overwrite', default=False, action='store_true')
    p.add_argument('--device', default='cuda', choices=['cuda', 'cpu'])
    return p


def latent_rows(seed, indices, restarts, latent_dim):
    """float32 [len(indices) * restarts, latent_dim]: row k * restarts + r is restart r of file indices[k]."""
    return np.stack([np.random.default_rng([seed, int(i), r]).standard_normal(latent_dim, dtype=np.float32)
                     for i in indices for r in range(restarts)])


def lr_at(i, args):
    """The learning rate of iteration i = 0 .. steps - 1 (SCHEDULE): never 0 inside the loop."""
    up = min(1.0, (i + 1) / (args.lr_rampup * args.steps)) if args.lr_rampup > 0 else 1.0
    down = min(1.0, (1.0 - i / args.steps) / args.lr_rampdown) if args.lr_rampdown > 0 else 1.0
    return args.lr * up * (0.5 - 0.5 * math.cos(math.pi * down))


def plan(args):
    """The checked settings of a run; ValueError / FileExistsError before any work is done, nothing is written."""
    from . import preview
    if (args.data_mean is None) != (args.data_stddev is None):
        raise ValueError('give both --data_mean and --data_stddev, or neither')
    if args.steps < 1 or args.restarts < 1 or args.batch_size < 1 or (args.max_samples is not None and args.max_samples < 1):
        raise ValueError('--steps, --restarts, --batch_size and --max_samples are at least 1')
    if not (args.lr > 0 and math.isfinite(args.lr)) or not 0 <= args.lr_rampup <= 1 or not 0 <= args.lr_rampdown <= 1:
        raise ValueError('--lr is positive, --lr_rampup and --lr_rampdown lie in [0, 1]')
    if not 1 <= args.levels <= 6:
        raise ValueError(f'--levels is 1 .. 6, got {args.levels}')
    weights = [1.0] * args.levels if args.level_weights is None else list(_numbers(args.level_weights, args.levels, '--level_weights'))
    if any(not (math.isfinite(v) and v >= 0) for v in weights):
        raise ValueError(f'--level_weights are finite and >= 0, got {args.level_weights!r}')
    clip = None
    if args.clip is not None:
        clip = _numbers(args.clip, 2, '--clip')
        if args.out_dtype != 'float32':
            if any(not math.isfinite(v) or int(v) != v for v in clip):
                raise ValueError(f'--clip for --out_dtype {args.out_dtype} is two integers, got {args.clip!r}')
            clip = tuple(int(v) for v in clip)
    if args.png and args.device == 'cpu':
        raise ValueError('--png renders on the device: not with --device cpu')
    views = preview.parse_views(args.preview_views) if args.png else None
    scale, shift = (1.0, 0.0) if args.data_mean is None else (float(args.data_stddev), float(args.data_mean))
    if scale == 0.0:
        raise ValueError('--data_stddev is not 0')
    window = None
    if args.png:
        window = preview.default_window(args.data_mean, args.data_stddev) if args.window is None else preview.parse_window(args.window)
    if not os.path.isdir(args.target_dir):
        raise ValueError(f'{args.target_dir} is not a directory')
    names = sorted(n for n in os.listdir(args.target_dir) if n.endswith('.npy'))
    if args.max_samples is not None:
        names = names[:args.max_samples]
    if not names:
        raise ValueError(f'{args.target_dir} holds no .npy volume')
    c, d, h, w = get_current_input_shape(args.phase, 1, args.start_shape)[1:]
    want = ((d, h, w),) if c == 1 else ()
    first = None
    for n in names:
        a = np.load(os.path.join(args.target_dir, n), mmap_mode='r')
        if first is None:
            first = (a.shape, a.dtype)
        if (a.shape, a.dtype) != first:
            raise ValueError(f'{n} is {a.dtype} {a.shape}, {names[0]} is {first[1]} {first[0]}: one shape and one dtype per directory')
    if first[1].name not in TARGET_DTYPES:
        raise ValueError(f'volumes are {", ".join(TARGET_DTYPES)}, got {first[1]}')
    if tuple(first[0]) not in want + ((c, d, h, w),):
        raise ValueError(f'the volumes are {tuple(first[0])}, phase {args.phase} of {args.start_shape} makes {(c, d, h, w)}')
    for name, s in zip('dhw', (d, h, w)):
        if s % (1 << (args.levels - 1)):
            raise ValueError(f'{name} = {s} is not a multiple of 2^{args.levels - 1} for --levels {args.levels}')
    directory = os.path.join(args.output_dir or '.', f'projected_{args.phase}')
    outputs = [os.path.join(directory, n) for n in names + ['latents.npy', 'projection.json']]
    if args.residual_dir:
        outputs += [os.path.join(args.residual_dir, n) for n in names]
    taken = [o for o in outputs if os.path.exists(o)]
    if taken and not args.overwrite:
        raise FileExistsError(f'{taken[0]} exists ({len(taken)} of the outputs do): give --overwrite to replace them')
    return dict(names=names, shape=(c, d, h, w), file_shape=tuple(first[0]), dtype=first[1].name, weights=weights, clip=clip,
                scale=scale, shift=shift, directory=directory, views=views, window=window)


def _grad_free(store):
    """The generator's variables take no gradient: `_wants` asks ctx.needs_input_grad first, which is False for a leaf that
    does not require grad -- so no weight- or bias-gradient kernel runs, and every .grad stays None."""
    for v in store.grad_leaves(''):
        v.requires_grad_(False)
        v.grad = None


def _residual(x, recon, out_dtype):
    """|x - recon| in data units, in the output type (integers: exact, clipped to the type's range)."""
    if out_dtype == 'float32':
        return np.abs(x.astype(np.float32) - recon).astype(np.float32)
    info = np.iinfo(out_dtype)
    diff = np.abs(np.rint(x.astype(np.float64)) - recon.astype(np.float64))
    return np.clip(diff, info.min, info.max).astype(out_dtype)


def _sheet(p, args, target, recon, resid):
    """Per view three row bands: target, reconstruction, residual (data units; the residual's window starts at 0)."""
    from . import preview
    lo, hi = p['window']
    bands = [preview.sheet(t, p['views'], win, 1.0, 0.0) for t, win in ((target, (lo, hi)), (recon, (lo, hi)), (resid, (0.0, hi - lo)))]
    dims = tuple(p['shape'][1:])
    tops, heights, _ = preview.sheet_layout(dims, p['views'])
    rows = [b[t:t + hgt] for t, hgt in zip(tops, heights) for b in bands]
    return np.concatenate(rows, axis=0)


def run(args, device=None, out=sys.stdout, generator=None):
    """Projects the directory.  generator: a differentiable callable (z [rows, L], labels or None) -> y [rows, c, d, h, w] used
    instead of the checkpoint's (what --device cpu needs: the package's generator runs on the device only).  Returns the record
    also written as projection.json."""
    from . import functional as F
    p = plan(args)
    names, (c, d, h, w) = p['names'], p['shape']
    N, R, B, L = len(names), args.restarts, args.batch_size, args.latent_dim
    args.num_samples = N
    labels = label_rows(args)
    t_start = time.perf_counter()
    store = None
    if generator is None:
        if args.device == 'cpu':
            raise ValueError('--device cpu runs the numpy twins of the loss and the update; the generator runs on MI355X only: hand '
                             'run() a generator')
        if not torch.cuda.is_available():
            raise RuntimeError('saragan_amd projects on MI355X only: no CPU fallback')
        device = device or 'cuda'
        if torch.device(device).index is not None:
            torch.cuda.set_device(torch.device(device))
        g = RestoredGenerator(args, device)
        g(torch.zeros(min(B, N) * R, L, device=device),
          None if labels is None else torch.zeros(min(B, N) * R, labels.shape[1], device=device))      # creates the variables
        g.restore(labels is not None)
        store = g.store
        _grad_free(store)

        def generator(z, cond):
            return g(z, cond, grad=z.requires_grad)
    else:
        device = device or args.device
    out_dtype = getattr(torch, args.out_dtype)
    sphere = args.latent_norm == 'sphere'
    spent = dict.fromkeys(('load', 'optimise', 'reconstruct', 'save'), 0.0)
    os.makedirs(p['directory'], exist_ok=True)
    if args.residual_dir:
        os.makedirs(args.residual_dir, exist_ok=True)
    records, latents, iterations = [], np.zeros((N, L), np.float32), 0
    for at in range(0, N, B):
        t0 = time.perf_counter()
        batch = list(range(at, min(at + B, N)))
        nb = len(batch)
        vols = np.stack([np.load(os.path.join(args.target_dir, names[i])).reshape(c, d, h, w) for i in batch])
        table = torch.from_numpy(vols).to(device)      # once per batch, in the stored type
        idx = torch.arange(nb, dtype=torch.int32).repeat_interleave(R).to(device)
        z0 = latent_rows(args.seed, batch, R, L)
        z = torch.from_numpy(z0.copy()).to(device).requires_grad_(True)
        cond = None if labels is None else torch.from_numpy(np.repeat(labels[batch], R, axis=0)).to(device)
        rows = nb * R
        m, v = torch.zeros(rows, L, device=device), torch.zeros(rows, L, device=device)
        best_loss = torch.full((rows,), math.inf, device=device)
        z_best = z.detach().clone()
        best_step = torch.full((rows,), -1, dtype=torch.int32, device=device)
        terms_best = torch.full((rows, args.levels), math.nan, dtype=torch.float64, device=device)
        first_loss = None
        t1 = time.perf_counter()
        spent['load'] += t1 - t0
        for i in range(args.steps + 1):
            scoring = i == args.steps      # one more forward pass scores the final latents: lr = 0 moves nothing
            with torch.set_grad_enabled(not scoring):
                y = generator(z if not scoring else z.detach(), cond)
            loss, terms, grad = F.multiscale_residual_raw(y.detach(), table, idx, p['shift'], p['scale'], args.levels, p['weights'])
            gz = torch.zeros_like(m) if scoring else torch.autograd.grad(y, z, grad)[0].float().contiguous()
            terms_best = torch.where((loss < best_loss)[:, None], terms, terms_best)
            F.latent_step_(z.detach(), m, v, gz, loss, best_loss, z_best, best_step, 0.0 if scoring else lr_at(i, args), i + 1,
                           sphere=sphere)
            if first_loss is None:
                first_loss = loss.clone()
            del y, grad, gz
        iterations += args.steps
        # ---- the one read-back of the batch
        bl, bs = best_loss.cpu().numpy().reshape(nb, R), best_step.cpu().numpy().reshape(nb, R)
        fl, tb = first_loss.cpu().numpy().reshape(nb, R), terms_best.cpu().numpy().reshape(nb, R, args.levels)
        t2 = time.perf_counter()
        spent['optimise'] += t2 - t1
        finite = np.isfinite(bl)
        chosen = np.where(finite, bl, np.inf).argmin(axis=1)
        pick = torch.from_numpy(np.arange(nb) * R + chosen).to(device)
        zb = z_best[pick]
        with torch.no_grad():
            yb = generator(zb, None if cond is None else cond[pick])
        recon_t = F.store_volumes(yb, out_dtype, scale=p['scale'], shift=p['shift'], clip=p['clip'], rounding=args.rounding)
        recon = recon_t.cpu().numpy()
        latents[batch] = zb.cpu().numpy()
        resid = np.stack([_residual(vols[k], recon[k], args.out_dtype) for k in range(nb)])
        if args.png:
            from . import preview
            img = _sheet(p, args, table.reshape(nb, c, d, h, w), recon_t, torch.from_numpy(resid).to(device))
            preview.write_png(os.path.join(p['directory'], f'sheet_{at // B:04d}.png'), img,
                              dict(phase=args.phase, views=args.preview_views, window=f'{p["window"][0]},{p["window"][1]}', bands='target,reconstruction,residual'))
        t3 = time.perf_counter()
        spent['reconstruct'] += t3 - t2
        for k, i in enumerate(batch):
            shape = p['file_shape']
            np.save(os.path.join(p['directory'], names[i]), recon[k].reshape(shape))
            if args.residual_dir:
                np.save(os.path.join(args.residual_dir, names[i]), resid[k].reshape(shape))
            diff = vols[k].astype(np.float64) - recon[k].astype(np.float64)
            r = int(chosen[k])
            failed = not bool(finite[k].any())
            records.append(dict(index=i, name=names[i], failed=failed, restart=r, best_loss=None if failed else float(bl[k, r]),
                                terms=None if failed else [float(t) for t in tb[k, r]], best_step=int(bs[k, r]),
                                initial_loss=float(fl[k, r]) if math.isfinite(float(fl[k, r])) else None,
                                rms=float(np.sqrt(np.mean(diff * diff))),
                                restart_losses=[float(x) if math.isfinite(float(x)) else None for x in bl[k]]))
        spent['save'] += time.perf_counter() - t3
    np.save(os.path.join(p['directory'], 'latents.npy'), latents)
    rms = np.array([r['rms'] for r in records if not r['failed']])
    pooled = dict(files=N, failed=sum(r['failed'] for r in records))
    if rms.size:
        q = np.percentile(rms, [25, 50, 75])
        pooled.update(rms_q1=float(q[0]), rms_median=float(q[1]), rms_q3=float(q[2]), rms_min=float(rms.min()), rms_max=float(rms.max()))
    wall = time.perf_counter() - t_start
    record = dict(arguments=dict(vars(args)), definition=F.PROJECT_DEFINITION, latent_step=F.LATENT_STEP_DEFINITION, latent=LATENT_RULE,
                  schedule=SCHEDULE, seed=args.seed, latent_dim=L, restarts=R, levels=args.levels, level_weights=p['weights'],
                  scale=p['scale'], shift=p['shift'], dtype=args.out_dtype, target_dtype=p['dtype'], shape=list(p['file_shape']),
                  best_step_note='steps count from 1: best_step s means the latent after s - 1 updates; steps + 1 is the final latent',
                  files=records, pooled=pooled, seconds=dict(spent, wall=wall),
                  seconds_per_iteration=spent['optimise'] / iterations if iterations else None,
                  seconds_note='load: files read and uploaded; optimise: the loop and its one read-back; reconstruct: the best '
                               'latents\' forward pass, store_volumes, residuals and sheets; save: files written; wall: everything, '
                               'restore included.  seconds_per_iteration: optimise per loop iteration of one batch')
    with open(os.path.join(p['directory'], 'projection.json'), 'w') as f:
        json.dump(record, f, indent=1)
        f.write('\n')
    if store is not None:
        record['variables_with_grad'] = [k for k, v_ in store.vars.items() if v_.grad is not None]
    print(f'Projected {N} volumes of shape {list(p["file_shape"])} to {p["directory"]} ({R} restarts, {args.steps} steps, '
          f'{pooled["failed"]} failed); median RMS {pooled.get("rms_median", float("nan")):.4g}', file=out)
    return record


def main(argv=None, device=None):
    args = build_parser().parse_args(argv)
    try:
        return run(args, device)
    except (ValueError, FileExistsError) as e:
        raise SystemExit(f'project: {e}') from None


if __name__ == '__main__':
    main()
