"""Memorisation audit of a synthetic dataset (not in the reference): are the generated volumes new, or copies of
training volumes?  For integer data (what prepare_data and generate store) every decision is a comparison of EXACT integer
squared distances, computed on the device by sg_sqdist_exact (byte-split int8 MFMAs) and kept as the k nearest per query by
sg_topk_merge while the training set streams through a pinned buffer, a chunk at a time.

  * every fake f: its k nearest training files and d^2 to them, and the RMS difference per voxel sqrt(d^2 / v) in data units;
  * every training file t: loo(t), the squared distance to its nearest OTHER training file;
  * duplicates: fakes with d^2 = 0 to some training file;
  * unauthentic: fakes with d^2(f, nn(f)) < loo(nn(f)) -- closer to a patient than any other patient is (the authenticity
    test of Alaa et al., "How faithful is your synthetic data?", ICML 2022); the report gives the authentic share;
  * with --holdout_dir: the data-copying statistic of Meehan et al. ("A non-parametric test to detect data-copying in
    generative models", AISTATS 2020): the Mann-Whitney z of the fakes' nearest-training distances against the holdout's
    (negative: fakes sit closer to the training set than unseen real data does), and the holdout's own unauthentic share as
    the baseline.

    python -m saragan_amd.metrics.memorisation TRAIN_DIR FAKE_DIR [--k 3] [--holdout_dir DIR] [--chunk N] [--query_block N]
                     [--max_queries N] [--max_train N] [--report PATH] [--png PATH --png_pairs P --window LO,HI] [--device cuda|cpu]

reads .npy volumes in their own dtype (uint8, int8, int16, uint16; float32 takes the f32 path of sample_metrics in f64 and is
reported as "exact": false).  The report is the same whatever --chunk and --query_block are.  Mirrored or shifted copies are
not looked for."""
import json
import math
import os
import time

import numpy as np
import torch

DEFINITION = ('d2(a, b) = sum over voxels of (a - b)^2, an exact integer for integer data; nearest: ascending by (d2, training index); '
              'rms = sqrt(d2 / voxels); loo(t) = min over training files u != t of d2(t, u); duplicate: d2(f, nn(f)) == 0; '
              'unauthentic: d2(f, nn(f)) < loo(nn(f)); ratio = d2(f, nn(f)) / loo(nn(f)) (null when loo is 0); authentic_share = '
              '1 - unauthentic / fakes; data_copying_z = (U - n m / 2) / sqrt(n m (n + m + 1) / 12), U = R - n (n + 1) / 2, R the sum of '
              'the n fakes\' mid-ranks among the pooled n + m nearest-training d2 of fakes and holdout volumes')
QUANTILES = (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 1.0)
_EXACT = ('uint8', 'int8', 'int16', 'uint16')
_TORCH = {'uint8': torch.uint8, 'int8': torch.int8, 'int16': torch.int16, 'uint16': torch.uint16, 'float32': torch.float32}


def list_volumes(path, limit=None):
    """The sorted .npy files of a directory with the (shape, dtype name) they share, read from the headers alone."""
    if not os.path.isdir(path):
        raise ValueError(f'{path}: not a directory')
    files = [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith('.npy')]
    if limit is not None:
        files = files[:limit]
    if not files:
        raise ValueError(f'{path}: no .npy files')
    kinds = {}
    for f in files:
        a = np.load(f, mmap_mode='r')
        kinds.setdefault((tuple(a.shape), a.dtype.name), f)
    if len({s for s, _ in kinds}) != 1:
        raise ValueError(f'{path}: volumes of different shapes: ' + ', '.join(f'{os.path.basename(f)} {s}' for (s, _), f in kinds.items()))
    if len(kinds) != 1:
        raise ValueError(f'{path}: mixed dtypes: ' + ', '.join(f'{os.path.basename(f)} {d}' for (_, d), f in kinds.items()))
    (shape, dtype), = kinds
    return files, shape, dtype


def _read_into(dst, files):
    for j, f in enumerate(files):
        np.copyto(dst[j], np.load(f).reshape(-1))


class _Clock:
    """Seconds per stage: host stages by perf_counter, device stages by event pairs read after the last synchronisation."""

    def __init__(self, cuda):
        self.cuda, self.host, self.pairs = cuda, {'read': 0.0, 'upload': 0.0, 'distances': 0.0, 'topk': 0.0}, []

    def host_add(self, stage, seconds):
        self.host[stage] += seconds

    def begin(self, stream=None):
        if not self.cuda:
            return time.perf_counter()
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        return e

    def end(self, stage, start, stream=None):
        if not self.cuda:
            self.host[stage] += time.perf_counter() - start
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        self.pairs.append((stage, start, e))

    def result(self):
        if self.cuda:
            torch.cuda.synchronize()
            for stage, a, b in self.pairs:
                self.host[stage] += a.elapsed_time(b) * 1e-3
            self.pairs = []
        return dict(self.host)


def stream_chunks(files, chunk, voxels, dtype, device, clock):
    """Yields (start, rows [count, voxels] on `device`) over `files`, `chunk` at a time.  On the device two pinned host buffers
    and two device buffers alternate: chunk i + 1 is read and its upload queued on a copy stream while chunk i is in use."""
    starts = list(range(0, len(files), chunk))
    np_dtype = np.dtype(dtype)
    if device.type != 'cuda':
        for s in starts:
            part = files[s:s + chunk]
            t0 = time.perf_counter()
            buf = np.empty((len(part), voxels), np_dtype)
            _read_into(buf, part)
            clock.host_add('read', time.perf_counter() - t0)
            yield s, torch.from_numpy(buf)
        return
    rows = min(chunk, len(files))
    pinned = [torch.empty((rows, voxels), dtype=_TORCH[dtype], pin_memory=True) for _ in range(2)]
    dev = [torch.empty((rows, voxels), dtype=_TORCH[dtype], device=device) for _ in range(2)]
    copied = [torch.cuda.Event() for _ in range(2)]
    used = [torch.cuda.Event() for _ in range(2)]
    copy, main = torch.cuda.Stream(device), torch.cuda.current_stream(device)

    def issue(i):
        slot, part = i % 2, files[starts[i]:starts[i] + chunk]
        if i >= 2:
            copied[slot].synchronize()      # the pinned buffer's previous upload has left it
        t0 = time.perf_counter()
        _read_into(pinned[slot].numpy(), part)
        clock.host_add('read', time.perf_counter() - t0)
        if i >= 2:
            copy.wait_event(used[slot])      # the device buffer's previous chunk has been consumed
        with torch.cuda.stream(copy):
            e = clock.begin(copy)
            dev[slot][:len(part)].copy_(pinned[slot][:len(part)], non_blocking=True)
            clock.end('upload', e, copy)
            copied[slot].record(copy)
        return len(part)

    counts = {0: issue(0)}
    for i, s in enumerate(starts):
        if i + 1 < len(starts):
            counts[i + 1] = issue(i + 1)
        main.wait_event(copied[i % 2])
        yield s, dev[i % 2][:counts[i]]
        used[i % 2].record(main)
    torch.cuda.synchronize(device)      # the buffers go away with this frame


def _distances(q, r, same, exact):
    """int64 [mq, mr] whose order is the distances' order: the exact integers, or the bit patterns of non-negative f64."""
    from .. import table_ops as T
    if exact:
        return T.sqdist_exact(q) if same else T.sqdist_exact(q, r)
    if not q.is_cuda:
        a, b = q.numpy().astype(np.float64), r.numpy().astype(np.float64)
        d = np.stack([((b - a[i]) ** 2).sum(axis=1) for i in range(a.shape[0])])
        return torch.from_numpy(d).view(torch.int64)
    from .sample_metrics import pairwise_sqdist
    rows = lambda t: T.gather_rows(t, torch.arange(t.shape[0], device=t.device, dtype=torch.int32))
    a = rows(q)
    return pairwise_sqdist(a, None if same else rows(r)).view(torch.int64)      # (max(0, .): never negative, so the bits sort)


def nearest_training(query_files, train_files, voxels, dtype, k, chunk, query_block, device, clock, self_set=False):
    """(d [n, k], id [n, k]) numpy: the k nearest training files of every query file, ascending by (d2, training index); d is
    int64 for integer data and float64 otherwise, empty entries (fewer than k candidates) have id -1.  self_set: the queries ARE
    the training files, each skips itself, and a query block that meets its own chunk takes the symmetric kernel."""
    from .. import table_ops as T
    exact = dtype in _EXACT
    out_d, out_id = [], []
    for q0, q in stream_chunks(query_files, query_block, voxels, dtype, device, clock):
        q = q.clone() if q.is_cuda else q      # resident while the training set streams through the other buffers
        q_ids = torch.arange(q0, q0 + q.shape[0], dtype=torch.int64, device=q.device) if self_set else None
        best = None
        for r0, r in stream_chunks(train_files, chunk, voxels, dtype, device, clock):
            same = self_set and r0 == q0 and r.shape[0] == q.shape[0]
            t = clock.begin()
            d = _distances(r if same else q, r, same, exact)
            clock.end('distances', t)
            t = clock.begin()
            best = T.nearest_rows(d, k, r_base=r0, q_ids=q_ids, best=best)
            clock.end('topk', t)
        out_d.append(best[0].cpu().numpy())
        out_id.append(best[1].cpu().numpy())
    d, ids = np.concatenate(out_d), np.concatenate(out_id)
    if not exact:
        d = np.where(ids >= 0, d.view(np.float64), np.inf)
    return d, ids


def mann_whitney_z(x, y):
    """The z of Meehan et al.: U of x against y from mid-ranks in the pooled sample, f64; negative when x sits below y."""
    x, y = np.asarray(x), np.asarray(y)
    n, m = len(x), len(y)
    _, inv, counts = np.unique(np.concatenate([x, y]), return_inverse=True, return_counts=True)
    mid = np.cumsum(counts).astype(np.float64) - (counts.astype(np.float64) - 1.0) / 2.0
    u = mid[inv[:n]].sum() - n * (n + 1) / 2.0
    return float((u - n * m / 2.0) / math.sqrt(n * m * (n + m + 1) / 12.0))


def _num(x, exact):
    return int(x) if exact else float(x)


def query_rows(files, d, ids, train_files, loo, voxels, exact):
    """The per-file rows of the report for one query set."""
    rows = []
    for i, f in enumerate(files):
        have = [j for j in range(d.shape[1]) if ids[i, j] >= 0]
        d2, nn = _num(d[i, 0], exact), int(ids[i, 0])
        loo_nn = _num(loo[nn], exact)
        rows.append({'file': os.path.basename(f),
                     'nearest': [os.path.basename(train_files[ids[i, j]]) for j in have],
                     'nearest_index': [int(ids[i, j]) for j in have],
                     'd2': [_num(d[i, j], exact) for j in have],
                     'rms': [math.sqrt(_num(d[i, j], exact) / voxels) for j in have],
                     'loo_of_nearest': loo_nn,
                     'ratio': d2 / loo_nn if loo_nn > 0 else None,
                     'duplicate': d2 == 0,
                     'authentic': not d2 < loo_nn})
    return rows


def worst_order(rows):
    """Indices of the rows, the smallest d2 / loo first (an undefined ratio last); ties by position."""
    return sorted(range(len(rows)), key=lambda i: (math.inf if rows[i]['ratio'] is None else rows[i]['ratio'], i))


def _quantiles(values):
    q = np.quantile(np.asarray(values, np.float64), QUANTILES)
    return {f'{p:g}': float(v) for p, v in zip(QUANTILES, q)}


def pair_sheet(rows, order, pairs, fake_files, train_files, window, device):
    """numpy uint8 sheet: per drawn fake two columns, the fake and its nearest training volume (preview.sheet)."""
    from .. import preview
    picks = order[:pairs]
    vols = []
    for i in picks:
        vols += [np.load(fake_files[i]), np.load(train_files[rows[i]['nearest_index'][0]])]
    x = np.stack(vols)
    if x.ndim == 5 and x.shape[1] == 1:
        x = x[:, 0]
    if window is None:
        lo, hi = float(x.min()), float(x.max())
        window = (lo, hi if hi > lo else lo + 1.0)
    return preview.sheet(torch.from_numpy(np.ascontiguousarray(x)).to(device), preview.DEFAULT_VIEWS, window), picks, window


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog='python -m saragan_amd.metrics.memorisation', description=__doc__.split('\n\n')[0])
    p.add_argument('train_dir')
    p.add_argument('fake_dir')
    p.add_argument('--k', type=int, default=3, help='nearest training files kept per generated volume (1 .. 16)')
    p.add_argument('--holdout_dir', default=None, help='real volumes the generator never saw: the baseline and the data-copying z')
    p.add_argument('--chunk', type=int, default=256, help='training volumes per upload')
    p.add_argument('--query_block', type=int, default=256, help='query volumes resident on the device at a time')
    p.add_argument('--max_queries', type=int, default=None, help='the first N files of FAKE_DIR (and of the holdout)')
    p.add_argument('--max_train', type=int, default=None, help='the first N files of TRAIN_DIR')
    p.add_argument('--report', default=None, help='default: FAKE_DIR/memorisation.json')
    p.add_argument('--png', default=None, help='a sheet of the worst pairs: each fake next to its nearest training volume')
    p.add_argument('--png_pairs', type=int, default=8)
    p.add_argument('--window', default=None, help='LO,HI in data units for --png (default: the range of the volumes drawn)')
    p.add_argument('--device', default='cuda', choices=('cuda', 'cpu'))
    return p


def main(argv=None):
    from .. import table_ops as T
    args = build_parser().parse_args(argv)
    t_start = time.perf_counter()
    try:
        if not 1 <= args.k <= T.TOPK_MAX:
            raise ValueError(f'--k is 1 .. {T.TOPK_MAX}, got {args.k}')
        for name in ('chunk', 'query_block', 'png_pairs'):
            if getattr(args, name) < 1:
                raise ValueError(f'--{name} is at least 1')
        for name in ('max_queries', 'max_train'):
            if getattr(args, name) is not None and getattr(args, name) < 1:
                raise ValueError(f'--{name} is at least 1')
        window = None
        if args.window is not None:
            from ..preview import parse_window
            window = parse_window(args.window)
        train_files, shape, dtype = list_volumes(args.train_dir, args.max_train)
        sets = [('fakes', args.fake_dir)] + ([('holdout', args.holdout_dir)] if args.holdout_dir else [])
        queries = {}
        for name, path in sets:
            files, s, dt = list_volumes(path, args.max_queries)
            if s != shape:
                raise ValueError(f'volumes differ in shape: {args.train_dir} {shape}, {path} {s}')
            if dt != dtype:
                raise ValueError(f'volumes differ in dtype: {args.train_dir} {dtype}, {path} {dt}')
            queries[name] = files
        if dtype not in _TORCH:
            raise ValueError(f'{args.train_dir}: {dtype} volumes; the audit reads uint8, int8, int16, uint16 and float32')
        voxels = int(np.prod(shape, dtype=np.int64))
        if not 1 <= voxels < 2 ** 31:
            raise ValueError(f'volumes of {voxels} voxels; 1 .. 2^31 - 1 are supported')
        if len(train_files) < 2:
            raise ValueError(f'{args.train_dir}: the nearest OTHER training file needs at least 2 files')
        dims = shape[1:] if len(shape) == 4 and shape[0] == 1 else shape
        if args.png is not None and (len(dims) != 3 or args.device != 'cuda'):
            raise ValueError('--png draws [d, h, w] volumes on the device (--device cuda)')
    except ValueError as e:
        raise SystemExit(f'memorisation: {e}') from None
    if args.device == 'cuda' and not torch.cuda.is_available():
        raise RuntimeError('memorisation: --device cuda needs the GPU (--device cpu runs the numpy path)')
    device = torch.device('cuda', torch.cuda.current_device()) if args.device == 'cuda' else torch.device('cpu')
    exact = dtype in _EXACT
    clock = _Clock(device.type == 'cuda')
    stream = dict(voxels=voxels, dtype=dtype, chunk=args.chunk, device=device, clock=clock)
    print(f'{len(train_files)} training and {len(queries["fakes"])} generated volumes of shape {tuple(shape)}, {dtype}')
    if not exact:
        print('float32 volumes: distances are f32 products summed in f64 (sg_pairwise_sqdist), not exact integers -- "exact": false')

    loo_d, loo_id = nearest_training(train_files, train_files, k=1, query_block=args.chunk, self_set=True, **stream)
    loo = loo_d[:, 0]
    report = {'tool': 'saragan_amd.metrics.memorisation', 'arguments': vars(args), 'definition': DEFINITION, 'exact': exact,
              'dtype': dtype, 'shape': list(shape), 'voxels': voxels, 'k': args.k,
              'train': [{'file': os.path.basename(f), 'loo': _num(loo[i], exact), 'loo_rms': math.sqrt(_num(loo[i], exact) / voxels),
                         'loo_nearest': os.path.basename(train_files[loo_id[i, 0]])} for i, f in enumerate(train_files)]}
    pooled = {'train': len(train_files), 'quantiles': {'train_loo_rms': _quantiles([r['loo_rms'] for r in report['train']])}}
    nearest = {}
    for name, files in queries.items():
        d, ids = nearest_training(files, train_files, k=args.k, query_block=args.query_block, **stream)
        rows = query_rows(files, d, ids, train_files, loo, voxels, exact)
        report[name] = rows
        nearest[name] = [r['d2'][0] for r in rows]
        bad = sum(not r['authentic'] for r in rows)
        pooled[name] = len(rows)
        pooled[f'{name}_duplicates' if name != 'fakes' else 'duplicates'] = sum(r['duplicate'] for r in rows)
        pooled[f'{name}_unauthentic' if name != 'fakes' else 'unauthentic'] = bad
        pooled[f'{name}_authentic_share' if name != 'fakes' else 'authentic_share'] = 1.0 - bad / len(rows)
        pooled['quantiles'][f'{name}_nn_rms'] = _quantiles([r['rms'][0] for r in rows])
    if 'holdout' in nearest:
        pooled['data_copying_z'] = mann_whitney_z(nearest['fakes'], nearest['holdout'])
    report['pooled'] = pooled
    order = worst_order(report['fakes'])
    report['worst'] = [report['fakes'][i]['file'] for i in order[:args.png_pairs]]

    print(f"Duplicates (d2 = 0): {pooled['duplicates']} of {pooled['fakes']}")
    print(f"Unauthentic (closer to a training file than any other training file is): {pooled['unauthentic']} of {pooled['fakes']}; "
          f"authentic share {pooled['authentic_share']:.4f}")
    if 'holdout' in nearest:
        print(f"Holdout baseline: unauthentic {pooled['holdout_unauthentic']} of {pooled['holdout']}; authentic share "
              f"{pooled['holdout_authentic_share']:.4f}")
        print(f"Data-copying z (fakes against holdout; negative: fakes closer to the training set): {pooled['data_copying_z']:.4f}")
    for key, label in (('fakes_nn_rms', 'fake -> nearest training'), ('train_loo_rms', 'training -> nearest other training')):
        print(f'RMS per voxel, {label}, quantiles ' + ' '.join(f'{p}: {v:.6g}' for p, v in pooled['quantiles'][key].items()))
    print(f'Worst {min(args.png_pairs, len(order))} by d2 / loo:')
    for i in order[:args.png_pairs]:
        r = report['fakes'][i]
        ratio = 'n/a' if r['ratio'] is None else f"{r['ratio']:.6g}"
        print(f"  {r['file']} -> {r['nearest'][0]}: d2 {r['d2'][0]}, rms {r['rms'][0]:.6g}, loo {r['loo_of_nearest']}, ratio {ratio}"
              + (' DUPLICATE' if r['duplicate'] else '' if r['authentic'] else ' UNAUTHENTIC'))

    if args.png is not None:
        from ..preview import write_png
        img, picks, window = pair_sheet(report['fakes'], order, args.png_pairs, queries['fakes'], train_files, window, device)
        write_png(args.png, img, dict(pairs=','.join(f"{report['fakes'][i]['file']}|{report['fakes'][i]['nearest'][0]}" for i in picks),
                                      window=f'{window[0]},{window[1]}', views='slice_d,slice_h,max_h'))
        print(f'Wrote {args.png}: {len(picks)} pairs, {img.shape[1]} x {img.shape[0]} pixels')
    seconds = clock.result()
    seconds['total'] = time.perf_counter() - t_start
    report['seconds'] = seconds
    print('Seconds: ' + ', '.join(f'{k_} {v:.3f}' for k_, v in seconds.items()))
    path = args.report or os.path.join(args.fake_dir, 'memorisation.json')
    with open(path, 'w') as f:
        json.dump(report, f, indent=1)
    print(f'Wrote {path}')
    return report


if __name__ == '__main__':
    main()
