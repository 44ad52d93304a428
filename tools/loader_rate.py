"""What the device-resident dataset (--device_dataset_gib) costs and buys, measured on the GPU in ONE process with
the two loaders alternating: for each phase shape of the benchmarked 's' configuration (1x4x4 ... 32x128x128; synthetic int16
volumes, 256 files, batch 32)

  1. loader alone:   batches/s of next() with a stream synchronise per batch, PinnedPrefetcher and ResidentLoader;
  2. loader in loop: volumes/s of train.run_training restricted to that phase, both loaders, hipGraph replay forced and forbidden
                     (timed from a device synchronise after the warm-up steps to one after the last step);
  3. load cost:      the one-off time of DeviceTable (files in the page cache) and its bytes;
  4. kernel alone:   sg_gather_rows at the phase-6 shape by device events, as bytes read + written over its time.

Every figure is the median of --repeats runs with their minimum and maximum.  Nothing here is asserted: the file this prints
(profiles/device_dataset_cost.txt) is the record.

  python tools/loader_rate.py --out profiles/device_dataset_cost.txt [--phases 1,2,3,4,5,6] [--repeats 5] [--no_loop]
"""
import argparse
import contextlib
import io
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {p: (2 ** (p - 1), 4 * 2 ** (p - 1), 4 * 2 ** (p - 1)) for p in range(1, 7)}      # phase -> (Z, Y, X)
LOOP_STEPS = {1: 150, 2: 150, 3: 150, 4: 150, 5: 60, 6: 24}                                 # timed steps per run
WARM_STEPS = 8                                                                               # (two eager steps, then the capture)


def spread(vals):
    return f'{statistics.median(vals):11.1f}  [{min(vals):.1f} .. {max(vals):.1f}]'


def write_files(root, phases, nfiles):
    from benchlib.workload import synthetic_volume
    for p in range(1, 7):      # run_training opens every phase directory up to the one it trains
        d = os.path.join(root, f'{SHAPES[p][-1]}x{SHAPES[p][-1]}')
        os.makedirs(d)
        for i in range(nfiles if p in phases else 0):
            np.save(os.path.join(d, f'{i:04d}.npy'), synthetic_volume(SHAPES[p], 10_000 + i))


def dataset(root, phase):
    from saragan_amd.dataset import NumpyPathDataset
    with contextlib.redirect_stdout(io.StringIO()):
        return NumpyPathDataset(os.path.join(root, f'{SHAPES[phase][-1]}x{SHAPES[phase][-1]}/'), None, False, True, seed=42)


def loader_alone(root, phase, batch, repeats, emit):
    import torch
    from saragan_amd.dataset import DeviceTable, PinnedPrefetcher, ResidentLoader
    stream = torch.cuda.current_stream()
    loads = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table = DeviceTable(dataset(root, phase), 'cuda:0')
        torch.cuda.synchronize()
        loads.append((time.perf_counter() - t0) * 1e3)
    nbatches = max(20, min(400, int(2e5 / (batch * np.prod(SHAPES[phase]) / 1e3 + 50))))
    rates = {'pinned': [], 'resident': []}
    for _ in range(repeats):
        for kind in ('pinned', 'resident'):      # alternating
            ds = dataset(root, phase)
            ld = PinnedPrefetcher(ds, batch, False, 1024.0, 1024.0, 'cuda:0') if kind == 'pinned' else \
                ResidentLoader(ds, batch, False, 1024.0, 1024.0, 'cuda:0', table=table)
            for _ in range(10):
                ld.next()
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(nbatches):
                ld.next()
                stream.synchronize()
            rates[kind].append(nbatches / (time.perf_counter() - t0))
            ld.close()
    emit(f'phase {phase}  {"x".join(map(str, SHAPES[phase])):>11}  loader alone, batches/s ({nbatches} batches per run)')
    emit(f'    PinnedPrefetcher  {spread(rates["pinned"])}')
    emit(f'    ResidentLoader    {spread(rates["resident"])}')
    emit(f'    DeviceTable load  {spread(loads)} ms   {table.nbytes} bytes')
    return table


class Timed:
    """A loader whose next() / close() bracket the timed steps with device synchronises."""

    def __init__(self, inner, warm):
        self.inner, self.warm, self.calls, self.t0, self.t1 = inner, warm, 0, None, None

    @property
    def labels(self):
        return self.inner.labels

    def next(self):
        import torch
        if self.calls == self.warm:
            torch.cuda.synchronize()
            self.t0 = time.perf_counter()
        self.calls += 1
        return self.inner.next()

    def close(self):
        import torch
        torch.cuda.synchronize()
        self.t1 = time.perf_counter()
        self.inner.close()


def loop_rate(root, logdir, phase, batch, gib, hipgraph):
    import saragan_amd.train as T
    from saragan_amd.main import build_parser, finalize_args
    # (get_num_phases counts the doublings from start to final shape: 128^2 is phase 6, the last of 4^2 -> 256^2)
    argv = ['pgan', root + '/', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 64, 256, 256)', '--network_size', 's',
            '--starting_phase', str(phase), '--ending_phase', str(phase), '--base_batch_size', str(batch * 2 ** (phase - 1)),
            '--latent_dim', '512', '--noise_stddev', '0.01', '--mixing_nimg', '0', '--stabilizing_nimg', str(1 << 30),
            '--starting_alpha', '0', '--loss_fn', 'wgan', '--gp_weight', '10', '--data_mean', '1024', '--data_stddev', '1024',
            '--logdir', logdir, '--checkpoint_every_nsteps', str(1 << 40), '--dtype', 'bf16', '--validation_fraction', '0',
            '--test_fraction', '0', '--device_dataset_gib', str(gib)]
    args, _ = build_parser().parse_known_args(argv)
    args = finalize_args(args)
    os.environ['SARAGAN_HIPGRAPH'] = '1' if hipgraph else '0'      # (what main.py does for --hipgraph / --no_hipgraph)
    made = []
    make = T.make_loader

    def timed(*a, **kw):
        made.append(Timed(make(*a, **kw), WARM_STEPS))
        return made[-1]

    T.make_loader = timed
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            T.run_training(args, max_steps_per_phase=WARM_STEPS + LOOP_STEPS[phase], log_every=1 << 40)
    finally:
        T.make_loader = make
    if len(made) != 1:
        raise RuntimeError(f'phase {phase} was not trained ({len(made)} loaders made)')
    ld = made[-1]
    want = 'ResidentLoader' if gib > 0 else 'PinnedPrefetcher'
    assert type(ld.inner).__name__ == want, (type(ld.inner).__name__, want)
    return (ld.calls - ld.warm) * batch / (ld.t1 - ld.t0)


def kernel_alone(table, batch, repeats, emit):
    import torch
    from saragan_amd import functional as F
    vol = int(np.prod(table.volumes.shape[1:]))
    idx = torch.randperm(len(table), device='cuda')[:batch].to(torch.int32)
    out = torch.empty((batch,) + tuple(table.volumes.shape[1:]), device='cuda')
    for _ in range(5):
        F.gather_rows(table.volumes, idx, 1024.0, 1024.0, out=out)
    nbytes = batch * vol * (table.volumes.element_size() + 4)
    rates, launches = [], 200
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            F.gather_rows(table.volumes, idx, 1024.0, 1024.0, out=out)
        e1.record()
        e1.synchronize()
        rates.append(nbytes * launches / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    emit(f'kernel alone: sg_gather_rows {batch} x {"x".join(map(str, table.volumes.shape[2:]))} {table.volumes.dtype} -> f32, '
         f'{nbytes / 1e6:.1f} MB read + written per launch, {launches} launches per run (device events)')
    emit(f'    GB/s              {spread(rates)}      (plain copy: about 6300 GB/s)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--phases', default='1,2,3,4,5,6')
    ap.add_argument('--files', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no_loop', action='store_true', help='skip the run_training part')
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('loader_rate.py measures on the GPU: no device found')
    phases = [int(p) for p in a.phases.split(',')]
    lines = []

    def emit(line=''):
        print(line, flush=True)
        lines.append(line)
        if a.out:      # written as it grows: a run that is cut short leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')

    tmp = tempfile.mkdtemp(prefix='saragan_loader_rate_')
    try:
        write_files(tmp, phases, a.files)
        emit(f'# tools/loader_rate.py: {torch.cuda.get_device_name(0)}, {a.files} int16 files per phase, batch {a.batch}, '
             f'{a.repeats} alternating runs each: median [min .. max]')
        table = None
        for p in phases:
            table = loader_alone(tmp, p, a.batch, a.repeats, emit)
            if p == 6:
                kernel_alone(table, a.batch, a.repeats, emit)
        del table
        torch.cuda.empty_cache()
        if not a.no_loop:
            emit()
            emit(f'# loader in the loop: volumes/s of run_training on one phase ({WARM_STEPS} untimed steps, then the timed ones)')
            for p in sorted(phases, key=lambda q: (q != 6, q)):      # the benchmarked phase first
                for hipgraph in (False, True):
                    rates = {0.0: [], 64.0: []}
                    for r in range(a.repeats):
                        for gib in (0.0, 64.0):      # alternating
                            logdir = os.path.join(tmp, 'log')
                            rates[gib].append(loop_rate(tmp, logdir, p, a.batch, gib, hipgraph))
                            shutil.rmtree(logdir, ignore_errors=True)
                    emit(f'phase {p}  {"x".join(map(str, SHAPES[p])):>11}  hipGraph {"forced" if hipgraph else "off   "}  '
                         f'{LOOP_STEPS[p]} timed steps per run')
                    emit(f'    PinnedPrefetcher  {spread(rates[0.0])}')
                    emit(f'    ResidentLoader    {spread(rates[64.0])}')
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
