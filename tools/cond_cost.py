"""Step time of a short training run without --conditioning_path and with label tables of width L = 1 and L = 10, in one process
on one GPU: the benchmarked configuration's last phase (pgan 's', phase 6, [32, 1, 32, 128, 128] per step, bf16, wgan,
simultaneous) through train.run_training on synthetic LIDC-shaped volumes.  Each setting runs `--rounds` times, alternating; the
first `--skip` steps of a run (lazy initialisation, the capture decision) are left out of its figure by timing a second, longer
run against a shorter one.  The spread of one setting over the rounds is the yardstick for the differences between settings.
Run it on the parent commit too (only `off` exists there: --widths "") for the "off equals parent" comparison.
profiles/conditioning_cost.txt is this tool's output.

    python tools/cond_cost.py [--steps 300] [--rounds 2] [--widths 1,10]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FILES = 36


def make_data(root, phases):
    from benchlib.workload import synthetic_volume
    for ph in range(1, phases + 1):
        z, xy = 2 ** (ph - 1), 4 * 2 ** (ph - 1)
        d = os.path.join(root, 'volumes', f'{xy}x{xy}')
        os.makedirs(d)
        for i in range(FILES):
            np.save(os.path.join(d, f'{i:04d}.npy'), synthetic_volume((z, xy, xy), i))


def make_labels(root, width):
    """One-hot rows (width 1: all ones), outside the phase directories."""
    path = os.path.join(root, f'labels_{width}.npy')
    np.save(path, np.eye(width, dtype=np.float32)[np.arange(FILES) % width])
    return path


def run(data, labels, steps):
    import torch
    from saragan_amd.main import build_parser, finalize_args
    from saragan_amd.train import run_training
    argv = ['pgan', os.path.join(data, 'volumes') + '/', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 64, 256, 256)',
            '--starting_phase', '6', '--ending_phase', '6', '--base_batch_size', '1024', '--latent_dim', '512', '--network_size', 's',
            '--noise_stddev', '0.01', '--mixing_nimg', '0', '--stabilizing_nimg', str(1 << 24), '--loss_fn', 'wgan', '--gp_weight',
            '10', '--data_mean', '1024', '--data_stddev', '1024', '--starting_alpha', '0', '--checkpoint_every_nsteps', str(1 << 30),
            '--validation_fraction', '0', '--test_fraction', '0']
    if labels:
        argv += ['--conditioning_path', labels]
    with tempfile.TemporaryDirectory() as logdir:
        args = finalize_args(build_parser().parse_args(argv + ['--logdir', logdir]))
        t0 = time.time()
        out = run_training(args, max_steps_per_phase=steps, log_every=1 << 30)
        torch.cuda.synchronize()
        return time.time() - t0, out['stats'][6]['batch_size']


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--skip', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--widths', type=str, default='1,10')
    a = ap.parse_args()
    widths = [int(w) for w in a.widths.split(',') if w]
    with tempfile.TemporaryDirectory() as data:
        make_data(data, 6)
        settings = [('off', None)] + [(f'L = {w}', make_labels(data, w)) for w in widths]
        ms = {name: [] for name, _ in settings}
        for r in range(a.rounds):
            for name, labels in settings:
                short, batch = run(data, labels, a.skip)
                long_, _ = run(data, labels, a.skip + a.steps)
                sps = a.steps / (long_ - short)
                ms[name].append(1000.0 / sps)
                print(f'round {r}  conditioning {name:6s}: {sps:7.3f} steps/s  ({1000.0 / sps:6.2f} ms per step of {batch} volumes; '
                      f'{a.steps} steps, runs of {a.skip} and {a.skip + a.steps} steps took {short:.2f} s and {long_:.2f} s)', flush=True)
        for name, v in ms.items():
            print(f'{name:6s}: mean {np.mean(v):6.2f} ms per step, spread over {len(v)} rounds {max(v) - min(v):5.2f} ms', flush=True)
