"""Steps per second of a short training run with --d_mbstd_group off and on, in one process on one GPU: the benchmarked
configuration's last phase (pgan 's', phase 6, [32, 1, 32, 128, 128] per step, bf16, wgan, simultaneous) through train.run_training
on synthetic LIDC-shaped volumes.  Each setting runs `--rounds` times, alternating; the first `--skip` steps of a run (lazy
initialisation, the capture decision) are left out of its figure by timing a second, longer run against a shorter one.
Part (a) of profiles/mbstd_cost.txt is this tool's output.

    python tools/mbstd_cost.py [--steps 300] [--rounds 2] [--group 4]"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_data(root, phases):
    from benchlib.workload import synthetic_volume
    for ph in range(1, phases + 1):
        z, xy = 2 ** (ph - 1), 4 * 2 ** (ph - 1)
        d = os.path.join(root, f'{xy}x{xy}')
        os.makedirs(d)
        for i in range(36):
            np.save(os.path.join(d, f'{i:04d}.npy'), synthetic_volume((z, xy, xy), i))


def run(data, group, steps):
    import torch
    from saragan_amd.main import build_parser, finalize_args
    from saragan_amd.train import run_training
    argv = ['pgan', data + '/', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 64, 256, 256)', '--starting_phase', '6',
            '--ending_phase', '6', '--base_batch_size', '1024', '--latent_dim', '512', '--network_size', 's', '--noise_stddev',
            '0.01', '--mixing_nimg', '0', '--stabilizing_nimg', str(1 << 24), '--loss_fn', 'wgan', '--gp_weight', '10',
            '--data_mean', '1024', '--data_stddev', '1024', '--starting_alpha', '0', '--checkpoint_every_nsteps', str(1 << 30),
            '--validation_fraction', '0', '--test_fraction', '0', '--d_mbstd_group', str(group)]
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
    ap.add_argument('--group', type=int, default=4)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as data:
        make_data(data, 6)
        for r in range(a.rounds):
            for group in (0, a.group):
                short, batch = run(data, group, a.skip)
                long_, _ = run(data, group, a.skip + a.steps)
                sps = a.steps / (long_ - short)
                print(f'round {r}  --d_mbstd_group {group}: {sps:7.3f} steps/s  ({1000.0 / sps:6.2f} ms per step of {batch} volumes; '
                      f'{a.steps} steps, runs of {a.skip} and {a.skip + a.steps} steps took {short:.2f} s and {long_:.2f} s)', flush=True)
