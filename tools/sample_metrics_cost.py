"""Part (a) and (c) of profiles/sample_metrics_cost.txt: sg_pairwise_sqdist (symmetric) against the same product through torch in
f32 on the same random data at M = 512 and M = 2048 rows of 32*128*128 voxels -- device events around warmed-up calls, the
variants alternating in one process -- and the wall time of one get_sample_metrics(256 real, 256 fake) next to
get_swd_for_volumes on the same samples.  Per-kernel times and fetched bytes (part (b)) come from rocprofv3 runs of
tools/sample_metrics_prof_target.py, each in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o pdist -- python tools/sample_metrics_prof_target.py
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -o pdist -- python tools/sample_metrics_prof_target.py

    python tools/sample_metrics_cost.py [OUTPUT.txt]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from saragan_amd import _lib                                             # noqa: E402
from saragan_amd.metrics import sample_metrics as SM                     # noqa: E402
from saragan_amd.metrics import swd as SWD                               # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, 'w')


def say(s):
    print(s, flush=True)
    out.write(s + '\n')
    out.flush()


def ev_time(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


V = 32 * 128 * 128
say(f'device {torch.cuda.get_device_name(0)}; chunk C = {_lib.load().sg_pairwise_sqdist_chunk()}; v = {V}')
for M in (512, 2048):
    need = M * V * 4 * 1.2 + 2 * M * M * 8
    if torch.cuda.mem_get_info()[0] < need + 2 ** 30:
        say(f'M = {M}: skipped, {torch.cuda.mem_get_info()[0]} bytes free')
        continue
    g = torch.Generator(device='cuda').manual_seed(3)
    Z = torch.randn((M, V), device='cuda', generator=g)
    ws_bytes = _lib.load().sg_pairwise_sqdist_workspace(M, M, V)
    hand = lambda: SM.pairwise_sqdist(Z)

    def gram():
        G = Z @ Z.t()
        n = (Z * Z).sum(1)
        return (n[:, None] + n[None, :] - 2 * G).clamp_(min=0)
    mm = lambda: Z @ Z.t()
    for f in (hand, gram, mm):
        f()
        f()
    torch.cuda.synchronize()
    th, tg, tm = [], [], []
    for _ in range(4):                      # interleaved rounds in one process
        th += ev_time(hand, 3)
        tg += ev_time(gram, 3)
        tm += ev_time(mm, 3)
    D = hand()
    G = gram().double()
    rel = float(((D - G).abs() / (D.abs() + 1e-30))[~torch.eye(M, dtype=torch.bool, device='cuda')].max())
    flop_sym, flop_full = M * M * V * 2 / 2, M * M * V * 2
    for name, ts, fl in (('sg_pairwise_sqdist symmetric (3 kernels + workspace alloc)', th, flop_sym),
                         ('torch f32 Gram form (matmul + norms + combine)', tg, flop_full),
                         ('torch.matmul f32 Z @ Z.T alone', tm, flop_full)):
        med, mn = float(np.median(ts)), float(np.min(ts))
        say(f'M = {M}: {name}: median {med:.3f} ms, min {mn:.3f} ms over {len(ts)}; {fl / med / 1e9:.1f} TFLOP/s counted '
            f'({"ma*mb*v*2/2" if fl == flop_sym else "ma*mb*v*2"}), {100 * fl / med / 1e9 / 157.3:.1f} % of the 157.3 TFLOP/s f32-MFMA peak')
    say(f'M = {M}: compulsory bytes M*v*4 = {M * V * 4 / 1e9:.3f} GB, workspace {ws_bytes / 1e6:.1f} MB; '
        f'max relative difference hand (f64 across chunks) vs torch f32 Gram form, off-diagonal: {rel:.3e}')
    del Z, D, G
    torch.cuda.empty_cache()

# one get_sample_metrics(256 real, 256 fake) next to SWD on the same samples
g = torch.Generator(device='cuda').manual_seed(4)
real = torch.randn((256, 1, 32, 128, 128), device='cuda', generator=g)
fake = 0.9 * torch.randn((256, 1, 32, 128, 128), device='cuda', generator=g) + 0.1


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


SM.get_sample_metrics(real, fake)
np.random.seed(0)
SWD.get_swd_for_volumes(real, fake)
t_sm, t_swd = [], []
for _ in range(3):
    t_sm += wall(lambda: SM.get_sample_metrics(real, fake), 2)
    t_swd += wall(lambda: SWD.get_swd_for_volumes(real, fake), 1)
m = SM.get_sample_metrics(real, fake)
say(f'get_sample_metrics(256 real, 256 fake of 1x32x128x128), wall incl. the host reductions: median {np.median(t_sm):.2f} ms, '
    f'min {np.min(t_sm):.2f} ms over {len(t_sm)}')
say(f'get_swd_for_volumes on the same samples, wall: median {np.median(t_swd):.2f} ms, min {np.min(t_swd):.2f} ms over {len(t_swd)}')
say(f'values on that synthetic pair: {m}')
out.close()
