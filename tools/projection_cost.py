"""profiles/projection_cost.txt: (a) the time and the rate of sg_multiscale_residual (csrc/project.hip: the pass and its finishing
launch) at [32, 1, 32, 128, 128], bf16 y, int16 targets, levels 1 and 4, beside the same loss and gradient composed from
gather_rows and torch ops (avg_pool3d, autograd) and the project's memory-bound yardstick, sg_axpby (out = wa * a, bf16), over the
same bytes; sg_latent_step at [32, 512]; (b) seconds per iteration of the projection loop at the benchmarked phase (bench.py
configuration 3: size s, phase 6, 32x128x128, bf16) with the fused loss against the same loop with the composed loss.  Device events
around windows of warmed-up launches, variants alternating; a rate is (y read + target read + grad written) over the median time.

    python tools/projection_cost.py [OUTPUT.txt] [--batch B] [--iterations K]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from saragan_amd import functional as F                                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('output', nargs='?', default=os.path.join(ROOT, 'profiles', 'projection_cost.txt'))
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--iterations', type=int, default=20)
opts = ap.parse_args()
out = open(opts.output, 'w')
WINDOWS = 5


def say(s):
    print(s, flush=True)
    out.write(s + '\n')
    out.flush()


def window(fn, launches):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def composed(y, table, idx, mean, stddev, levels, lam):
    """The same loss and d loss / d y from gather_rows and torch ops: (loss [n], grad like y)."""
    yy = y.detach().requires_grad_(True)
    r = yy.float() - F.gather_rows(table, idx, mean, stddev)
    total = 0
    for l in range(levels):
        m = torch.nn.functional.avg_pool3d(r, 2 ** l) if l else r
        total = total + lam[l] * (m * m).flatten(1).mean(dim=1)
    g, = torch.autograd.grad(total.sum(), yy)
    return total.detach(), g


def measure(variants, launches):
    times = {v[0]: [] for v in variants}
    for _, fn, _ in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for name, fn, _ in variants:
            times[name].append(window(fn, launches))
    for name, _, nbytes in variants:
        med, mn, mx = (float(f(times[name])) for f in (np.median, np.min, np.max))
        rate = f', {nbytes / 1e6:.2f} MB, {nbytes / med / 1e9:.3f} TB/s' if nbytes else ''
        say(f'{name}: median {med * 1e3:.1f} us (min {mn * 1e3:.1f}, max {mx * 1e3:.1f}) per call{rate}')


say(f'device {torch.cuda.get_device_name(0)}; {WINDOWS} windows per variant, variants alternating; rate = (y + target + grad bytes) / median time; '
    f'the HBM roof of the MI355X is 8 TB/s, sg_axpby is what a plain pass reaches')
g = torch.Generator(device='cuda').manual_seed(11)
n, d, h, w = 32, 32, 128, 128
elems = n * d * h * w
y = (torch.randn((n, 1, d, h, w), device='cuda', generator=g) * 1.2).to(torch.bfloat16)
table = torch.randint(-1024, 3072, (n, 1, d, h, w), device='cuda', generator=g, dtype=torch.int32).to(torch.int16)
idx = torch.arange(n, device='cuda', dtype=torch.int32)
grad = torch.empty_like(y)
a = torch.randn((1, 6 * elems // 4), device='cuda', generator=g).to(torch.bfloat16)      # reads 2 + writes 2 bytes per element
variants = []
for levels in (1, 4):
    lam = [1.0] * levels
    variants.append((f'sg_multiscale_residual levels {levels} (pass + finish)',
                     lambda levels=levels, lam=lam: F.multiscale_residual_raw(y, table, idx, 1024.0, 1024.0, levels, lam, out=grad), 6 * elems))
    variants.append((f'gather_rows + torch ops + autograd, levels {levels}',
                     lambda levels=levels, lam=lam: composed(y, table, idx, 1024.0, 1024.0, levels, lam), 6 * elems))
variants.append(('sg_axpby over the same bytes', lambda: F.lerp(a, None, 0.5, 0.0), 6 * elems))
say(f'--- {n} volumes of {d}x{h}x{w} ({elems / 1e6:.1f} M voxels), bf16 y, int16 targets, 50 calls per window')
measure(variants, 50)
L = 512
z, m_, v_, gz = (torch.randn(n, L, device='cuda', generator=g) for _ in range(4))
v_.abs_()
loss, best = torch.rand(n, device='cuda', generator=g), torch.full((n,), 0.5, device='cuda')
zb, bs = torch.zeros(n, L, device='cuda'), torch.zeros(n, dtype=torch.int32, device='cuda')
say(f'--- latents [{n}, {L}], 200 calls per window')
measure([('sg_latent_step', lambda: F.latent_step_(z, m_, v_, gz, loss, best, zb, bs, 0.01, 3), 0),
         ('sg_latent_step, sphere', lambda: F.latent_step_(z, m_, v_, gz, loss, best, zb, bs, 0.01, 3, sphere=True), 0)], 200)
del y, table, grad, a
torch.cuda.empty_cache()

# ---- the loop at the benchmarked phase
from benchlib.launch import CONFIGS                                      # noqa: E402
from saragan_amd import project                                          # noqa: E402
from saragan_amd.generation import RestoredGenerator                     # noqa: E402

c = CONFIGS[3]
B = opts.batch
base = ['pgan', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 128, 512, 512)', '--network_size', c['size'], '--latent_dim', str(c['latent']),
        '--phase', str(c['phase']), '--dtype', c['dtype'], '--batch_size', str(B), '--model_path', 'unused', 'unused_dir']
args = project.build_parser().parse_args(base)
net = RestoredGenerator(args, 'cuda')
net(torch.zeros(B, c['latent'], device='cuda'))              # freshly drawn variables stand for a checkpoint
project._grad_free(net.store)
shape = net(torch.zeros(B, c['latent'], device='cuda')).shape
table = torch.randint(0, 3072, tuple(shape), device='cuda', generator=g, dtype=torch.int32).to(torch.int16)
idx = torch.arange(B, device='cuda', dtype=torch.int32)
lam = [1.0] * 3
state = dict(z=torch.randn(B, c['latent'], device='cuda', generator=g).requires_grad_(True), m=torch.zeros(B, c['latent'], device='cuda'),
             v=torch.zeros(B, c['latent'], device='cuda'), best=torch.full((B,), float('inf'), device='cuda'),
             zb=torch.zeros(B, c['latent'], device='cuda'), bs=torch.zeros(B, dtype=torch.int32, device='cuda'), step=0)


def iteration(fused):
    z = state['z']
    yv = net(z, None, grad=True)
    if fused:
        loss, _, gy = F.multiscale_residual_raw(yv.detach(), table, idx, 1024.0, 1024.0, 3, lam)
    else:
        loss, gy = composed(yv, table, idx, 1024.0, 1024.0, 3, lam)
    gz, = torch.autograd.grad(yv, z, gy)
    state['step'] += 1
    F.latent_step_(z.detach(), state['m'], state['v'], gz.float().contiguous(), loss.float(), state['best'], state['zb'], state['bs'], 0.01, state['step'])


say(f'--- the projection loop at bench.py configuration 3 (size {c["size"]}, phase {c["phase"]}, {tuple(shape[2:])}, {c["dtype"]}), batch {B}, '
    f'levels 3: forward, loss, backward to z, latent step; {opts.iterations} iterations per window')
measure([('iteration with sg_multiscale_residual', lambda: iteration(True), 0),
         ('iteration with the loss composed from gather_rows and torch ops', lambda: iteration(False), 0)], opts.iterations)
out.close()
