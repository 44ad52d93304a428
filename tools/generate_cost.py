"""profiles/generate_cost.txt: (a) the rate of sg_store_volumes (csrc/export.hip) on 16 volumes of 32x128x128 and on 2 volumes of
128x512x512, bf16 -> i16 and f32 -> i16, with and without statistics, beside sg_gather_rows (its mirror: i16 rows -> f32) over the
same elements and the project's memory-bound yardstick, sg_axpby (out = wa * a, bf16), over the same bytes; (b) volumes per
second and the time split of python -m saragan_amd.generate against generate_minimal on one checkpoint at the benchmarked phase
(bench.py configuration 3: size s, phase 6, 32x128x128, bf16).  Device events around windows of warmed-up launches, variants
alternating; a rate is bytes read plus bytes written over the median window time per launch.

    python tools/generate_cost.py [OUTPUT.txt] [--samples N] [--batch B]"""
import argparse
import io
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from saragan_amd import functional as F                                  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('output', nargs='?', default=os.path.join(ROOT, 'profiles', 'generate_cost.txt'))
ap.add_argument('--samples', type=int, default=384)
ap.add_argument('--batch', type=int, default=8)
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


say(f'device {torch.cuda.get_device_name(0)}; {WINDOWS} windows per variant, variants alternating; rate = bytes / median time')
g = torch.Generator(device='cuda').manual_seed(11)
for n, d, h, w, launches in ((16, 32, 128, 128, 200), (2, 128, 512, 512, 50)):
    elems = n * d * h * w
    x32 = torch.randn((n, 1, d, h, w), device='cuda', generator=g) * 1.2
    x16 = x32.to(torch.bfloat16)
    y = torch.empty((n, 1, d, h, w), device='cuda', dtype=torch.int16)
    kw = dict(scale=1024.0, shift=0.0, clip=(-1024, 2048), out=y)
    table = y.view(n, -1)
    idx = torch.arange(n, device='cuda', dtype=torch.int32)
    rows = torch.empty((n, d * h * w), device='cuda', dtype=torch.float32)
    variants = [('sg_store_volumes bf16 -> i16', lambda: F.store_volumes(x16, torch.int16, **kw), 4 * elems),
                ('sg_store_volumes bf16 -> i16 + statistics', lambda: F.store_volumes(x16, torch.int16, stats=True, **kw), 4 * elems),
                ('sg_store_volumes f32 -> i16', lambda: F.store_volumes(x32, torch.int16, **kw), 6 * elems),
                ('sg_store_volumes f32 -> i16 + statistics', lambda: F.store_volumes(x32, torch.int16, stats=True, **kw), 6 * elems),
                ('sg_gather_rows i16 -> f32, same elements', lambda: F.gather_rows(table, idx, 0.0, 1024.0, out=rows), 6 * elems)]
    for name, nbytes in (('the bf16 -> i16 bytes', 4 * elems), ('the f32 -> i16 bytes', 6 * elems)):
        a = torch.randn((1, nbytes // 4), device='cuda', generator=g).to(torch.bfloat16)      # read 2 + write 2 bytes per element
        variants.append((f'sg_axpby over {name}', lambda a=a: F.lerp(a, None, 0.5, 0.0), nbytes))
    times = {v[0]: [] for v in variants}
    for _, fn, _ in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for name, fn, _ in variants:
            times[name].append(window(fn, launches))
    say(f'--- {n} volumes of {d}x{h}x{w} ({elems / 1e6:.1f} M voxels), {launches} launches per window')
    for name, _, nbytes in variants:
        med, mn, mx = (float(f(times[name])) for f in (np.median, np.min, np.max))
        say(f'{name}: median {med * 1e3:.1f} us (min {mn * 1e3:.1f}, max {mx * 1e3:.1f}) per launch, {nbytes / 1e6:.2f} MB, '
            f'{nbytes / med / 1e9:.3f} TB/s')
    del x32, x16, y, table, rows, variants
    torch.cuda.empty_cache()

# ---- end to end at the benchmarked phase: one checkpoint, both tools
from benchlib.launch import CONFIGS                                      # noqa: E402
from saragan_amd import generate, generate_minimal                       # noqa: E402
from saragan_amd.generation import RestoredGenerator                     # noqa: E402
from saragan_amd.utils import save_checkpoint                            # noqa: E402

c = CONFIGS[3]
work = tempfile.mkdtemp(prefix='generate_cost_')
try:
    base = ['pgan', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 128, 512, 512)', '--network_size', c['size'], '--latent_dim',
            str(c['latent']), '--phase', str(c['phase']), '--dtype', c['dtype'], '--batch_size', str(opts.batch), '--num_samples',
            str(opts.samples), '--data_mean', '1024', '--data_stddev', '1024', '--model_path', os.path.join(work, 'model')]
    args = generate.build_parser().parse_args(base)
    net = RestoredGenerator(args, 'cuda')
    net(torch.zeros(opts.batch, c['latent'], device='cuda'))              # freshly drawn variables are the checkpoint
    save_checkpoint(net.store, args.model_path)
    del net
    torch.cuda.empty_cache()
    say(f'--- end to end at bench.py configuration 3 (size {c["size"]}, phase {c["phase"]}, 32x128x128, {c["dtype"]}): '
        f'{opts.samples} samples in batches of {opts.batch}, files in a temporary directory')
    for label, more in (('generate --out_dtype uint16', []), ('generate --out_dtype uint16 --writers 1 --inflight 1', ['--writers', '1', '--inflight', '1']),
                        ('generate --out_dtype float32', ['--out_dtype', 'float32'])):
        target = os.path.join(work, label.replace(' ', '_'))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = generate.run(generate.build_parser().parse_args(base + ['--output_dir', target] + more), out=io.StringIO())
        wall = time.perf_counter() - t0
        s = m['seconds']
        writers = 1 if '--writers' in more else 4
        stages = {'generation': s['generation'], 'store': s['store'], 'download': s['download'], f'save / {writers} writers': s['save'] / writers}
        bound = max(stages, key=stages.get)
        say(f'{label}: {opts.samples / wall:.1f} volumes/s ({wall:.2f} s with the restore); device seconds: generation '
            f'{s["generation"]:.3f}, store {s["store"]:.3f}, download {s["download"]:.3f}; save {s["save"]:.3f} s summed over the writer '
            f'threads; the longest stage: {bound} ({stages[bound]:.3f} s), the rest of the wall time is the restore and host work between launches')
        shutil.rmtree(target)
    target = os.path.join(work, 'minimal')
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with open(os.devnull, 'w') as null:
        stdout, sys.stdout = sys.stdout, null
        try:
            generate_minimal.main(generate_minimal.build_parser().parse_args(base + ['--output_dir', target]))
        finally:
            sys.stdout = stdout
    wall = time.perf_counter() - t0
    say(f'generate_minimal (float32, one file, every sample in host memory): {opts.samples / wall:.1f} volumes/s ({wall:.2f} s with the restore)')
finally:
    shutil.rmtree(work, ignore_errors=True)
out.close()
