"""profiles/prepare_data_cost.txt: the rate of sg_block_pyramid (csrc/pyramid.hip) on 4 volumes of 160x512x512 int16 and on 16 of
32x128x128, six levels, uint16 out, with and without the statistics, beside the project's memory-bound yardstick, sg_axpby
(out = wa * a), over a bf16 tensor of the same byte count -- and the wall time per volume of python -m saragan_amd.prepare_data
on the large volumes, split into load, upload, kernel, download and save, on the device and on its numpy path (--device cpu).
Device events around windows of warmed-up launches, variants alternating; a rate is bytes over the median window time per
launch.  The pyramid's bytes are the volumes read plus every level written (8/7 of level 0); sg_axpby's the bytes read plus the
bytes written.

    python tools/pyramid_rate.py [OUTPUT.txt] [--bench LABEL=FILE ...]      (FILE: the JSON line of a bench.py run)"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from saragan_amd import functional as F                                  # noqa: E402
from saragan_amd import prepare_data                                     # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('output', nargs='?', default=os.path.join(ROOT, 'profiles', 'prepare_data_cost.txt'))
ap.add_argument('--bench', action='append', default=[])
ap.add_argument('--tool_volumes', type=int, default=4)
args = ap.parse_args()
out = open(args.output, 'w')
WINDOWS = 5
LEVELS = 6


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
for n, d, h, w, launches in ((4, 160, 512, 512, 20), (16, 32, 128, 128, 200)):
    x = torch.randint(-1024, 3072, (n, d, h, w), device='cuda', generator=g, dtype=torch.int16)
    src_bytes = x.numel() * 2
    nbytes = src_bytes + sum((x.numel() >> (3 * i)) * 2 for i in range(LEVELS))
    kw = dict(intercept=-1024, clip=(0, 4095), out_dtype=torch.uint16)
    variants = [('block_pyramid, mean, statistics', lambda: F.block_pyramid(x, (d, h, w), LEVELS, stats=True, **kw), nbytes),
                ('block_pyramid, mean', lambda: F.block_pyramid(x, (d, h, w), LEVELS, **kw), nbytes),
                ('block_pyramid, max', lambda: F.block_pyramid(x, (d, h, w), LEVELS, reduce='max', **kw), nbytes),
                ('block_pyramid, mean, level 0 only', lambda: F.block_pyramid(x, (d, h, w), 1, **kw), 2 * src_bytes)]
    a = torch.randn((1, nbytes // 4), device='cuda', generator=g).to(torch.bfloat16)
    variants.append(('sg_axpby over the same bytes', lambda: F.lerp(a, None, 0.5, 0.0), 2 * a.numel() * 2))
    times = {v[0]: [] for v in variants}
    for _, fn, _ in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for name, fn, _ in variants:
            times[name].append(window(fn, launches))
    say(f'--- {n} volumes of {d}x{h}x{w} int16 ({src_bytes / 1e6:.1f} MB), {LEVELS} levels, {launches} launches per window')
    for name, _, nb in variants:
        med, mn, mx = (float(f(times[name])) for f in (np.median, np.min, np.max))
        say(f'{name}: median {med * 1e3:.1f} us (min {mn * 1e3:.1f}, max {mx * 1e3:.1f}) per launch, {nb / 1e6:.2f} MB, '
            f'{nb / med / 1e9:.3f} TB/s')
    del x, a, variants
    torch.cuda.empty_cache()

# ---- the tool, end to end
work = tempfile.mkdtemp(prefix='pyramid_rate_')
try:
    src = os.path.join(work, 'src')
    os.makedirs(src)
    rng = np.random.default_rng(5)
    for k in range(args.tool_volumes):
        np.save(os.path.join(src, f'scan{k:02d}.npy'), rng.integers(-1024, 3072, (160, 512, 512)).astype(np.int16))
    say(f'--- python -m saragan_amd.prepare_data on {args.tool_volumes} volumes of 160x512x512 int16, --final_shape 160,512,512 '
        f'--levels {LEVELS} --intercept=-1024 --clip=0,4095, source and destination in the temporary directory; seconds per volume')
    for device, batch in (('cuda', 4), ('cuda', 4), ('cpu', 1)):
        dst = os.path.join(work, 'dst_' + device)
        a = prepare_data.parse_args([src, dst, '--final_shape', '160,512,512', '--levels', str(LEVELS), '--intercept=-1024',
                                     '--clip=0,4095', '--batch', str(batch), '--device', device, '--overwrite'])
        _, spent = prepare_data.run(a, out=open(os.devnull, 'w'))
        per = {k: v / args.tool_volumes for k, v in spent.items()}
        say(f'--device {device} --batch {batch}: ' + ', '.join(f'{k} {v:.3f}' for k, v in per.items())
            + f', total {sum(per.values()):.3f}')
    same = all(open(os.path.join(dp, f), 'rb').read() == open(os.path.join(dp.replace('dst_cuda', 'dst_cpu'), f), 'rb').read()
               for dp, _, fs in os.walk(os.path.join(work, 'dst_cuda')) for f in fs)
    say(f'(the first device run includes the first launch; the two trees are byte-identical, stats.json included: {same})')
finally:
    shutil.rmtree(work, ignore_errors=True)

for item in args.bench:
    label, _, path = item.partition('=')
    line = [ln for ln in open(path).read().splitlines() if ln.startswith('{')][-1]
    r = json.loads(line)
    say(f'bench.py --gpus 1 --steps 20 --warmup 5, {label}: {r["value"]} {r["unit"]} ({r["ms_per_step"]} ms/step)')
out.close()
