"""profiles/resample_cost.txt: the rate of sg_resample_axes (csrc/resample.hip) on 4 volumes of 160x512x512 int16 and on 16 of
32x128x128, resampled from a slice spacing of 1.25 mm to 3.0 mm (the d axis at step 2.4, h and w at step 1), linear and antialias,
and with all three axes resampled (0.7 mm to 1.0 mm in the plane), beside the project's memory-bound yardstick, sg_axpby (out = wa *
a), over a bf16 tensor of the same byte count -- and the wall time per volume of python -m saragan_amd.prepare_data --spacing on
the large volumes, on the device and on its numpy path (--device cpu).
Device events around windows of warmed-up launches, variants alternating; a rate is bytes over the median window time per launch.
The resampler's bytes are the algorithmic ones: the source read once plus the output written once.  The launches are timed with
their tap tables already on the device (table_ops.resample_launch); functional.resample_volume, which builds and uploads them on
every call, is timed beside them.

    python tools/resample_rate.py [OUTPUT.txt] [--bench LABEL=FILE ...]      (FILE: the JSON line of a bench.py run)"""
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
from saragan_amd import prepare_data, table_ops                          # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('output', nargs='?', default=os.path.join(ROOT, 'profiles', 'resample_cost.txt'))
ap.add_argument('--bench', action='append', default=[])
ap.add_argument('--tool_volumes', type=int, default=4)
args = ap.parse_args()
out = open(args.output, 'w')
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


def prepared(x, out_shape, step, start, mode):
    """A launch with its tables built and uploaded once."""
    taps = [table_ops.resample_taps(s, o, st, s0, mode) for s, o, st, s0 in zip(x.shape[1:], out_shape, step, start)]
    packed = [torch.from_numpy(table_ops._pack_taps(t)).cuda() for t in taps]
    counts = [t[1].shape[1] for t in taps]
    return lambda: table_ops.resample_launch(x, packed, counts, out_shape, -1024, torch.int16), counts


say(f'device {torch.cuda.get_device_name(0)}; {WINDOWS} windows per variant, variants alternating; rate = bytes / median time')
g = torch.Generator(device='cuda').manual_seed(11)
for n, d, h, w, launches in ((4, 160, 512, 512, 20), (16, 32, 128, 128, 200)):
    x = torch.randint(-1024, 3072, (n, d, h, w), device='cuda', generator=g, dtype=torch.int16)
    src_bytes = x.numel() * 2
    od = int(np.ceil(d * 1.25 / 3.0))
    slices = ((od, h, w), (2.4, 1.0, 1.0), (0.0, 0.0, 0.0))
    plane = (int(np.ceil(h * 0.7)), int(np.ceil(w * 0.7)))
    every = ((od,) + plane, (2.4, 1.0 / 0.7, 1.0 / 0.7), (0.0, 0.0, 0.0))
    variants, biggest = [], 0
    for label, (shape, step, start), mode in (('slices 1.25 -> 3.0, linear', slices, 'linear'), ('slices 1.25 -> 3.0, antialias', slices, 'antialias'),
                                              ('all axes (0.7 -> 1.0 in the plane), linear', every, 'linear'),
                                              ('all axes (0.7 -> 1.0 in the plane), antialias', every, 'antialias')):
        fn, counts = prepared(x, shape, step, start, mode)
        nb = src_bytes + n * shape[0] * shape[1] * shape[2] * 2
        biggest = max(biggest, nb)
        variants.append((f'sg_resample_axes, {label}, taps {counts}', fn, nb))
    variants.append(('resample_volume (tables built and uploaded per call), slices, linear',
                     lambda: F.resample_volume(x, slices[0], slices[1], slices[2], fill=-1024), src_bytes + n * od * h * w * 2))
    a = torch.randn((1, biggest // 4), device='cuda', generator=g).to(torch.bfloat16)
    variants.append(('sg_axpby over the bytes of the largest variant', lambda: F.lerp(a, None, 0.5, 0.0), 2 * a.numel() * 2))
    times = {v[0]: [] for v in variants}
    for _, fn, _ in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for name, fn, _ in variants:
            times[name].append(window(fn, launches))
    say(f'--- {n} volumes of {d}x{h}x{w} int16 ({src_bytes / 1e6:.1f} MB) to int16, {launches} launches per window')
    for name, _, nb in variants:
        med, mn, mx = (float(f(times[name])) for f in (np.median, np.min, np.max))
        say(f'{name}: median {med * 1e3:.1f} us (min {mn * 1e3:.1f}, max {mx * 1e3:.1f}) per launch, {nb / 1e6:.2f} MB, '
            f'{nb / med / 1e9:.3f} TB/s')
    del x, a, variants
    torch.cuda.empty_cache()

# ---- the tool, end to end
work = tempfile.mkdtemp(prefix='resample_rate_')
try:
    src = os.path.join(work, 'src')
    os.makedirs(src)
    rng = np.random.default_rng(5)
    for k in range(args.tool_volumes):
        np.save(os.path.join(src, f'scan{k:02d}.npy'), rng.integers(-1024, 3072, (160, 512, 512)).astype(np.int16))
    say(f'--- python -m saragan_amd.prepare_data on {args.tool_volumes} volumes of 160x512x512 int16, --src_spacing 1.25,1,1 --spacing 3,1,1 '
        f'--final_shape 64,512,512 --levels 6 --intercept=-1024 --clip=0,4095, source and destination in the temporary directory; '
        f'seconds per volume')
    for device, batch in (('cuda', 4), ('cuda', 4), ('cpu', 1)):
        dst = os.path.join(work, 'dst_' + device)
        a = prepare_data.parse_args([src, dst, '--final_shape', '64,512,512', '--levels', '6', '--intercept=-1024', '--clip=0,4095',
                                     '--src_spacing', '1.25,1,1', '--spacing', '3,1,1', '--batch', str(batch), '--device', device,
                                     '--overwrite'])
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
