"""profiles/preview_cost.txt: the rate of sg_render_view (csrc/render.hip), every axis x mode, on 16 volumes of 32x128x128 bf16
and on 2 volumes of 128x512x512 bf16, beside the project's memory-bound yardstick, sg_axpby (out = wa * a), over a bf16 tensor
of the same byte count -- and the wall time of one preview event (EMA weights in, 8 fixed latents generated, the default
three-view sheet rendered, copied and encoded, weights back) at the benchmarked phase (bench.py configuration 3).
Device events around windows of warmed-up launches, variants alternating; a rate is bytes over the median window time per
launch.  For a projection the bytes are the volumes read plus the canvas written; for a slice the planes read plus the canvas;
for sg_axpby the bytes read plus the bytes written.

    python tools/preview_cost.py [OUTPUT.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from saragan_amd import functional as F                                  # noqa: E402
from saragan_amd import preview                                          # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'preview_cost.txt'), 'w')
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
    x = torch.randn((n, d, h, w), device='cuda', generator=g).to(torch.bfloat16)
    vol_bytes = x.numel() * 2
    variants = []
    for axis, ax in enumerate('dhw'):
        for mode in ('slice', 'max', 'mean'):
            rows, cols = ((h, w), (d, w), (d, h))[axis]
            canvas = torch.zeros((rows, n * cols), dtype=torch.uint8, device='cuda')
            nbytes = canvas.numel() + (vol_bytes // (d, h, w)[axis] if mode == 'slice' else vol_bytes)
            variants.append((f'{mode}_{ax}', (lambda axis=axis, mode=mode, canvas=canvas:
                                              F.render_view(x, axis, mode, window=(-1.0, 2.0), canvas=canvas)), nbytes))
    a = torch.randn((1, vol_bytes // 2), device='cuda', generator=g).to(torch.bfloat16)
    variants.append(('sg_axpby over the volumes\' bytes', lambda: F.lerp(a, None, 0.5, 0.0), 2 * vol_bytes))
    small = a[:, :vol_bytes // 2 // d].contiguous()
    variants.append(('sg_axpby over one plane per volume', lambda: F.lerp(small, None, 0.5, 0.0), 2 * small.numel() * 2))
    times = {v[0]: [] for v in variants}
    for _, fn, _ in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for name, fn, _ in variants:
            times[name].append(window(fn, launches))
    say(f'--- {n} volumes of {d}x{h}x{w} bf16 ({vol_bytes / 1e6:.1f} MB), {launches} launches per window')
    for name, _, nbytes in variants:
        med, mn, mx = (float(f(times[name])) for f in (np.median, np.min, np.max))
        say(f'{name}: median {med * 1e3:.1f} us (min {mn * 1e3:.1f}, max {mx * 1e3:.1f}) per launch, {nbytes / 1e6:.2f} MB, '
            f'{nbytes / med / 1e9:.3f} TB/s')
    del x, a, small, variants
    torch.cuda.empty_cache()

# ---- one preview event at the benchmarked phase
from benchlib import workload                                            # noqa: E402
from benchlib.launch import CONFIGS                                      # noqa: E402
cfg_args = argparse.Namespace(loss='wgan', **CONFIGS[3])
cfg = workload.build(cfg_args, torch.device('cuda'), cfg_args.dtype)
graph, sess = cfg['graph'], cfg['sess']
ema = graph.ema
z = torch.randn(8, cfg_args.latent, device='cuda', generator=g)
path = os.path.join(os.environ.get('TMPDIR', '/tmp'), 'preview_cost.png')


def event():
    sess.run(ema.assign_ema_weights())
    chunks = [graph.generate(z)]
    img = preview.sheet(chunks, preview.DEFAULT_VIEWS, (-1.0, 2.0))
    sess.run(ema.restore_original_weights())
    preview.write_png(path, img)
    return img


def parts():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = graph.generate(z)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    img = preview.sheet(s, preview.DEFAULT_VIEWS, (-1.0, 2.0))
    t2 = time.perf_counter()
    data = preview.png_bytes(img)
    t3 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t2) * 1e3, len(data), img.shape


event()
walls = []
for _ in range(5):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    event()
    torch.cuda.synchronize()
    walls.append((time.perf_counter() - t0) * 1e3)
gen_ms, sheet_ms, png_ms, nbytes, shape = parts()
say(f'--- one preview event at bench.py configuration 3 (size {cfg_args.size}, phase {cfg_args.phase}, '
    f'{tuple(cfg["shape"][2:])} volumes, bf16): 8 latents, views {preview.DEFAULT_VIEWS}')
say(f'wall time per event, 5 events after one warm-up: median {np.median(walls):.1f} ms (min {min(walls):.1f}, max {max(walls):.1f})')
say(f'of which, measured apart: generation {gen_ms:.1f} ms, three launches + canvas copy {sheet_ms:.2f} ms, PNG encoding '
    f'{png_ms:.1f} ms ({shape[1]} x {shape[0]} pixels, {nbytes} bytes); the rest is the two weight swaps and the repacking of '
    f'the weight images they invalidate')
out.close()
