"""profiles/intensity_hist_cost.txt: the rate of sg_intensity_hist (csrc/hist.hip) on 512 volumes of 32x128x128 voxels -- f32
per volume, bf16 per volume, and f32 as ONE pooled row -- on three value patterns: uniform over the 4096 bins, N(0,1) mapped
into the 4096 bins, every voxel in one bin.  In the same process, alternating with it: a read-only pass over the same bytes
(torch.sum, the roof calibration) and the torch formulation of the histogram (mul, add, floor, clamp, bincount) on the f32
data.  Device events around windows of warmed-up launches; a rate is the input's bytes over the median window time per launch.
The kernel's counts are compared with the torch formulation's at the timed size.

    python tools/intensity_hist_cost.py [OUTPUT.txt]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from saragan_amd import functional as F                                  # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'intensity_hist_cost.txt'), 'w')
N, V, LO, HI = 512, 32 * 128 * 128, 0, 4096
SCALE, SHIFT = 512.0, 2048.0            # N(0,1) -> sigma = 512 bins about the middle; +-4 sigma fill the range
LAUNCHES, WINDOWS = 200, 5


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


def torch_hist(x):
    t = (x * SCALE + SHIFT).floor_().clamp_(LO, HI - 1).sub_(LO)
    return torch.bincount(t.flatten().long(), minlength=HI - LO)


say(f'device {torch.cuda.get_device_name(0)}; {N} x 32x128x128 voxels, {HI - LO} unit bins, scale {SCALE}, shift {SHIFT}; '
    f'{LAUNCHES} launches per window, {WINDOWS} windows per variant, variants alternating; rate = input bytes / median time')
g = torch.Generator(device='cuda').manual_seed(11)
patterns = (('uniform over the bins', lambda: (torch.rand((N, V), device='cuda', generator=g) - 0.5) * 7.99),
            ('N(0,1) into the bins', lambda: torch.randn((N, V), device='cuda', generator=g)),
            ('every voxel in one bin', lambda: torch.full((N, V), -1.5, device='cuda')))
for name, make in patterns:
    x32 = make()
    x16 = x32.to(torch.bfloat16)
    rows32 = torch.empty((N, HI - LO + 1), dtype=torch.int64, device='cuda')
    rows16 = torch.empty_like(rows32)
    pooled = torch.empty((1, HI - LO + 1), dtype=torch.int64, device='cuda')
    variants = (('sg_intensity_hist f32, 512 rows', lambda: F.intensity_hist(x32, LO, HI, SCALE, SHIFT, out=rows32), x32, LAUNCHES),
                ('sg_intensity_hist bf16, 512 rows', lambda: F.intensity_hist(x16, LO, HI, SCALE, SHIFT, out=rows16), x16, LAUNCHES),
                ('sg_intensity_hist f32, one pooled row', lambda: F.intensity_hist(x32, LO, HI, SCALE, SHIFT, pooled=True, out=pooled),
                 x32, LAUNCHES),
                ('read-only pass torch.sum f32', lambda: torch.sum(x32), x32, LAUNCHES),
                ('read-only pass torch.sum bf16', lambda: torch.sum(x16), x16, LAUNCHES),
                ('torch mul/add/floor/clamp/bincount f32', lambda: torch_hist(x32), x32, 10))
    times = {v[0]: [] for v in variants}
    for _, fn, _, _ in variants:
        fn()
        fn()
    torch.cuda.synchronize()
    for _ in range(WINDOWS):
        for vname, fn, _, launches in variants:
            times[vname].append(window(fn, launches))
    say(f'--- {name}')
    roof = {}
    for vname, _, src, _ in variants:
        nbytes = src.numel() * src.element_size()
        med, mn, mx = float(np.median(times[vname])), float(np.min(times[vname])), float(np.max(times[vname]))
        rate = nbytes / med / 1e9
        if vname.startswith('read-only'):
            roof[src.dtype] = rate
        say(f'{vname}: median {med:.3f} ms (min {mn:.3f}, max {mx:.3f}) per launch, {nbytes / 1e9:.3f} GB read, {rate:.3f} TB/s')
    for vname, _, src, _ in variants:
        if vname.startswith('sg_'):
            rate = src.numel() * src.element_size() / float(np.median(times[vname])) / 1e9
            say(f'{vname}: {100 * rate / roof[src.dtype]:.1f} % of the read-only pass over the same bytes')
    want = torch_hist(x32)
    same = bool(torch.equal(pooled[0, :-1], want)) and bool(torch.equal(rows32.sum(0), pooled[0])) and int(pooled[0, -1]) == 0
    same16 = bool(torch.equal(rows16.sum(0)[:-1], torch_hist(x16.float())))
    say(f'counts equal to the torch formulation at this size: f32 {same}, bf16 {same16}')
    del x32, x16, rows32, rows16, pooled, want
    torch.cuda.empty_cache()
out.close()
