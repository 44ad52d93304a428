"""profiles/power_spectrum_cost.txt: the rate of sg_power_spectrum (csrc/spectrum.hip) on 512 volumes of 32x128x128 voxels, f32
and int16, against (a) the bare v_mfma_f64_16x16x4_f64 ceiling of the same board in the same session (tools/probe/mfma_ceiling
with the argument f64, a child process), (b) the same statistic composed from torch: torch.fft.rfftn on f64, abs()**2,
index_add_ -- with its peak memory -- or, where this torch has no working FFT on the device, the numpy twin on the CPU, and
(c) the cost inside an evaluation: one SpectrumAccumulator.add of 16 real and 16 generated volumes next to SWD on the same
samples.  Device events around windows of warmed-up launches, variants alternating in one process; algorithmic work is
D H Wf (4 W + 8 H + 8 D) flop per volume.

    python tools/spectrum_cost.py [OUTPUT.txt]"""
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from saragan_amd import table_ops as T                                   # noqa: E402
from saragan_amd.metrics import spectrum_metrics as SPM                  # noqa: E402
from saragan_amd.metrics import swd as SWD                               # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'power_spectrum_cost.txt'), 'w')
N, SHAPE = 512, (32, 128, 128)
D, H, W = SHAPE
WF = W // 2 + 1
FLOP = D * H * WF * (4 * W + 8 * H + 8 * D)
LAUNCHES, WINDOWS = 3, 5


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


say(f'device {torch.cuda.get_device_name(0)}; {N} x {D}x{H}x{W} voxels, {max(SHAPE) // 2} radial columns; algorithmic work '
    f'{FLOP / 1e9:.3f} GFLOP per volume, {N * FLOP / 1e9:.1f} GFLOP in all; {LAUNCHES} calls per window, {WINDOWS} windows per '
    f'variant, variants alternating; times are medians per call over all {N} volumes')

# ---- (a) the bare f64 MFMA ceiling, a child process of its own
ceiling = None
probe = os.path.join(ROOT, 'tools', 'probe', 'mfma_ceiling')
if not os.path.exists(probe):
    subprocess.check_call(['hipcc', '--offload-arch=gfx950', '-O3', '-o', probe, probe + '.hip'])
res = subprocess.run([probe, '2', 'f64'], capture_output=True, text=True, timeout=120)
for line in res.stdout.splitlines():
    say('ceiling probe: ' + line)
    if line.startswith('SUSTAINED_PEAK_F64_16x16x4_TFLOPS'):
        ceiling = float(line.split()[1])
if ceiling is None:
    say(f'ceiling probe failed (rc {res.returncode}): {res.stderr[-300:]}')

# ---- (b) the kernel and the composed path
plan = T.SpectrumPlan(SHAPE)
g = torch.Generator(device='cuda').manual_seed(11)
x32 = torch.randn((N,) + SHAPE, device='cuda', generator=g) * 200.0 - 600.0
x16 = x32.round().clamp_(-32768, 32767).to(torch.int16)
col = torch.from_numpy(plan.columns().ravel()).cuda()
gw = torch.from_numpy(plan.g).cuda()
CHUNK = 32      # volumes per rfftn: the f64 spectrum of a chunk is 32 x 4.26 MB, the whole set's would be 2.2 GB


def composed(x):
    radial = torch.zeros((x.shape[0], plan.bins + 1), dtype=torch.float64, device='cuda')
    for i in range(0, x.shape[0], CHUNK):
        f = torch.fft.rfftn(x[i:i + CHUNK].to(torch.float64), dim=(1, 2, 3))
        p = (f.abs() ** 2 * gw).reshape(f.shape[0], -1)
        radial[i:i + CHUNK].index_add_(1, col, p)
    return radial


fft_ok = True
try:
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ref = composed(x32[:CHUNK])
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
except Exception as e:      # this build's torch may ship without a device FFT
    fft_ok = False
    say(f'torch.fft.rfftn on the device failed in this build ({type(e).__name__}: {str(e)[:120]}): the numpy twin on the CPU stands in')

variants = [('sg_power_spectrum f32', lambda: T.power_spectrum(x32, plan)), ('sg_power_spectrum int16', lambda: T.power_spectrum(x16, plan))]
if fft_ok:
    variants.append(('torch rfftn f64 + abs()**2 + index_add_ (radial only)', lambda: composed(x32)))
times = {v[0]: [] for v in variants}
for _, fn in variants:
    fn()
torch.cuda.synchronize()
for _ in range(WINDOWS):
    for name, fn in variants:
        times[name].append(window(fn, LAUNCHES))
for name, _ in variants:
    med, mn, mx = float(np.median(times[name])), float(np.min(times[name])), float(np.max(times[name]))
    rate = N * FLOP / med / 1e9
    say(f'{name}: median {med:.2f} ms (min {mn:.2f}, max {mx:.2f}), {rate:.2f} algorithmic TFLOP/s'
        + (f', {100 * rate / ceiling:.1f} % of the bare f64 MFMA ceiling of {ceiling:.2f} TFLOP/s' if ceiling and name.startswith('sg_') else ''))
if fft_ok:
    got = T.power_spectrum(x32[:CHUNK], plan)[0]
    rel = float(((got - ref).abs() / ref.abs().clamp_min(1e-300)).max())
    say(f'composed path: peak memory {peak / 2 ** 20:.1f} MiB above the input for a chunk of {CHUNK} volumes (the whole set at once: '
        f'{N * D * H * WF * 16 / 1e9:.2f} GB of f64 spectrum before the squares); largest relative difference of a radial column '
        f'against the kernel {rel:.3g}')
else:
    t0 = time.time()
    T.power_spectrum(x32[:8].cpu(), plan)
    say(f'numpy twin on the CPU: {(time.time() - t0) / 8 * 1e3:.1f} ms per volume ({N} volumes: {(time.time() - t0) / 8 * N:.1f} s)')
ws = int(T._lib.load().sg_power_spectrum_workspace(1, D, H, W))
say(f'workspace of the kernel: {ws / 2 ** 20:.2f} MiB per volume in flight (power_spectrum launches chunks under 512 MiB)')

# ---- (c) inside an evaluation: 16 real + 16 generated volumes, as save_metrics hands them over
real, fake = x32[:16, None].contiguous(), x32[16:32, None].contiguous()
acc = SPM.SpectrumAccumulator(SHAPE)
ev = {'SpectrumAccumulator.add (both sets, rows to the host)': lambda: acc.add(real, fake), 'SWD.get_swd_for_volumes': lambda: SWD.get_swd_for_volumes(real, fake)}
tv = {k: [] for k in ev}
for fn in ev.values():
    fn()
torch.cuda.synchronize()
for _ in range(WINDOWS):
    for name, fn in ev.items():
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        tv[name].append((time.time() - t0) * 1e3)
for name in ev:
    say(f'evaluation batch of 16 + 16 volumes, {name}: median {float(np.median(tv[name])):.2f} ms wall (min {min(tv[name]):.2f}, max {max(tv[name]):.2f})')
say('with --compute_power_spectrum off nothing is imported, allocated or launched: the cost without the flag is zero')
say('not measured: extents of 512 and 1024; the 2-D configuration; MFMA-busy counters of the passes; whether lsd and hf_excess track perceived quality on real CT')
out.close()
