"""profiles/memorisation_cost.txt: (a) sg_sqdist_exact on 512 x 512 int16 volumes of 32x128x128 against the path a user had
before for the same data, gather_rows to f32 plus sg_pairwise_sqdist -- device events around warmed-up calls, the variants
alternating in one process; the achieved int8 operation rate against the spec int8 peak and the bytes read; (b) the seconds per
stage of python -m saragan_amd.metrics.memorisation on a synthetic directory of 2000 training and 2000 generated volumes.

    python tools/memorisation_cost.py [OUTPUT.txt] [--files N]"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from saragan_amd import _lib                                             # noqa: E402
from saragan_amd import functional as F                                  # noqa: E402
from saragan_amd.metrics import memorisation                             # noqa: E402
from saragan_amd.metrics import sample_metrics as SM                     # noqa: E402

argv = [a for a in sys.argv[1:] if not a.startswith('--')]
N_FILES = int(sys.argv[sys.argv.index('--files') + 1]) if '--files' in sys.argv else 2000
if '--files' in sys.argv:
    argv = [a for a in argv if a != str(N_FILES)]
out = open(argv[0] if argv else os.devnull, 'w')
I8_PEAK = 5.0e15      # int8 MFMA, dense: twice the ~2.5 PF of bf16 (operations = 2 per multiply-add)


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


M, V = 512, 32 * 128 * 128
lib = _lib.load()
say(f'device {torch.cuda.get_device_name(0)}; i32 chunk = {lib.sg_sqdist_exact_chunk()} voxels; M = {M} x {M} rows of v = {V} int16')
g = torch.Generator(device='cuda').manual_seed(3)
q = torch.randint(-1024, 2048, (M, V), generator=g, device='cuda', dtype=torch.int32).to(torch.int16)
r = torch.randint(-1024, 2048, (M, V), generator=g, device='cuda', dtype=torch.int32).to(torch.int16)
idx = torch.arange(M, device='cuda', dtype=torch.int32)
variants = {
    'sg_sqdist_exact, q against r': lambda: F.sqdist_exact(q, r),
    'sg_sqdist_exact, q against itself (symmetric)': lambda: F.sqdist_exact(q),
    'gather_rows to f32 + sg_pairwise_sqdist, q against r': lambda: SM.pairwise_sqdist(F.gather_rows(q, idx), F.gather_rows(r, idx)),
    'gather_rows to f32 + sg_pairwise_sqdist, symmetric': lambda: SM.pairwise_sqdist(F.gather_rows(q, idx)),
    'sg_pairwise_sqdist alone on resident f32 rows, q against r': None,
}
qf, rf = F.gather_rows(q, idx), F.gather_rows(r, idx)
variants['sg_pairwise_sqdist alone on resident f32 rows, q against r'] = lambda: SM.pairwise_sqdist(qf, rf)
for f in variants.values():
    f()
    f()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for _ in range(3):      # interleaved rounds in one process
    for k, f in variants.items():
        times[k] += ev_time(f, 2)
exact, f64 = F.sqdist_exact(q, r), SM.pairwise_sqdist(qf, rf)
rel = float(((exact.double() - f64).abs() / exact.double()).max())
for k, ts in times.items():
    med, mn, mx = float(np.median(ts)), float(np.min(ts)), float(np.max(ts))
    line = f'{k}: median {med:.3f} ms (min {mn:.3f}, max {mx:.3f}) over {len(ts)}'
    if k.startswith('sg_sqdist_exact'):
        pairs = M * (M + 1) / 2 if 'symmetric' in k else M * M      # row pairs whose four byte products are formed (whole tiles on the diagonal count more)
        ops = pairs * V * 4 * 2
        line += (f'; {ops / med / 1e9:.1f} int8 TOP/s counted (pairs * v * 4 products * 2), {100 * ops / (med * 1e-3) / I8_PEAK:.1f} % of '
                 f'the ~5 POP/s spec int8 peak; compulsory bytes {(1 if "symmetric" in k else 2) * M * V * 2 / 1e9:.3f} GB')
    else:
        line += f'; f32 bytes behind the MFMAs {(1 if "symmetric" in k else 2) * M * V * 4 / 1e9:.3f} GB'
    say(line)
say(f'workspace: exact {lib.sg_sqdist_exact_workspace(M, M, V) / 1e6:.1f} MB, f32 path {lib.sg_pairwise_sqdist_workspace(M, M, V) / 1e6:.1f} MB; '
    f'largest relative difference of the f32 path from the exact integers on this data: {rel:.3e}')
del q, r, qf, rf, exact, f64
torch.cuda.empty_cache()

# (b) the tool end to end on a synthetic directory
with tempfile.TemporaryDirectory() as tmp:
    rng = np.random.default_rng(0)
    pool = rng.integers(-1024, 2048, size=V + 2 * N_FILES * 997, dtype=np.int16)
    t0 = time.perf_counter()
    for name, base in (('train', 0), ('fake', N_FILES)):
        os.makedirs(os.path.join(tmp, name))
        for i in range(N_FILES):
            at = (base + i) * 997
            np.save(os.path.join(tmp, name, f'{name}_{i:05d}.npy'), pool[at:at + V].reshape(32, 128, 128))
    np.save(os.path.join(tmp, 'fake', 'fake_00000.npy'), pool[5 * 997:5 * 997 + V].reshape(32, 128, 128))      # one planted copy
    say(f'--- {N_FILES} training and {N_FILES} generated int16 volumes of 32x128x128 written in {time.perf_counter() - t0:.1f} s')
    for extra in ([], ['--chunk', '500', '--query_block', '1000']):
        rep = memorisation.main([os.path.join(tmp, 'train'), os.path.join(tmp, 'fake'), '--report', os.path.join(tmp, 'r.json')] + extra)
        s = rep['seconds']
        say(f"memorisation {' '.join(extra) or '(defaults: --chunk 256 --query_block 256)'}: total {s['total']:.2f} s; read {s['read']:.2f} s "
            f"(host, files to the pinned buffer), upload {s['upload']:.3f} s, distances {s['distances']:.3f} s, top-k {s['topk']:.3f} s (device "
            f"events); duplicates {rep['pooled']['duplicates']}, unauthentic {rep['pooled']['unauthentic']}")
out.close()
