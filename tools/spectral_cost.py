#!/usr/bin/env python
"""Cost of spectral normalisation on one MI355X (profiles/spectral_norm_cost.txt).

  python tools/spectral_cost.py kernels            refresh and pull-back on the flat D parameter buffer of the benchmarked network
                                                   against sg_axpby: one command, alternating, three rounds
  python tools/spectral_cost.py step [bench args]  bench.py's own step with every D weight normalised (same entry point, same line)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, warm=20, reps=100):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3      # microseconds per call


def kernels():
    import torch
    from benchlib.launch import parse
    from benchlib.workload import specs
    from saragan_amd import _lib
    from saragan_amd import functional as F
    from saragan_amd.networks.pgan.variables import pgan_variable_shapes
    sys.argv = [sys.argv[0]]
    args = parse()
    base_shape, ks, fs = specs(args)
    shapes = pgan_variable_shapes(args.phase, base_shape, args.latent, ks, fs)
    segs, total = [], 0
    for name, shp in shapes.items():      # varstore.flatten's layout of the discriminator
        if not name.startswith('discriminator/'):
            continue
        n = 1
        for d in shp:
            n *= int(d)
        if name.endswith('/weight'):
            segs.append((total, n // int(shp[-1]), int(shp[-1])))
        total += (n + 3) // 4 * 4
    tab = F.SpectralTable(segs, total, 'cuda')
    nw = sum(r * c for _, r, c in segs)
    print(f"size '{args.size}' phase {args.phase}: {len(segs)} normalised layers, {nw} weights of {total} flat elements "
          f"({total * 4 / 1e6:.1f} MB), {tab.nblocks} row blocks, column workspace {tab.collen * 4 / 1e6:.2f} MB")
    print('largest layers (R, C, rows per block):', sorted(((r, c, e[4]) for (_, r, c), e in zip(sorted(segs), tab.layout)),
                                                              key=lambda t: -t[0] * t[1])[:4])
    gen = torch.Generator(device='cuda').manual_seed(0)
    p = torch.randn(total, device='cuda', generator=gen)
    g = torch.randn(total, device='cuda', generator=gen)
    g0 = g.clone()
    eff = torch.zeros(total, device='cuda')
    tab.u.copy_(torch.randn(tab.ulen, device='cuda', generator=gen))
    lib = _lib.load()
    big = torch.randn(2 * total, device='cuda', generator=gen)
    out = torch.empty(2 * total, device='cuda')

    def axpby(n):
        _lib.check(lib.sg_axpby(big.data_ptr(), None, out.data_ptr(), 1.0, 0.0, n, _lib.SG_F32, F._stream()), 'sg_axpby')

    def pullback():
        F.spectral_pullback_(tab, g, eff)
    F.spectral_refresh_(tab, p, eff, 1)
    refresh_bytes = 8 * nw + 8 * tab.collen      # one read and one write of W, the column partials written and read once
    pull_bytes = 16 * nw                         # two reads of g, one of W / sigma, one write
    for rnd in range(3):
        t_copy = _time(lambda: axpby(nw))                     # 8 bytes per element: the refresh's bytes
        t_copy2 = _time(lambda: axpby(2 * nw))                # 16 bytes per weight: the pull-back's bytes
        t_ref = _time(lambda: F.spectral_refresh_(tab, p, eff, 1))
        t_ref3 = _time(lambda: F.spectral_refresh_(tab, p, eff, 3))
        g.copy_(g0)
        t_pull = _time(pullback, warm=5, reps=20)             # (in place: few repetitions keep g finite)
        print(f'round {rnd}: sg_axpby {8 * nw / 1e6:.0f} MB {t_copy:8.1f} us ({8 * nw / t_copy / 1e6:5.2f} TB/s)   '
              f'{16 * nw / 1e6:.0f} MB {t_copy2:8.1f} us ({16 * nw / t_copy2 / 1e6:5.2f} TB/s)   '
              f'refresh k=1 {t_ref:8.1f} us ({refresh_bytes / t_ref / 1e6:5.2f} TB/s, {t_ref / t_copy:4.2f} x copy)   '
              f'k=3 {t_ref3:8.1f} us   pull-back {t_pull:8.1f} us ({pull_bytes / t_pull / 1e6:5.2f} TB/s, {t_pull / t_copy2:4.2f} x copy)')


def step():
    from saragan_amd.networks import ops as nops
    nops.set_spectral_norm(('discriminator/',), int(os.environ.get('SN_ITERATIONS', '1')))
    sys.argv = [os.path.join(ROOT, 'bench.py')] + sys.argv[2:]
    import bench
    bench.main()


if __name__ == '__main__':
    {'kernels': kernels, 'step': step}[sys.argv[1]]()
