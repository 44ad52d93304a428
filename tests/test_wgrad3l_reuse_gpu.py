"""The sliding-halo weight gradient (conv_wgrad3l, csrc/wgrad.hip) under both tap schedules and both MFMA shapes:
SG_WGRAD3L_REUSE = 1 (the default: a wave owns whole tap columns (kd, kw) and reads each halo row once for its three kh taps)
against 0 (tap = wave + 4 j, a read per tap and K step), each with SG_WGRAD3L_16 = 0 | 1.

The inputs are the integer-valued ones of tests/wgref.py: every f32 sum is exact in any order of accumulation, so the
permuted K order of the row-reuse loop cannot show and the comparison against the fp64 reference is torch.equal, for dw and
for db (the bias slot: wave 3's slot 6 on the image of ones).  The shapes are the smallest that cross each boundary of the
loop; the launch helpers and the reference cache are those of tests/test_wgrad_exact_gpu.py.

The up-sampled ragged case is 6 x 6 x 64, not 5 x 6 x 64: a nearest-x2 tensor has even extents (an odd D with ups is not this
kernel's), so that variant has three full D tiles, the partial H tile, the W seam and the partial channel tiles."""
import itertools

import pytest
import torch

from tests import test_wgrad_exact_gpu as E
from tests import wgref as R

pytestmark = pytest.mark.gpu

Case = E.Case
SHAPES = [
    # two columns (both wave groups work) of two D tiles (the plane ring wraps)
    Case('two_columns', 'conv_wgrad3l', 1, 32, 32, (4, 8, 32)),
    # half-filled last D tile, 2-of-4-row last H tile, a W seam, partial channel tiles
    Case('ragged', 'conv_wgrad3l', 1, 40, 72, (5, 6, 64)),
    Case('ups_two_columns', 'conv_wgrad3l<ups>', 1, 32, 32, (4, 8, 32), ups=True),
    Case('ups_ragged', 'conv_wgrad3l<ups>', 1, 40, 72, (6, 6, 64), ups=True),
    Case('gather', 'conv_wgrad3l<dy gather>', 1, 32, 32, (4, 8, 32), gain=0.125),
    Case('gather_ragged', 'conv_wgrad3l<dy gather>', 1, 40, 96, (6, 6, 64), gain=1.0),
    Case('w16', 'conv_wgrad3l<w16>', 2, 32, 32, (4, 8, 16)),
    Case('w16_ragged', 'conv_wgrad3l<w16>', 2, 40, 72, (6, 24, 16)),
]
MODES = list(itertools.product((0, 1), (0, 1), (False, True)))      # (reuse, m16, slabs)
RUNS = [(c, m) for c in SHAPES for m in MODES]


@pytest.fixture(scope='module', autouse=True)
def _release_case_data():
    yield
    E._data.cache_clear()


def _with_switches(c, reuse, m16):
    return Case(c.id, c.kernel, c.n, c.cin, c.cout, c.sp, c.k, ups=c.ups, dt=c.dt, gain=c.gain,
                env={'SG_WGRAD3L_REUSE': reuse, 'SG_WGRAD3L_16': m16})


@pytest.mark.parametrize('run', RUNS, ids=[f'{c.id}-reuse{r}-m16_{m}-{"slabs" if s else "atomics"}' for c, (r, m, s) in RUNS])
def test_both_schedules_both_mfma_shapes_are_exact(run, sg_env):
    """dw and db bit for bit against fp64, the kernel asserted by name (E._run_exact)."""
    c, (reuse, m16, slabs) = run
    coef = 0.25 if (SHAPES.index(c) + reuse) % 2 == 0 else 0.37
    E._run_exact(_with_switches(c, reuse, m16), coef, slabs, sg_env)


# one voxel of x at a time: an interior one and one on each of the six faces of the 4 x 8 x 32 volume
D, H, W = 4, 8, 32
VOXELS = [('interior', (1, 5, 17)), ('d_lo', (0, 3, 9)), ('d_hi', (3, 4, 20)), ('h_lo', (2, 0, 13)), ('h_hi', (1, 7, 30)),
          ('w_lo', (2, 2, 0)), ('w_hi', (1, 6, 31))]


@pytest.mark.parametrize('m16', (0, 1), ids=['32x32x16', '16x16x32'])
@pytest.mark.parametrize('vox', VOXELS, ids=[v[0] for v in VOXELS])
def test_one_tap_at_a_time(vox, m16, sg_env):
    """dy all ones, x = 1 in a single voxel p and channel ci: dw[tap][ci][:] is 1 where p - (tap - 1) is a voxel of the volume and
    0 elsewhere (other channels: 0), db is the voxel count.  A slot that stores to the wrong tap, or a halo row that meets the
    dy row of another kh, moves a 1 of a face voxel's pattern: the message names the first such tap."""
    _lib, lib = E._libs()
    name, p = vox
    ci = (7 * VOXELS.index(vox) + 3) % 32
    c = Case(f'one_tap_{name}', 'conv_wgrad3l', 1, 32, 32, (D, H, W))
    x = torch.zeros((1, 32, D, H, W), dtype=E.BF).contiguous(memory_format=torch.channels_last_3d)
    x[0, ci, p[0], p[1], p[2]] = 1.0
    dy = torch.ones((1, 32, D, H, W), dtype=E.BF).contiguous(memory_format=torch.channels_last_3d)
    want = torch.zeros((3, 3, 3, 32, 32))
    for kd, kh, kw in itertools.product(range(3), repeat=3):
        v = (p[0] - kd + 1, p[1] - kh + 1, p[2] - kw + 1)
        if 0 <= v[0] < D and 0 <= v[1] < H and 0 <= v[2] < W:
            want[kd, kh, kw, ci, :] = 1.0
    dw64, db64 = R.wgrad_ref(x, dy, E.K333)
    assert torch.equal(want.double(), dw64), 'the closed form of the pattern'
    sg_env(SG_WGRAD3L_REUSE=1, SG_WGRAD3L_16=m16)
    dw, db = E._outputs(c)
    rc, names = E._launch(c, x.to(E.dev()), dy.to(E.dev()), None, dw, db, 1.0)
    _lib.check(rc, c.id)
    assert names == [c.kernel], names
    got = dw.cpu()
    for kd, kh, kw in itertools.product(range(3), repeat=3):
        g, w = got[kd, kh, kw], want[kd, kh, kw]
        if not torch.equal(g, w):
            bad = (g != w).nonzero()[0].tolist()
            raise AssertionError(f'{name} voxel {p}: tap (kd, kh, kw) = {(kd, kh, kw)} (index {kd * 9 + kh * 3 + kw}) is wrong, first at '
                                 f'[ci, co] = {bad}: {float(g[tuple(bad)])!r} != {float(w[tuple(bad)])!r} (x is in channel {ci})')
    assert torch.equal(db.cpu(), torch.full((32,), float(D * H * W))), 'db'


@pytest.mark.parametrize('cid', ['ragged', 'w16_ragged'])
def test_reproducible_mode_is_bit_identical_run_to_run(cid):
    """SG_DETERMINISTIC with the default schedule on N(0, 1) data, where the order of the f32 sums does matter: two runs, same bits."""
    import saragan_amd
    _lib, lib = E._libs()
    c = {s.id: s for s in SHAPES}[cid]
    g = torch.Generator().manual_seed(11)
    x = torch.randn((c.n, c.cin, *c.sp), generator=g).to(E.BF).contiguous(memory_format=torch.channels_last_3d).to(E.dev())
    dy = torch.randn((c.n, c.cout, *c.sp), generator=g).to(E.BF).contiguous(memory_format=torch.channels_last_3d).to(E.dev())
    outs = []
    saragan_amd.set_deterministic(True)
    try:
        for _ in range(2):
            dw, db = E._outputs(c)
            rc, names = E._launch(c, x, dy, None, dw, db, 0.37)
            _lib.check(rc, c.id)
            assert names == [c.kernel], names
            outs.append((dw.cpu(), db.cpu()))
    finally:
        saragan_amd.set_deterministic(False)
    assert torch.isfinite(outs[0][0]).all() and float(outs[0][0].abs().max()) > 1.0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
