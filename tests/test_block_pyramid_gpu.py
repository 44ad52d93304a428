"""sg_block_pyramid (csrc/pyramid.hip) against tests/pyrref.py, with ==: the definition is exact.
Integer inputs are drawn over CT-like ranges (tests/test_render_view_gpu.make); floats are k / 16 with bounded k, so that every
f64 sum of them is exact in any order and the kernel's order of summation cannot show."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import pyrref
from tests.test_render_view_gpu import make

pytestmark = pytest.mark.gpu

T_OUT = {'u16': torch.uint16, 'i16': torch.int16, 'f32': torch.float32}
N_OUT = {'u16': np.uint16, 'i16': np.int16, 'f32': np.float32}
INT_SRC = ('u8', 'i8', 'i16', 'u16')
INTERCEPT = {'u8': 7, 'i8': -100, 'i16': -1024, 'u16': 0, 'f16': -3.5, 'f32': 100.25}
SG_OK, SG_EINVAL, SG_EALIGN = 0, -1, -3


def pyramid(x, target, levels, out='u16', **kw):
    from saragan_amd import functional as F
    return F.block_pyramid(x if x.is_cuda else x.cuda(), target, levels, out_dtype=T_OUT[out], **kw)


def same(got, ref, what=None):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        g = g.cpu().numpy()
        assert g.shape == r.shape and g.dtype == r.dtype, (what, i, g.shape, r.shape, g.dtype, r.dtype)
        assert np.array_equal(g, r, equal_nan=True), (what, i, np.argwhere(g != r)[:4])


def check(x, target, levels, out='u16', **kw):
    ref = pyrref.pyramid(x.cpu().numpy(), target, levels, out_dtype=N_OUT[out], **kw)
    same(pyramid(x, target, levels, out, **kw), ref, (tuple(x.shape), target, levels, out, kw))
    return ref


@pytest.mark.parametrize('name', INT_SRC + ('f16', 'f32'))
@pytest.mark.parametrize('mode', ('mean', 'max'))
def test_every_dtype_mode_and_output(name, mode):
    """(3, 5, 9, 13) into (8, 8, 16): D and W padded by an odd amount, H cropped; one, two and three levels."""
    x = make(name, (3, 5, 9, 13))
    for out in (('u16', 'i16', 'f32') if name in INT_SRC else ('f32',)):
        for levels in (1, 2, 3):
            check(x, (8, 8, 16), levels, out, reduce=mode, intercept=INTERCEPT[name])


@pytest.mark.parametrize('source', [(8, 8, 16), (5, 7, 13), (6, 6, 14), (11, 13, 21), (1, 1, 1), (1, 9, 40)])
def test_window_geometry(source):
    """L = 2, i16: the source equal to the target, smaller and larger on all axes, of extent 1; every anchor on every axis."""
    x = make('i16', (2,) + source)
    for anchor in [('center',) * 3, ('start',) * 3, ('end',) * 3, ('start', 'end', 'center'), ('end', 'center', 'start'),
                   ('center', 'start', 'end')]:
        check(x, (8, 8, 16), 2, 'i16', intercept=-1024, anchor=anchor)


def test_a_target_that_no_source_voxel_reaches():
    from saragan_amd import table_ops
    x = make('i16', (2, 4, 6, 10)).cuda()
    for off in ((100, 0, 0), (0, -50, 0), (0, 0, 10), (-8, 0, 0)):
        outs, _ = table_ops.block_pyramid_launch(x, (8, 8, 16), off, 2, 'mean', -1024, 5000, -32768, 2000, torch.int16)
        assert all((o == 2000).all() for o in outs), off      # clamp(5000 + 1024, ., 2000)
        outs, _ = table_ops.block_pyramid_launch(x, (8, 8, 16), off, 2, 'max', -1024, 300, -32768, 2000, torch.int16)
        assert all((o == 1324).all() for o in outs), off


@pytest.mark.parametrize('shape,target', [((1, 4, 8, 63), (4, 8, 64)), ((1, 4, 8, 65), (4, 8, 64)), ((2, 4, 5, 1030), (4, 4, 1024)),
                                          ((1, 4, 8, 200), (4, 8, 192))])
def test_row_paths(shape, target):
    """Source rows that start off a 16-byte boundary (odd widths; a centred crop of 3 and of 4 columns), longer than a tile."""
    for name in ('i16', 'u8', 'f32'):
        x = make(name, shape)
        check(x, target, 3, 'u16' if name != 'f32' else 'f32', intercept=-1024 if name == 'i16' else 0)


@pytest.mark.parametrize('name,shape', [('i16', (2, 4, 8, 64)), ('u8', (1, 4, 8, 70)), ('f32', (1, 4, 8, 24)), ('u16', (1, 5, 9, 13))])
def test_base_pointer_one_element_off(name, shape):
    """A [1:] view of a flat buffer: aligned to the element, not to 16 bytes."""
    x = make(name, shape)
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device='cuda')
    flat[1:] = x.cuda().reshape(-1)
    off = flat[1:].reshape(shape)
    assert off.data_ptr() % 16 == x.element_size() and off.is_contiguous()
    out = 'f32' if name == 'f32' else 'u16'
    target = (4, 8, 16 * ((shape[3] + 15) // 16))
    same(pyramid(off, target, 3, out), pyrref.pyramid(x.numpy(), target, 3, out_dtype=N_OUT[out]))


@pytest.mark.parametrize('width', (8, 16, 32))
def test_short_output_rows(width):
    """Output rows of 2, 4 and 8 elements at the deepest of three levels."""
    for out in ('u16', 'f32'):
        check(make('u16', (2, 4, 8, width)), (4, 8, width), 3, out)


@functools.lru_cache(maxsize=None)
def deep_case():
    x = make('u16', (2, 32, 64, 96))
    return x, pyrref.pyramid(x.numpy(), (32, 64, 96), 6)


def test_full_depth_in_one_launch():
    """(2, 32, 64, 96) at L = 6: bricks side by side on two axes, one brick deep, a tile that ends inside the block's columns."""
    x, ref = deep_case()
    same(pyramid(x, (32, 64, 96), 6), ref)
    same(pyramid(x, (32, 64, 96), 6, reduce='max'), pyrref.pyramid(x.numpy(), (32, 64, 96), 6, 'max'))
    for levels in (4, 5):
        same(pyramid(x, (32, 64, 96), levels, 'f32'), pyrref.pyramid(x.numpy(), (32, 64, 96), levels, out_dtype=np.float32))


def test_width_of_the_sums():
    """v = 131070 in every voxel: the 32 768-voxel sum passes 2^32."""
    big = torch.full((1, 32, 32, 32), 65535, dtype=torch.uint16)
    ref = check(big, (32, 32, 32), 6, 'f32', intercept=-65535)
    assert all((r == 131070.0).all() for r in ref)
    got = pyramid(big, (32, 32, 32), 6, 'i16', intercept=-65535)
    assert all((g == 32767).all() for g in got)


def test_negative_means_truncate_toward_zero():
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(-1030, -1018, (2, 8, 16, 16)).astype(np.int16))
    ref = check(x, (8, 16, 16), 4, 'i16', intercept=-1024, clip=(-2000, 2000))
    v = x.numpy().astype(np.int64) + 1024
    s1 = v.reshape(2, 4, 2, 8, 2, 8, 2).sum(axis=(2, 4, 6))
    odd_negative = (s1 < 0) & (s1 % 8 != 0)
    assert odd_negative.any() and (ref[1][odd_negative] == -((-s1[odd_negative]) // 8)).all()      # -1.5 -> -1, a floor gives -2
    assert (ref[1][odd_negative] != s1[odd_negative] // 8).all()


def test_the_clamp_follows_each_levels_reduction():
    rng = np.random.default_rng(6)
    x = torch.from_numpy((rng.integers(0, 2, (1, 8, 8, 16)) * 6000).astype(np.uint16))
    ref = check(x, (8, 8, 16), 3, 'u16', clip=(0, 3072))
    assert (ref[0] == 3072).any() and (ref[1] < 3072).any() and ((ref[1] > 0) & (ref[1] < 3072)).any()


@pytest.mark.parametrize('name', ('f16', 'f32'))
def test_float_sources_and_nan(name):
    x = make(name, (2, 8, 16, 24))
    for mode in ('mean', 'max'):
        check(x, (8, 16, 24), 4, 'f32', reduce=mode, intercept=0.75, clip=(-30.0, 40.0))
    x[0, 3, 5, 7] = float('nan')
    x[1, 0:2, 0:2, 0:2] = float('nan')      # an all-NaN 2-cube
    mean = check(x, (8, 16, 24), 4, 'f32', reduce='mean')
    assert all(np.isnan(m[0, 3 >> i, 5 >> i, 7 >> i]) for i, m in enumerate(mean)) and not np.isnan(mean[1][0, 0, 0, 0])
    mx = check(x, (8, 16, 24), 4, 'f32', reduce='max')
    assert not any(np.isnan(m).any() for m in mx) and mx[1][1, 0, 0, 0] == -np.inf and np.isfinite(mx[2]).all()


def test_statistics():
    x, ref = deep_case()
    got, st = pyramid(x, (32, 64, 96), 6, stats=True)
    same(got, ref)
    assert st.dtype == torch.int64 and np.array_equal(st.cpu().numpy(), pyrref.stats(ref))
    again = pyramid(x, (32, 64, 96), 6, stats=True)[1]
    assert torch.equal(st, again)
    p = make('i16', (3, 5, 9, 13))
    for mode in ('mean', 'max'):
        ref = pyrref.pyramid(p.numpy(), (8, 8, 16), 3, mode, -1024, out_dtype=np.int16)
        got, st = pyramid(p, (8, 8, 16), 3, 'i16', reduce=mode, intercept=-1024, stats=True)
        same(got, ref)
        assert np.array_equal(st.cpu().numpy(), pyrref.stats(ref))


def test_a_batch_equals_its_volumes_one_by_one():
    x = make('i16', (5, 9, 20, 70)).cuda()
    kw = dict(intercept=-1024, clip=(-500, 2500), stats=True)
    outs, st = pyramid(x, (8, 16, 64), 4, 'i16', **kw)
    for k in range(5):
        one, st1 = pyramid(x[k:k + 1].contiguous(), (8, 16, 64), 4, 'i16', **kw)
        assert all(torch.equal(o[k:k + 1], q) for o, q in zip(outs, one)) and torch.equal(st[k:k + 1], st1)


# ---- return codes, through the C ABI
def call(lib, src, outs, **over):
    a = dict(x=src.data_ptr(), dt=2, n=src.shape[0], sd=src.shape[1], sh=src.shape[2], sw=src.shape[3], D=8, H=8, W=16, od=0, oh=0, ow=0,
             levels=2, mode=0, ii=0, ip=0, ilo=-32768, ihi=32767, fi=0.0, fp=0.0, flo=0.0, fhi=1.0, odt=2,
             out=[o.data_ptr() for o in outs], stats=None)
    a.update(over)
    ptrs = (C.c_void_p * max(len(a['out']), 1))(*a['out']) if a['out'] is not None else None
    return lib.sg_block_pyramid(a['x'], a['dt'], a['n'], a['sd'], a['sh'], a['sw'], a['D'], a['H'], a['W'], a['od'], a['oh'], a['ow'],
                                a['levels'], a['mode'], a['ii'], a['ip'], a['ilo'], a['ihi'], a['fi'], a['fp'], a['flo'], a['fhi'],
                                a['odt'], ptrs, a['stats'], None)


def test_return_codes():
    from saragan_amd import _lib
    lib = _lib.load()
    x = make('i16', (2, 8, 8, 16)).cuda()
    outs = [torch.zeros((2, 8 >> i, 8 >> i, 16 >> i), dtype=torch.int16, device='cuda') for i in range(6)]
    wide = torch.zeros((2, 8, 8, 16), dtype=torch.float32, device='cuda')
    stats = torch.zeros((2, 2, 4), dtype=torch.int64, device='cuda')
    assert call(lib, x, outs[:2], stats=stats.data_ptr()) == SG_OK
    torch.cuda.synchronize()
    einval = [dict(x=None), dict(out=None), dict(out=[outs[0].data_ptr(), None]), dict(n=-1), dict(sd=-1), dict(W=-16),
              dict(levels=0), dict(levels=7), dict(levels=5), dict(levels=3, H=10, out=[o.data_ptr() for o in outs[:3]]),
              dict(dt=6), dict(dt=9), dict(dt=-1), dict(mode=2), dict(odt=0), dict(odt=4), dict(dt=5, odt=2), dict(dt=4, odt=3),
              dict(ilo=5, ihi=4), dict(odt=3, ilo=-1, ihi=10), dict(odt=3, ilo=0, ihi=65536), dict(ilo=-32769), dict(ihi=32768),
              dict(dt=5, odt=5, flo=2.0, fhi=1.0), dict(dt=5, odt=5, flo=float('nan')), dict(ii=2 ** 30 + 1), dict(ip=-2 ** 30 - 1)]
    for over in einval:
        assert call(lib, x, outs[:2], **over) == SG_EINVAL, over
    ealign = [dict(x=x.data_ptr() + 1), dict(out=[outs[0].data_ptr() + 1, outs[1].data_ptr()]),
              dict(stats=stats.data_ptr() + 4), dict(dt=5, odt=5, x=x.data_ptr() + 2, out=[wide.data_ptr(), stats.data_ptr()])]
    for over in ealign:
        assert call(lib, x, outs[:2], **over) == SG_EALIGN, over
    for over in (dict(n=0), dict(n=0, x=None, out=None), dict(D=0), dict(W=0, x=None)):
        assert call(lib, x, outs[:2], **over) == SG_OK, over
    torch.cuda.synchronize()
