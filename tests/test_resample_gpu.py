"""sg_resample_axes (csrc/resample.hip) against functional.resample_volume's numpy twin, with ==: the definition is exact, and the
twin is pinned by tests/test_resample_host.py (scipy, dense matrices, exact cases), so no tolerance appears here.

The kernel's tile is 4 x 4 x 64 output voxels (d, h, w) per block of 256 threads; the sweep's output (7, 26, 70) exceeds it on every
axis by a non-multiple (3, 2 and 6 voxels into the second, seventh and second tile), and its last planes, rows and columns lie
outside the source."""
import functools

import numpy as np
import pytest
import torch

from tests.test_render_view_gpu import make
from tests.test_resample_host import ALL_SRC, INT_SRC, OUT, SHAPE, STARTS, STEPS, T_OUT, coords, inside_mask

pytestmark = pytest.mark.gpu

SG_OK, SG_EINVAL, SG_EALIGN = 0, -1, -3
TILE = (4, 4, 64)


def both(x, out_shape, step, start, **kw):
    """(device result, twin result) as numpy arrays, after asserting they are the same bits."""
    from saragan_amd import functional as F
    if 'out' in kw:
        kw['out_dtype'] = T_OUT[kw.pop('out')]
    ref = F.resample_volume(x.cpu(), out_shape, step, start, **kw).numpy()
    got = F.resample_volume(x if x.is_cuda else x.cuda(), out_shape, step, start, **kw)
    assert got.is_cuda and got.is_contiguous()
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == ref.dtype, (got.shape, ref.shape, got.dtype, ref.dtype)
    assert np.array_equal(got, ref, equal_nan=True), (kw, np.argwhere(~((got == ref) | ((got != got) & (ref != ref))))[:4])
    return got, ref


@functools.lru_cache(maxsize=None)
def outside():
    return ~inside_mask(SHAPE, coords())


@pytest.mark.parametrize('name', ALL_SRC)
@pytest.mark.parametrize('mode', ('nearest', 'linear', 'antialias'))
def test_every_dtype_mode_and_output(name, mode):
    """Rows of 45 elements: for the 2-byte types neither a multiple of 16 bytes nor 16-byte aligned from row to row."""
    assert all(o > t and o % t for o, t in zip(OUT, TILE))
    x = make(name, (2,) + SHAPE)
    out = outside()
    assert out.any() and not out.all()
    for o in (('u16', 'i16', 'f32') if name in INT_SRC else ('f32',)):
        fill = 7 if name in INT_SRC else -2.5
        got, _ = both(x, OUT, STEPS, STARTS, mode=mode, fill=fill, out=o)
        assert (got[:, out] == fill).all() and (got[:, ~out] != fill).any()


def test_wide_taps_on_every_axis():
    """antialias at |step| 2.4, 1.7 and 3.1: 5, 4 and 7 taps, the d axis flipped, more than one tile along w."""
    x = make('i16', (2, 11, 23, 230))
    for o in ('i16', 'f32'):
        both(x, (6, 14, 75), (-2.4, 1.7, 3.1), (10.0, 0.35, 1.05), mode='antialias', fill=-1000, out=o)
    both(x, (6, 14, 75), (-2.4, 1.7, 3.1), (10.0, 0.35, 1.05), mode=('antialias', 'nearest', 'linear'), out='u16')


@pytest.mark.parametrize('axis', (0, 1, 2))
def test_extent_one(axis):
    """S = 1 on each axis in turn (every tap lands on the one voxel), and O = 1."""
    shape = [3, 5, 6, 9]
    shape[1 + axis] = 1
    x = make('i16', tuple(shape))
    for mode in ('nearest', 'linear', 'antialias'):
        both(x, (5, 7, 11), (0.6, 0.6, 0.6), (-0.3, -0.3, -0.3), mode=mode)
    y = make('u8', (3, 5, 6, 9))
    out_shape = [6, 8, 12]
    out_shape[axis] = 1
    both(y, out_shape, (0.8, 0.7, 0.7), (0.4, 0.0, 0.0), out='f32')


def test_batch_of_one_and_a_source_one_element_off():
    both(make('i16', (1,) + SHAPE), OUT, STEPS, STARTS)
    for name in ('i16', 'u8', 'f32'):
        x = make(name, (3,) + SHAPE)
        flat = torch.empty(x.numel() + 1, dtype=x.dtype, device='cuda')
        flat[1:] = x.cuda().reshape(-1)
        off = flat[1:].reshape(x.shape)
        assert off.data_ptr() % 16 == x.element_size() and off.is_contiguous()
        from saragan_amd import functional as F
        got = F.resample_volume(off, OUT, STEPS, STARTS, fill=-5).cpu().numpy()
        assert np.array_equal(got, F.resample_volume(x, OUT, STEPS, STARTS, fill=-5).numpy())


def test_an_output_wholly_outside_the_source():
    x = torch.full((2, 4, 5, 6), float('nan'), dtype=torch.float32)
    for step, start in (((1, 1, 1), (10, 0, 0)), ((1, 1, 1), (0, -9, 0)), ((1, -1, 1), (0, -1, 0)), ((1, 1, 2), (0, 0, 5.6))):
        got, _ = both(x, (5, 6, 70), step, start, fill=1.25)
        assert (got == 1.25).all()
    got, _ = both(make('i16', (2, 4, 5, 6)), (5, 6, 70), (1, 1, 1), (0, 0, 6), fill=-40000, out='i16')
    assert (got == -32768).all()      # the fill is stored as a value is: clamped


@pytest.mark.parametrize('name', ('f16', 'f32'))
def test_non_finite_sources(name):
    x = make(name, (2, 6, 7, 20))
    x[0, 2, 3, 4] = float('inf')
    x[0, 3, 1, 7] = float('nan')
    x[1, 5, 6, 19] = float('-inf')
    x[1, 0, 0, 0] = float('nan')
    # behind zero weights (step 1 / 2: every other output sits on a voxel) and behind weights that are not
    got, _ = both(x, (11, 13, 39), (0.5, 0.5, 0.5), (0, 0, 0))
    assert np.isnan(got[0, 6, 2, 14]) and got[0, 4, 6, 8] == np.inf and np.isfinite(got[0, 4, 6, 10]) and np.isfinite(got[0, 4, 6, 6])
    assert got[1, 10, 12, 38] == -np.inf and np.isnan(got[1, 0, 0, 0]) and np.isfinite(got[1, 0, 0, 2])
    for mode in ('nearest', 'linear', 'antialias'):
        got, _ = both(x, (4, 9, 30), (1.7, 0.8, -0.65), (0.1, 0.2, 19.3), mode=mode)
        assert np.isnan(got).any() and np.isinf(got).any() and np.isfinite(got).any()


# ---- return codes, through the C ABI
def call(lib, src, tabs, dst, **over):
    a = dict(x=src.data_ptr(), dt=2, n=src.shape[0], sd=src.shape[1], sh=src.shape[2], sw=src.shape[3], od=dst.shape[1], oh=dst.shape[2],
             ow=dst.shape[3], td=tabs[0].data_ptr(), kd=2, th=tabs[1].data_ptr(), kh=2, tw=tabs[2].data_ptr(), kw=2, fi=0, ff=0.0, odt=2,
             y=dst.data_ptr())
    a.update(over)
    return lib.sg_resample_axes(a['x'], a['dt'], a['n'], a['sd'], a['sh'], a['sw'], a['od'], a['oh'], a['ow'], a['td'], a['kd'], a['th'],
                                a['kh'], a['tw'], a['kw'], a['fi'], a['ff'], a['odt'], a['y'], None)


def test_return_codes():
    from saragan_amd import _lib, table_ops
    lib = _lib.load()
    x = make('i16', (2, 4, 5, 6)).cuda()
    tabs = [torch.from_numpy(table_ops._pack_taps(table_ops.resample_taps(s, s, 1.0, 0.0, 'linear'))).cuda() for s in (4, 5, 6)]
    y = torch.full((2, 4, 5, 6), -1, dtype=torch.int16, device='cuda')
    wide = torch.zeros((2, 4, 5, 6), dtype=torch.float32, device='cuda')
    assert call(lib, x, tabs, y) == SG_OK
    torch.cuda.synchronize()
    assert torch.equal(y, x)
    y.fill_(-1)
    einval = [dict(x=None), dict(y=None), dict(td=None), dict(th=None), dict(tw=None), dict(n=-1), dict(sd=-1), dict(sw=-6), dict(od=-1),
              dict(ow=-1), dict(kd=0), dict(kh=33), dict(kw=-1), dict(dt=6), dict(dt=9), dict(dt=-1), dict(odt=0), dict(odt=4), dict(odt=6),
              dict(dt=5, odt=2), dict(dt=4, odt=3), dict(od=2 ** 29 + 1)]
    for over in einval:
        assert call(lib, x, tabs, y, **over) == SG_EINVAL, over
    ealign = [dict(x=x.data_ptr() + 1), dict(y=y.data_ptr() + 1), dict(td=tabs[0].data_ptr() + 2), dict(tw=tabs[2].data_ptr() + 1),
              dict(dt=5, odt=5, x=x.data_ptr() + 2, y=wide.data_ptr()), dict(odt=5, y=wide.data_ptr() + 2)]
    for over in ealign:
        assert call(lib, x, tabs, y, **over) == SG_EALIGN, over
    for over in (dict(n=0), dict(n=0, x=None, y=None, td=None), dict(od=0), dict(ow=0, x=None, tw=None)):
        assert call(lib, x, tabs, y, **over) == SG_OK, over
    torch.cuda.synchronize()
    assert (y == -1).all() and (wide == 0).all()      # none of these launched anything
