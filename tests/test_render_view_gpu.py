"""sg_render_view (csrc/render.hip) against tests/viewref.py, with ==: the definition is exact.  Every shape case runs every
axis x mode.  MEAN inputs are integers, or floats k * 2^-4 with |k| <= 128 (bf16), 1024 (f16), 2^14 (f32): every f64 sum of them
is exact in any order (4096 such terms stay far under 2^53 granules), so the kernel's order of summation cannot show."""
import numpy as np
import pytest
import torch

from tests import viewref

pytestmark = pytest.mark.gpu

MODES = ('slice', 'max', 'mean')
VIEWS = [(axis, mode) for axis in (0, 1, 2) for mode in MODES]
DTYPES = {'u8': torch.uint8, 'i8': torch.int8, 'i16': torch.int16, 'u16': torch.uint16, 'f16': torch.float16,
          'f32': torch.float32, 'bf16': torch.bfloat16}
# a window inside each type's value range below, so that both clamps and the levels between them occur
WINDOWS = {'u8': (20.0, 200.0), 'i8': (-100.0, 90.0), 'i16': (-500.0, 2000.0), 'u16': (100.0, 3000.0), 'f16': (-40.0, 50.0),
           'f32': (-700.0, 900.0), 'bf16': (-5.0, 6.0)}


def make(name, shape, seed=0):
    """A CPU tensor of dtype `name`: integers over the type's range (16-bit: CT-like), floats k / 16 (see the module docstring)."""
    rng = np.random.default_rng(seed + 17 * len(shape) + sum(shape))
    if name in ('u8', 'i8', 'i16', 'u16'):
        lo, hi = {'u8': (0, 256), 'i8': (-128, 128), 'i16': (-1024, 3072), 'u16': (0, 4096)}[name]
        a = rng.integers(lo, hi, shape).astype({'u8': np.uint8, 'i8': np.int8, 'i16': np.int16, 'u16': np.uint16}[name])
        return torch.from_numpy(a)
    kmax = {'bf16': 128, 'f16': 1024, 'f32': 2 ** 14}[name]
    a = (rng.integers(-kmax, kmax + 1, shape) / 16.0).astype(np.float32)
    t = torch.from_numpy(a).to(DTYPES[name])
    assert (t.float().numpy() == a).all()      # representable: nothing was rounded
    return t


def render(x, axis, mode, **kw):
    from saragan_amd import functional as F
    return F.render_view(x.cuda(), axis, mode, **kw).cpu().numpy()


def want(x, axis, mode, index=None, window=(-1.0, 2.0), scale=1.0, shift=0.0, zoom=(1, 1), channel=0):
    t = viewref.tiles(x, axis, mode, index, window, scale, shift, zoom, channel)
    return viewref.place(np.zeros((t.shape[1], t.shape[0] * t.shape[2]), np.uint8), t)


def check_all_views(x, name, **kw):
    for axis, mode in VIEWS:
        got, ref = render(x, axis, mode, window=WINDOWS[name], **kw), want(x, axis, mode, window=WINDOWS[name], **kw)
        assert got.shape == ref.shape and (got == ref).all(), (name, tuple(x.shape), axis, mode, kw)
        assert mode != 'slice' or x.numel() < 64 or len(np.unique(ref)) > 2      # (the window shows grey levels, not two)


SHAPES = [(1, 1, 1, 1), (1, 2, 3, 5), (3, 4, 8, 8), (2, 5, 7, 63), (2, 3, 9, 65), (5, 8, 16, 200), (1, 33, 17, 1030),
          (2, 32, 128, 128)]


@pytest.mark.parametrize('shape', SHAPES)
def test_every_view_of_every_shape(shape):
    """f32 and bf16 (the networks' types); (1, 33, 17, 1030) has W rows longer than the block's first pass of 16-byte loads,
    (2, 3, 9, 65) one element past a wave, (2, 32, 128, 128) several blocks per sample."""
    for name in ('f32', 'bf16'):
        check_all_views(make(name, shape), name)
        check_all_views(make(name, shape, 1), name, scale=0.75, shift=1.5)


@pytest.mark.parametrize('name', list(DTYPES))
def test_every_dtype(name):
    for shape in ((3, 4, 8, 8), (2, 3, 9, 65), (1, 2, 3, 2100)):      # (2100 bytes of u8: a row for the block in every type)
        check_all_views(make(name, shape), name)


@pytest.mark.parametrize('name,shape', [('f32', (3, 4, 8, 8)), ('f32', (2, 3, 9, 65)), ('bf16', (2, 4, 6, 72)), ('bf16', (1, 3, 5, 1100)),
                                        ('u8', (2, 4, 6, 48)), ('i16', (2, 3, 4, 16))])
def test_base_pointer_one_element_off(name, shape):
    """A [1:] view of a flat buffer: aligned to the element, not to 16 bytes -- the element path in front of the first boundary."""
    x = make(name, shape)
    flat = torch.empty(x.numel() + 1, dtype=x.dtype, device='cuda')
    flat[1:] = x.cuda().reshape(-1)
    off = flat[1:].reshape(shape)
    assert off.data_ptr() % 16 == x.element_size() and off.is_contiguous()
    from saragan_amd import functional as F
    for axis, mode in VIEWS:
        got = F.render_view(off, axis, mode, window=WINDOWS[name]).cpu().numpy()
        assert (got == want(x, axis, mode, window=WINDOWS[name])).all(), (axis, mode)


@pytest.mark.parametrize('name,shape', [('f32', (2, 3, 5, 9)), ('bf16', (2, 4, 8, 8)), ('f32', (1, 2, 3, 600))])
def test_channels(name, shape):
    x = make(name, shape + (3,))
    for channel in range(3):
        check_all_views(x, name, channel=channel)


@pytest.mark.parametrize('zoom', [(1, 1), (3, 1), (2, 5)])
def test_zooms(zoom):
    for name, shape in (('f32', (2, 3, 4, 12)), ('bf16', (3, 4, 8, 8)), ('i16', (2, 5, 7, 63))):
        check_all_views(make(name, shape), name, zoom=zoom)


def test_tile_placement_and_untouched_pixels():
    """grid_cols that does not divide n, an origin, pitches larger than the tile: pixels outside the tiles keep the sentinel."""
    from saragan_amd import functional as F
    x = make('f32', (5, 4, 6, 10))
    for axis, mode in VIEWS:
        for zoom in ((1, 1), (2, 3)):
            t = viewref.tiles(x, axis, mode, None, WINDOWS['f32'], zoom=zoom)
            th, tw = t.shape[1:]
            origin, pitch, cols = (3, 5), (th + 2, tw + 7), 2
            shape = (origin[0] + 2 * pitch[0] + th + 1, origin[1] + pitch[1] + tw + 4)
            ref = viewref.place(np.full(shape, 0xA5, np.uint8), t, origin, cols, pitch)
            canvas = torch.full(shape, 0xA5, dtype=torch.uint8, device='cuda')
            out = F.render_view(x.cuda(), axis, mode, window=WINDOWS['f32'], zoom=zoom, canvas=canvas, origin=origin, grid_cols=cols,
                                pitch=pitch)
            assert out is canvas and (canvas.cpu().numpy() == ref).all(), (axis, mode, zoom)
            assert (ref[:origin[0]] == 0xA5).all() and (ref[:, :origin[1]] == 0xA5).all() and (ref[-1] == 0xA5).all()


def test_slices_first_last_and_middle():
    for name, shape in (('f32', (2, 5, 7, 12)), ('bf16', (2, 4, 6, 8))):
        x = make(name, shape)
        for axis in (0, 1, 2):
            extent = shape[1 + axis]
            for index in (0, extent - 1, None):
                got = render(x, axis, 'slice', index=index, window=WINDOWS[name])
                assert (got == want(x, axis, 'slice', index=index, window=WINDOWS[name])).all()
            assert (render(x, 'dhw'[axis], 'slice', window=WINDOWS[name]) ==
                    want(x, axis, 'slice', index=extent // 2, window=WINDOWS[name])).all()


def test_window_edges_and_ties():
    """Values exactly at lo and hi, at the .5 ties of the grey levels and one f32 step beside them, outside on both sides."""
    ties = np.array([0.0, 255.0, 0.5, 1.5, 2.5, 253.5, 254.5, -0.5, 255.5, 1e9, -1e9, 127.5, 128.5], np.float32)
    vals = np.concatenate([ties, np.nextafter(ties, np.float32(np.inf)), np.nextafter(ties, np.float32(-np.inf))])
    x = torch.from_numpy(vals.reshape(1, 1, 1, -1))
    for window, scale, shift in (((0.0, 255.0), 1.0, 0.0), ((0.0, 510.0), 2.0, 0.0), ((10.0, 265.0), 1.0, 10.0),
                                 ((-1.0, 2.0), 1.0 / 85.0, -1.0), ((-1024.0, 2048.0), 12.0, -1024.0)):
        got = render(x, 0, 'slice', window=window, scale=scale, shift=shift)
        ref = want(x, 0, 'slice', window=window, scale=scale, shift=shift)
        assert (got == ref).all(), (window, got, ref)
    ref = want(x, 0, 'slice', window=(0.0, 255.0))[0]
    assert list(ref[:9]) == [0, 255, 1, 2, 3, 254, 255, 0, 255]      # ties go up: floor(u + 0.5)


def test_nan_and_infinities():
    rng = np.random.default_rng(11)
    a = (rng.integers(-64, 65, (2, 6, 7, 70)) / 16.0).astype(np.float32)
    a[rng.random(a.shape) < 0.15] = np.nan
    a[rng.random(a.shape) < 0.05] = np.inf
    a[rng.random(a.shape) < 0.05] = -np.inf
    a[0, :, 2, 3] = np.nan      # all-NaN columns along each axis: MAX stays -inf, MEAN is NaN -> 0
    a[0, 1, :, 5] = np.nan
    a[1, 2, 3, :] = np.nan
    a[1, :, 0, 0] = np.inf
    a[1, 0, :, 1] = -np.inf
    a[1, 3, 4, :] = -np.inf
    a[1, 3, 5, :2] = (np.inf, -np.inf)      # a MEAN that is NaN in any order
    for name in ('f32', 'bf16', 'f16'):
        x = torch.from_numpy(a).to(DTYPES[name])
        for axis, mode in VIEWS:
            got, ref = render(x, axis, mode, window=(-3.0, 3.5)), want(x, axis, mode, window=(-3.0, 3.5))
            assert (got == ref).all(), (name, axis, mode)
    assert want(torch.from_numpy(a), 0, 'max', window=(-3.0, 3.5))[2, 3] == 0      # -inf: black


def test_batch_layouts_of_the_networks():
    """[n, 1, d, h, w] in either memory format and [n, d, h, w] are one memory; a DeviceTable row block is [n, d, h, w] int16."""
    x = make('f32', (3, 4, 6, 8))
    ref = want(x, 1, 'max', window=WINDOWS['f32'])
    for t in (x[:, None], x[:, None].contiguous(memory_format=torch.channels_last_3d), x[..., None]):
        assert (render(t, 1, 'max', window=WINDOWS['f32']) == ref).all()


def _raw(lib, x, canvas, n, d, h, w, c=1, channel=0, axis=0, mode=1, index=0, zoom=(1, 1), scale=1.0, shift=0.0, lo=0.0, hi=1.0,
         canvas_shape=None, origin=(0, 0), grid_cols=1, pitch=(0, 0), dt=5):
    from saragan_amd._launch import _stream
    ch, cw = canvas_shape if canvas_shape is not None else canvas.shape
    return lib.sg_render_view(x, dt, n, d, h, w, c, channel, axis, mode, index, zoom[0], zoom[1], scale, shift, lo, hi,
                              255.0 / (hi - lo) if hi != lo else 1.0, canvas.data_ptr() if torch.is_tensor(canvas) else canvas, ch,
                              cw, origin[0], origin[1], grid_cols, pitch[0], pitch[1], _stream())


def test_error_codes_launch_nothing():
    """Refused arguments, not faults: every case returns its code and the canvas keeps its sentinel."""
    from saragan_amd import _lib
    lib = _lib.load()
    EINVAL, EALIGN = -1, -3
    xt = torch.ones(2, 3, 4, 5, device='cuda')
    x, dims = xt.data_ptr(), dict(n=2, d=3, h=4, w=5)
    canvas = torch.full((8, 10), 0x5A, dtype=torch.uint8, device='cuda')      # two 4 x 5 tiles side by side fit exactly
    ok = dict(grid_cols=2, pitch=(4, 5))
    inf, nan = float('inf'), float('nan')
    cases = [dict(x=None), dict(canvas=None), dict(n=-1), dict(d=-1), dict(h=-1), dict(w=-1), dict(c=0), dict(channel=1),
             dict(channel=-1), dict(c=2, channel=2), dict(dt=7), dict(dt=-1), dict(axis=3), dict(axis=-1), dict(mode=3), dict(mode=-1),
             dict(mode=0, index=3), dict(mode=0, index=-1), dict(mode=0, axis=1, index=4), dict(mode=0, axis=2, index=5),
             dict(zoom=(0, 1)), dict(zoom=(1, 0)), dict(grid_cols=0), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(lo=nan),
             dict(hi=inf), dict(lo=-inf), dict(scale=inf), dict(scale=nan),
             dict(canvas_shape=(8, 9)), dict(canvas_shape=(3, 10)),                  # a tile one pixel past the canvas
             dict(origin=(0, 1)), dict(origin=(5, 0)), dict(origin=(-1, 0)), dict(origin=(0, -1)),
             dict(zoom=(3, 1)), dict(zoom=(1, 2), pitch=(4, 10)),
             dict(grid_cols=1, pitch=(5, 5)), dict(pitch=(4, 6)), dict(pitch=(4, 4)), dict(grid_cols=1, pitch=(3, 5)),
             dict(axis=1, canvas_shape=(2, 10)), dict(axis=2, canvas_shape=(3, 7))]
    for case in cases:
        kw = dict(dims, **ok)
        kw.update(case)
        px, pc = kw.pop('x', x), kw.pop('canvas', canvas)
        assert _raw(lib, px, pc, canvas_shape=kw.pop('canvas_shape', (8, 10)), **kw) == EINVAL, case
    assert _raw(lib, x + 2, canvas, **dims, **ok) == EALIGN
    assert _raw(lib, x + 1, canvas, **dims, **ok, dt=2) == EALIGN
    # nothing to do: SG_OK without a launch, NULL pointers included
    for case in (dict(n=0), dict(d=0), dict(h=0), dict(w=0), dict(d=0, mode=0, index=0)):
        assert _raw(lib, None, None, canvas_shape=(8, 10), **dict(dims, **ok, **case)) == 0, case
    torch.cuda.synchronize()
    assert (canvas.cpu().numpy() == 0x5A).all()
    assert _raw(lib, x, canvas, **dims, **ok) == 0      # and the accepted call draws: max of ones in the window [0, 1]
    torch.cuda.synchronize()
    assert (canvas.cpu().numpy()[:4] == 255).all() and (canvas.cpu().numpy()[4:] == 0x5A).all()


def test_sheets_and_slice_grid():
    from saragan_amd import preview
    for name, shape, views, zoom_d in (('f32', (3, 4, 8, 16), ('slice_d', 'slice_h', 'max_h'), 1),
                                       ('bf16', (5, 8, 16, 24), ('max_w', 'mean_d', 'slice_w:3', 'slice_h'), 3),
                                       ('i16', (2, 5, 7, 3), ('mean_w', 'max_d'), 2)):
        x = make(name, shape)
        ref = viewref.sheet(x, views, WINDOWS[name], 0.5, 1.0, zoom_d)
        got = preview.sheet(x.cuda(), ','.join(views), WINDOWS[name], 0.5, 1.0, zoom_d)
        assert got.dtype == np.uint8 and got.shape == ref.shape and (got == ref).all(), name
        chunks = [x[:2].cuda(), x[2:].cuda()]      # chunks of one set of samples, side by side
        assert (preview.sheet(chunks, ','.join(views), WINDOWS[name], 0.5, 1.0, zoom_d) == ref).all()
    for name, shape in (('f32', (32, 16, 16)), ('bf16', (5, 6, 9)), ('i16', (1, 4, 4)), ('f32', (17, 3, 8))):
        x0 = make(name, shape)
        ref = viewref.slice_grid(x0, WINDOWS[name], 0.5, 1.0)
        assert (preview.slice_grid(x0.cuda(), WINDOWS[name], 0.5, 1.0) == ref).all()
        assert (preview.slice_grid(x0.cuda()[None, None], WINDOWS[name], 0.5, 1.0) == ref).all()
