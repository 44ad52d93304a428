"""sg_intensity_hist (csrc/hist.hip) through functional.intensity_hist against tests/histref.py, compared with ==: the
definition is exact (two-rounding f32 map, floor, saturation decided on the float, closed top bin, NaN column), counts are
integers and every row sums to its element count."""
import os

import numpy as np
import pytest
import torch

from tests import histref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kms_reference.npz')
SHAPES = [(1, 1), (1, 63), (3, 65), (2, 255), (5, 4097), (7, 12345), (64, 8191), (1, 2 ** 20 + 3), (512, 1024)]
DTYPES = ['float32', 'bfloat16', 'float16', 'int16', 'uint16', 'uint8', 'int8']


def _max_bins():
    from saragan_amd import _lib
    return int(_lib.load().sg_intensity_hist_max_bins())


def _make(dtype, shape, rng, centre=0.0, spread=40.0):
    """(device tensor of `dtype`, its values as float32 numpy): about a tenth of the values lie outside +-1.6 spread."""
    v = rng.normal(centre, spread, shape)
    if dtype in ('float32', 'bfloat16', 'float16'):
        t = torch.from_numpy(v.astype(np.float32)).to(getattr(torch, dtype))
        return t.cuda(), t.to(torch.float32).numpy()
    info = np.iinfo(dtype)
    a = np.clip(np.rint(v + (0 if info.min < 0 else 1.6 * spread)), info.min, info.max).astype(dtype)
    return torch.from_numpy(a).cuda(), a.astype(np.float32)


def _check(x, ref_vals, lo, hi, scale=1.0, shift=0.0, pooled=False):
    from saragan_amd import functional as F
    got = F.intensity_hist(x, lo, hi, scale, shift, pooled=pooled)
    want = histref.hist(ref_vals.reshape(x.shape[0], -1), lo, hi, scale, shift, pooled=pooled)
    assert got.dtype == torch.int64 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    assert (got.sum(axis=1) == (x.numel() if pooled else x.numel() // x.shape[0])).all()
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    return got


def test_the_restated_cap_is_the_library_s():
    from saragan_amd import _lib
    assert _max_bins() == _lib.INTENSITY_HIST_MAX_BINS >= 4096


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_shapes_and_bins(shape):
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1])
    x, ref = _make('float32', shape, rng, spread=1.0)
    for bins in (1, 2, 64, 1000, 4096, _max_bins()):
        lo = -(bins // 2) - 3
        # the data spread over about 1.2 times the range: both saturating ends are populated
        _check(x, ref, lo, lo + bins, scale=0.3 * bins + 0.77, shift=-3.25)


@pytest.mark.parametrize('dtype', DTYPES)
def test_dtypes(dtype):
    rng = np.random.default_rng(DTYPES.index(dtype) + 11)
    for shape in ((3, 65), (5, 4097), (7, 12345)):
        x, ref = _make(dtype, shape, rng)
        assert str(x.dtype) == 'torch.' + dtype
        _check(x, ref, -64, 64)
        _check(x, ref, -300, 700, scale=7.3, shift=11.5)
        _check(x, ref, -64, 64, pooled=True)


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16', 'uint8'])
@pytest.mark.parametrize('skip', [1, 3])
def test_misaligned_base(dtype, skip):
    rng = np.random.default_rng(skip)
    for rows, row_elems in ((3, 65), (5, 4097), (2, 40000)):
        flat, ref = _make(dtype, (rows * row_elems + skip,), rng)
        x = flat[skip:].reshape(rows, row_elems)
        assert x.is_contiguous() and x.data_ptr() % 16 != 0
        _check(x, ref[skip:].reshape(rows, row_elems), -50, 50)


def test_contention_patterns():
    n = 2 ** 20
    one = torch.full((1, n), 5.0, device='cuda')
    got = _check(one, np.full((1, n), 5.0, np.float32), 0, 4096)
    assert got[0, 5] == n
    two = np.tile(np.array([3.0, 900.0], np.float32), n // 2).reshape(1, n)
    _check(torch.from_numpy(two).cuda(), two, 0, 4096)
    _check(torch.from_numpy(two).cuda(), two, 0, 8)          # (replicated images: both land in bins 3 and 7)
    for dtype, width in (('float32', 4), ('bfloat16', 8), ('uint8', 16)):      # elements of one 16-byte load
        rng = np.random.default_rng(width)
        for run in range(1, 10):
            for run_len in (run, run + width - 4):      # runs of 1..9 elements and runs around the width of a lane's load
                reps = 20000 // run_len + 1
                vals = np.repeat(rng.integers(0, 100, reps), run_len)[:20000 - run].astype(np.float32)
                x = torch.from_numpy(vals).to(getattr(torch, dtype)).cuda().reshape(1, -1)
                _check(x, vals.reshape(1, -1), 0, 100)


def test_edges_and_non_finite():
    lo, hi = -7, 9
    f = np.float32
    up, down = lambda v: np.nextafter(f(v), f(np.inf)), lambda v: np.nextafter(f(v), f(-np.inf))
    vals = np.array([lo, up(lo), down(lo), lo - 1, hi, up(hi), down(hi), hi - 1, down(hi - 1), hi + 1, np.inf, -np.inf, np.nan,
                     -0.0, 0.0, down(0), up(0), -1, 3e38, -3e38, 2147483648.0, -2147483904.0, 1e-45, -1e-45], dtype=np.float32)
    got = _check(torch.from_numpy(vals).cuda().reshape(1, -1), vals.reshape(1, -1), lo, hi)
    assert got[0, -1] == 1                                   # the NaN
    assert got[0, hi - lo - 1] >= 6 and got[0, 0] >= 6       # the closed top bin, the saturated bottom
    # every run length of the edge values around a lane's four elements, and a row that is NaN throughout
    many = np.tile(vals, 700)[:16381].reshape(1, -1)
    _check(torch.from_numpy(many).cuda(), many, lo, hi)
    nan_row = np.stack([np.full(4099, np.nan, np.float32), np.linspace(-20, 20, 4099, dtype=np.float32)])
    got = _check(torch.from_numpy(nan_row).cuda(), nan_row, lo, hi)
    assert got[0, -1] == 4099 and got[0, :-1].sum() == 0 and got[1, -1] == 0
    # a range whose bounds no float32 holds: the comparison is still the integer's
    lo2 = 2 ** 30 + 1
    big = np.array([2.0 ** 30, 2.0 ** 30 + 128, 2.0 ** 30 + 4096, 2.0 ** 30 + 4224], dtype=np.float32).reshape(1, -1)
    _check(torch.from_numpy(big).cuda(), big, lo2, lo2 + 4097)


def test_the_map_is_not_contracted():
    """Inputs where floor(fma(x, scale, shift)) differs from floor of the product-then-sum value: a contracted map would
    move them to the neighbouring bin."""
    scale, shift = 347.3, -1024.5
    rng = np.random.default_rng(7)
    k = rng.integers(-200, 4300, size=20000)
    x0 = ((k + 1024.5) / 347.3).astype(np.float32)
    cands = [x0]
    for toward in (np.inf, -np.inf):
        x = x0
        for _ in range(2):
            x = np.nextafter(x, np.float32(toward))
            cands.append(x)
    x = np.unique(np.concatenate(cands))
    two = histref.mapped(x, scale, shift)
    fused = (x.astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(shift))).astype(np.float32)
    x = x[np.floor(two) != np.floor(fused)]
    assert x.size >= 100
    _check(torch.from_numpy(x).cuda().reshape(1, -1), x.reshape(1, -1), 0, 4096, scale, shift)
    _check(torch.from_numpy(x[:x.size // 3 * 3]).cuda().reshape(3, -1), x[:x.size // 3 * 3].reshape(3, -1), 0, 4096, scale, shift)


def test_accumulate_and_pooled():
    from saragan_amd import functional as F
    rng = np.random.default_rng(3)
    a, ra = _make('float32', (6, 5001), rng)
    b, rb = _make('int16', (6, 5001), rng)
    out = torch.full((6, 129), -12345678901, dtype=torch.int64, device='cuda')      # garbage: accumulate=False overwrites it
    res = F.intensity_hist(a, -64, 64, out=out)
    assert res is out
    ha, hb = histref.hist(ra, -64, 64), histref.hist(rb, -64, 64)
    assert np.array_equal(out.cpu().numpy(), ha)
    F.intensity_hist(b, -64, 64, out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy(), ha + hb)
    pooled = F.intensity_hist(a, -64, 64, pooled=True)
    assert np.array_equal(pooled.cpu().numpy(), ha.sum(axis=0, keepdims=True))
    with pytest.raises(ValueError):
        F.intensity_hist(a, -64, 64, out=out, pooled=True)            # [1, 129] is the pooled shape
    with pytest.raises(ValueError):
        F.intensity_hist(a, -64, 64, accumulate=True)                 # nothing to add to


def test_two_identical_calls_give_identical_tensors():
    from saragan_amd import functional as F
    x, _ = _make('bfloat16', (9, 70001), np.random.default_rng(5))
    assert torch.equal(F.intensity_hist(x, -100, 100), F.intensity_hist(x, -100, 100))


def test_offsets_are_64_bit():
    from saragan_amd import functional as F
    n = 2 ** 32 + 5
    x = torch.zeros(n, dtype=torch.uint8, device='cuda')
    x[-3:] = 7
    got = F.intensity_hist(x.reshape(1, n), 0, 16).cpu().numpy()
    want = np.zeros((1, 17), np.int64)
    want[0, 0], want[0, 7] = n - 3, 3
    assert np.array_equal(got, want)


def test_the_c_entry_point_refuses_bad_arguments():
    from saragan_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, device='cuda')
    out = torch.full((1, 9), 77, dtype=torch.int64, device='cuda')
    st = torch.cuda.current_stream().cuda_stream

    def call(dt=_lib.SG_SRC_F32, rows=1, row_elems=64, scale=1.0, bins=8):
        return lib.sg_intensity_hist(x.data_ptr(), dt, rows, row_elems, scale, 0.0, 0, bins, out.data_ptr(), 1, st)
    assert call() == 0
    for bad in (dict(bins=0), dict(bins=_max_bins() + 1), dict(rows=-1), dict(row_elems=-1), dict(scale=float('inf')),
                dict(scale=float('nan')), dict(dt=7), dict(dt=-1)):
        assert call(**bad) != 0, bad
    torch.cuda.synchronize()
    assert out.cpu().numpy().tolist() == [[77 + 64] + [77] * 8]      # the one good call, and nothing else, was launched
    # the table gather still refuses the type it never read
    idx = torch.zeros(1, dtype=torch.int32, device='cuda')
    dst = torch.zeros(64, device='cuda')
    assert lib.sg_gather_rows(x.data_ptr(), _lib.SG_SRC_BF16, 1, 64, idx.data_ptr(), 1, dst.data_ptr(), 0, 0.0, 1.0, st) != 0


def test_the_reference_s_statistic_from_the_kernel_s_counts():
    from saragan_amd import functional as F
    from saragan_amd.metrics.intensity_metrics import histogram_distances
    g = np.load(GOLDEN)
    lo, hi = (int(v) for v in g['clip_range'])
    ic = float(g['intercept'])
    n = g['real'].shape[0]
    hr = F.intensity_hist(torch.from_numpy(g['real']).cuda(), lo, hi, ic, ic, pooled=True)
    hf = F.intensity_hist(torch.from_numpy(g['fake']).cuda(), lo, hi, ic, ic, pooled=True)
    d = histogram_distances(hr, hf)
    assert abs(d['max_density_gap'] - float(g['value'])) <= 4 * n * 2.0 ** -53
