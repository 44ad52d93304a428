"""sg_power_spectrum (csrc/spectrum.hip) against the numpy twin within the derived bound of tests/specref.py
(the device and the FFT sum in different orders), exact cases with ==, every input type, the same bits whatever surrounds a
sample, guards around inputs and outputs, and the limits.  The twin itself is pinned in tests/test_spectrum_host.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import specref as R

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7),          # odd extents, below one MFMA tile
          (2, 6, 10),         # neither powers of two nor multiples of 4
          (1, 16, 16),        # an axis of extent 1
          (17, 33, 66),       # one past a tile in every axis, K not a multiple of 4
          (8, 16, 48),        # the aligned case
          (4, 4, 260)]        # W past one block's tile
TORCH_DT = [torch.uint8, torch.int8, torch.int16, torch.uint16, torch.float16, torch.bfloat16, torch.float32]


def T():
    from saragan_amd import table_ops
    return table_ops


def rows(x, plan, *a, **k):
    """(radial, (d, h, w)) of power_spectrum as numpy."""
    radial, axes = T().power_spectrum(x, plan, *a, **k)
    return radial.cpu().numpy(), tuple(v.cpu().numpy() for v in axes)


def flat(r):
    return np.concatenate([r[0]] + list(r[1]), axis=1)


def one(r, i):
    return r[0][i], tuple(a[i] for a in r[1])


def within_bound(x_np, plan, scale=1.0, shift=0.0, x_dev=None):
    want = rows(torch.from_numpy(x_np) if x_dev is None else x_dev.cpu(), plan, scale, shift)
    got = rows(torch.from_numpy(x_np).cuda() if x_dev is None else x_dev, plan, scale, shift)
    worst = 0.0
    for i in range(x_np.shape[0]):
        t = x_np[i].astype(np.float64) * scale + shift
        worst = max(worst, R.worst_ratio(one(got, i), one(want, i), t, plan))
    print(f'{plan.shape} {plan.window}: worst |device - twin| / bound = {worst:.3g}')
    assert worst <= 1.0
    return got


@pytest.mark.parametrize('shape', SHAPES)
def test_device_against_the_twin_within_the_bound(shape):
    plan = T().SpectrumPlan(shape, R.SPACING)
    within_bound(R.make_data(3, shape, 21), plan)


@pytest.mark.parametrize('shape', [(8, 16, 48), (3, 5, 7)])
def test_hann_window_within_the_bound(shape):
    plan = T().SpectrumPlan(shape, R.SPACING, window='hann')
    within_bound(R.make_data(3, shape, 22), plan)


@pytest.mark.parametrize('shape', [(3, 5, 7), (17, 33, 66), (8, 16, 48)])
def test_exact_cases(shape):
    plan = T().SpectrumPlan(shape, R.SPACING)
    d, h, w = shape
    x = np.zeros((2,) + shape, np.int16)
    x[0, 0, 0, 0] = 3          # a delta at the origin: every product is with an exact 1 or 0, F = 3 everywhere
    x[1] = -7                  # a constant: DC is the exact integer sum
    radial, axes = rows(torch.from_numpy(x).cuda(), plan)
    assert np.array_equal(radial[0], 9.0 * plan.counts)
    for a, cnt in zip(axes, plan.axis_counts):
        assert np.array_equal(a[0], 9.0 * cnt)
    assert radial[1, 0] == float(7 * d * h * w) ** 2
    assert axes[0][1, 0] >= radial[1, 0]      # (the q = 0 profile bins hold DC)


@pytest.mark.parametrize('dtype', TORCH_DT)
def test_every_input_type_and_a_nan(dtype):
    shape = (5, 12, 20)
    plan = T().SpectrumPlan(shape, R.SPACING)
    rng = np.random.default_rng(23)
    info = {torch.uint8: (0, 256), torch.int8: (-128, 128), torch.int16: (-1024, 3072), torch.uint16: (0, 65536)}
    lo, hi = info.get(dtype, (-256, 256))      # f16 and bf16 take integers they hold exactly (|v| <= 256)
    vals = rng.integers(lo, hi, size=(3,) + shape)
    np_dt = {torch.uint8: np.uint8, torch.int8: np.int8, torch.int16: np.int16, torch.uint16: np.uint16}
    x = torch.from_numpy(vals.astype(np.float32)).to(dtype) if dtype.is_floating_point else torch.from_numpy(vals.astype(np_dt[dtype]))
    back = x.float().numpy() if dtype.is_floating_point else x.numpy()
    assert np.array_equal(back.astype(np.float64), vals.astype(np.float64))      # every value is held exactly
    assert not (plan.counts == 0).any()
    got = within_bound(vals.astype(np.float64), plan, 1024.0, -1024.0, x_dev=x.cuda())
    if dtype.is_floating_point:
        y = x.clone()
        y[1, 2, 3, 4] = float('nan')
        bad = rows(y.cuda(), plan, 1024.0, -1024.0)
        assert np.isnan(flat(bad)[1]).all()
        for i in (0, 2):      # the neighbours keep the bits they have without it
            assert np.array_equal(flat(bad)[i], flat(got)[i])


def test_same_bits_whatever_surrounds_a_sample(monkeypatch):
    shape = (17, 33, 66)
    plan = T().SpectrumPlan(shape, R.SPACING)
    x = torch.from_numpy(R.make_data(5, shape, 24)).cuda()
    full = flat(rows(x, plan))
    assert np.array_equal(full, flat(rows(x, plan)))                        # two calls
    for i in range(5):                                                      # sample i alone
        assert np.array_equal(flat(rows(x[i:i + 1], plan))[0], full[i]), i
    from saragan_amd import _lib
    per = _lib.load().sg_power_spectrum_workspace(1, *shape)
    small = 1.5 * per / 2 ** 20                                             # room for one sample per launch
    spy = []
    real = _lib.load().sg_power_spectrum
    monkeypatch.setattr(_lib.load(), 'sg_power_spectrum', lambda *a: (spy.append(a[2]), real(*a))[1])
    chunked = flat(rows(x, plan, workspace_mib=small))
    assert spy == [1] * 5 and np.array_equal(chunked, full)


@pytest.mark.parametrize('dtype', [torch.int16, torch.uint8, torch.float32])
def test_views_one_element_past_a_boundary_and_guards(dtype):
    """The library call itself, on an input that starts one element past a 16-byte boundary inside a guard-filled buffer, with
    guard-filled outputs and workspace tail: nothing outside the views is touched."""
    from saragan_amd import _lib
    from saragan_amd._launch import _ptr, _stream
    lib = _lib.load()
    shape, n = (3, 5, 7), 2
    plan = T().SpectrumPlan(shape, R.SPACING)
    d, h, w = shape
    vol = d * h * w
    data = R.make_data(n, shape, 25)
    x = torch.from_numpy((data & 255).astype(np.uint8)) if dtype == torch.uint8 else torch.from_numpy(data).to(dtype)
    want = flat(rows(x.cuda(), plan))
    per16 = 16 // x.element_size()
    buf = torch.full((per16 + 1 + n * vol + 64,), 7, dtype=dtype).cuda()
    start = per16 + 1
    buf[start:start + n * vol] = x.reshape(-1).cuda()
    xv = buf[start:start + n * vol]
    assert xv.data_ptr() % 16 == x.element_size()
    nrad, alen = plan.bins + 1, sum(plan.axis_len)
    rbuf = torch.full((3 + n * nrad + 5,), -7.0, dtype=torch.float64).cuda()
    abuf = torch.full((3 + n * alen + 5,), -7.0, dtype=torch.float64).cuda()
    need = lib.sg_power_spectrum_workspace(n, d, h, w)
    ws = torch.full((need // 8 + 9,), -7.0, dtype=torch.float64).cuda()
    mats, f2, edges2 = plan.device_tables(buf.device)
    rc = lib.sg_power_spectrum(_ptr(xv), T().HIST_DT[dtype], n, d, h, w, 1.0, 0.0, _ptr(mats), _ptr(f2), _ptr(edges2), plan.bins,
                               _ptr(rbuf[3:]), _ptr(abuf[3:]), _ptr(ws), need, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    got = np.concatenate([rbuf[3:3 + n * nrad].cpu().numpy().reshape(n, nrad), abuf[3:3 + n * alen].cpu().numpy().reshape(n, alen)], 1)
    assert np.array_equal(got, want)
    for b, lo, hi in ((rbuf, 3, 3 + n * nrad), (abuf, 3, 3 + n * alen), (ws, 0, need // 8)):
        assert (torch.cat([b[:lo], b[hi:]]) == -7.0).all()
    assert (torch.cat([buf[:start], buf[start + n * vol:]]).to(torch.float32) == 7).all()
    assert np.array_equal(xv.cpu().numpy(), x.reshape(-1).numpy())


def test_limits(monkeypatch):
    from saragan_amd import _lib
    from saragan_amd._launch import _ptr, _stream
    lib = _lib.load()
    assert lib.sg_power_spectrum_max_extent() == _lib.POWER_SPECTRUM_MAX_EXTENT
    launches = []
    real = lib.sg_power_spectrum
    monkeypatch.setattr(lib, 'sg_power_spectrum', lambda *a: (launches.append(a), real(*a))[1])
    plan = T().SpectrumPlan((4, 8, 8))
    x = torch.zeros(2, 4, 8, 8, device='cuda')
    with pytest.raises(ValueError, match='extents'):
        T().SpectrumPlan((4, 8, _lib.POWER_SPECTRUM_MAX_EXTENT + 1))
    with pytest.raises(ValueError, match='bins'):
        T().SpectrumPlan((4, 8, 8), bins=0)
    with pytest.raises(ValueError, match='finite'):
        T().power_spectrum(x, plan, scale=float('nan'))
    with pytest.raises(ValueError, match='finite'):
        T().power_spectrum(x, plan, shift=float('inf'))
    radial, axes = T().power_spectrum(x[:0], plan)      # n = 0: empty results, nothing launched
    assert radial.shape == (0, 5) and [tuple(a.shape) for a in axes] == [(0, 3), (0, 5), (0, 5)] and radial.is_cuda
    assert launches == []
    # the library's own refusals, each before any launch (the outputs keep their fill)
    mats, f2, edges2 = plan.device_tables(x.device)
    out_r = torch.full((2, 5), -7.0, dtype=torch.float64, device='cuda')
    out_a = torch.full((2, 13), -7.0, dtype=torch.float64, device='cuda')
    need = lib.sg_power_spectrum_workspace(2, 4, 8, 8)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')

    def call(n=2, d=4, h=8, w=8, dt=_lib.SG_SRC_F32, scale=1.0, shift=0.0, bins=4, nbytes=need):
        return real(_ptr(x), dt, n, d, h, w, scale, shift, _ptr(mats), _ptr(f2), _ptr(edges2), bins, _ptr(out_r), _ptr(out_a),
                    _ptr(ws), nbytes, _stream())
    SG_EINVAL, SG_EWORKSPACE = -1, -2
    assert call(nbytes=need - 1) == SG_EWORKSPACE
    for kw in (dict(d=0), dict(w=_lib.POWER_SPECTRUM_MAX_EXTENT + 1), dict(bins=0), dict(bins=_lib.POWER_SPECTRUM_MAX_BINS + 1),
               dict(dt=7), dict(dt=-1), dict(scale=float('inf')), dict(shift=float('nan')), dict(n=-1)):
        assert call(**kw) == SG_EINVAL, kw
    assert call(n=0, nbytes=0) == 0
    torch.cuda.synchronize()
    assert (out_r == -7.0).all() and (out_a == -7.0).all()
    assert lib.sg_power_spectrum_workspace(0, 4, 8, 8) == 0 and lib.sg_power_spectrum_workspace(1, 4, 8, 2000) == 0
    assert call() == 0


def test_accumulator_on_the_device_is_independent_of_the_batching():
    from saragan_amd.metrics import spectrum_metrics as SPM
    shape = (8, 16, 48)
    a, b = torch.from_numpy(R.make_data(5, shape, 26)).cuda(), torch.from_numpy(R.make_data(5, shape, 27)).cuda()
    whole, parts = SPM.SpectrumAccumulator(shape, R.SPACING), SPM.SpectrumAccumulator(shape, R.SPACING)
    whole.add(a[:, None], b[:, None])      # [n, 1, d, h, w] reads as one channel
    parts.add(a[:2], b[:2])
    parts.add(a[2:], b[2:])
    assert np.array_equal(whole.real, parts.real) and np.array_equal(whole.fake, parts.fake)
    m = whole.result()
    assert m == parts.result() and all(math.isfinite(v) for v in m.values())
    same = SPM.get_spectrum_metrics(a, a.clone())
    assert same['spectrum_lsd'] == 0.0 and same['spectrum_hf_excess'] == 0.0 and same['spectrum_lsd_d'] == 0.0
