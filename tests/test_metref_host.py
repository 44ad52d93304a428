"""CPU checks of tests/metref.py, the reference that tests/test_metrics_exact_gpu.py holds the metric kernels to:
(a) it agrees with independent implementations (scipy.ndimage, oracle/metrics_oracle.py);
(b) on every input set of the GPU tests a deliberately wrong variant of it gives another answer, so a green GPU test
    could not have come from a kernel with that mistake.  Where a mistake cannot show by its own definition (a border rule
    on a one-sample line, crop0 == crop, ...) the case is named as such and at least one other case of the set must show it.
Also here, because it needs no GPU: the host-side refusal of neighbourhood centres that would read outside the volume."""
import itertools

import numpy as np
import pytest
import scipy.ndimage

from oracle import metrics_oracle as M
from tests import metref as R

BINOMIAL = (1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16)


# ---- (a) agreement -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('border,name,pad', [(0, 'mirror', 'reflect'), (1, 'reflect', 'symmetric')])
def test_border_index_is_scipys(border, name, pad):
    for n in (1, 2, 3, 7, 16):
        line = np.arange(n)
        far = 5 * n + 3
        want = np.pad(line, far, mode=pad)                  # numpy's 'reflect' / 'symmetric' are scipy's 'mirror' / 'reflect'
        got = [R.border_index(i, n, border) for i in range(-far, n + far)]
        assert got == list(want), (n, name)


@pytest.mark.parametrize('border,name', [(0, 'mirror'), (1, 'reflect')])
def test_filter_mode0_is_scipy_correlate1d(border, name):
    rng = np.random.default_rng(1)
    for n, ntaps in itertools.product((1, 2, 3, 7, 16), (1, 5, 11, 15)):
        x = rng.normal(size=(2, n, 3))
        taps = rng.normal(size=ntaps)                       # asymmetric
        want = scipy.ndimage.correlate1d(x, taps, axis=1, mode=name)
        np.testing.assert_allclose(R.filter_axis(x, taps, 0, border), want, rtol=0, atol=1e-13 * np.abs(taps).sum() * np.abs(x).max())


def _three_axes(x, mode, alpha):
    for dim in (4, 3, 2):
        sh = list(x.shape)
        outer, inner = int(np.prod(sh[:dim])), int(np.prod(sh[dim + 1:]))
        y = R.filter_axis(x.reshape(outer, sh[dim], inner), BINOMIAL, mode, R.MIRROR, alpha)
        sh[dim] = y.shape[1]
        x = y.reshape(sh)
    return x


@pytest.mark.parametrize('shape', [(2, 2, 5, 6, 7), (1, 1, 8, 16, 12)])
def test_filter_modes_1_and_2_compose_to_the_oracles_pyramid_steps(shape):
    """Integer volumes: the oracle's 5x5x5 results are exact multiples of 1/4096 (pyr_down) and 1/512 (pyr_up), so `==`."""
    x = np.random.default_rng(2).integers(-8, 9, size=shape).astype(np.float32)
    down = _three_axes(x.astype(np.float64), 1, 1.0)
    assert np.array_equal(down, M.pyr_down(x)) and np.array_equal(down * 4096, np.round(down * 4096))
    up = _three_axes(x.astype(np.float64), 2, 2.0)
    assert np.array_equal(up, M.pyr_up(x))
    assert np.array_equal(down.astype(np.float32), down) and np.array_equal(up.astype(np.float32), up)   # float32 holds them


@pytest.mark.parametrize('shape,nhood', [((2, 2, 6, 20, 20), (2, 8, 8)), ((2, 2, 6, 20, 28), (2, 8, 8)), ((3, 1, 5, 12, 17), (2, 4, 4))])
def test_gather_is_the_oracles_descriptor_draw(shape, nhood):
    x = R.gather_volume(shape)
    per_image = 7
    np.random.seed(31)
    want = M.get_descriptors_for_minibatch(x, nhood, per_image)
    np.random.seed(31)
    N = per_image * shape[0]
    D, H, W = (v // 2 for v in nhood)
    d0 = np.random.randint(D, shape[2] - D, size=N)             # the reference's draws: D, then the W centre, then the H one
    w0 = np.random.randint(W, shape[4] - W, size=N)
    h0 = np.random.randint(H, shape[3] - H, size=N)
    assert np.array_equal(R.gather(x, d0, h0, w0, per_image, D, H, W), want)


def test_gather_refuses_a_coordinate_outside_the_volume():
    x = R.gather_volume()
    with pytest.raises(IndexError):
        R.gather(x, [1, 1, 1], [3, 3, 3], [1, 5, 5], 1, 1, 2, 3)          # W centre 1 - rh 2 < 0
    with pytest.raises(IndexError):
        R.gather(x, [1, 1, 1], [8, 3, 3], [5, 5, 5], 1, 1, 2, 3)          # H centre 8 + rw 3 >= 11
    assert not R.gather_centres_in_bounds(x.shape, [1], [8], [5], 1, 2, 3)
    assert R.gather_centres_in_bounds(x.shape, [1, 5], [3, 7], [2, 10], 1, 2, 3)


def test_normalize_and_distance_are_the_oracles():
    rng = np.random.default_rng(4)
    desc = (rng.normal(size=(40, 3, 3, 5, 5)) * [[[[[2.0]]], [[[0.5]]], [[[9.0]]]]] + 3).astype(np.float32)
    want = M.finalize_descriptors(desc.copy()).reshape(desc.shape)          # float32 arithmetic
    np.testing.assert_allclose(R.normalize(desc), want, rtol=0, atol=2e-6 * np.abs(want).max())
    a, b = rng.normal(size=(50, 30)).astype(np.float32), rng.normal(size=(50, 30)).astype(np.float32)
    np.random.seed(5)
    want = M.sliced_wasserstein(a, b, 1, 20)
    np.random.seed(5)
    dirs = np.random.randn(30, 20)
    dirs = (dirs / np.sqrt(np.sum(np.square(dirs), axis=0, keepdims=True))).astype(np.float32)
    pa, pb = (R.sort_rows(R.project(m, dirs, 64).astype(np.float32)) for m in (a, b))
    assert np.isinf(pa[:, 50:]).all() and abs(R.distance(pa, pb, 50) / want - 1) < 1e-5      # float32 matmul and mean in the oracle
    np.testing.assert_allclose(R.project(a, dirs, 64)[:, :50], np.matmul(a, dirs).T, rtol=0, atol=1e-5)
    err = np.abs(np.matmul(a, dirs).T - R.project(a, dirs, 64)[:, :50])
    assert (err <= R.project_bound(a, dirs)).all()          # numpy's own float32 matmul is inside the derived bound too


def test_ssim_mean_is_the_oracles_ssim():
    rng = np.random.default_rng(6)
    r = 5
    for shape in ((14, 15), (12, 13, 12)):
        x, y = rng.normal(size=shape), rng.normal(size=shape) * 0.8 + 0.1
        filt = lambda v: scipy.ndimage.gaussian_filter(v, 1.5, truncate=3.5, mode='reflect')
        NP = 11 ** len(shape)
        C1, C2 = (0.01 * 3) ** 2, (0.03 * 3) ** 2
        s = (1,) * (3 - len(shape)) + shape
        got = R.ssim_mean(filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y), s, 1, r if len(shape) == 3 else 0, r,
                          NP / (NP - 1), C1, C2)
        want = M._ssim_single(x, y, 3)
        assert abs(float(got) - want) <= 1e-13 * max(1.0, abs(want)), (float(got), want)
    assert R.sqdiff_mean([1, 2, 3], [3, 2, 0]) == 13 / 3 and R.minmax([-3, -7, -1]) == (-7.0, -1.0)


# ---- (b) sensitivity -----------------------------------------------------------------------------------------------
def _filter_sets():
    for n, ntaps, outer, inner in itertools.product(R.FILTER_N, R.FILTER_NTAPS, R.FILTER_OUTER, R.FILTER_INNER):
        yield R.filter_input(outer, n, inner), R.filter_taps(ntaps)
    outer, n, inner, ntaps, _, _ = R.FILTER_WRAP
    yield R.filter_input(outer, n, inner), R.filter_taps(ntaps)


def test_filter_inputs_tell_the_border_rules_and_the_tap_order_apart():
    """A mistake that cannot show on a shape at all (one tap; a one-sample line; the mirrored lines of two or three samples,
    which are symmetric about every sample that modes 0 and 1 visit, so both tap orders agree) is recognised by trying it on
    generic real-valued data of the same shape: where it changes nothing there, it is the same function.  Everywhere else
    the GPU test's own integers must show it."""
    rng = np.random.default_rng(9)
    shown = {'border': 0, 'taps': 0}
    same = {'border': set(), 'taps': set()}
    for x, taps in _filter_sets():
        n, ntaps = x.shape[1], len(taps)
        generic = rng.normal(size=x.shape) if x.size < 10 ** 5 else None
        for mode, border in itertools.product((0, 1, 2), (0, 1)) if generic is not None else [R.FILTER_WRAP[4:]]:
            want = R.filter_axis(x, taps, mode, border)
            for what, args in (('border', (taps, mode, 1 - border)), ('taps', (taps[::-1], mode, border))):
                if generic is not None and np.allclose(R.filter_axis(generic, *args), R.filter_axis(generic, taps, mode, border),
                                                       rtol=1e-12, atol=1e-12):
                    same[what].add((n, ntaps, mode, border))
                    continue
                assert not np.array_equal(R.filter_axis(x, *args), want), (what, n, ntaps, mode, border, x.shape)
                shown[what] += 1
    assert all(n == 1 or ntaps == 1 for n, ntaps, _, _ in same['border']), same['border']
    assert all(n <= 3 or ntaps == 1 for n, ntaps, _, _ in same['taps']), same['taps']
    assert min(shown.values()) > 400, shown             # of 6 * 120 + 1 cases


def _gather_sets():
    x = R.gather_volume()
    for (rd, rh, rw), per_image in itertools.product(R.GATHER_RADII, R.GATHER_PER_IMAGE):
        for d0, h0, w0 in R.gather_calls(x.shape[0], per_image, R.gather_centres(x.shape, rd, rh, rw)):
            yield x, d0, h0, w0, per_image, rd, rh, rw
    w = R.GATHER_WRAP
    d0, h0, w0 = R.gather_wrap_centres()
    yield (R.gather_volume(w['shape']), d0, h0, w0, w['per_image']) + w['radii']


def _gather_flat(x, d0, h0, w0, per_image, rd, rh, rw, swap_strides=False, other_axis=False):
    """The gather by flat addresses (wrapping past the end, as memory would not), with one of two mistakes."""
    n_img, c, d, h, w = x.shape
    nh, ch, i, j, k = np.ogrid[0:len(d0), 0:c, -rd:rd + 1, -rh:rh + 1, -rw:rw + 1]
    r5 = lambda v: np.asarray(v).reshape(-1, 1, 1, 1, 1)
    dd = r5(d0) + i
    hh, ww = (r5(h0) + j, r5(w0) + k) if other_axis else (r5(h0) + k, r5(w0) + j)
    base = ((nh // per_image) * c + ch) * d + dd
    idx = (base * w + hh) * h + ww if swap_strides else (base * h + hh) * w + ww
    return np.take(x.reshape(-1), idx, mode='wrap')


def test_gather_inputs_tell_the_strides_and_the_offset_axes_apart():
    calls = 0
    for args in _gather_sets():
        want = R.gather(*args)
        assert R.gather_centres_in_bounds(args[0].shape, *args[1:4], *args[5:])
        assert np.array_equal(_gather_flat(*args), want)                       # the helper itself is right without a mistake
        assert not np.array_equal(_gather_flat(*args, swap_strides=True), want), args[4:]
        rd, rh, rw = args[5:]
        if rh == rw == 0:
            assert np.array_equal(_gather_flat(*args, other_axis=True), want)  # no H / W offsets at all: nothing to attach
        else:
            assert not np.array_equal(_gather_flat(*args, other_axis=True), want), args[4:]
        calls += 1
    assert calls >= 3 * (4 + 1) + 1


def _normalize_without_modulo(desc):
    """channel = e / inner without % c: past the first image it names channels that do not exist (no statistics: the value
    stays as it is)."""
    desc = np.asarray(desc, dtype=np.float64)
    n, c, inner = desc.shape
    out = desc.copy()
    out[0] = R.normalize(desc)[0]
    return out


@pytest.mark.parametrize('shape', R.NORMALIZE_SHAPES + (R.NORMALIZE_WRAP,))
def test_normalize_inputs_tell_the_channel_index_apart(shape):
    for desc in (R.normalize_exact_input(*shape)[0],) + ((R.normalize_float_input(*shape),) if shape != R.NORMALIZE_WRAP else ()):
        want = R.normalize(desc)
        assert not np.array_equal(_normalize_without_modulo(desc), want)
    desc, sign = R.normalize_exact_input(*shape)
    assert np.array_equal(R.normalize(desc), sign)           # the exact case's mean and std are exact in the reference


def test_distance_inputs_tell_the_divisor_apart():
    for rows, n, npad in R.DISTANCE_CASES:
        pa, pb = R.distance_input(rows, n, npad)
        want = R.distance(pa, pb, n)
        assert n != npad and want > 0
        assert want * n / npad != want                       # rows * npad as the divisor
        rs = R.distance_rows(pa, pb, n)
        assert np.array_equal(rs * 8, np.round(rs * 8)) and rs.max() < 2 ** 40        # dyadic: every order sums alike


@pytest.mark.parametrize('case', R.SSIM_CASES[:3] + ((6, 14, 13, 1, 1, 5),))
def test_ssim_inputs_tell_the_crop_box_apart(case):
    """(The 40 x 90 x 90 case is the same generator as (6, 14, 13, 1, 1, 5), at a size where 30 exact means are affordable.)"""
    s0, s1, s2, c, crop0, crop = case
    mom = R.ssim_moments(s0, s1, s2, c)
    lo, hi = [crop0, crop, crop], [s0 - crop0, s1 - crop, s2 - crop]

    def mean(lo_, hi_):
        total, _, count = R.ssim_box_sums(*mom, (s0, s1, s2), c, lo_, hi_, *R.SSIM_CONST)
        return total / count if count else None

    want = mean(lo, hi)
    assert want == R.ssim_mean(*mom, (s0, s1, s2), c, crop0, crop, *R.SSIM_CONST)
    for axis, (face, step) in itertools.product(range(3), (('lo', 1), ('lo', -1), ('hi', 1), ('hi', -1))):
        lo_, hi_ = list(lo), list(hi)
        (lo_ if face == 'lo' else hi_)[axis] += step
        if lo_[axis] < 0 or hi_[axis] > (s0, s1, s2)[axis]:
            continue                                         # that face is the volume's own: nothing lies outside it
        assert mean(lo_, hi_) != want, (axis, face, step)
    if crop0 != crop:
        assert mean([crop0] * 3, [s0 - crop0, s1 - crop0, s2 - crop0]) != want      # crop0 on every axis
        if min(s0, s1, s2) > 2 * crop:
            assert mean([crop] * 3, [s0 - crop, s1 - crop, s2 - crop]) != want      # crop on every axis


def test_ssim_cases_include_unequal_crops():
    assert sum(1 for c in R.SSIM_CASES if c[4] != c[5]) >= 2


# ---- the out-of-bounds neighbourhoods ------------------------------------------------------------------------------
def test_descriptor_centres_outside_the_volume_are_refused_on_the_host():
    """nhood_size (2, 8, 4): the reference draws the W centre from [2, w - 2) but moves it by +-4 (its fourth-axis offsets).
    numpy would wrap or raise; a kernel would read foreign memory.  The wrapper refuses before it uploads or launches
    anything (this test runs without a GPU), after exactly the reference's three draws."""
    from saragan_amd.metrics import swd as G
    x = np.zeros((2, 1, 4, 12, 12), dtype=np.float32)
    np.random.seed(12)
    with pytest.raises(ValueError, match='nhood_size'):
        G.get_descriptors_for_minibatch(x, (2, 8, 4), 16)
    after = np.random.get_state()
    np.random.seed(12)
    d0 = np.random.randint(1, 4 - 1, size=(32, 1, 1, 1, 1))
    w0 = np.random.randint(2, 12 - 2, size=(32, 1, 1, 1, 1))
    h0 = np.random.randint(4, 12 - 4, size=(32, 1, 1, 1, 1))
    want = np.random.get_state()
    assert after[0] == want[0] and np.array_equal(after[1], want[1]) and after[2:] == want[2:]
    assert not R.gather_centres_in_bounds(x.shape, d0, h0, w0, 1, 4, 2)       # these very draws do leave the volume
    np.random.seed(12)
    with pytest.raises(ValueError, match='nhood_size'):
        G.get_descriptors_for_minibatch(x, (2, 4, 8), 16)         # the mirrored case, on H
