"""Every kernel of csrc/metrics.hip against the plain reference tests/metref.py, branch by branch, through the C ABI.
Small integers and dyadic taps make every float64 accumulation and every float32 store exact in any order, so those cases
compare with `==` (np.array_equal): a dropped, doubled or misplaced element cannot hide.  The float cases carry a bound
computed by a metref helper whose docstring derives it; they print measured error / bound.  No tolerance here is a literal,
but for get_ssim against the oracle at the end, held to the tolerance tests/test_metrics.py holds it to.
The inputs come from tests/metref.py, where tests/test_metref_host.py shows on the CPU that each of them tells the
reference from its deliberately wrong variants."""
import ctypes as C
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import metrics_oracle as M
from tests import metref as R

pytestmark = pytest.mark.gpu
SG_EINVAL, SG_EWORKSPACE = -1, -2
SENTINEL = -7.0


def _lib():
    from saragan_amd import _lib
    return _lib.load()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a).astype(dtype))
    return torch.as_tensor(a).to('cuda')


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _taps_c(taps):
    return (C.c_double * len(taps))(*[float(t) for t in taps])


# ---- sg_filter_axis ------------------------------------------------------------------------------------------------
FILTER_TYPES = {0: (np.float32, np.float32), 1: (np.float64, np.float64), 2: (np.float32, np.float64), 3: (np.float64, np.float32)}


@pytest.mark.parametrize('mode', (0, 1, 2))
@pytest.mark.parametrize('f64', (0, 1, 2, 3), ids=('f32', 'f64', 'f32_to_f64', 'f64_to_f32'))
def test_filter_axis_every_branch_exact(f64, mode):
    """border x ntaps x n x outer x inner x alpha x add, the full product (1920 launches per instantiation and mode)."""
    lib, st = _lib(), _st()
    dt_in, dt = FILTER_TYPES[f64]
    combos = list(itertools.product((R.MIRROR, R.REFLECT), R.FILTER_NTAPS, R.FILTER_ALPHA, (False, True)))
    for outer, n, inner in itertools.product(R.FILTER_OUTER, R.FILTER_N, R.FILTER_INNER):
        x = R.filter_input(outer, n, inner)
        n_out = R.filter_n_out(n, mode)
        add = R.filter_add((outer, n_out, inner))
        xd, addd = _dev(x, dt_in), _dev(add, dt)
        y = torch.full((len(combos), outer, n_out, inner), SENTINEL, dtype=addd.dtype, device='cuda')
        keep = []
        for i, (border, ntaps, alpha, with_add) in enumerate(combos):
            keep.append(_taps_c(R.filter_taps(ntaps)))
            rc = lib.sg_filter_axis(_p(xd), _p(y[i]), _p(addd) if with_add else None, outer, n, inner, keep[-1], ntaps, mode,
                                    border, alpha, f64, st)
            assert rc == 0, (rc, border, ntaps, alpha, with_add)
        got = _host(y)
        base = {}
        for i, (border, ntaps, alpha, with_add) in enumerate(combos):
            if (border, ntaps) not in base:
                base[border, ntaps] = R.filter_axis(x, R.filter_taps(ntaps), mode, border)
            want = alpha * base[border, ntaps] + (add if with_add else 0.0)
            assert np.array_equal(want.astype(np.float32).astype(np.float64), want)        # float32 holds the exact value
            assert got[i].dtype == dt and np.array_equal(got[i], want), \
                (outer, n, inner, border, ntaps, alpha, with_add, np.argwhere(got[i] != want)[:5])


def test_filter_axis_grid_stride_wrap():
    outer, n, inner, ntaps, mode, border = R.FILTER_WRAP
    assert outer * n * inner > 16384 * 256
    x, taps = R.filter_input(outer, n, inner), R.filter_taps(ntaps)
    xd = _dev(x, np.float32)
    y = torch.full((outer, n, inner), SENTINEL, dtype=torch.float32, device='cuda')
    assert _lib().sg_filter_axis(_p(xd), _p(y), None, outer, n, inner, _taps_c(taps), ntaps, mode, border, 1.0, 0, _st()) == 0
    got, want = _host(y), R.filter_axis(x, taps, mode, border)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_filter_axis_refusals_leave_the_output_untouched():
    lib, st = _lib(), _st()
    x = _dev(np.ones((2, 6, 3)), np.float32)
    y = torch.full((2, 12, 3), SENTINEL, dtype=torch.float32, device='cuda')
    taps = _taps_c([1 / 64] * 17)
    good = dict(x=_p(x), y=_p(y), outer=2, n=6, inner=3, ntaps=5, mode=0, border=0, f64=0)
    bad = [dict(ntaps=4), dict(ntaps=2), dict(ntaps=17), dict(ntaps=0), dict(mode=3), dict(mode=-1), dict(border=2),
           dict(border=-1), dict(y=_p(x)), dict(n=0), dict(n=-1), dict(outer=0), dict(inner=0), dict(x=None), dict(y=None),
           dict(f64=4), dict(f64=-1)]
    for change in bad:
        k = dict(good, **change)
        rc = lib.sg_filter_axis(k['x'], k['y'], None, k['outer'], k['n'], k['inner'], taps, k['ntaps'], k['mode'], k['border'],
                                1.0, k['f64'], st)
        assert rc == SG_EINVAL, (change, rc)
    assert lib.sg_filter_axis(_p(x), _p(y), None, 2, 6, 3, None, 5, 0, 0, 1.0, 0, st) == SG_EINVAL      # taps == NULL
    assert bool((_host(y) == SENTINEL).all()) and bool((_host(x) == 1.0).all())


# ---- the pyramid wrappers ------------------------------------------------------------------------------------------
def _int_volume(shape, amp, seed=3):
    return np.random.default_rng(seed).integers(-amp, amp + 1, size=shape).astype(np.float32)


@pytest.mark.parametrize('shape', [(2, 2, 5, 6, 7), (1, 1, 8, 16, 12)])
def test_pyr_down_and_pyr_up_equal_the_oracle(shape):
    """Integers |x| <= 8: every pass's values are multiples of 1/16, 1/256, 1/4096 (1/8, 1/64, 1/512 for pyr_up) below 16."""
    from saragan_amd.metrics import swd as G
    x = _int_volume(shape, 8)
    for got, want in ((G.pyr_down(x), M.pyr_down(x)), (G.pyr_up(x), M.pyr_up(x))):
        got = _host(got)
        assert got.shape == want.shape and np.array_equal(got, want), np.argwhere(got != want)[:5]


def _oracle_reconstruct(pyramid):
    """swd.py:85-89 on the oracle's pyr_up."""
    minibatch = pyramid[-1]
    for level in pyramid[-2::-1]:
        minibatch = M.pyr_up(minibatch) + level
    return minibatch


@pytest.mark.parametrize('shape', [(2, 2, 4, 8, 12), (1, 1, 8, 16, 12)])
def test_laplacian_pyramid_of_two_levels_equals_the_oracle(shape):
    """Integers |x| <= 2: pyr_down gives multiples of 2^-12 below 2, pyr_up of those multiples of 2^-21 below 2, the level
    difference multiples of 2^-21 below 4: 24 bits at the most, nothing rounds, on either side.  The reconstruction returns
    the integers themselves."""
    from saragan_amd.metrics import swd as G
    x = _int_volume(shape, 2)
    got, want = G.generate_laplacian_pyramid(x, 2), M.generate_laplacian_pyramid(x.copy(), 2)
    assert len(got) == len(want) == 2
    for g, w in zip(got, want):
        assert np.array_equal(_host(g), w), np.argwhere(_host(g) != w)[:5]
    back = _host(G.reconstruct_laplacian_pyramid([_dev(w) for w in want]))
    assert np.array_equal(back, _oracle_reconstruct(want)) and np.array_equal(back, x)


def test_laplacian_pyramid_needs_extents_that_halve_evenly():
    """(2, 2, 5, 6, 7) has no Laplacian pyramid: pyr_up(pyr_down(x)) is 6 x 6 x 8.  The oracle and the wrapper both refuse."""
    from saragan_amd.metrics import swd as G
    x = _int_volume((2, 2, 5, 6, 7), 2)
    with pytest.raises(ValueError):
        M.generate_laplacian_pyramid(x.copy(), 3)
    with pytest.raises(AssertionError):
        G.generate_laplacian_pyramid(x, 3)


@pytest.mark.parametrize('shape', [(1, 1, 8, 16, 12), (2, 2, 8, 4, 12)])
def test_laplacian_pyramid_of_three_levels_equals_the_oracle(shape):
    """The coarsest level, pyr_down twice, is a multiple of 2^-24 below 2: 25 bits, it rounds; pyr_up of it rounds again.
    The oracle convolves 5 x 5 x 5 in float64, rounds to float32 once and subtracts in float32.  The wrapper's separable
    passes keep float64 between them (exact here: 24 + 12 bits), round once and add in float32: the same bits.  (With
    float32 between the passes, as this wrapper first had it, 15 of the 192 level-1 elements of (1, 1, 8, 16, 12) and 50 of
    the 1536 reconstructed ones were one float32 ulp off; this test found that.)"""
    from saragan_amd.metrics import swd as G
    x = _int_volume(shape, 2)
    got, want = G.generate_laplacian_pyramid(x, 3), M.generate_laplacian_pyramid(x.copy(), 3)
    assert len(got) == len(want) == 3
    for lv, (g, w) in enumerate(zip(got, want)):
        g = _host(g)
        assert g.dtype == np.float32 and np.array_equal(g, w), (lv, int((g != w).sum()), w.size)
    back, wback = _host(G.reconstruct_laplacian_pyramid([_dev(w) for w in want])), _oracle_reconstruct(want)
    assert np.array_equal(back, wback), (int((back != wback).sum()), wback.size)


# ---- sg_swd_gather -------------------------------------------------------------------------------------------------
def _gather(x, d0, h0, w0, per_image, rd, rh, rw, xd=None):
    n_img, c, d, h, w = x.shape
    xd = _dev(x) if xd is None else xd
    cd, chh, cw = (_dev(v, np.int32) for v in (d0, h0, w0))
    out = torch.full((n_img * per_image, c, 2 * rd + 1, 2 * rh + 1, 2 * rw + 1), SENTINEL, dtype=torch.float32, device='cuda')
    assert R.gather_centres_in_bounds(x.shape, d0, h0, w0, rd, rh, rw)              # never launched with centres that read outside
    rc = _lib().sg_swd_gather(_p(xd), _p(out), _p(cd), _p(chh), _p(cw), n_img, c, d, h, w, per_image, rd, rh, rw, _st())
    assert rc == 0, rc
    return _host(out)


@pytest.mark.parametrize('per_image', R.GATHER_PER_IMAGE)
@pytest.mark.parametrize('radii', R.GATHER_RADII)
def test_gather_hand_placed_centres_exact(radii, per_image):
    """H != W, rh != rw, every centre combination that touches a border of the volume."""
    x = R.gather_volume()
    xd = _dev(x)
    calls = list(R.gather_calls(x.shape[0], per_image, R.gather_centres(x.shape, *radii)))
    assert len(calls) * x.shape[0] * per_image >= 12
    for d0, h0, w0 in calls:
        got, want = _gather(x, d0, h0, w0, per_image, *radii, xd=xd), R.gather(x, d0, h0, w0, per_image, *radii)
        assert np.array_equal(got, want), (radii, per_image, np.argwhere(got != want)[:5])


def test_gather_grid_stride_wrap():
    w = R.GATHER_WRAP
    x = R.gather_volume(w['shape'])
    d0, h0, w0 = R.gather_wrap_centres()
    got = _gather(x, d0, h0, w0, w['per_image'], *w['radii'])
    assert got.size > 16384 * 256
    want = R.gather(x, d0, h0, w0, w['per_image'], *w['radii'])
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_gather_refusals():
    lib, st = _lib(), _st()
    x = _dev(R.gather_volume())
    n_img, c, d, h, w = R.GATHER_SHAPE
    cen = _dev(np.full(n_img, 5), np.int32)
    out = torch.full((n_img, c, 9, 13, 13), SENTINEL, dtype=torch.float32, device='cuda')
    good = dict(x=_p(x), out=_p(out), d0=_p(cen), h0=_p(cen), w0=_p(cen), n_img=n_img, c=c, per_image=1, rd=0, rh=0, rw=0)
    bad = [dict(rd=4),                 # 2 * 4 + 1 > d = 7
           dict(rh=7),                 # the W extent carries the 2 rh + 1 offsets: 15 > w = 13  (rh = 6 fits: 13)
           dict(rw=6),                 # the H extent carries the 2 rw + 1 offsets: 13 > h = 11  (rw = 5 fits: 11)
           dict(x=None), dict(out=None), dict(d0=None), dict(h0=None), dict(w0=None), dict(per_image=0), dict(n_img=0),
           dict(c=0), dict(rd=-1), dict(rh=-1), dict(rw=-1)]
    for change in bad:
        k = dict(good, **change)
        rc = lib.sg_swd_gather(k['x'], k['out'], k['d0'], k['h0'], k['w0'], k['n_img'], k['c'], d, h, w, k['per_image'], k['rd'],
                               k['rh'], k['rw'], st)
        assert rc == SG_EINVAL, (change, rc)
    assert bool((_host(out) == SENTINEL).all())
    # the largest radii that fit are accepted (centres at the only legal position: the middle)
    mid = [np.full(n_img, v) for v in (3, 5, 6)]
    got = _gather(R.gather_volume(), *mid, 1, 3, 6, 5)
    assert np.array_equal(got, R.gather(R.gather_volume(), *mid, 1, 3, 6, 5))


def test_descriptors_wrapper_on_a_volume_with_h_not_w():
    from saragan_amd.metrics import swd as G
    x = np.random.default_rng(2).normal(size=(2, 2, 6, 20, 28)).astype(np.float32)
    np.random.seed(3)
    want = M.get_descriptors_for_minibatch(x, (2, 8, 8), 16)
    np.random.seed(3)
    got = _host(G.get_descriptors_for_minibatch(x, (2, 8, 8), 16))
    assert np.array_equal(got, want)


# ---- sg_sort_rows --------------------------------------------------------------------------------------------------
SORT_KINDS = ('random', 'sorted', 'reversed', 'equal', 'ties', 'inf', 'zeros')


def _sort_content(kind, rng, npad):
    v = rng.standard_normal(npad).astype(np.float32)
    if kind == 'sorted':
        v = np.sort(v)
    elif kind == 'reversed':
        v = np.sort(v)[::-1].copy()
    elif kind == 'equal':
        v[:] = 0.25
    elif kind == 'ties':
        v = rng.integers(0, max(npad // 2, 1), size=npad).astype(np.float32)
    elif kind == 'inf':
        v[rng.integers(0, npad, size=npad // 8 + 1)] = np.inf
        v[rng.integers(0, npad, size=npad // 8 + 1)] = -np.inf
    elif kind == 'zeros':
        v = rng.choice(np.array([0.0, -0.0, 1.0, -1.0], dtype=np.float32), size=npad)
    return v


@pytest.mark.parametrize('npad', (2, 4, 32, 64, 2048, 4096, 8192, 32768))
def test_sort_rows_equals_np_sort(npad):
    """Fewer pairs than threads (2 .. 32), one LDS chunk (<= 4096), one global stride (8192), three (32768); one and three
    rows of every content."""
    lib, st = _lib(), _st()
    rng = np.random.default_rng(npad)
    for rows, kind in itertools.product((1, 3), SORT_KINDS):
        v = np.stack([_sort_content(kind, rng, npad) for _ in range(rows)])
        buf = _dev(v)
        assert lib.sg_sort_rows(_p(buf), rows, npad, st) == 0
        got, want = _host(buf), R.sort_rows(v)
        assert np.array_equal(got, want), (rows, kind, np.argwhere(got != want)[:5])
        if kind == 'zeros':                                     # -0.0 == 0.0: also nothing but the input's values came back
            assert np.array_equal(np.sort(got.view(np.uint32), axis=1), np.sort(v.view(np.uint32), axis=1))


def test_sort_rows_global_pass_wrap():
    """520 rows of 65536: 17 039 360 pairs > 65536 * 256, the second trip of bitonic_global_kernel's loop.  Row r is the
    permutation i -> (odd_r * i + r) mod 65536 of 0 .. 65535, so every sorted row is 0 .. 65535."""
    rows, npad = 520, 65536
    assert rows * npad // 2 > 65536 * 256
    i = np.arange(npad, dtype=np.uint32)[None, :]
    r = np.arange(rows, dtype=np.uint32)[:, None]
    v = (((2 * r + 1) * np.uint32(40503) * i + r * np.uint32(977)) & np.uint32(npad - 1)).astype(np.float32)
    assert np.array_equal(np.sort(v[517]), np.arange(npad, dtype=np.float32))
    buf = _dev(v)
    assert _lib().sg_sort_rows(_p(buf), rows, npad, _st()) == 0
    want = torch.arange(npad, dtype=torch.float32, device='cuda').expand(rows, npad)
    wrong = torch.nonzero(buf != want)
    assert wrong.numel() == 0, wrong[:5].tolist()


@pytest.mark.parametrize('npad', (64, 8192))
def test_sort_rows_with_a_nan_returns_a_permutation(npad):
    rng = np.random.default_rng(5)
    v = rng.standard_normal((3, npad)).astype(np.float32)
    v[1, npad // 3] = np.nan
    buf = _dev(v)
    assert _lib().sg_sort_rows(_p(buf), 3, npad, _st()) == 0
    got = _host(buf)
    assert np.array_equal(np.sort(got.view(np.uint32), axis=1), np.sort(v.view(np.uint32), axis=1))
    assert np.array_equal(got[[0, 2]], np.sort(v[[0, 2]], axis=1))              # the other rows are untouched by it


def test_sliced_wasserstein_of_a_nan_is_not_finite():
    from saragan_amd.metrics import swd as G
    rng = np.random.default_rng(6)
    a, b = rng.standard_normal((100, 27)).astype(np.float32), rng.standard_normal((100, 27)).astype(np.float32)
    np.random.seed(1)
    assert np.isfinite(G.sliced_wasserstein(a, b, 1, 16))
    a[40, 3] = np.nan
    np.random.seed(1)
    assert not np.isfinite(G.sliced_wasserstein(a, b, 1, 16))


def test_sort_rows_refusals():
    lib, st = _lib(), _st()
    buf = torch.full((3, 64), SENTINEL, dtype=torch.float32, device='cuda')
    buf[:, ::2] = 1.0
    before = _host(buf).copy()
    for rows, npad in ((3, 1), (3, 48), (0, 64), (-1, 64), (3, 0), (3, 96)):
        assert lib.sg_sort_rows(_p(buf), rows, npad, st) == SG_EINVAL, (rows, npad)
    assert lib.sg_sort_rows(None, 3, 64, st) == SG_EINVAL
    assert np.array_equal(_host(buf), before)


# ---- sg_swd_project ------------------------------------------------------------------------------------------------
PROJECT_N, PROJECT_F, PROJECT_NDIRS = (1, 63, 64, 65, 333), (1, 15, 16, 17, 243), (1, 63, 64, 65, 130)


@pytest.mark.parametrize('n', PROJECT_N)
def test_project_integer_inputs_exact(n):
    """One below, at and above the 64 x 64 tile and the 16-deep K step.  Integers in [-3, 3]: 9 f < 2^24."""
    lib, st = _lib(), _st()
    npad = lib.sg_swd_padded_rows(n)
    assert npad >= max(n, 64) and npad & (npad - 1) == 0 and (npad == 64 or npad < 2 * n)
    for f, ndirs in itertools.product(PROJECT_F, PROJECT_NDIRS):
        assert 9 * f < 2 ** 24
        rng = np.random.default_rng(n * 1000 + f * 10 + ndirs)
        a = rng.integers(-3, 4, size=(n, f)).astype(np.float32)
        dirs = rng.integers(-3, 4, size=(f, ndirs)).astype(np.float32)
        pt = torch.full((ndirs, npad), SENTINEL, dtype=torch.float32, device='cuda')
        ad, dd = _dev(a), _dev(dirs)
        assert lib.sg_swd_project(_p(ad), _p(dd), _p(pt), n, f, ndirs, npad, st) == 0
        got, want = _host(pt), R.project(a, dirs, npad)
        assert np.array_equal(got, want), (n, f, ndirs, np.argwhere(got != want)[:5])
        assert np.isposinf(got[:, n:]).all()


def test_project_float_inputs_within_the_fma_chain_bound():
    lib, st = _lib(), _st()
    n, f, ndirs = 333, 243, 70
    rng = np.random.default_rng(12)
    a = rng.standard_normal((n, f)).astype(np.float32)
    dirs = rng.standard_normal((f, ndirs))
    dirs = (dirs / np.sqrt((dirs * dirs).sum(axis=0, keepdims=True))).astype(np.float32)
    npad = lib.sg_swd_padded_rows(n)
    pt = torch.empty((ndirs, npad), dtype=torch.float32, device='cuda')
    ad, dd = _dev(a), _dev(dirs)
    assert lib.sg_swd_project(_p(ad), _p(dd), _p(pt), n, f, ndirs, npad, st) == 0
    got = _host(pt)
    err = np.abs(got[:, :n] - R.project(a, dirs, npad)[:, :n])
    bound = R.project_bound(a, dirs)
    print(f'swd_project ({n}, {f}, {ndirs}): max error / bound = {(err / bound).max():.3e} (gamma_f = {R.gamma(f):.3e})')
    assert (err <= bound).all() and np.isposinf(got[:, n:]).all()


def test_project_refusals():
    lib, st = _lib(), _st()
    a, dirs = _dev(np.ones((70, 5)), np.float32), _dev(np.ones((5, 3)), np.float32)
    pt = torch.full((3, 128), SENTINEL, dtype=torch.float32, device='cuda')
    assert lib.sg_swd_padded_rows(70) == 128
    for npad in (64, 70, 127, 256):
        assert lib.sg_swd_project(_p(a), _p(dirs), _p(pt), 70, 5, 3, npad, st) == SG_EINVAL, npad
    for args in ((None, _p(dirs), _p(pt), 70, 5, 3), (_p(a), None, _p(pt), 70, 5, 3), (_p(a), _p(dirs), None, 70, 5, 3),
                 (_p(a), _p(dirs), _p(pt), 0, 5, 3), (_p(a), _p(dirs), _p(pt), 70, 0, 3), (_p(a), _p(dirs), _p(pt), 70, 5, 0)):
        assert lib.sg_swd_project(*args, 128, st) == SG_EINVAL, args[3:]
    assert bool((_host(pt) == SENTINEL).all())


# ---- sg_swd_distance -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows,n,npad', R.DISTANCE_CASES)
def test_distance_dyadic_rows_exact(rows, n, npad):
    """n below, at and above one trip of the 256 threads; rows > 256 is the second trip of sum_final_kernel's loop."""
    pa, pb = R.distance_input(rows, n, npad)
    out = torch.full((1 + rows,), SENTINEL, dtype=torch.float64, device='cuda')
    pad, pbd = _dev(pa), _dev(pb)
    assert _lib().sg_swd_distance(_p(pad), _p(pbd), _p(out), rows, n, npad, _st()) == 0
    got = _host(out)
    assert np.array_equal(got[1:], R.distance_rows(pa, pb, n))
    assert got[0] == R.distance(pa, pb, n), (got[0], R.distance(pa, pb, n))


def test_distance_refusals():
    lib, st = _lib(), _st()
    pa = _dev(np.zeros((2, 64)), np.float32)
    out = torch.full((3,), SENTINEL, dtype=torch.float64, device='cuda')
    for args in ((None, _p(pa), _p(out), 2, 10, 64), (_p(pa), None, _p(out), 2, 10, 64), (_p(pa), _p(pa), None, 2, 10, 64),
                 (_p(pa), _p(pa), _p(out), 0, 10, 64), (_p(pa), _p(pa), _p(out), 2, 0, 64), (_p(pa), _p(pa), _p(out), 2, 65, 64)):
        assert lib.sg_swd_distance(*args, st) == SG_EINVAL, args[3:]
    assert bool((_host(out) == SENTINEL).all())


# ---- sg_desc_normalize ---------------------------------------------------------------------------------------------
def _normalize(desc, nbytes=None, n=None, c=None, inner=None, null=()):
    lib = _lib()
    n0, c0, inner0 = desc.shape
    need = lib.sg_desc_normalize_workspace(c0)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    dd = _dev(desc)
    rc = lib.sg_desc_normalize(None if 'desc' in null else _p(dd), n0 if n is None else n, c0 if c is None else c,
                               inner0 if inner is None else inner, None if 'ws' in null else _p(ws),
                               need if nbytes is None else nbytes, _st())
    return rc, _host(dd), need


@pytest.mark.parametrize('shape', R.NORMALIZE_SHAPES + (R.NORMALIZE_WRAP,))
def test_normalize_exact_case(shape):
    """m +- s in equal numbers, s a power of two: sums, mean, variance and 1 / std are exact, the output is +-1 exactly.
    (1536, 2, 243) has 373 248 values per channel: past the 256 blocks of 256 of desc_stats_kernel's grid; (8700, 2, 243)
    has 4 228 200 elements: past the 16384 blocks of 256 of desc_normalize_kernel's."""
    desc, sign = R.normalize_exact_input(*shape)
    rc, got, _ = _normalize(desc)
    assert rc == 0 and np.array_equal(got, sign), np.argwhere(got != sign)[:5]
    assert np.array_equal(R.normalize(desc), sign)


@pytest.mark.parametrize('shape', R.NORMALIZE_SHAPES)
def test_normalize_float_case_within_the_derived_bound(shape):
    desc = R.normalize_float_input(*shape)
    rc, got, _ = _normalize(desc)
    assert rc == 0
    want = R.normalize(desc)
    bound = R.normalize_bound(desc, want)
    err = np.abs(got.astype(np.float64) - want)
    print(f'desc_normalize {shape}: max error / bound = {(err / bound).max():.3e}, max error / (2^-24 |want|) = '
          f'{(err / (R.U32 * np.maximum(np.abs(want), 1e-30))).max():.3e}')
    assert (err <= bound).all()


def test_normalize_refusals():
    desc, _ = R.normalize_exact_input(300, 3, 45)
    rc, got, need = _normalize(desc, nbytes=_lib().sg_desc_normalize_workspace(3) - 1)
    assert rc == SG_EWORKSPACE and np.array_equal(got, desc) and need == (256 * 3 * 2 + 2 * 3) * 8
    for kw in (dict(null=('desc',)), dict(null=('ws',)), dict(n=0), dict(c=0), dict(inner=0)):
        rc, got, _ = _normalize(desc, **kw)
        assert rc == SG_EINVAL and np.array_equal(got, desc), kw


# ---- sg_sqdiff_mean / sg_minmax / sg_ssim_products -----------------------------------------------------------------
REDUCE_NUMEL = (1, 255, 256, 257, 2047, 2048, 2049, 600001)          # around one wave trip, one block's 2048, the 1024-block cap


def _workspace():
    nbytes = _lib().sg_metric_workspace()
    return torch.empty(nbytes, dtype=torch.uint8, device='cuda'), nbytes


@pytest.mark.parametrize('numel', REDUCE_NUMEL)
def test_sqdiff_mean_and_minmax_exact(numel):
    lib, st = _lib(), _st()
    ws, nbytes = _workspace()
    rng = np.random.default_rng(numel)
    a, b = rng.integers(-8, 9, size=numel).astype(np.float64), rng.integers(-8, 9, size=numel).astype(np.float64)
    out = torch.full((2,), SENTINEL, dtype=torch.float64, device='cuda')
    ad, bd = _dev(a), _dev(b)
    assert lib.sg_sqdiff_mean(_p(ad), _p(bd), _p(out), numel, _p(ws), nbytes, st) == 0
    got = _host(out)
    assert got[0] == R.sqdiff_mean(a, b) and got[1] == SENTINEL, (got, R.sqdiff_mean(a, b))
    last_block = (numel - 1) // 256 * 256 + ((numel - 1) % 256) // 2          # inside the last, partly filled, 256-thread trip
    positions = sorted({0, numel - 1, last_block})
    pairs = list(itertools.permutations(positions, 2)) if len(positions) > 1 else [(0, 0)]
    for data, (ilo, ihi) in itertools.product((a, -np.abs(a) - 1.0), pairs):      # mixed signs; negative only
        v = data.copy()
        if ilo != ihi:
            v[ilo], v[ihi] = -100.0, (100.0 if data is a else -0.5)
        vd = _dev(v)
        assert lib.sg_minmax(_p(vd), _p(out), numel, _p(ws), nbytes, st) == 0
        got = tuple(_host(out).tolist())
        assert got == R.minmax(v), (numel, ilo, ihi, got, R.minmax(v))
        if ilo != ihi:
            assert got == (v[ilo], v[ihi])


def test_ssim_products_exact():
    lib, st = _lib(), _st()
    for numel in (1, 257, 70001):
        rng = np.random.default_rng(numel)
        x, y = rng.integers(-8, 9, size=numel).astype(np.float64), rng.integers(-8, 9, size=numel).astype(np.float64)
        outs = [torch.full((numel,), SENTINEL, dtype=torch.float64, device='cuda') for _ in range(3)]
        xd, yd = _dev(x), _dev(y)
        assert lib.sg_ssim_products(_p(xd), _p(yd), *(_p(o) for o in outs), numel, st) == 0
        for got, want in zip(outs, (x * x, y * y, x * y)):
            assert np.array_equal(_host(got), want)
    big = 16384 * 256 + 77                                          # the second trip of the grid-stride loop
    x = (np.arange(big) % 17 - 8).astype(np.float64)
    y = (np.arange(big) % 13 - 6).astype(np.float64)
    outs = [torch.full((big,), SENTINEL, dtype=torch.float64, device='cuda') for _ in range(3)]
    xd, yd = _dev(x), _dev(y)
    assert lib.sg_ssim_products(_p(xd), _p(yd), *(_p(o) for o in outs), big, st) == 0
    for got, want in zip(outs, (x * x, y * y, x * y)):
        assert np.array_equal(_host(got), want)


def test_reduction_refusals():
    lib, st = _lib(), _st()
    ws, nbytes = _workspace()
    assert nbytes == 1024 * 2 * 8
    a = _dev(np.ones(10))
    out = torch.full((2,), SENTINEL, dtype=torch.float64, device='cuda')
    assert lib.sg_sqdiff_mean(_p(a), _p(a), _p(out), 10, _p(ws), nbytes - 1, st) == SG_EWORKSPACE
    assert lib.sg_minmax(_p(a), _p(out), 10, _p(ws), nbytes - 1, st) == SG_EWORKSPACE
    assert lib.sg_sqdiff_mean(_p(a), _p(a), _p(out), 0, _p(ws), nbytes, st) == SG_EINVAL
    assert lib.sg_sqdiff_mean(None, _p(a), _p(out), 10, _p(ws), nbytes, st) == SG_EINVAL
    assert lib.sg_minmax(_p(a), _p(out), 0, _p(ws), nbytes, st) == SG_EINVAL
    assert lib.sg_minmax(_p(a), None, 10, _p(ws), nbytes, st) == SG_EINVAL
    assert lib.sg_ssim_products(_p(a), _p(a), _p(out), _p(out), None, 2, st) == SG_EINVAL
    assert bool((_host(out) == SENTINEL).all())


# ---- sg_ssim_mean --------------------------------------------------------------------------------------------------
def _ssim_mean(mom, case, out=None):
    s0, s1, s2, c, crop0, crop = case
    ws, nbytes = _workspace()
    out = torch.full((1,), SENTINEL, dtype=torch.float64, device='cuda') if out is None else out
    md = [_dev(m) for m in mom]
    rc = _lib().sg_ssim_mean(*(_p(m) for m in md), _p(out), s0, s1, s2, c, crop0, crop, *R.SSIM_CONST, _p(ws), nbytes, _st())
    return rc, float(_host(out)[0])


@pytest.mark.parametrize('case', R.SSIM_CASES)
def test_ssim_mean_dyadic_moments_within_the_rounding_bound(case):
    """2-D use (s0 = 1, crop0 = 0), a single kept voxel, crop0 != crop with three channels, and 324 000 elements: past the
    1024 blocks of 256 x 4 of ssim_partial_kernel's grid."""
    s0, s1, s2, c, crop0, crop = case
    mom = R.ssim_moments(s0, s1, s2, c)
    rc, got = _ssim_mean(mom, case)
    assert rc == 0
    total, total_abs, count = R.ssim_box_sums(*mom, (s0, s1, s2), c, (crop0, crop, crop), (s0 - crop0, s1 - crop, s2 - crop),
                                              *R.SSIM_CONST)
    want = R.ssim_mean(*mom, (s0, s1, s2), c, crop0, crop, *R.SSIM_CONST)
    assert want == total / count
    bound = R.ssim_mean_bound(total_abs, count)
    err = abs(Fraction(got) - want)
    print(f'ssim_mean {case}: {count} kept, error / bound = {float(err / bound):.3e}')
    assert err <= bound, (got, float(want))


@pytest.mark.parametrize('case', R.SSIM_CASES)
def test_ssim_mean_of_identical_moments_is_exactly_one(case):
    """ux == uy and uxx == uyy == uxy: numerator and denominator of every S are the same float64, S is exactly 1, the sum is
    exactly the number of kept elements and the mean exactly 1.0 -- unless the kernel keeps another number of elements than
    the (s0 - 2 crop0)(s1 - 2 crop)(s2 - 2 crop) c it divides by."""
    s0, s1, s2, c, crop0, crop = case
    ux, _, uxx, _, _ = R.ssim_moments(s0, s1, s2, c)
    rc, got = _ssim_mean((ux, ux, uxx, uxx, uxx), case)
    assert rc == 0 and got == 1.0, got
    assert R.ssim_mean(ux, ux, uxx, uxx, uxx, (s0, s1, s2), c, crop0, crop, *R.SSIM_CONST) == 1


def test_ssim_mean_crop_box_face_by_face():
    """crop0 on the first axis only, crop on the other two: a voxel just outside each of the six faces does not count (the
    same bits come back), each of the eight corner voxels of the kept box does."""
    case = s0, s1, s2, c, crop0, crop = R.SSIM_CASES[2]
    assert crop0 != crop
    mom = R.ssim_moments(s0, s1, s2, c)
    rc, base = _ssim_mean(mom, case)
    assert rc == 0
    lo, hi = (crop0, crop, crop), (s0 - crop0, s1 - crop, s2 - crop)
    mid = [(l + h) // 2 for l, h in zip(lo, hi)]

    def changed(voxel, ch):
        m = [v.copy() for v in mom]
        m[2][voxel + (ch,)] += 1.0                # uxx: the denominator grows
        m[4][voxel + (ch,)] += 0.25               # uxy: the numerator changes wherever 2 ux uy + C1 != 0
        return _ssim_mean(m, case)[1]

    for axis in range(3):
        for pos in (lo[axis] - 1, hi[axis]):
            voxel = tuple(pos if a == axis else mid[a] for a in range(3))
            for ch in range(c):
                assert changed(voxel, ch) == base, (axis, pos, ch)
    for corner in itertools.product(*((l, h - 1) for l, h in zip(lo, hi))):
        ch = next(k for k in range(c) if 2 * mom[0][corner + (k,)] * mom[1][corner + (k,)] + R.SSIM_CONST[1] != 0)
        assert changed(corner, ch) != base, corner


def test_ssim_mean_refusals():
    mom = R.ssim_moments(7, 13, 12, 3)
    for case in ((7, 13, 12, 3, 4, 5), (8, 13, 12, 3, 4, 5), (7, 10, 12, 3, 2, 5), (7, 13, 10, 3, 2, 5), (7, 13, 9, 3, 2, 5),
                 (7, 13, 12, 0, 2, 5), (7, 13, 12, 3, -1, 5), (7, 13, 12, 3, 2, -1), (0, 13, 12, 3, 0, 5)):
        rc, got = _ssim_mean(mom, case)
        assert rc == SG_EINVAL and got == SENTINEL, case


# ---- wrapper level -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 2, 12, 14, 13), (2, 2, 12, 13, 14)], ids=('per_slice_2d', 'per_volume_3d'))
def test_get_ssim_with_two_channels_matches_the_oracle(shape):
    from saragan_amd.metrics import skim_metrics as G
    rng = np.random.default_rng(8)
    a = (np.clip(rng.normal(size=shape), -1, 2) * 1024).astype(np.int16)
    b = (np.clip(rng.normal(size=shape), -1, 2) * 1024).astype(np.int16)
    got, want = G.get_ssim(a, b), M.get_ssim(a, b)
    assert len(got) == len(want) == (12 if shape[0] == 1 else 2)
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-12)       # the tolerance tests/test_metrics.py holds get_ssim to
