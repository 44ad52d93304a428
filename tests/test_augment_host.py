"""CPU tests of the discriminator augmentation's numpy definition (tests/augref.py) and of its command-line flags.  The
reference is what the device results are compared against bit for bit (tests/test_augment_gpu.py), so its own properties are
checked here on integer-valued data, with exact equality: the adjoint identity, permutations, the draw's statistics and the
controller's rule."""
import numpy as np
import pytest

from tests import augref as R

SHAPE = (3, 2, 6, 6, 2)      # n, d, h, w, c


def _ints(seed, shape=SHAPE):
    return np.random.default_rng(seed).integers(-8, 9, shape).astype(np.float64)


def _same(prm, n=SHAPE[0]):
    return np.tile(np.asarray(prm, np.int32), (n, 1))


SINGLES = ([R.params_of(flip_d=1), R.params_of(flip_h=1), R.params_of(flip_w=1)] +
           [R.params_of(k=k) for k in (1, 2, 3)] +
           [R.params_of(t=t) for t in ((1, 0, 0), (-1, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 3), (0, 0, -3), (0, 6, 0), (2, 0, 0))])


@pytest.mark.parametrize('prm', SINGLES)
def test_adjoint_identity_for_every_single_transform(prm):
    x, y = _ints(1), _ints(2)
    p = _same(prm)
    assert (R.apply(x, p, 0.0) * y).sum() == (x * R.apply(y, p, 0.0, adjoint=True)).sum()


def test_adjoint_identity_for_random_compositions():
    for trial in range(20):
        x, y = _ints(10 + trial), _ints(50 + trial)
        p = R.draw(SHAPE[0], R.ALL, (1, 3, 3), 0.8, seed=trial, offset=3 * trial)
        assert (R.apply(x, p, 0.0) * y).sum() == (x * R.apply(y, p, 0.0, adjoint=True)).sum()
    # a nonzero fill adds a constant to the forward and nothing to the adjoint
    p = _same(R.params_of(t=(0, 2, -1)))
    x = _ints(3)
    assert np.array_equal(R.apply(x, p, -1.0, adjoint=True), R.apply(x, p, 0.0, adjoint=True))
    assert (R.apply(x, p, -1.0) == -1.0).sum() >= (R.apply(np.ones_like(x), p, 0.0) == 0).sum()


def test_adjoint_of_a_permutation_is_its_inverse_and_identity_returns_the_input():
    x = _ints(4)
    assert np.array_equal(R.apply(x, _same(R.IDENTITY), -1.0), x)
    assert np.array_equal(R.apply(x, _same(R.IDENTITY), 0.0, adjoint=True), x)
    for prm in (R.params_of(flip_d=1, flip_w=1, k=1), R.params_of(flip_h=1, k=3), R.params_of(k=2, flip_d=1)):
        p = _same(prm)
        assert np.array_equal(R.apply(R.apply(x, p, 0.0), p, 0.0, adjoint=True), x)
        assert np.array_equal(R.apply(R.apply(x, p, 0.0, adjoint=True), p, 0.0), x)
    # per-sample parameters: each sample follows its own row
    rows = np.asarray([R.params_of(flip_w=1), R.IDENTITY, R.params_of(k=1)], np.int32)
    y = R.apply(x, rows)
    assert np.array_equal(y[0], x[0][:, :, ::-1]) and np.array_equal(y[1], x[1])
    assert np.array_equal(y[2], np.rot90(x[2], 1, axes=(1, 2)))
    with pytest.raises(ValueError):
        R.apply(np.zeros((1, 1, 4, 8, 1)), [R.params_of(k=1)])


def test_philox_known_answers():
    """Random123's kat vectors for philox4x32-10."""
    z = R.philox4x32_10(np.zeros((1, 4), np.uint32), np.zeros(2, np.uint32))[0]
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = R.philox4x32_10(np.full((1, 4), 0xFFFFFFFF, np.uint32), np.full(2, 0xFFFFFFFF, np.uint32))[0]
    assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_draw_reference():
    m = (2, 5, 7)
    assert not R.draw(4096, R.ALL, m, 0.0, seed=7, offset=0).any()
    p1, g1 = R.draw(4096, R.ALL, m, 1.0, seed=7, offset=0, return_gates=True)
    assert g1.all()
    assert set(np.unique(p1[:, :3])) == {0, 1} and set(np.unique(p1[:, 3])) == {0, 1, 2, 3}
    for ax in range(3):
        t = p1[:, 4 + ax]
        assert np.abs(t).max() <= m[ax] and set(np.unique(t)) == set(range(-m[ax], m[ax] + 1))
    assert not p1[:, 7].any()
    # a disabled transform yields 0 whatever p is
    po = R.draw(4096, R.FLIP_W | R.TRANSLATE, m, 1.0, seed=7, offset=0)
    assert not po[:, [0, 1, 3]].any() and po[:, 2].any() and po[:, 4:7].any()
    # gate frequencies at p = 0.3: within 6 standard deviations of N p
    n, p = 4096, 0.3
    _, g = R.draw(n, R.ALL, m, p, seed=7, offset=0, return_gates=True)
    bound = 6.0 * np.sqrt(n * p * (1 - p))
    for j in range(5):
        assert abs(int(g[:, j].sum()) - n * p) <= bound, (j, int(g[:, j].sum()))
    # sample i of a draw at offset o is sample 0 of a draw at offset o + i; seeds and offsets above 2^32 matter
    a = R.draw(8, R.ALL, m, 0.7, seed=11, offset=(1 << 40) + 5)
    b = R.draw(1, R.ALL, m, 0.7, seed=11, offset=(1 << 40) + 8)
    assert np.array_equal(a[3], b[0])
    assert not np.array_equal(a, R.draw(8, R.ALL, m, 0.7, seed=11, offset=5))
    assert not np.array_equal(a, R.draw(8, R.ALL, m, 0.7, seed=11 + (1 << 32), offset=(1 << 40) + 5))


def test_controller_reference():
    cfg = dict(interval=3, target_num=600000, target_den=1000000, delta=np.float32(0.25), p_max=np.float32(0.8))
    st, p = (0, 0, 0, 0), np.float32(0.5)
    hist = []
    for _ in range(9):      # all signs +1: p rises every third call and stops at p_max
        st, p = R.ada_update(st, p, [1.0, 2.0, 0.5, 3.0], **cfg)
        hist.append(float(p))
    assert hist == [0.5, 0.5, 0.75, 0.75, 0.75, float(np.float32(0.8)), float(np.float32(0.8))] + [float(np.float32(0.8))] * 2
    assert st == (0, 0, 9, 3)
    for _ in range(12):     # all signs -1: p falls and stops at 0
        st, p = R.ada_update(st, p, [-1.0, -2.0], **cfg)
    assert float(p) == 0.0 and st == (0, 0, 21, 7)
    # zeros and NaN count as samples with sign 0; the sums are kept between adjustments and cleared by one
    st, p = R.ada_update((0, 0, 0, 0), np.float32(0.1), [0.0, -0.0, float('nan'), 4.0], **cfg)
    assert st == (1, 4, 1, 0) and p == np.float32(0.1)
    # exactly at the target (3 of 5 net positive = 0.6) is not above it: p falls
    st, p = R.ada_update((0, 0, 2, 0), np.float32(0.5), [1, 1, 1, 1, -1], **cfg)
    assert st == (0, 0, 3, 1) and p == np.float32(0.25)


BASE = ['pgan', '/data/', '--start_shape', '(1, 5, 16, 16)', '--final_shape', '(1, 20, 64, 64)', '--starting_phase', '1',
        '--ending_phase', '2', '--latent_dim', '16', '--noise_stddev', '0.01', '--network_size', 'xs']


def _parse(extra):
    from saragan_amd.main import build_parser, finalize_args
    return finalize_args(build_parser().parse_args(BASE + extra))


def test_cli_defaults_leave_augmentation_off():
    a = _parse([])
    assert a.augment == 'none' and a.augment_p == 0.0 and a.augment_ops == 'flip_w,translate'
    assert (a.augment_max_shift, a.augment_fill) == (0.125, 0.0)
    assert (a.ada_target, a.ada_interval, a.ada_kimg, a.ada_p_max) == (0.6, 4, 500.0, 0.8)
    a = _parse(['--augment', 'ada', '--augment_p', '0.2', '--ada_interval', '2', '--augment_ops', 'flip_w,rot90'])
    assert (a.augment, a.augment_p, a.ada_interval, a.ada_target) == ('ada', 0.2, 2, 0.6)


@pytest.mark.parametrize('extra, match', [
    (['--augment', 'ada', '--loss_fn', 'wgan'], 'logistic'),
    (['--augment', 'fixed', '--augment_ops', 'flip_w,rot90', '--final_shape', '(1, 20, 32, 64)'], 'square'),
    (['--ada_target', '0.5'], 'needs --augment ada'),
    (['--augment', 'fixed', '--ada_interval', '2'], 'needs --augment ada'),
    (['--augment', 'fixed', '--augment_ops', 'shear'], 'unknown transform'),
])
def test_cli_refusals(extra, match):
    with pytest.raises(SystemExit, match=match):
        _parse(extra)
