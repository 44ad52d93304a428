"""Spectral normalisation at kernel level (sg_spectral_refresh / sg_spectral_pullback through functional.SpectralTable): one
table holding five layers at once with sentinels in the alignment padding, and a table of one layer, against the fp64 statement
of tests/snref.py -- exact integer-valued sums, general floats within the a-priori bound of their own sums, convergence to the
largest singular value, run-to-run bits and the launch count."""
import os
import types

import numpy as np
import pytest
import torch

from tests import snref

pytestmark = pytest.mark.gpu

SENTINEL = 7.5
GAP = 4                           # sentinel elements after every layer, on top of the alignment padding
TABLES = {
    'all': [(1, 16),              # from_rgb on one channel
            (512, 1),             # the logit layer
            (81, 5),              # C not a multiple of 4: unaligned rows
            (864, 32),            # 3x3x3x32 -> 32
            (4096, 600)],         # several row blocks, C beyond one pass of a block
    'one': [(81, 5)],
}


def _layout(layers):
    starts, total = [], 0
    for r, c in layers:
        starts.append(total)
        total += (r * c + 3) // 4 * 4 + GAP
    return starts, total


def _table(layers):
    from saragan_amd import functional as F
    starts, total = _layout(layers)
    return F.SpectralTable([(s, r, c) for s, (r, c) in zip(starts, layers)], total, 'cuda'), starts, total


def _flat(layers, mats):
    """float32 CPU buffer: the matrices at their starts, sentinels everywhere else."""
    starts, total = _layout(layers)
    buf = np.full(total, SENTINEL, np.float32)
    for s, m in zip(starts, mats):
        buf[s:s + m.size] = np.asarray(m, np.float32).reshape(-1)
    return torch.from_numpy(buf)


def _pad_mask(layers):
    starts, total = _layout(layers)
    mask = np.ones(total, bool)
    for s, (r, c) in zip(starts, layers):
        mask[s:s + r * c] = False
    return torch.from_numpy(mask)


def _set_state(tab, name, vecs):
    buf = getattr(tab, name)
    host = buf.cpu()
    for s, x in enumerate(vecs):
        off = tab.layout[s][{'u': 5, 'v': 6}[name]]
        host[off:off + len(x)] = torch.from_numpy(np.asarray(x, np.float32))
    buf.copy_(host)


def _state(tab, layers):
    """[(u, v, sigma)] as numpy float32 copies."""
    out = []
    for s in range(len(layers)):
        u, v, sg = tab.views(s)
        out.append((u.reshape(-1).cpu().numpy().copy(), v.reshape(-1).cpu().numpy().copy(), np.float32(sg.item())))
    return out


def _mats(buf, layers):
    starts, _ = _layout(layers)
    host = buf.cpu().numpy()
    return [host[s:s + r * c].reshape(r, c).copy() for s, (r, c) in zip(starts, layers)]


def _sparse_int(rows, cols, rng, lo=1):
    """Integer-valued [rows, cols] with entries in {-2..2}, at most 8 non-zeros per row and per column: eight rounds, each a
    partial matching of rows and columns.  The rows are taken from one cyclic permutation, so every row has an entry wherever
    8 * min(rows, cols) >= rows."""
    w = np.zeros((rows, cols), np.float64)
    m = min(rows, cols)
    order = rng.permutation(rows)
    for k in range(8):
        rs = order[(np.arange(m) + k * m) % rows]
        cs = rng.permutation(cols)[:m]
        w[rs, cs] = rng.choice([-2, -1, 1, 2], size=m)
    assert (np.count_nonzero(w, axis=1) <= 8).all() and (np.count_nonzero(w, axis=0) <= 8).all()
    return w


def _ulps(got, want64):
    """|got - fl32(want)| in units of the spacing of fl32(want)."""
    want = np.asarray(want64, np.float64).astype(np.float32)
    return np.abs(np.asarray(got, np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)


_EXACT = {}


def _exact_case(key):
    """(W list, u list) of the integer-valued case and its fp64 refresh (iteration 1), computed once and never modified; the
    reference side first shows that every sum an f32 kernel can form, in any order, is an integer below 2^24."""
    if key not in _EXACT:
        layers = TABLES[key]
        rng = np.random.default_rng(5)
        ws = [_sparse_int(r, c, rng) for r, c in layers]
        us = [rng.choice([-1.0, 1.0], size=c) for _, c in layers]
        refs = []
        for w, u in zip(ws, us):
            ref = snref.refresh(w, u, 1)
            t, s = ref['t'], ref['s']
            assert (t == np.round(t)).all() and (s == np.round(s)).all()
            assert (np.abs(w) @ np.abs(u)).max() < 2 ** 24 and (np.abs(t) @ np.abs(w)).max() < 2 ** 24       # partial sums
            assert ref['T'] == round(ref['T']) and ref['S'] == round(ref['S']) and 0 < ref['T'] < 2 ** 24 and 0 < ref['S'] < 2 ** 24
            refs.append(ref)
        _EXACT[key] = (ws, us, refs)
    return _EXACT[key]


def _refresh(layers, ws, us, iteration=1, calls=1):
    from saragan_amd import functional as F
    tab, _, total = _table(layers)
    p = _flat(layers, ws).cuda()
    eff = torch.full((total,), SENTINEL, device='cuda')
    _set_state(tab, 'u', us)
    for _ in range(calls):
        F.spectral_refresh_(tab, p, eff, iteration)
    return tab, p, eff


@pytest.mark.parametrize('key', list(TABLES))
def test_refresh_of_integer_valued_weights_is_exact(key):
    """Every order of summation is exact in f32, so sigma, u, v and every element of W / sigma lie within 4 ulp of the fp64
    result rounded to f32: a square root, a division and a multiply, each correctly rounded, composed in the kernel's order.
    A dropped or doubled row or column would move sigma by at least 1 / S relative."""
    layers = TABLES[key]
    ws, us, refs = _exact_case(key)
    tab, p, eff = _refresh(layers, ws, us)
    got_w = _mats(eff, layers)
    for i, ((u, v, sg), ref) in enumerate(zip(_state(tab, layers), refs)):
        worst = {k: float(np.max(_ulps(g, ref[k]))) for k, g in (('sigma', sg), ('u', u), ('v', v), ('wbar', got_w[i]))}
        print(key, layers[i], 'ulp', worst, 'S', ref['S'])
        assert max(worst.values()) <= 4, (layers[i], worst)
    pad = _pad_mask(layers)
    assert bool((eff.cpu()[pad] == SENTINEL).all()) and torch.equal(p.cpu(), _flat(layers, ws))


def _dyadic_int(rows, cols, u, rng):
    """Integer-valued W whose power iteration stays exact in f32 at EVERY pass: 4^m non-zeros of one magnitude a (1 or 2) -- a
    partial matching of rows and columns, or, where the layer is one row or one column, four entries of it (signed so that the
    row's product with u does not cancel).  Then sum t^2 and sum s^2 are powers of 4, nt and nu are powers of two and
    u = s / (nt nu) stays a dyadic fraction: sigma = a for a matching (2a for the one-row / one-column layers)."""
    w = np.zeros((rows, cols), np.float64)
    a = float(rng.choice([1, 2]))
    if rows == 1:
        cs = rng.permutation(cols)[:4]
        w[0, cs] = a * u[cs]
    elif cols == 1:
        w[rng.permutation(rows)[:4], 0] = a * rng.choice([-1.0, 1.0], size=4)
    else:
        n = 4 ** int(np.floor(np.log(min(rows, cols, 256)) / np.log(4) + 1e-9))
        w[rng.permutation(rows)[:n], rng.permutation(cols)[:n]] = a * rng.choice([-1.0, 1.0], size=n)
    assert (np.count_nonzero(w, axis=1) <= 8).all() and (np.count_nonzero(w, axis=0) <= 8).all()
    return w


def _sums_are_exact(terms, axis=None):
    """Whether f32 adds `terms` (dyadic fractions) exactly in any order: with q the largest power of two that divides every
    term, each sum of absolute terms is an integer below 2^24 in units of q (every partial sum then has at most 24 bits)."""
    scaled = np.round(np.abs(terms) * 2.0 ** 40)
    if not (scaled == np.abs(terms) * 2.0 ** 40).all() or scaled.max() >= 2.0 ** 62:
        return False
    n = scaled.astype(np.int64)
    if not n.any():
        return True
    q = int(np.min((n & -n)[n != 0]))
    return bool((n.sum(axis=axis) // q < 2 ** 24).all())


def _is_power_of_4(x):
    m, e = np.frexp(x)
    return x > 0 and m == 0.5 and (e - 1) % 2 == 0


@pytest.mark.parametrize('key', list(TABLES))
def test_three_iterations_of_dyadic_weights_are_exact(key):
    """iteration = 3 at 4 ulp.  The reference side shows for each of the three passes that every term of every sum is a dyadic
    fraction, that each sum of absolute terms is an integer below 2^24 in units of its terms' common power of two
    (_sums_are_exact), and that sum t^2 and sum s^2 are powers of 4: every order of summation is exact in f32 in all three
    passes, and so are the two norms."""
    layers = TABLES[key]
    rng = np.random.default_rng(21)
    us = [rng.choice([-1.0, 1.0], size=c) for _, c in layers]
    ws = [_dyadic_int(r, c, u, rng) for (r, c), u in zip(layers, us)]
    refs = []
    for w, u0 in zip(ws, us):
        u = u0
        for it in range(3):
            ref = snref.refresh(w, u, 1)
            t, s = ref['t'], ref['s']
            assert _sums_are_exact(w * u[None, :], axis=1) and _sums_are_exact(t[:, None] * w, axis=0), it      # t = W u, s = W^T t
            assert _sums_are_exact(t * t) and _sums_are_exact(s * s), it                                       # sum t^2, sum s^2
            assert (t.astype(np.float32) == t).all() and (s.astype(np.float32) == s).all()
            assert _is_power_of_4(ref['T']) and _is_power_of_4(ref['S']), (it, ref['T'], ref['S'])
            u = ref['u']
        assert ref['sigma'] in (1.0, 2.0, 4.0)
        refs.append(snref.refresh(w, u0, 3))
        assert refs[-1]['sigma'] == ref['sigma'] and (refs[-1]['u'] == ref['u']).all()
    tab, p, eff = _refresh(layers, ws, us, iteration=3)
    got_w = _mats(eff, layers)
    for i, ((u, v, sg), ref) in enumerate(zip(_state(tab, layers), refs)):
        worst = {k: float(np.max(_ulps(g, ref[k]))) for k, g in (('sigma', sg), ('u', u), ('v', v), ('wbar', got_w[i]))}
        print(key, layers[i], 'iteration 3 ulp', worst, 'sigma', ref['sigma'])
        assert max(worst.values()) <= 4, (layers[i], worst)
    assert bool((eff.cpu()[_pad_mask(layers)] == SENTINEL).all())


def test_the_clamps_engage_on_the_device():
    """An all-zero layer and a layer of one element 1e-9 beside an ordinary one: both 1e-12 clamps engage (sum t^2 = 0 and
    1e-18; U2 = 0 and 1e-24), sigma = 0 is not protected against (W / sigma is NaN there, as in the reference), and the ordinary
    layer is not disturbed."""
    layers = [(3, 2), (1, 1), (12, 8)]
    rng = np.random.default_rng(2)
    ws = [np.zeros((3, 2), np.float32), np.full((1, 1), 1e-9, np.float32), rng.standard_normal((12, 8)).astype(np.float32)]
    us = [np.ones(2, np.float32), np.ones(1, np.float32), rng.standard_normal(8).astype(np.float32)]
    tab, p, eff = _refresh(layers, ws, us)
    got_w = _mats(eff, layers)
    state = _state(tab, layers)
    u, v, sg = state[0]
    assert (u == 0).all() and (v == 0).all() and sg == 0 and np.isnan(got_w[0]).all()
    ref = snref.refresh(ws[1], us[1], 1)
    u, v, sg = state[1]
    for got, key in ((u, 'u'), (v, 'v'), (sg, 'sigma'), (got_w[1], 'wbar')):
        np.testing.assert_allclose(np.asarray(got, np.float64).reshape(-1), np.asarray(ref[key]).reshape(-1), rtol=1e-5)
    assert abs(float(v[0]) - 1e-3) < 1e-8 and abs(float(u[0]) - 1e-6) < 1e-11      # divided by the clamps' 1e-6, not by the norms
    ref, bound = snref.refresh(ws[2], us[2], 1), snref.refresh_bounds(ws[2], us[2])
    u, v, sg = state[2]
    for got, key in ((u, 'u'), (v, 'v'), (sg, 'sigma'), (got_w[2], 'wbar')):
        assert (np.abs(np.asarray(got, np.float64) - ref[key]) <= bound[key]).all(), key


@pytest.mark.parametrize('key', list(TABLES))
def test_iteration_3_is_three_refreshes_bit_for_bit(key):
    """On weights whose later passes are NOT exact (the sparse integers above: after the first pass u = s / |s| is no binary
    fraction): iteration = 3 equals three refreshes of iteration = 1 in every bit (the loop adds nothing of its own), and its
    last pass, from the f32 u the first two left, lies within the a-priori bound of that pass's own sums
    (snref.refresh_bounds).  The 4-ulp check of three passes is test_three_iterations_of_dyadic_weights_are_exact."""
    from saragan_amd import functional as F
    layers = TABLES[key]
    ws, us, _ = _exact_case(key)
    tab3, _, eff3 = _refresh(layers, ws, us, iteration=3)
    tab1, p, eff1 = _refresh(layers, ws, us, iteration=1, calls=2)
    before = [s[0] for s in _state(tab1, layers)]
    F.spectral_refresh_(tab1, p, eff1, 1)
    assert torch.equal(eff3, eff1)
    for name in ('u', 'v', 'sigma'):
        assert torch.equal(getattr(tab3, name), getattr(tab1, name)), name
    got_w = _mats(eff3, layers)
    for i, (u, v, sg) in enumerate(_state(tab3, layers)):
        w32 = ws[i].astype(np.float32)
        ref, bound = snref.refresh(w32, before[i], 1), snref.refresh_bounds(w32, before[i])
        for k, g in (('sigma', sg), ('u', u), ('v', v), ('wbar', got_w[i])):
            err = np.abs(np.asarray(g, np.float64) - ref[k])
            assert (err <= bound[k]).all(), (layers[i], k, float(np.max(err)), float(np.max(bound[k])))


@pytest.mark.parametrize('key', list(TABLES))
def test_pullback_of_integer_values_is_bit_exact(key):
    """Integer G and Wbar with few non-zeros, small-integer u and v, sigma 0.5 or 2: every product and sum is exact, so the
    result equals the fp64 statement bit for bit, and so do the sentinels."""
    from saragan_amd import functional as F
    layers = TABLES[key]
    rng = np.random.default_rng(9)
    tab, _, _ = _table(layers)
    gs, wbs, us, vs, sgs = [], [], [], [], []
    for i, (r, c) in enumerate(layers):
        wb = _sparse_int(r, c, rng)
        g = _sparse_int(r, c, rng) + wb * rng.integers(1, 3, size=(r, c))      # (shares Wbar's support: the dot is not trivial)
        gs.append(g); wbs.append(wb)
        us.append(rng.integers(-2, 3, size=c).astype(np.float64)); vs.append(rng.integers(-2, 3, size=r).astype(np.float64))
        sgs.append(0.5 if i % 2 == 0 else 2.0)
    assert any(float(np.sum(g * wb)) != 0 for g, wb in zip(gs, wbs))
    g_dev, eff = _flat(layers, gs).cuda(), _flat(layers, wbs).cuda()
    _set_state(tab, 'u', us)
    _set_state(tab, 'v', vs)
    tab.sigma.copy_(torch.tensor(sgs))
    F.spectral_pullback_(tab, g_dev, eff)
    want = [snref.pullback(g, wb, u, v, sg) for g, wb, u, v, sg in zip(gs, wbs, us, vs, sgs)]
    for w in want:
        assert (w.astype(np.float32).astype(np.float64) == w).all()      # the fp64 result is itself an f32 value
    assert torch.equal(g_dev.cpu(), _flat(layers, want))
    assert torch.equal(eff.cpu(), _flat(layers, wbs))


_FLOATS = {}


def _float_case(key):
    if key not in _FLOATS:
        layers = TABLES[key]
        rng = np.random.default_rng(13)
        _FLOATS[key] = tuple([rng.standard_normal(shape(r, c)).astype(np.float32) for r, c in layers]
                             for shape in (lambda r, c: (r, c), lambda r, c: (r, c), lambda r, c: (c,)))
    return _FLOATS[key]


def _float_run(key):
    from saragan_amd import functional as F
    layers = TABLES[key]
    ws, gs, us = _float_case(key)
    tab, p, eff = _refresh(layers, ws, us)
    g = _flat(layers, gs).cuda()
    F.spectral_pullback_(tab, g, eff)
    return tab, p, eff, g


@pytest.mark.parametrize('key', list(TABLES))
def test_general_floats_within_the_bound_of_their_own_sums(key):
    """N(0, 1) W, G, u against fp64: each output may differ by at most gamma_n * sum |terms| of its own sums, carried through the
    quotients (snref.refresh_bounds / pullback_bound) -- true for any summation order, so nothing here is measured."""
    layers = TABLES[key]
    ws, gs, us = _float_case(key)
    tab, p, eff, g = _float_run(key)
    got_w, got_g, pad = _mats(eff, layers), _mats(g, layers), _pad_mask(layers)
    for i, (u, v, sg) in enumerate(_state(tab, layers)):
        ref, bound = snref.refresh(ws[i], us[i], 1), snref.refresh_bounds(ws[i], us[i])
        for k, got in (('sigma', sg), ('u', u), ('v', v), ('wbar', got_w[i])):
            err = np.abs(np.asarray(got, np.float64) - ref[k])
            print(key, layers[i], k, 'err/bound', float(np.max(err / np.maximum(bound[k], 1e-300))))
            assert (err <= bound[k]).all(), (layers[i], k, float(np.max(err)), float(np.max(bound[k])))
        # the pull-back from the f32 state the device holds
        want = snref.pullback(gs[i], got_w[i], u, v, sg)
        err = np.abs(got_g[i].astype(np.float64) - want)
        bnd = snref.pullback_bound(gs[i], got_w[i], u, v, sg)
        print(key, layers[i], 'pullback err/bound', float(np.max(err / bnd)))
        assert (err <= bnd).all(), (layers[i], float(np.max(err)))
    for buf in (eff, g):
        assert bool((buf.cpu()[pad] == SENTINEL).all())
    assert torch.equal(p.cpu(), _flat(layers, ws))


def test_twenty_refreshes_converge_to_the_largest_singular_value():
    """W = Q1 diag(4, 1, ..., 1) Q2^T, [96, 40]: the gap ratio is 1/4, the iteration error (1/16)^20 is below f32."""
    from saragan_amd import functional as F
    layers = [(96, 40)]
    rng = np.random.default_rng(17)
    q1, _ = np.linalg.qr(rng.standard_normal((96, 40)))
    q2, _ = np.linalg.qr(rng.standard_normal((40, 40)))
    w = (q1 @ np.diag([4.0] + [1.0] * 39) @ q2.T).astype(np.float32)
    tab, p, eff = _refresh(layers, [w], [rng.standard_normal(40)], iteration=1, calls=19)
    u_before = _state(tab, layers)[0][0]
    F.spectral_refresh_(tab, p, eff, 1)
    sg = float(_state(tab, layers)[0][2])
    top = float(np.linalg.svd(w.astype(np.float64), compute_uv=False)[0])
    bound = snref.refresh_bounds(w, u_before)
    assert abs(sg - top) <= bound['sigma'] + top * 16.0 ** -20, (sg, top, bound['sigma'])
    norm = float(np.linalg.svd(_mats(eff, layers)[0].astype(np.float64), compute_uv=False)[0])
    rel = bound['sigma'] / top + snref.gamma(8) + 16.0 ** -20
    assert abs(norm - 1.0) <= rel * (1 + 1e-3), (norm, rel)


def test_two_runs_give_identical_bits():
    a, b = _float_run('all'), _float_run('all')
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    for name in ('u', 'v', 'sigma'):
        assert torch.equal(getattr(a[0], name), getattr(b[0], name)), name


def test_launch_count_does_not_depend_on_the_number_of_layers(monkeypatch):
    from saragan_amd import functional as F
    lib = F._lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if not name.startswith('sg_') or name == 'sg_prof_enabled':
                return fn

            def wrapped(*a):
                calls.append(name)
                return fn(*a)
            return wrapped
    rng = np.random.default_rng(3)
    for layers in ([(12, 8), (7, 3)], [(12, 8), (7, 3)] * 6):
        ws = [rng.standard_normal(s).astype(np.float32) for s in layers]
        us = [rng.standard_normal(c).astype(np.float32) for _, c in layers]
        tab, p, eff = _refresh(layers, ws, us)
        g = _flat(layers, ws).cuda()
        with monkeypatch.context() as mp:
            mp.setattr(F._lib, 'load', lambda: Counting())
            F.spectral_refresh_(tab, p, eff, 2)
            F.spectral_pullback_(tab, g, eff)
            assert calls == ['sg_spectral_refresh', 'sg_spectral_pullback'], (len(layers), calls)
            del calls[:]


def test_arguments_are_validated_before_the_device_is_touched():
    from saragan_amd import functional as F
    layers = TABLES['one']
    tab, _, total = _table(layers)
    p = torch.zeros(total, device='cuda')
    with pytest.raises(ValueError):
        F.spectral_refresh_(tab, p, p)
    with pytest.raises(ValueError):
        F.spectral_refresh_(tab, p, torch.zeros(total, device='cuda'), iteration=0)
    with pytest.raises(ValueError):
        F.spectral_refresh_(tab, p, torch.zeros(total + 4, device='cuda'))
    with pytest.raises(RuntimeError):
        F.spectral_pullback_(tab, torch.zeros(total), torch.zeros(total))
    lib = F._lib.load()
    assert lib.sg_spectral_pullback(None, None, total, None, None, 1, 1, None, 1, None, 1, None, None, None) != 0
    with pytest.raises(ValueError):
        F.spectral_table_arrays([(2, 3, 3)], 16)            # a start that is no multiple of 4
    with pytest.raises(ValueError):
        F.spectral_table_arrays([(0, 3, 3), (8, 2, 2)], 16)   # overlapping segments


# ---------------------------------------------------------------------------------------------------------------------
# whole steps: the toy pgan of the step fixtures (tests/stepfix.py) with every discriminator weight normalised
# ---------------------------------------------------------------------------------------------------------------------
P2, P3 = 'oracle_step_p2_wgan_a060.npz', 'oracle_step_p3_wgan_a000.npz'      # phase 2 while mixing, phase 3 stabilising


@pytest.fixture
def deterministic(sg_env):
    from saragan_amd import functional as F
    F.clear_kept_workspaces()
    sg_env(SG_DETERMINISTIC=1)
    yield
    F.clear_kept_workspaces()


class _Step:
    """One step graph over the fixture's weights and randomness; `spectral` turns the normalisation of D on."""

    def __init__(self, golden_dir, name, dtype, loss_fn='wgan', strategy='simultaneous', spectral=True, iterations=1,
                 guard=False, optimizer='Adam', rnd='injected', seed=0):
        import saragan_amd.optimization as opt
        from saragan_amd.ExtendedEMA import ExtendedEMA
        from saragan_amd.networks import loss as L
        from saragan_amd.networks import ops as nops
        from saragan_amd.networks.ops import ScalarVariable
        from saragan_amd.networks.pgan.discriminator import discriminator
        from saragan_amd.networks.pgan.generator import generator
        from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
        import os
        from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture
        self.fx = fx = load_step_fixture(os.path.join(golden_dir, name), torch.float64)
        set_compute_dtype(dtype)
        self.store = store = VariableStore('cuda', seed=seed)
        if rnd == 'injected':
            L.set_random_source(L.InjectedRandom({k: v.float() for k, v in fx['rnd'].items()}))
        else:
            L.set_random_source(L.RandomSource(1234, 'cuda'))
        make = (lambda: opt.AdamOptimizer(ScalarVariable(1e-3), 0.0, 0.9)) if optimizer == 'Adam' else \
            (lambda: opt.GradientDescentOptimizer(ScalarVariable(1e-2)))
        self.og, self.od = make(), make()
        self.ph = opt.Placeholder([4, 1, 1, 1, 1])
        self.net_args = (LATENT, float(ScalarVariable(fx['alpha']).eval()), fx['phase'],      # (alpha as the step graph reads it: f32)
                         BASE_SHAPE, KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, loss_fn)
        self.generator, self.discriminator = generator, discriminator
        prev = nops.set_spectral_norm(('discriminator/',) if spectral else (), iterations)
        try:
            with use_store(store):
                self.tup = opt.optimize_step(self.og, self.od, generator, discriminator, self.ph, LATENT,
                                             ScalarVariable(fx['alpha'], 'alpha'), fx['phase'], BASE_SHAPE, KERNEL_SPEC, FILTER_SPEC,
                                             'leaky_relu', 0.2, loss_fn, fx['cfg']['gp_weight'], strategy, False, False, 0.01,
                                             None if fx['freeze'] is None else list(fx['freeze']))
        finally:
            nops.set_spectral_norm(*prev)
        store.load_state_dict(dict(fx['p0']))
        self.graph = self.tup[0].graph
        if guard:
            self.graph.configure_guard(True)
        self.ema = ExtendedEMA(list(store.vars.keys()), 0.99, graph=self.graph)
        self.ema_op = self.ema.apply()
        self.sess = opt.Session('cuda')
        mixing = fx['freeze'] is not None
        self.train = [self.tup[12], self.tup[16]] if mixing else [self.tup[0], self.tup[1]]
        self.real = fx['real'].float().cuda()

    def step(self, real=None, fetch=None):
        res = self.sess.run(self.train + [self.tup[2], self.tup[3]] if fetch is None else fetch,
                            feed_dict={self.ph: self.real if real is None else real})
        self.sess.run(self.ema_op)
        return res

    def flat(self):
        self.graph._ensure_flat()
        return self.store.flat['discriminator/']

    def layer_state(self):
        """{weight name: (u, v, sigma)} as float32 numpy copies."""
        flat = self.flat()
        out = {}
        for s, k in enumerate(flat['normalised']):
            u, v, sg = flat['spectral'].views(s)
            out[k] = (u.reshape(-1).cpu().numpy().copy(), v.reshape(-1).cpu().numpy().copy(), np.float32(sg.item()))
        return out

    def snapshot(self):
        snap = {k: v.detach().clone() for k, v in self.store.vars.items()}
        snap.update({k: v.detach().clone() for k, v in self.store.state.items()})
        return snap


@pytest.fixture
def fresh_step_state():
    from saragan_amd import functional as F
    from saragan_amd.networks import loss as L
    from saragan_amd.varstore import set_compute_dtype
    yield
    set_compute_dtype(torch.float32)
    L.set_random_source(None)
    F.clear_pack_cache()
    F.clear_kept_workspaces()


CASES = [(name, loss, dtype) for name in (P2, P3) for loss in ('wgan', 'logistic') for dtype in (torch.float32, torch.bfloat16)]
CASE_IDS = [f"{'p2' if n == P2 else 'p3'}-{l}-{'f32' if d == torch.float32 else 'bf16'}" for n, l, d in CASES]


@pytest.mark.parametrize('name,loss_fn,dtype', CASES, ids=CASE_IDS)
def test_step_gradient_is_the_pullback_of_the_effective_weights_gradient(golden_dir, deterministic, fresh_step_state, name, loss_fn,
                                                                         dtype):
    """D's `gradients` of a step against G = autograd.grad(disc_loss, effective leaves) through the public loss function on the
    same state, pulled back in fp64 with the layer's own u, v, sigma: within the a-priori bound of the pull-back's sums; biases
    bit for bit.  Pins the plumbing: the right layer's state, the raw parameter's slot, _land."""
    from saragan_amd import functional as F
    from saragan_amd.networks.loss import forward_simultaneous
    from saragan_amd.varstore import use_store
    st = _Step(golden_dir, name, dtype, loss_fn)
    grads, = st.sess.run([st.tup[8]], feed_dict={st.ph: st.real})      # D's gradients only: nothing is updated
    names = [v.key for v in st.tup[9]]
    got = {k: g.detach().clone() for k, g in zip(names, grads)}
    state = st.layer_state()
    flat = st.flat()
    assert 'discriminator/' not in st.store.rewritten                  # the step refreshed; the weights have not moved since
    leaves = [st.store.stand_in(k) for k in names]
    with use_store(st.store), torch.enable_grad():
        _, disc_loss, _, _ = forward_simultaneous(st.generator, st.discriminator, st.real, *st.net_args, st.fx['cfg']['gp_weight'],
                                                  0.01)
        # (buffers of the test's own as the kernels' destinations: the backward then takes the kernel routes of a step, whose
        # sums the bit comparison of the biases and the bound of the pull-back both presuppose)
        dest = {leaf.data_ptr(): torch.zeros_like(leaf) for leaf in leaves}
        with F.grads_into(dest):
            G = torch.autograd.grad(disc_loss, leaves, allow_unused=True)
    reached = 0
    for k, leaf, g in zip(names, leaves, G):
        g = torch.zeros_like(leaf) if g is None else g.float()
        if k not in st.store.effective:
            assert torch.equal(got[k], g), k                           # biases: the same kernels, nothing in between
            continue
        u, v, sg = state[k]
        o, n = flat['offsets'][k]
        wbar = snref.weight_matrix(flat['eff'][o:o + n].view(leaf.shape).cpu().numpy())
        g64 = snref.weight_matrix(g.cpu().numpy())
        want, bound = snref.pullback(g64, wbar, u, v, sg), snref.pullback_bound(g64, wbar, u, v, sg)
        err = np.abs(snref.weight_matrix(got[k].cpu().numpy()).astype(np.float64) - want)
        worst = float(np.max(err / np.maximum(bound, 1e-300))) if g64.any() else 0.0
        print(k, 'err/bound', worst)
        assert (err <= bound).all(), (k, float(np.max(err)), float(np.max(bound)))
        reached += bool(g64.any())
        if g64.any():                                                   # the pull-back did something: G itself is not the answer
            assert not np.array_equal(snref.weight_matrix(got[k].cpu().numpy()), g64.astype(np.float32)), k
    assert reached >= 4


@pytest.mark.parametrize('strategy', ['simultaneous', 'alternate'])
@pytest.mark.parametrize('name,dtype', [(P2, torch.float32), (P3, torch.bfloat16)], ids=['p2-f32', 'p3-bf16'])
def test_convolutions_consume_the_effective_weights(golden_dir, deterministic, fresh_step_state, monkeypatch, name, dtype, strategy):
    """After a step: every D layer read its effective leaf with coefficient 1 and no raw D weight; each refresh wrote W / sigma of
    the raw weights of that moment (fp64, within the bound of the refresh's own sums); the raw weights moved; u advanced once
    for `simultaneous` and twice for `alternate` (before forward_discriminator, and before forward_generator on the updated D)."""
    from saragan_amd import functional as F
    st = _Step(golden_dir, name, dtype, 'wgan', strategy)
    flat = st.flat()
    raw = {st.store.vars[k].data_ptr(): k for k in flat['normalised']}
    eff = {st.store.effective[k].data_ptr(): k for k in flat['normalised']}
    used, refreshes = [], []
    for fn_name, wpos in (('conv3d', 1), ('conv3d_act_pool', 1)):
        def spy(*a, _fn=getattr(F, fn_name), _wpos=wpos, **kw):
            used.append((a[_wpos].data_ptr(), float(a[_wpos + 1]) if len(a) > _wpos + 1 else float(kw.get('coef', 1.0))))
            return _fn(*a, **kw)
        monkeypatch.setattr(F, fn_name, spy)
    real_refresh = F.spectral_refresh_

    def refresh_spy(table, p, e, iteration=1):
        before = (p.clone(), table.u.clone())
        real_refresh(table, p, e, iteration)
        refreshes.append(before + (table.u.clone(), table.sigma.clone(), e.clone()))
    monkeypatch.setattr(F, 'spectral_refresh_', refresh_spy)
    w_pre = flat['param'].clone()
    st.step()
    assert len(refreshes) == (1 if strategy == 'simultaneous' else 2)
    assert torch.equal(refreshes[0][0], w_pre) and not torch.equal(flat['param'], w_pre)
    assert not (set(p for p, _ in used) & set(raw)), 'a discriminator layer read its raw weight'
    seen = {eff[p] for p, c in used if p in eff}
    assert all(c == 1.0 for p, c in used if p in eff)
    alpha = st.fx['alpha']
    expect = [k for k in flat['normalised'] if alpha > 0 or f"from_rgb_{st.fx['phase'] - 1}" not in k]
    assert seen >= set(expect), set(expect) - seen
    for p_before, u_before, u_after, sigma, e_after in refreshes:
        assert not torch.equal(u_before, u_after)
        for s, k in enumerate(flat['normalised']):
            o, n = flat['offsets'][k]
            _, rows, cols, _, _, uo, _, _ = flat['spectral'].layout[s]
            w = p_before[o:o + n].view(rows, cols).cpu().numpy()
            u0 = u_before[uo:uo + cols].cpu().numpy()
            ref, bound = snref.refresh(w, u0, 1), snref.refresh_bounds(w, u0)
            for key, g in (('u', u_after[uo:uo + cols]), ('sigma', sigma[s]), ('wbar', e_after[o:o + n].view(rows, cols))):
                err = np.abs(g.cpu().numpy().astype(np.float64) - ref[key])
                assert (err <= bound[key]).all(), (k, key, float(np.max(err)))
    assert torch.equal(flat['eff'], refreshes[-1][4]) and torch.equal(flat['spectral'].u, refreshes[-1][2])


@pytest.mark.parametrize('strategy', ['simultaneous', 'alternate'])
def test_launch_statistics_are_no_worse_than_without_the_feature(golden_dir, deterministic, fresh_step_state, strategy):
    """Counts, not times: gradients copied into their slots, and weight images packed one by one or in batches -- the effective
    leaves keep the fast paths of the raw parameters (one batched re-pack per refresh, not one pack per D pass)."""
    from saragan_amd import functional as F
    stats = {}
    for spectral in (False, True):
        F.clear_pack_cache()
        st = _Step(golden_dir, P3, torch.float32, 'wgan', strategy, spectral=spectral)
        for _ in range(2):
            st.step()
        before = (dict(F.GRAD_DEST_STATS), dict(F.PACK_STATS))
        st.step()
        stats[spectral] = ({k: F.GRAD_DEST_STATS[k] - before[0][k] for k in before[0]},
                           {k: F.PACK_STATS[k] - before[1][k] for k in before[1]})
    print(strategy, stats)
    off, on = stats[False], stats[True]
    assert on[0]['copied'] <= off[0]['copied'] and on[0]['claimed'] >= off[0]['claimed']
    assert on[1]['single'] <= off[1]['single'] and on[1]['batches'] <= off[1]['batches']


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('strategy', ['simultaneous', 'alternate'])
@pytest.mark.parametrize('name,loss_fn', [(P3, 'wgan'), (P2, 'logistic')], ids=['p3-wgan', 'p2-mixing-logistic'])
def test_captured_step_equals_eager_steps_bit_for_bit(golden_dir, deterministic, fresh_step_state, monkeypatch, dtype, strategy,
                                                      name, loss_fn):
    """Two eager warm-up steps, a capture, two replays against five eager steps: weights, u and losses in every bit.  The phase-2
    case is a mixing phase: the frozen train ops run, whose pull-back first clears the frozen layers' slots."""
    runs = {}
    for mode in ('0', '1'):
        monkeypatch.setenv('SARAGAN_HIPGRAPH', mode)
        st = _Step(golden_dir, name, dtype, loss_fn, strategy, rnd='device')
        gen = torch.Generator().manual_seed(5)
        losses = []
        for i in range(5):
            real = (st.fx['real'].float() + 0.1 * torch.randn(st.fx['real'].shape, generator=gen)).cuda()
            res = st.step(real)
            losses.append((float(res[2]), float(res[3])))
        ncap = sum(1 for e in st.graph.__dict__.get('_captures', {}).values() if 'graph' in e)
        runs[mode] = (st.snapshot(), losses, ncap)
        st = None
    monkeypatch.setenv('SARAGAN_HIPGRAPH', '0')
    (w0, l0, n0), (w1, l1, n1) = runs['0'], runs['1']
    assert (n0, n1) == (0, 1)
    assert l0 == l1, (l0, l1)
    assert any(k.endswith('/u') for k in w0)
    bad = [k for k in w0 if not torch.equal(w0[k], w1[k])]
    assert not bad, bad


def test_nonfinite_guard_keeps_the_raw_weights_and_the_next_step_clean(golden_dir, deterministic, fresh_step_state, monkeypatch):
    """A NaN in the real batch of step 2 makes D's gradient NaN (through the pull-back's dot too): with the guard D's raw weights
    stay put.  Step 3 then equals step 3 of a run whose step 2 never trained D: nothing non-finite survives in u, v, sigma, the
    effective weights or the partial sums.  (The host cannot see the device's decision: after the skipped update the refresh
    runs again on unchanged weights -- one more power iteration -- which the comparison run asks for explicitly.)"""
    monkeypatch.setenv('SARAGAN_HIPGRAPH', '0')
    bad = None
    snaps = {}
    for run in ('skipped', 'untrained'):
        st = _Step(golden_dir, P3, torch.float32, 'logistic', guard=True)
        bad = st.real.clone()
        bad.view(-1)[3] = float('nan')
        st.step()
        after1 = st.snapshot()
        if run == 'skipped':
            st.step(bad)
            after2 = st.snapshot()
            d_raw = [k for k in after1 if k.startswith('discriminator/') and not k.endswith('/u')]
            assert all(torch.equal(after1[k], after2[k]) for k in d_raw)
            assert any(not torch.equal(after1[k], after2[k]) for k in after1 if k.startswith('generator/'))
            assert st.graph.skipped_steps == {'generator': 0, 'discriminator': 1}
        else:
            st.step(bad, fetch=[st.train[0]])                   # the generator alone: its gradient does not depend on the real batch
            st.store.mark_rewritten('discriminator/')
        st.step()
        snaps[run] = st.snapshot()
        for k, v in snaps[run].items():
            assert torch.isfinite(v).all(), (run, k)
        flat = st.flat()
        assert torch.isfinite(flat['spectral'].sigma).all() and torch.isfinite(flat['spectral'].v).all()
    bad_keys = [k for k in snaps['skipped'] if not torch.equal(snaps['skipped'][k], snaps['untrained'][k])]
    assert not bad_keys, bad_keys


def test_checkpoint_round_trip_and_resume(golden_dir, deterministic, fresh_step_state, monkeypatch, tmp_path):
    """save -> restore brings u back; a run resumed from the checkpoint continues bit-identically to the uninterrupted one
    (stateless optimiser, injected randomness: the checkpoint holds all there is); a checkpoint without u loads and leaves u fresh."""
    from saragan_amd.utils import load_checkpoint, restore_variables, save_checkpoint
    monkeypatch.setenv('SARAGAN_HIPGRAPH', '0')
    whole = _Step(golden_dir, P3, torch.float32, 'wgan', optimizer='SGD')
    for _ in range(4):
        whole.step()
    want = whole.snapshot()
    first = _Step(golden_dir, P3, torch.float32, 'wgan', optimizer='SGD')
    for _ in range(2):
        first.step()
    path = str(tmp_path / 'model_3')
    save_checkpoint(first.store, path)
    half = first.snapshot()
    sd = load_checkpoint(path)
    u_keys = [k for k in sd if k.endswith('/u')]
    assert sorted(u_keys) == sorted(first.store.state) and u_keys
    resumed = _Step(golden_dir, P3, torch.float32, 'wgan', optimizer='SGD', seed=7)
    fresh_u = {k: v.clone() for k, v in resumed.store.state.items()}
    assert not any(torch.equal(fresh_u[k], half[k]) for k in u_keys)
    restore_variables(resumed.store, 3, 3, str(tmp_path), path, list(resumed.store.vars), False, resumed.ema)
    for k, v in resumed.snapshot().items():
        assert torch.equal(v, half[k]), k
    for _ in range(2):
        resumed.step()
    got = resumed.snapshot()
    bad = [k for k in want if not torch.equal(want[k], got[k])]
    assert not bad, bad
    # a checkpoint written without u
    np.savez(str(tmp_path / 'old.npz'), **{k: v for k, v in sd.items() if not k.endswith('/u')})
    old = _Step(golden_dir, P3, torch.float32, 'wgan', optimizer='SGD', seed=7)
    restore_variables(old.store, 3, 3, str(tmp_path), str(tmp_path / 'old'), list(old.store.vars), False, old.ema)
    for k in u_keys:
        assert torch.equal(old.store.state[k], fresh_u[k]), k
    assert all(torch.equal(old.store.vars[k], half[k]) for k in old.store.vars)
    old.step()
    assert all(torch.isfinite(v).all() for v in old.snapshot().values())


def test_default_off_calls_no_spectral_entry_point(golden_dir, fresh_step_state, monkeypatch):
    from saragan_amd import functional as F
    from saragan_amd.networks import ops as nops
    from saragan_amd.varstore import use_store, variable_scope
    calls = []
    monkeypatch.setattr(F, 'spectral_refresh_', lambda *a, **k: calls.append('refresh'))
    monkeypatch.setattr(F, 'spectral_pullback_', lambda *a, **k: calls.append('pullback'))
    st = _Step(golden_dir, P3, torch.float32, 'wgan', spectral=False)
    st.step()
    st.step()
    assert not calls and not st.store.state and not st.store.effective and 'eff' not in st.flat()
    with use_store(st.store), variable_scope('discriminator'), variable_scope('discriminator_out'), variable_scope('dense_2'):
        shape = list(st.store.vars['discriminator/discriminator_out/dense_2/weight'].shape)
        w = nops.get_weight(shape, 'linear')
    assert w.var is st.store.vars['discriminator/discriminator_out/dense_2/weight']
    assert w.coef == pytest.approx(1.0 / np.sqrt(shape[0]))            # the equalised-LR coefficient, as before


def _dp_worker(rank, world, port, golden, q):
    import os
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0',
                      SARAGAN_DIST_BACKEND='gloo', HSA_ENABLE_IPC_MODE_LEGACY='0', SARAGAN_HIPGRAPH='0')
    import saragan_amd.optimization as opt
    from saragan_amd import parallel
    from saragan_amd.ExtendedEMA import ExtendedEMA
    from saragan_amd.networks import loss as L
    from saragan_amd.networks import ops as nops
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture
    if world > 1:
        parallel.init_distributed()
    fx = load_step_fixture(os.path.join(golden, P3), torch.float64)
    n = fx['real'].shape[0] // world
    sl = slice(rank * n, (rank + 1) * n)
    set_compute_dtype(torch.float32)
    store = VariableStore('cuda', seed=100 + rank)                      # the ranks draw different weights AND different u
    L.set_random_source(L.InjectedRandom({k: v[sl].float() for k, v in fx['rnd'].items()}))
    mk = lambda: opt.AdamOptimizer(ScalarVariable(1e-3), 0.0, 0.9)
    og, od = (parallel.DistributedOptimizer(mk()), parallel.DistributedOptimizer(mk())) if world > 1 else (mk(), mk())
    ph = opt.Placeholder([n, 1, 1, 1, 1])
    nops.set_spectral_norm(('discriminator/',))
    with use_store(store):
        tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, ScalarVariable(fx['alpha']), fx['phase'], BASE_SHAPE,
                                KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, fx['loss_fn'], fx['cfg']['gp_weight'], 'simultaneous',
                                False, False, 0.01, None)
    nops.set_spectral_norm(())
    if rank == 0:
        sd = dict(fx['p0'])
        gen = torch.Generator().manual_seed(3)
        sd.update({k: torch.randn(v.shape, generator=gen) for k, v in store.state.items()})      # the same u for every world size
        store.load_state_dict(sd, strict=True)
    graph = tup[0].graph
    ema = ExtendedEMA(list(store.vars), 0.99, graph=graph)
    graph._ensure_flat()
    if world > 1:
        parallel.broadcast_global_variables(store, 0)
    ema.reset_to_variables()
    sess = opt.Session('cuda')
    sess.run([tup[0], tup[1]], feed_dict={ph: fx['real'][sl].float()})
    sess.run(ema.apply())
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy() for k, v in store.vars.items()}
    out.update({k: v.detach().cpu().numpy() for k, v in store.state.items()})
    q.put((rank, out))
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


def test_two_ranks_reproduce_the_full_batch_step(golden_dir, fresh_step_state, monkeypatch):
    """Two gloo ranks on one GPU, half the batch each, against the same step on the full batch in one process: the comparison
    and tolerance of tests/test_dp_gpu.py's two-rank test; replicas (u included, broadcast from rank 0) stay bit-identical."""
    import torch.multiprocessing as mp
    from tests.test_dp_gpu import _free_port
    ctx = mp.get_context('spawn')
    res = {}
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, golden_dir, q)) for r in range(2)]
    for p in procs:
        p.start()
    full = []                                       # the full-batch step in this process, while the ranks start up
    for k in ('MASTER_ADDR', 'MASTER_PORT', 'RANK', 'WORLD_SIZE', 'LOCAL_RANK', 'SARAGAN_DIST_BACKEND',
              'HSA_ENABLE_IPC_MODE_LEGACY', 'SARAGAN_HIPGRAPH'):
        monkeypatch.setenv(k, os.environ.get(k, ''))      # (the worker writes them: restored after the test)
    _dp_worker(0, 1, port, golden_dir, types.SimpleNamespace(put=full.append))
    res[1] = dict(full)
    res[2] = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    full = res[1][0]
    assert any(k.endswith('/u') for k in full)
    for k, ref in full.items():
        for r in range(2):
            np.testing.assert_allclose(res[2][r][k], ref, rtol=1e-4, atol=3e-5, err_msg=f'rank {r} {k}')
        np.testing.assert_array_equal(res[2][0][k], res[2][1][k])


def test_two_phase_training_run_hands_the_state_over(tmp_path, fresh_step_state):
    """--d_spectral_norm through the training loop: two phases (the hand-off drops from_rgb_1's successor-less state and keeps
    the rest), the end-of-phase checkpoints hold u, a run continued from model_1 starts from its u, and the switch is off again
    when the run returns."""
    from saragan_amd.networks import ops as nops
    from saragan_amd.train import run_training
    from saragan_amd.utils import load_checkpoint
    from tests.test_train_gpu import _args, _make_data
    import os
    data, logdir = tmp_path / 'data', tmp_path / 'log'
    _make_data(data)
    out = run_training(_args(data, logdir, d_spectral_norm=True, sn_iterations=2))
    assert nops.spectral_norm_settings() == ((), 1)
    st, store = out['stats'], out['store']
    assert all(np.isfinite(st[p]['d_loss']) and np.isfinite(st[p]['g_loss']) for p in (1, 2))
    d_weights = [k for k in store.vars if k.startswith('discriminator/') and k.endswith('/weight')]
    assert sorted(store.state) == sorted(store.u_name(k) for k in d_weights) and list(store.effective) == d_weights
    ck1, ck2 = (load_checkpoint(os.path.join(str(logdir), f'model_{p}')) for p in (1, 2))
    assert sorted(k for k in ck2 if k.endswith('/u')) == sorted(store.state)
    assert all(np.isfinite(v).all() for v in ck2.values())
    shared = [k for k in ck1 if k.endswith('/u') and k in ck2]
    assert shared and 'discriminator/from_rgb_1/u' in ck1
    # continued from model_1: phase 2 starts from the checkpoint's u for the layers phase 1 had
    args = _args(data, tmp_path / 'log2', starting_phase=2, continue_path=os.path.join(str(logdir), 'model_1'),
                 d_spectral_norm=True)
    out2 = run_training(args, max_steps_per_phase=1)
    assert set(out2['store'].state) == set(store.state)
    plain = run_training(_args(data, tmp_path / 'log3', ending_phase=1), max_steps_per_phase=1)
    assert not plain['store'].state and not any(k.endswith('/u') for k in load_checkpoint(os.path.join(str(tmp_path / 'log3'), 'model_1')))
