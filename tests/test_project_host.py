"""The projection's host side: the numpy twins of sg_multiscale_residual and sg_latent_step against independent
statements (tests/projref.py), the argument refusals, the tool's refusals, and one whole run of the tool on the CPU with a small
linear generator handed to run() -- the initial-latent rule replayed from projection.json alone, and the batch size changing nothing.

Exactness: with integer-valued y, integer targets, mean 0, stddev 1 and power-of-two weights every sum of the definition is exact
in any order; where the element count is a power of two as well (the shapes of EXACT) the divisions and the gradient's factors are
exact too, and the loss, the terms and the gradient EQUAL the float64 reference.  On a shape whose count is no power of two the
terms (one division of an exact sum) are still equal."""
import json
import os

import numpy as np
import pytest
import torch

from tests import projref as R

EXACT = [((1, 4, 8, 8), 3, 2), ((2, 4, 8, 8), 2, 2), ((1, 8, 16, 32), 4, 1), ((1, 2, 4, 4), 1, 2), ((1, 16, 16, 16), 4, 2)]
GENERAL = [((1, 4, 8, 8), 3, 3), ((1, 2, 6, 10), 2, 2), ((1, 8, 16, 48), 4, 2), ((1, 3, 5, 7), 1, 3), ((2, 4, 8, 8), 2, 2)]
# Measured once on GENERAL x seeds 0 .. 5 (float32 y, int16 targets, mean 1000, stddev 500): projref.reference against itself on the
# mirrored volume (numpy then adds in another order) differs by at most 3.3e-16 of the largest term -- the terms, the f64 loss and
# the f64 gradient alike (the gradient: 0).  Times 4:
ORDER_BOUND = 1.4e-15
F32_HALF_ULP = 2.0 ** -24      # loss and a float32 gradient are the f64 value rounded once


def F():
    from saragan_amd import functional
    return functional


@pytest.mark.parametrize('shape,levels,n', EXACT)
def test_integer_values_equal_the_reference(shape, levels, n):
    y, table = R.make_integer_case(n, 3, shape, seed=5)
    pos = np.array([2, 0, 1][:n])
    lam = [1.0, 0.5, 2.0, 0.25][:levels]
    loss, terms, grad = F().multiscale_residual_raw(y, table, pos, 0.0, 1.0, levels, lam)
    rl, rt, rg = R.reference(R.residual(y, table, pos, 0.0, 1.0), levels, lam)
    assert terms.dtype == torch.float64 and loss.dtype == torch.float32 and grad.dtype == y.dtype and grad.shape == y.shape
    assert np.array_equal(terms.numpy(), rt)
    assert np.array_equal(loss.numpy(), rl.astype(np.float32))
    assert np.array_equal(grad.numpy(), rg.astype(np.float32))


def test_integer_values_on_a_count_that_is_no_power_of_two():
    y, table = R.make_integer_case(2, 2, (3, 2, 6, 10), seed=6)
    loss, terms, grad = F().multiscale_residual_raw(y, table, [1, 1], 0.0, 1.0, 2, [1.0, 4.0])
    rl, rt, rg = R.reference(R.residual(y, table, [1, 1], 0.0, 1.0), 2, [1.0, 4.0])
    assert np.array_equal(terms.numpy(), rt)
    assert np.allclose(loss.numpy(), rl, rtol=2 * F32_HALF_ULP, atol=0) and np.allclose(grad.numpy(), rg, rtol=2 * F32_HALF_ULP, atol=1e-15)


@pytest.mark.parametrize('shape,levels,n', GENERAL)
@pytest.mark.parametrize('seed', [0, 3])
def test_general_values_within_the_measured_bound(shape, levels, n, seed):
    y, table = R.make_y(n, shape, torch.float32, seed), R.make_table(4, shape, torch.int16, seed)
    pos, lam = np.arange(n) % 4, [float(v) for v in np.float32([1.0, 0.7, 1.3, 0.9][:levels])]      # (the weights are float32 numbers)
    loss, terms, grad = F().multiscale_residual_raw(y, table, pos, 1000.0, 500.0, levels, lam)
    rl, rt, rg = R.reference(R.residual(y, table, pos, 1000.0, 500.0), levels, lam)
    assert np.abs(terms.numpy() - rt).max() <= ORDER_BOUND * np.abs(rt).max()
    assert np.all(np.abs(loss.numpy().astype(np.float64) - rl) <= F32_HALF_ULP * np.abs(rl) + ORDER_BOUND * np.abs(rl).max())
    assert np.all(np.abs(grad.numpy().astype(np.float64) - rg) <= F32_HALF_ULP * np.abs(rg) + ORDER_BOUND * np.abs(rg).max())


@pytest.mark.parametrize('ydt', R.Y_DTYPES)
def test_types_formats_repeats_and_positions_outside(ydt):
    shape, levels = (2, 4, 8, 8), 2
    for tdt in R.TABLE_DTYPES:
        table = R.make_table(3, shape, tdt, 2)
        for cl in (False, True):
            y = R.make_y(4, shape, ydt, 2, channels_last=cl)
            pos = np.array([2, 2, 7, 0])      # a repeat, one outside
            loss, terms, grad = F().multiscale_residual_raw(y, table, pos, 3.0, 2.0, levels)
            assert grad.dtype == ydt and grad.is_contiguous() == y.is_contiguous() and grad.stride() == y.stride()
            assert np.isnan(loss[2].item()) and torch.isnan(terms[2]).all() and torch.isnan(grad[2].float()).all()
            ok = [0, 1, 3]
            rl, rt, rg = R.reference(R.residual(y[ok], table, pos[ok], 3.0, 2.0), levels, [1.0, 1.0])
            assert np.abs(terms[ok].numpy() - rt).max() <= ORDER_BOUND * np.abs(rt).max()
            ulp = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}[ydt]      # 24, 8 and 11 significant bits
            got = grad[ok].float().numpy().astype(np.float64)
            assert np.all(np.abs(got - rg) <= ulp * np.abs(rg) + 2.0 ** -25)      # one rounding (f16: its subnormal step 2^-24 / 2)


def test_gradients_are_rounded_once():
    from saragan_amd.table_ops import _round_once
    # 1 + 2^-8 + 2^-30 lies just above a bf16 tie: through a float32 rounded to nearest it would fall on the tie and go down to 1
    g = np.array([1 + 2.0 ** -8 + 2.0 ** -30, -(1 + 2.0 ** -8 + 2.0 ** -30), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1e300, -1e-300, 0.0])
    assert _round_once(g, torch.bfloat16).float().tolist() == [1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1.0, 1 + 2.0 ** -6, np.inf, -0.0, 0.0]
    h = np.array([1 + 2.0 ** -11 + 2.0 ** -40, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 70000.0])
    assert _round_once(h, torch.float16).float().tolist() == [1 + 2.0 ** -10, 1.0, 1 + 2.0 ** -9, np.inf]
    assert _round_once(g[:3], torch.float32).dtype == torch.float32


def test_autograd_delivers_the_gradient():
    y, table = R.make_y(3, (1, 4, 8, 8), torch.float32, 1), R.make_table(3, (1, 4, 8, 8), torch.uint16, 1)
    _, _, grad = F().multiscale_residual_raw(y, table, [0, 1, 2], 100.0, 50.0, 3, [1.0, 2.0, 0.5])
    yg = y.clone().requires_grad_(True)
    loss, terms = F().multiscale_residual(yg, table, [0, 1, 2], 100.0, 50.0, 3, [1.0, 2.0, 0.5])
    assert not terms.requires_grad
    loss.sum().backward()
    assert torch.equal(yg.grad, grad)


def test_argument_refusals():
    f = F()
    y, table = R.make_y(2, (1, 4, 8, 8), torch.float32, 0), R.make_table(3, (1, 4, 8, 8), torch.int16, 0)
    with pytest.raises(TypeError, match='float32, bfloat16 or float16'):
        f.multiscale_residual_raw(y.double(), table, [0, 1])
    with pytest.raises(TypeError, match='tables are'):
        f.multiscale_residual_raw(y, table.long(), [0, 1])
    with pytest.raises(ValueError, match='contiguous table'):
        f.multiscale_residual_raw(y, table[:, :, :2], [0, 1])
    with pytest.raises(ValueError, match='levels is 1 .. 6'):
        f.multiscale_residual_raw(y, table, [0, 1], levels=7)
    with pytest.raises(ValueError, match='not a multiple of 2\\^3'):
        f.multiscale_residual_raw(y, table, [0, 1], levels=4)
    with pytest.raises(ValueError, match='weights are 3'):
        f.multiscale_residual_raw(y, table, [0, 1], levels=3, weights=[1.0, 2.0])
    with pytest.raises(ValueError, match='weights are 2'):
        f.multiscale_residual_raw(y, table, [0, 1], levels=2, weights=[1.0, -2.0])
    with pytest.raises(ValueError, match='integer positions'):
        f.multiscale_residual_raw(y, table, [0, 1, 2])
    with pytest.raises(ValueError, match='stddev is not 0'):
        f.multiscale_residual_raw(y, table, [0, 1], 0.0, 0.0)
    with pytest.raises(ValueError, match='channels_last_3d'):
        f.multiscale_residual_raw(y.expand(2, 2, 4, 8, 8)[:, :, :, ::2], R.make_table(3, (2, 4, 4, 8), torch.int16, 0), [0, 1], levels=1)
    z = torch.zeros(2, 8)
    good = dict(z=z, m=z.clone(), v=z.clone(), grad_z=z.clone(), loss=torch.zeros(2), best_loss=torch.zeros(2), z_best=z.clone(),
                best_step=torch.zeros(2, dtype=torch.int32))
    for name, bad, match in (('m', torch.zeros(2, 7), 'm must be'), ('best_step', torch.zeros(2, dtype=torch.int64), 'best_step must be'),
                             ('loss', torch.zeros(2, 1), 'loss must be'), ('z', torch.zeros(2, 8, dtype=torch.float64), 'must be')):
        with pytest.raises(ValueError, match=match):
            f.latent_step_(**dict(good, **{name: bad}), lr=0.1, step=1)
    with pytest.raises(ValueError, match='step counts from 1'):
        f.latent_step_(**good, lr=0.1, step=0)
    with pytest.raises(ValueError, match='lr >= 0'):
        f.latent_step_(**good, lr=-0.1, step=1)
    with pytest.raises(ValueError, match='betas'):
        f.latent_step_(**good, lr=0.1, step=1, beta1=1.0)


# ---- the latents' update
def _state(n, L, seed):
    rng = np.random.default_rng(seed)
    a = [rng.standard_normal((n, L)).astype(np.float32) for _ in range(2)]
    return dict(z=a[0], m=np.zeros((n, L), np.float32), v=np.zeros((n, L), np.float32), g=a[1],
                best_loss=np.full(n, np.inf, np.float32), z_best=np.zeros((n, L), np.float32), best_step=np.full(n, -1, np.int32))


@pytest.mark.parametrize('L,n', [(8, 1), (64, 3), (200, 2)])
@pytest.mark.parametrize('sphere', [False, True])
def test_latent_step_twin_against_the_scalar_loop(L, n, sphere):
    rng = np.random.default_rng(L + n)
    s = _state(n, L, L)
    mine = {k: torch.from_numpy(v.copy()) for k, v in s.items()}
    for step in range(1, 5):
        g = rng.standard_normal((n, L)).astype(np.float32)
        loss = rng.random(n).astype(np.float32)
        if step == 3:
            loss[0] = np.nan
        lr = 0.05 * step
        R.latent_step_scalar(s['z'], s['m'], s['v'], g, loss, s['best_loss'], s['z_best'], s['best_step'], lr, 0.9, 0.999, 1e-8, step, sphere)
        F().latent_step_(mine['z'], mine['m'], mine['v'], torch.from_numpy(g), torch.from_numpy(loss), mine['best_loss'], mine['z_best'],
                         mine['best_step'], lr, step, sphere=sphere)
        for k in ('z', 'm', 'v', 'best_loss', 'z_best', 'best_step'):
            assert np.array_equal(mine[k].numpy(), s[k]), (k, step)
    if sphere:
        assert np.allclose(np.linalg.norm(mine['z'].numpy().astype(np.float64), axis=1), np.sqrt(L), rtol=1e-6)


def test_latent_step_best_bookkeeping_and_lr_zero():
    s = {k: torch.from_numpy(v) for k, v in _state(3, 16, 1).items()}
    z0 = s['z'].clone()
    step = lambda loss, lr, t: F().latent_step_(s['z'], s['m'], s['v'], s['g'], torch.tensor(loss, dtype=torch.float32), s['best_loss'],  # noqa: E731
                                                s['z_best'], s['best_step'], lr, t)
    step([3.0, float('nan'), 2.0], 0.1, 1)
    assert s['best_loss'].tolist() == [3.0, float('inf'), 2.0] and s['best_step'].tolist() == [1, -1, 1]      # a NaN never wins
    assert torch.equal(s['z_best'][0], z0[0]) and torch.equal(s['z_best'][1], torch.zeros(16)) and not torch.equal(s['z'], z0)
    z1 = s['z'].clone()
    step([3.0, 5.0, 1.0], 0.1, 2)      # an equal loss does not replace the best
    assert s['best_loss'].tolist() == [3.0, 5.0, 1.0] and s['best_step'].tolist() == [1, 2, 2]
    assert torch.equal(s['z_best'][0], z0[0]) and torch.equal(s['z_best'][2], z1[2])
    z2, m2, v2 = s['z'].clone(), s['m'].clone(), s['v'].clone()
    step([0.5, 9.0, 9.0], 0.0, 3)      # lr = 0 scores and leaves z, m and v alone
    assert torch.equal(s['z'], z2) and torch.equal(s['m'], m2) and torch.equal(s['v'], v2)
    assert s['best_step'].tolist() == [3, 2, 2] and torch.equal(s['z_best'][0], z2[0])


# ---- the tool
LAT, SHAPE = 8, (1, 4, 8, 8)


def _argv(target, out, *more):
    return ['pgan', '--start_shape', '(1, 1, 2, 2)', '--final_shape', '(1, 4, 8, 8)', '--network_size', 'xs', '--latent_dim', str(LAT),
            '--model_path', 'unused', '--phase', '3', '--output_dir', str(out), '--data_mean', '1000', '--data_stddev', '500', '--seed', '11',
            '--device', 'cpu', '--steps', '25', '--lr', '0.1', '--levels', '3', '--out_dtype', 'int16', str(target), *more]


def _linear_generator():
    rng = np.random.default_rng(99)
    A = torch.from_numpy(rng.standard_normal((LAT, int(np.prod(SHAPE)))).astype(np.float32) * 0.3)
    # (a product and a sum over one axis, row by row: a row's values do not depend on what else is in the batch, as a BLAS call's might)
    return lambda z, cond: (z[:, :, None] * A[None]).sum(dim=1).view(z.shape[0], *SHAPE)


@pytest.fixture(scope='module')
def targets(tmp_path_factory):
    root = tmp_path_factory.mktemp('project_host')
    gen = _linear_generator()
    z = torch.from_numpy(np.random.default_rng(5).standard_normal((5, LAT)).astype(np.float32))
    vols = (gen(z, None).numpy() * 500 + 1000).astype(np.int16)
    os.makedirs(root / 'targets')
    for i, v in enumerate(vols):
        np.save(root / 'targets' / f'vol_{i}.npy', v[0])
    return dict(root=root, dir=root / 'targets', vols=vols)


def _run(argv):
    from saragan_amd import project as P
    return P.run(P.build_parser().parse_args(argv), generator=_linear_generator(), out=open(os.devnull, 'w'))


def test_tool_on_the_cpu_replays_from_its_record(targets):
    from saragan_amd import project as P
    out = targets['root'] / 'run_a'
    rec = _run(_argv(targets['dir'], out, '--batch_size', '2', '--restarts', '2', '--residual_dir', str(out / 'resid')))
    d = out / 'projected_3'
    names = [f'vol_{i}.npy' for i in range(5)]
    assert sorted(os.listdir(d)) == sorted(names + ['latents.npy', 'projection.json'])
    js = json.load(open(d / 'projection.json'))
    assert js['files'] == rec['files'] and [f['name'] for f in js['files']] == names and js['definition'] == F().PROJECT_DEFINITION
    assert js['latent'] == P.LATENT_RULE and set(js['seconds']) == {'load', 'optimise', 'reconstruct', 'save', 'wall'}
    lat = np.load(d / 'latents.npy')
    assert lat.shape == (5, LAT) and lat.dtype == np.float32
    gen = _linear_generator()
    for f in js['files']:
        # the initial latent from the record alone: its loss is the recorded one, to the bit
        z0 = np.random.default_rng([js['seed'], f['index'], f['restart']]).standard_normal(js['latent_dim'], dtype=np.float32)
        table = torch.from_numpy(targets['vols'][f['index']][None])
        loss0, _, _ = F().multiscale_residual_raw(gen(torch.from_numpy(z0)[None], None), table, [0], js['shift'], js['scale'], js['levels'],
                                                  js['level_weights'])
        assert float(loss0[0]) == f['initial_loss'] and not f['failed']
        assert f['best_loss'] < 0.5 * f['initial_loss'] and 1 <= f['best_step'] <= 26
        # the saved latent reproduces the best loss, the terms and the reconstruction file
        y = gen(torch.from_numpy(lat[f['index']])[None], None)
        loss, terms, _ = F().multiscale_residual_raw(y, table, [0], js['shift'], js['scale'], js['levels'], js['level_weights'])
        assert float(loss[0]) == f['best_loss'] and terms[0].tolist() == f['terms']
        recon = np.load(d / f['name'])
        assert recon.dtype == np.int16 and recon.shape == (4, 8, 8)
        want = F().store_volumes(y, torch.int16, scale=500.0, shift=1000.0).numpy()[0, 0]
        assert np.array_equal(recon, want)
        x = targets['vols'][f['index']][0].astype(np.int64)
        assert np.array_equal(np.load(out / 'resid' / f['name']).astype(np.int64), np.abs(x - recon))
        assert f['rms'] == float(np.sqrt(np.mean((x - recon).astype(np.float64) ** 2)))
    assert js['pooled']['files'] == 5 and js['pooled']['rms_q1'] <= js['pooled']['rms_median'] <= js['pooled']['rms_q3']
    # another batch size: the same latents, to the bit (every row's arithmetic is its own)
    rec_b = _run(_argv(targets['dir'], targets['root'] / 'run_b', '--batch_size', '5', '--restarts', '2'))
    assert np.array_equal(np.load(targets['root'] / 'run_b' / 'projected_3' / 'latents.npy'), lat)
    assert [f['best_loss'] for f in rec_b['files']] == [f['best_loss'] for f in js['files']]
    # sphere: the latents sit on the sphere of radius sqrt(L)
    _run(_argv(targets['dir'], targets['root'] / 'run_c', '--latent_norm', 'sphere', '--max_samples', '2'))
    lat_c = np.load(targets['root'] / 'run_c' / 'projected_3' / 'latents.npy')
    assert lat_c.shape == (2, LAT)


def test_tool_refusals(targets, tmp_path):
    from saragan_amd import project as P
    plan = lambda argv: P.plan(P.build_parser().parse_args(argv))  # noqa: E731
    empty = tmp_path / 'empty'
    os.makedirs(empty)
    with pytest.raises(ValueError, match='holds no .npy'):
        plan(_argv(empty, tmp_path))
    mixed = tmp_path / 'mixed'
    os.makedirs(mixed)
    np.save(mixed / 'a.npy', np.zeros((4, 8, 8), np.int16))
    np.save(mixed / 'b.npy', np.zeros((4, 8, 4), np.int16))
    with pytest.raises(ValueError, match='one shape and one dtype'):
        plan(_argv(mixed, tmp_path))
    np.save(mixed / 'b.npy', np.zeros((4, 8, 8), np.uint16))
    with pytest.raises(ValueError, match='one shape and one dtype'):
        plan(_argv(mixed, tmp_path))
    os.remove(mixed / 'b.npy')
    np.save(mixed / 'a.npy', np.zeros((4, 8, 8), np.float64))
    with pytest.raises(ValueError, match='volumes are uint8'):
        plan(_argv(mixed, tmp_path))
    np.save(mixed / 'a.npy', np.zeros((8, 16, 16), np.int16))
    with pytest.raises(ValueError, match='phase 3 of'):
        plan(_argv(mixed, tmp_path))
    with pytest.raises(ValueError, match='not a multiple of 2\\^3'):
        plan(_argv(targets['dir'], tmp_path, '--levels', '4'))
    with pytest.raises(ValueError, match='--level_weights is 3 numbers'):
        plan(_argv(targets['dir'], tmp_path, '--level_weights', '1,2'))
    with pytest.raises(ValueError, match='--png renders on the device'):
        plan(_argv(targets['dir'], tmp_path, '--png'))
    with pytest.raises(ValueError, match='hand run\\(\\) a generator'):
        P.run(P.build_parser().parse_args(_argv(targets['dir'], tmp_path)))
    os.makedirs(tmp_path / 'projected_3')
    np.save(tmp_path / 'projected_3' / 'vol_3.npy', np.zeros(1))
    with pytest.raises(FileExistsError, match='--overwrite'):
        plan(_argv(targets['dir'], tmp_path))
    with pytest.raises(SystemExit, match='project: .*--overwrite'):
        P.main(_argv(targets['dir'], tmp_path))
    assert plan(_argv(targets['dir'], tmp_path, '--overwrite'))['names'][3] == 'vol_3.npy'
    assert os.listdir(tmp_path / 'projected_3') == ['vol_3.npy']      # nothing was written


def test_schedule_ramps_up_linearly_and_down_by_a_cosine():
    from saragan_amd import project as P
    a = P.build_parser().parse_args(_argv('x', 'y', '--steps', '100', '--lr', '0.05'))
    lrs = [P.lr_at(i, a) for i in range(100)]
    assert lrs[0] == pytest.approx(0.01) and lrs[4] == pytest.approx(0.05) and all(v == pytest.approx(0.05) for v in lrs[4:76])
    assert all(x > y_ for x, y_ in zip(lrs[75:], lrs[76:])) and lrs[-1] > 0 and lrs[-1] < 0.001


def test_generate_takes_a_latent_table(tmp_path):
    from saragan_amd import generate as G
    np.save(tmp_path / 'lat.npy', np.zeros((7, LAT), np.float32))
    base = ['pgan', '--start_shape', '(1, 1, 2, 2)', '--final_shape', '(1, 4, 8, 8)', '--network_size', 'xs', '--latent_dim', str(LAT),
            '--model_path', 'unused', '--phase', '3', '--output_dir', str(tmp_path)]
    args = G.build_parser().parse_args(base + ['--latents_path', str(tmp_path / 'lat.npy')])
    p = G.plan(args, env={})
    assert args.num_samples == 7 and p['indices'] == list(range(7)) and p['latents'].shape == (7, LAT)
    assert G.plan(G.build_parser().parse_args(base + ['--latents_path', str(tmp_path / 'lat.npy'), '--num_samples', '3']), env={})['indices'] == [0, 1, 2]
    with pytest.raises(ValueError, match='exceeds the 7 rows'):
        G.plan(G.build_parser().parse_args(base + ['--latents_path', str(tmp_path / 'lat.npy'), '--num_samples', '8']), env={})
    np.save(tmp_path / 'bad.npy', np.zeros((7, LAT + 1), np.float32))
    with pytest.raises(ValueError, match='expected float32'):
        G.plan(G.build_parser().parse_args(base + ['--latents_path', str(tmp_path / 'bad.npy')]), env={})
    with pytest.raises(ValueError, match='--num_samples is required'):
        G.plan(G.build_parser().parse_args(base), env={})
    assert G.plan(G.build_parser().parse_args(base + ['--num_samples', '2']), env={})['latents'] is None
