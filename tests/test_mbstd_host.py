"""Host-side checks of the minibatch-stddev feature (no GPU): the fp64 closed forms of tests/mbstdref.py against torch's own
double backward, the rank-1 identity against the reference layer followed by a convolution, segments against separate calls, the
product's tap mask, the --d_mbstd_group flag with its start-up refusals, the module switch, the variable plan and the
zero-initialised restore of a checkpoint written without the flag."""
import os

import numpy as np
import pytest
import torch

from oracle import pgan_oracle as O
from tests import mbstdref as M

CASES = [(8, 16, (1, 4, 4), 4, 1), (8, 16, (2, 4, 4), 4, 2), (2, 8, (1, 4, 4), 4, 1), (1, 8, (1, 4, 4), 4, 1),
         (12, 24, (1, 4, 4), 4, 1), (4, 20, (1, 3, 5), 4, 1)]


def _x(n, c, ext, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, c, *ext), generator=g, dtype=torch.float64)


@pytest.mark.parametrize('n,c,ext,group,nseg', CASES)
def test_closed_forms_equal_torchs_double_backward(n, c, ext, group, nseg):
    x = _x(n, c, ext, 1).requires_grad_(True)
    gstat = _x(n, 1, (1, 1, 1), 2).reshape(n).requires_grad_(True)
    h = _x(n, c, ext, 3)
    s = M.stat_torch(x, group, nseg)
    assert torch.allclose(s, M.stat(x.detach(), group, nseg)[0], rtol=1e-14, atol=0)
    (dx,) = torch.autograd.grad(s, x, gstat, create_graph=True)
    assert torch.allclose(dx, M.stat_bwd(gstat.detach(), x.detach(), group, nseg), rtol=1e-12, atol=1e-15)
    ggstat, gx = torch.autograd.grad(dx, [gstat, x], h)
    want_gg, _, want_gx = M.stat_bwd2(h, x.detach(), gstat.detach(), group, nseg)
    assert torch.allclose(ggstat, want_gg, rtol=1e-11, atol=1e-15)
    assert torch.allclose(gx, want_gx, rtol=1e-10, atol=1e-14)


def test_statistic_is_the_reference_layers_channel():
    x = _x(8, 6, (2, 3, 4), 4)
    y = O.minibatch_stddev_layer(x, 4)
    s, _ = M.stat(x, 4)
    assert torch.allclose(y[:, -1], s.reshape(-1, 1, 1, 1).expand(-1, 2, 3, 4), rtol=1e-14, atol=0)
    # G = 1: every deviation is zero, the statistic is sqrt(1e-8)
    assert torch.allclose(M.stat(_x(1, 8, (1, 4, 4), 5), 4)[0], torch.full((1,), 1e-4, dtype=torch.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize('k', [(3, 3, 3), (1, 3, 3)])
def test_rank_one_identity_against_the_concatenated_convolution(k):
    n, c, ext, cout = 8, 5, (2, 4, 4), 7
    x = _x(n, c, ext, 6)
    g = torch.Generator().manual_seed(7)
    w = torch.randn((*k, c + 1, cout), generator=g, dtype=torch.float64)
    want = O.conv3d(O.minibatch_stddev_layer(x, 4), w, 'leaky_relu', 0.2)
    coef = O.runtime_coef(w.shape, 'leaky_relu', 0.2)
    y = torch.nn.functional.conv3d(x, (w[..., :c, :] * coef).permute(4, 3, 0, 1, 2), padding=tuple(kk // 2 for kk in k))
    got = M.term(y, M.stat(x, 4)[0], M.plane(w[..., c:, :], coef, ext))
    assert float((got - want).abs().max()) < 1e-12


def test_two_segments_equal_two_separate_calls():
    x, gstat, h = _x(8, 16, (2, 4, 4), 8), _x(8, 1, (1, 1, 1), 9).reshape(8), _x(8, 16, (2, 4, 4), 10)
    for fn, args in ((lambda a, b: M.stat(a, 4, b)[0], (x,)), (lambda g_, a, b: M.stat_bwd(g_, a, 4, b), (gstat, x)),
                     (lambda h_, a, g_, b: M.stat_bwd2(h_, a, g_, 4, b)[0], (h, x, gstat)),
                     (lambda h_, a, g_, b: M.stat_bwd2(h_, a, g_, 4, b)[2], (h, x, gstat))):
        both = fn(*args, 2)
        halves = torch.cat([fn(*[a[:4] for a in args], 1), fn(*[a[4:] for a in args], 1)], dim=0)
        assert torch.equal(both, halves)
    assert not torch.equal(M.stat(x, 4, 2)[0], M.stat(x, 4, 1)[0])      # one segment groups the samples m, m + 2, ... instead


def test_the_products_tap_mask_is_the_helpers():
    from saragan_amd import functional as F
    for ext, k in (((2, 4, 4), (3, 3, 3)), ((1, 4, 4), (1, 3, 3)), ((1, 3, 5), (3, 3, 3))):
        m = F.mbstd_tap_mask(ext, k, 0.5, 'cpu')
        assert m.dtype == torch.float32 and torch.equal(m.double(), 0.5 * M.tap_mask(ext, k))
        assert F.mbstd_tap_mask(ext, k, 0.5, 'cpu') is m                 # built once


BASE = ['pgan', '/data/', '--start_shape', '(1, 5, 16, 16)', '--final_shape', '(1, 160, 512, 512)', '--starting_phase', '1',
        '--ending_phase', '4', '--latent_dim', '128', '--network_size', 's', '--noise_stddev', '0.01', '--base_batch_size', '32']


def test_flag_and_start_up_refusals():
    from saragan_amd.main import build_parser, finalize_args
    a = finalize_args(build_parser().parse_args(BASE))
    assert a.d_mbstd_group == 0
    a = finalize_args(build_parser().parse_args(BASE + ['--d_mbstd_group', '4']))      # batches 32, 16, 8, 4
    assert a.d_mbstd_group == 4
    help_text = build_parser().format_help()
    assert '--d_mbstd_group' in help_text and 'local to a rank' in ' '.join(help_text.split())
    with pytest.raises(SystemExit, match='>= 0'):
        finalize_args(build_parser().parse_args(BASE + ['--d_mbstd_group', '-1']))
    with pytest.raises(SystemExit, match='pgan architecture only'):
        finalize_args(build_parser().parse_args(['pgandeep'] + BASE[1:] + ['--d_mbstd_group', '4']))
    with pytest.raises(SystemExit, match='does not divide the per-process batch 6 of phase 3'):
        finalize_args(build_parser().parse_args(BASE[:-1] + ['24', '--d_mbstd_group', '4']))      # batches 24, 12, 6
    # a batch smaller than the group is one group of that size (G = min(group, n))
    finalize_args(build_parser().parse_args(BASE[:-1] + ['2', '--d_mbstd_group', '4']))


def test_module_switch_plan_and_segments():
    from saragan_amd.networks import ops as nops
    from saragan_amd.networks.pgan.variables import pgan_variable_shapes
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT
    assert nops.minibatch_stddev_settings() == 0
    off = pgan_variable_shapes(3, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC)
    assert not any('mbstd' in k for k in off)
    prev = nops.set_minibatch_stddev(4)
    try:
        assert prev == 0 and nops.minibatch_stddev_settings() == 4
        on = pgan_variable_shapes(3, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC)
        assert [k for k in on if k not in off] == [M.MBSTD_WEIGHT]
        assert on[M.MBSTD_WEIGHT] == (*KERNEL_SPEC[0][1], 1, FILTER_SPEC[0][0])
        want = M.variable_shapes(3, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC)
        assert {k: tuple(v) for k, v in on.items()} == {k: tuple(v) for k, v in want.items()}
        with pytest.raises(ValueError):
            nops.set_minibatch_stddev(-1)
        assert nops._MBSTD['segments'] == 1
        with nops.mbstd_segments(2):
            assert nops._MBSTD['segments'] == 2
        assert nops._MBSTD['segments'] == 1
        from saragan_amd.networks.pgandeep.discriminator import discriminator as deep
        from saragan_amd.networks2d.pgan.discriminator import discriminator as flat
        with pytest.raises(NotImplementedError, match='pgandeep'):
            deep(None, 0.0, 1, LATENT, 'leaky_relu', KERNEL_SPEC, FILTER_SPEC, param=0.2)
        with pytest.raises(NotImplementedError, match='2-D'):
            flat(None, 0.0, 1, 3, 4, LATENT, 'leaky_relu', param=0.2)
    finally:
        nops.set_minibatch_stddev(prev)
    assert nops.minibatch_stddev_settings() == 0


def test_restore_of_a_checkpoint_without_the_weight_starts_it_from_zeros(tmp_path, capsys):
    from saragan_amd.utils import restore_variables, save_checkpoint
    from saragan_amd.varstore import VariableStore
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT
    shapes = M.variable_shapes(1, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC)
    old = VariableStore('cpu', seed=1)
    for k, s in shapes.items():
        if k != M.MBSTD_WEIGHT:
            old.get(k, s, 'normal')
    save_checkpoint(old, str(tmp_path / 'model_1'))
    new = VariableStore('cpu', seed=2)
    for k, s in shapes.items():
        new.get(k, s, 'normal')
    assert float(new.vars[M.MBSTD_WEIGHT].detach().abs().max()) > 0
    restore_variables(new, 1, 1, str(tmp_path), str(tmp_path / 'model_1'), list(new.vars), False)
    assert 'written without --d_mbstd_group' in capsys.readouterr().out
    assert float(new.vars[M.MBSTD_WEIGHT].detach().abs().max()) == 0
    assert all(torch.equal(new.vars[k], old.vars[k]) for k in old.vars)
    # the other way round: the checkpoint has the weight, the run does not
    save_checkpoint(new, str(tmp_path / 'with'))
    with pytest.raises(ValueError, match='--d_mbstd_group'):
        restore_variables(old, 1, 1, str(tmp_path), str(tmp_path / 'with'), list(old.vars), False)
    # any other missing variable is still an error
    del old.vars['discriminator/discriminator_out/bias']
    save_checkpoint(old, str(tmp_path / 'short'))
    with pytest.raises(KeyError):
        restore_variables(new, 1, 1, str(tmp_path), str(tmp_path / 'short'), list(new.vars), False)


def _share(got, ref, rtol, atol):
    """The largest |got - ref| / (atol + rtol |ref|): the share of an assert_allclose tolerance that an error uses."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(got - ref) / (atol + rtol * np.abs(ref))))


STEP_CASES = [(name, loss, strat) for name in ('oracle_step_p2_wgan_a060.npz', 'oracle_step_p3_wgan_a000.npz')
              for loss in ('wgan', 'logistic') for strat in ('simultaneous', 'alternate')]


@pytest.mark.parametrize('name,loss_fn,strategy', STEP_CASES)
def test_oracle_architecture_in_float32_uses_less_than_half_of_the_step_tolerances(golden_dir, name, loss_fn, strategy):
    """Before tests/test_mbstd_gpu.py relies on tests/test_step_gpu.py's tolerances for the architecture with the layer: the oracle
    itself in float32 against float64, on that test's inputs (the fixture's weights and randomness, the statistic channel's filter
    as a store of seed 0 draws it), must stay within half of each of them."""
    from saragan_amd.networks import ops as nops
    from saragan_amd.networks.pgan.variables import pgan_variable_shapes
    from saragan_amd.varstore import VariableStore
    from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture
    fx = load_step_fixture(os.path.join(golden_dir, name), torch.float64)
    prev = nops.set_minibatch_stddev(4)
    try:
        store = VariableStore('cpu', seed=0)
        for k, shp in pgan_variable_shapes(fx['phase'], BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC).items():
            store.get(k, shp, 'normal' if k.endswith('weight') else 'zeros')
    finally:
        nops.set_minibatch_stddev(prev)
    store.load_state_dict(dict(fx['p0']))
    M.register()
    cfg = dict(fx['cfg'], loss_fn=loss_fn, arch=M.ARCH)
    fn = O.step_simultaneous if strategy == 'simultaneous' else O.step_alternate
    res = {}
    for dt in (torch.float64, torch.float32):
        p = {k: v.detach().to(dt).clone() for k, v in store.vars.items()}
        with M.configured(4):
            res[dt] = fn(p, O.TFAdam(0.0, 0.9), O.TFAdam(0.0, 0.9), None, {k: v.to(dt) for k, v in fx['rnd'].items()},
                         fx['real'].to(dt), fx['alpha'], cfg, 1e-3, 1e-3, freeze=fx['freeze'])
            if dt == torch.float64:
                logits = {d: M.discriminator({k: v.detach().to(d) for k, v in store.vars.items()}, fx['real'].to(d), fx['alpha'],
                                             fx['phase'], LATENT, 'leaky_relu', KERNEL_SPEC, FILTER_SPEC, param=0.2)
                          for d in (torch.float64, torch.float32)}
    r64, r32 = res[torch.float64], res[torch.float32]
    shares = {'logits': _share(logits[torch.float32], logits[torch.float64], 1e-4, 1e-5)}
    for k in ('gen_loss', 'disc_loss'):
        shares[k] = _share(r32[k], r64[k], 1e-4, 1e-5)
    gp = r64['gp_loss'].numpy()
    shares['gp_loss'] = _share(r32['gp_loss'], gp, 1e-3, 1e-5 * max(1.0, np.abs(gp).max()))
    assert M.MBSTD_WEIGHT in r64['d_grads']
    for k, g in r64['d_grads'].items():
        shares[k] = _share(r32['d_grads'][k], g, 1e-3, 1e-4 * float(g.abs().max()) + 1e-9)
    worst = max(shares, key=shares.get)
    print(name, loss_fn, strategy, 'largest share of a tolerance:', worst, shares[worst])
    assert shares[worst] <= 0.5, shares
