"""Host side of --optimizer LAMB / AdamW (SURFGAN_2D/optim.py:60-80): get_optimizer, the command line, the block map of the
segment table, and the fp64 statement of the two rules (tests/lamb_rules.py) that the GPU tests compare against."""
import argparse

import pytest
import torch

from tests.lamb_rules import AdamWRule, LAMBRule, decays, trust_ratio


def _ns(kind, **kw):
    base = dict(optimizer=kind, d_optimizer=kind, adam_beta1=0.1, adam_beta2=0.9, d_adam_beta1=0.2, d_adam_beta2=0.8)
    base.update(kw)
    return argparse.Namespace(**base)


@pytest.mark.parametrize('kind', ['LAMB', 'AdamW'])
def test_get_optimizer_builds_the_new_classes_for_both_networks(kind):
    import saragan_amd.optimization as opt
    cls = {'LAMB': opt.LAMBOptimizer, 'AdamW': opt.AdamWOptimizer}[kind]
    og, od = opt.get_optimizer(2e-3, 1e-3, _ns(kind, weight_decay=0.01, d_weight_decay=0.02))
    assert type(og) is cls and type(od) is cls
    assert (og.lr, og.beta1, og.beta2, og.weight_decay_rate, og.epsilon) == (1e-3, 0.1, 0.9, 0.01, 1e-6)
    assert (od.lr, od.beta1, od.beta2, od.weight_decay_rate, od.epsilon) == (2e-3, 0.2, 0.8, 0.02, 1e-6)
    og, od = opt.get_optimizer(2e-3, 1e-3, _ns(kind))               # no decay flags: 0
    assert og.weight_decay_rate == 0.0 and od.weight_decay_rate == 0.0
    og, od = opt.get_optimizer(2e-3, 1e-3, _ns(kind, weight_decay=0.03))
    assert od.weight_decay_rate == 0.03                             # D inherits G's rate
    assert og.t == 0 and og.t_dev is None


def test_unknown_optimizer_still_raises():
    import saragan_amd.optimization as opt
    with pytest.raises(NotImplementedError):
        opt.get_optimizer(1e-3, 1e-3, _ns('Lion'))


def test_command_line_takes_the_new_choices_and_decay_flags():
    from saragan_amd.main import build_parser, finalize_args
    base = ['pgan', '/data/', '--start_shape', '(1, 5, 16, 16)', '--final_shape', '(1, 160, 512, 512)', '--starting_phase', '1',
            '--ending_phase', '4', '--latent_dim', '128', '--network_size', 's', '--noise_stddev', '0.01']
    a = finalize_args(build_parser().parse_args(base))
    assert (a.optimizer, a.d_optimizer, a.weight_decay, a.d_weight_decay) == ('Adam', 'Adam', 0.0, 0.0)
    a = finalize_args(build_parser().parse_args(base + ['--optimizer', 'LAMB', '--weight_decay', '0.01', '--d_weight_decay', '0.5']))
    assert (a.optimizer, a.d_optimizer, a.weight_decay, a.d_weight_decay) == ('LAMB', 'LAMB', 0.01, 0.01)
    a = finalize_args(build_parser().parse_args(base + ['--optimizer', 'AdamW', '--d_use_different_optimizer', '--d_optimizer', 'LAMB',
                                                        '--weight_decay', '0.01', '--d_use_different_weight_decay',
                                                        '--d_weight_decay', '0.5']))
    assert (a.optimizer, a.d_optimizer, a.weight_decay, a.d_weight_decay) == ('AdamW', 'LAMB', 0.01, 0.5)
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ['--optimizer', 'Lion'])


def test_block_map_of_the_segment_table():
    from saragan_amd import _lib
    from saragan_amd.functional import segment_table_arrays
    ch = _lib.SG_SEG_CHUNK
    segs, blocks = segment_table_arrays([(0, 1, True), (4, 3 * ch + 5, False), (4 * ch + 12, ch, True)], 6 * ch)
    assert segs == [[0, 1, 1, 0], [4, 3 * ch + 5, 0, 1], [4 * ch + 12, ch, 1, 5]]
    assert blocks == [[0, 0], [1, 0], [1, 1], [1, 2], [1, 3], [2, 0]]
    for bad in ([(2, 4, True)], [(0, 8, True), (4, 4, True)], [(0, 0, True)], [(0, 6 * ch + 1, True)], []):
        with pytest.raises(ValueError):
            segment_table_arrays(bad, 6 * ch)


def test_decay_exclusion_is_by_the_substring_bias():
    import saragan_amd.optimization as opt
    names = {'generator/generator_in/dense/weight': True, 'generator/generator_in/dense/bias': False,
             'discriminator/from_rgb_3/bias': False, 'discriminator/biased/weight': False, 'generator/to_rgb_2/weight': True}
    for n, want in names.items():
        assert decays(n) is want and opt.decays(n) is want, n
    g = {n: torch.zeros(3, dtype=torch.float64) for n in names}      # zero gradient: only the decay moves a weight
    for rule in (AdamWRule(0.5, 0.9, 0.25), LAMBRule(0.5, 0.9, 0.25)):
        p = {n: torch.full((3,), 2.0, dtype=torch.float64) for n in names}
        rule.apply(p, g, 0.1)
        for n, want in names.items():
            assert bool((p[n] != 2.0).all()) is want, n


@pytest.mark.parametrize('lam', [0.0, 0.01])
def test_rules_agree_with_the_closed_form_at_step_one(lam):
    """beta1 = 0, t = 1: m = g, v = (1-b2) g^2; LAMB's corrections give m^ = g, v^ = g^2, so u = g / (|g| + eps) + lam*w."""
    gen = torch.Generator().manual_seed(0)
    w = torch.randn(37, dtype=torch.float64, generator=gen)
    g = torch.randn(37, dtype=torch.float64, generator=gen)
    lr, b2, eps = 1e-2, 0.9, 1e-6
    rule = LAMBRule(0.0, b2, lam)
    p = {'x/weight': w.clone()}
    rule.apply(p, {'x/weight': g}, lr)
    u = g / (g.abs() + eps) + lam * w
    r = float(torch.linalg.vector_norm(w) / torch.linalg.vector_norm(u))
    torch.testing.assert_close(p['x/weight'], w - lr * r * u, rtol=1e-13, atol=1e-15)
    assert rule.ratios['x/weight'] == pytest.approx(r, rel=1e-13)
    rule = AdamWRule(0.0, b2, lam)                                   # no bias correction: sqrt(v) = sqrt(1-b2) |g|
    p = {'x/weight': w.clone()}
    rule.apply(p, {'x/weight': g}, lr)
    u = g / ((1 - b2) ** 0.5 * g.abs() + eps) + lam * w
    torch.testing.assert_close(p['x/weight'], w - lr * u, rtol=1e-13, atol=1e-15)


def test_both_ratio_fallbacks_are_exactly_one():
    z, x = torch.zeros(5, dtype=torch.float64), torch.full((5,), 3.0, dtype=torch.float64)
    assert trust_ratio(z, x) == 1.0 and trust_ratio(x, z) == 1.0 and trust_ratio(z, z) == 1.0
    assert trust_ratio(x, 2 * x) == 0.5
    rule = LAMBRule(0.5, 0.9, 0.0)
    p = {'a/bias': z.clone(), 'b/weight': x.clone()}                 # |w| = 0 with a gradient; |u| = 0 (g = 0, no decay)
    rule.apply(p, {'a/bias': x, 'b/weight': z}, 0.1)
    assert rule.ratios == {'a/bias': 1.0, 'b/weight': 1.0}
    assert torch.equal(p['b/weight'], x)
    u = (0.5 * x / 0.5) / (torch.sqrt(0.1 * x * x / 0.1) + 1e-6)
    torch.testing.assert_close(p['a/bias'], -0.1 * u, rtol=1e-13, atol=0)
