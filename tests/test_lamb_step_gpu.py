"""--optimizer LAMB / AdamW through the whole training step (optimization.optimize_step + Session.run): three steps against
the fp64 oracle stepping with the rules of tests/lamb_rules.py, both strategies, and the captured step against the eager one."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests.lamb_rules import RULES
from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT, load_step_fixture
from tests.test_step_gpu import FIXTURES

pytestmark = pytest.mark.gpu
DECAY = 0.01


@pytest.mark.parametrize('kind', ['LAMB', 'AdamW'])
@pytest.mark.parametrize('strategy', ['simultaneous', 'alternate'])
def test_lamb_and_adamw_steps_match_oracle(golden_dir, kind, strategy):
    import saragan_amd
    saragan_amd.set_deterministic(True)
    try:
        _steps_match_oracle(golden_dir, kind, strategy)
    finally:
        saragan_amd.set_deterministic(False)


def _steps_match_oracle(golden_dir, kind, strategy):
    """The pattern of test_other_optimizers_match_oracle: same fixture, f32, get_optimizer from the command line's
    namespace, global-norm clipping on for 'simultaneous' (the clipped gradient reaches the rule with gscale = 1), EMA fused.
    Losses, weights and shadows to that test's non-Adadelta tolerances, plus, element by element, the distance between the
    exact oracle and oracle runs whose rules read f32 gradients (tests/lamb_rules.py, f32_error).  The steps run in the
    reproducible mode, so the gradient sums have one order and the case has one outcome."""
    import saragan_amd.optimization as opt
    from oracle import pgan_oracle as O
    from saragan_amd.ExtendedEMA import ExtendedEMA
    from saragan_amd.networks import loss as L
    from saragan_amd.networks.ops import ScalarVariable
    from saragan_amd.networks.pgan.discriminator import discriminator
    from saragan_amd.networks.pgan.generator import generator
    from saragan_amd.varstore import VariableStore, set_compute_dtype, use_store
    fx = load_step_fixture(os.path.join(golden_dir, FIXTURES[3]), torch.float64)
    lr = 1e-3
    set_compute_dtype(torch.float32)
    store = VariableStore('cuda', seed=0)
    L.set_random_source(L.InjectedRandom({k: v.float() for k, v in fx['rnd'].items()}))
    a = argparse.Namespace(optimizer=kind, d_optimizer=kind, adam_beta1=0.0, adam_beta2=0.9, d_adam_beta1=0.0,
                           d_adam_beta2=0.9, weight_decay=DECAY, d_weight_decay=DECAY)
    og, od = opt.get_optimizer(ScalarVariable(lr, 'd_lr'), ScalarVariable(lr, 'g_lr'), a)
    ph = opt.Placeholder([4, 1, 1, 1, 1])
    clip = strategy == 'simultaneous'
    with use_store(store):
        tup = opt.optimize_step(og, od, generator, discriminator, ph, LATENT, ScalarVariable(fx['alpha'], 'alpha'), fx['phase'],
                                BASE_SHAPE, KERNEL_SPEC, FILTER_SPEC, 'leaky_relu', 0.2, fx['loss_fn'], fx['cfg']['gp_weight'],
                                strategy, clip, clip, 0.01, None)
    store.load_state_dict(fx['p0'], strict=True)
    ema = ExtendedEMA(list(store.vars.keys()), 0.99, graph=tup[0].graph)
    sess = opt.Session('cuda')
    # Three oracle runs: the fp64 rule on exact gradients, and on gradients as f32 hands them over, moved up and moved down
    # (lamb_rules f32_error = +1, -1).  Both rules divide by sqrt(v) + eps with eps = 1e-6, and AdamW, without bias correction,
    # starts at u = g / (0.316 |g| + eps): where |g| is under eps, u follows the absolute error of g at 1 / eps, and lr / eps
    # = 1e3 times an error of 2e-8 is the whole atol.  The fixture has such elements: 9 of the 16 of discriminator_out/dense_1/
    # bias are sums that cancel to 1e-7 beside a largest element of 0.3.  There the runs lie up to 1.8e-5 (step 1) to 4.5e-5
    # (step 3) apart for AdamW and 4e-6 for LAMB; 4e-6 and less in every other variable; rounding alone moves nothing (2e-10).
    runs = []
    for err in (None, 1, -1):
        p = {k: v.clone() for k, v in fx['p0'].items()}
        runs.append(dict(p=p, shadow={k: v.clone() for k, v in p.items()},
                         rg=RULES[kind](0.0, 0.9, DECAY, f32_error=err), rd=RULES[kind](0.0, 0.9, DECAY, f32_error=err)))
    p, shadow = runs[0]['p'], runs[0]['shadow']

    def close(got, name, what, step):
        want = runs[0][what][name]
        err = (got.double().cpu() - want).abs()
        bound = 2e-5 + 2e-4 * want.abs() + torch.maximum((want - runs[1][what][name]).abs(), (want - runs[2][what][name]).abs())
        over = err - bound
        assert bool((over <= 0).all()), (f'{kind} {strategy} step {step} {what} {name}: {int((over > 0).sum())} of {err.numel()} '
                                          f'elements outside rtol 2e-4, atol 2e-5 + the oracles\' distance; worst |err| '
                                          f'{float(err.flatten()[over.argmax()]):.3e} against {float(bound.flatten()[over.argmax()]):.3e}')

    for step in range(3):
        _, _, gl, dl = sess.run([tup[0], tup[1], tup[2], tup[3]], feed_dict={ph: fx['real'].float()})
        sess.run(ema.apply())
        for r in runs:
            if strategy == 'simultaneous':
                out = O.step_simultaneous(r['p'], r['rg'], r['rd'], r['shadow'], fx['rnd'], fx['real'], fx['alpha'], fx['cfg'], lr,
                                          lr, g_clipping=True, d_clipping=True)
            else:
                out = O.step_alternate(r['p'], r['rg'], r['rd'], r['shadow'], fx['rnd'], fx['real'], fx['alpha'], fx['cfg'], lr, lr)
            r['out'] = out
        ref = runs[0]['out']
        np.testing.assert_allclose(float(gl), float(ref['gen_loss']), rtol=1e-4, atol=1e-5, err_msg=f'step {step}')
        np.testing.assert_allclose(float(dl), float(ref['disc_loss']), rtol=1e-4, atol=1e-5, err_msg=f'step {step}')
        worst = max(float((v.detach().double().cpu() - p[k]).abs().max()) for k, v in store.vars.items())
        allow = max(float((p[k] - r['p'][k]).abs().max()) for k in p for r in runs[1:])
        print(f'{kind} {strategy} step {step}: max |w - oracle| = {worst:.3e}, max oracle distance = {allow:.3e}')
        for k, v in store.vars.items():
            close(v.detach(), k, 'p', step)
            close(ema.average(k), k, 'shadow', step)
    assert (og.sync_step_count(), od.sync_step_count()) == (3, 3)
    if kind == 'LAMB':
        assert int(og.t_dev) == 3 and int(od.t_dev) == 3


@pytest.mark.parametrize('kind', ['LAMB', 'AdamW'])
def test_captured_step_equals_eager_step_bit_for_bit(golden_dir, kind, monkeypatch):
    """What tests/test_hipgraph_gpu.py asserts for Adam, on its own harness with the optimiser swapped: in reproducible mode
    the captured run (two eager warm-up steps, one capture, replays) gives the eager run's losses, weights and shadows bit
    for bit under a moving learning rate -- LAMB's step count lives on the device and is advanced by the replayed launches."""
    import saragan_amd
    import saragan_amd.optimization as opt
    from tests.test_hipgraph_gpu import _run
    cls = {'LAMB': opt.LAMBOptimizer, 'AdamW': opt.AdamWOptimizer}[kind]
    made = []

    def make(lr, beta1, beta2):
        made.append(cls(lr, beta1, beta2, weight_decay_rate=DECAY))
        return made[-1]
    monkeypatch.setattr(opt, 'AdamOptimizer', make)
    steps = 6
    saragan_amd.set_deterministic(True)
    try:
        w0, l0, n0 = _run(golden_dir, steps, torch.float32, captured=False)
        w1, l1, n1 = _run(golden_dir, steps, torch.float32, captured=True)
    finally:
        saragan_amd.set_deterministic(False)
    assert len(made) == 4 and all(type(o) is cls for o in made)
    assert n0 == 0 and n1 == 1
    assert l0 == l1, (l0, l1)
    bad = [k for k in w0 if not torch.equal(w0[k], w1[k])]
    assert not bad, bad
    assert all(abs(v) < 1e6 for pair in l0 for v in pair)
    assert [o.sync_step_count() for o in made] == [steps] * 4      # host count == applied steps, eager and captured
    if kind == 'LAMB':
        assert [int(o.t_dev) for o in made] == [steps] * 4
