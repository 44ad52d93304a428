"""sg_latent_step against its numpy twin, bit for bit: ten chained steps of z, m, v, best_loss, z_best and
best_step, with a NaN loss in one row on the way and an equal loss that must not replace the best.  The twin itself is pinned to a
scalar Python loop in tests/test_project_host.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ('z', 'm', 'v', 'best_loss', 'z_best', 'best_step')


def fresh(n, L, seed):
    rng = np.random.default_rng([seed, n, L])
    return dict(z=torch.from_numpy(rng.standard_normal((n, L)).astype(np.float32)), m=torch.zeros(n, L), v=torch.zeros(n, L),
                best_loss=torch.full((n,), float('inf')), z_best=torch.zeros(n, L), best_step=torch.full((n,), -1, dtype=torch.int32))


@pytest.mark.parametrize('L', [8, 64, 200, 512])
@pytest.mark.parametrize('n', [1, 5])
@pytest.mark.parametrize('sphere', [False, True])
def test_ten_chained_steps_bit_for_bit(L, n, sphere):
    from saragan_amd import functional as F
    host = fresh(n, L, 1)
    dev = {k: v.clone().cuda() for k, v in host.items()}
    rng = np.random.default_rng([2, n, L])
    prev = None
    for step in range(1, 11):
        g = torch.from_numpy((rng.standard_normal((n, L)) * 10.0 ** rng.integers(-3, 2)).astype(np.float32))
        loss = torch.from_numpy(rng.random(n).astype(np.float32) * (12 - step))
        if step == 4:
            loss[n - 1] = float('nan')
        if step == 6:
            loss = prev.clone()      # equal to the best wherever step 5 was one: no replacement
        lr = 0.0 if step == 8 else 0.02 * step      # (one scoring launch in the chain)
        F.latent_step_(host['z'], host['m'], host['v'], g, loss, host['best_loss'], host['z_best'], host['best_step'], lr, step, sphere=sphere)
        F.latent_step_(dev['z'], dev['m'], dev['v'], g.cuda(), loss.cuda(), dev['best_loss'], dev['z_best'], dev['best_step'], lr, step,
                       sphere=sphere)
        for k in KEYS:
            assert np.array_equal(dev[k].cpu().numpy(), host[k].numpy(), equal_nan=True), (k, step)
        prev = loss
    assert torch.isfinite(dev['best_loss']).all() and (dev['best_step'] >= 1).all()
    if sphere:
        norms = dev['z'].double().norm(dim=1).cpu().numpy()
        assert np.allclose(norms, np.sqrt(L), rtol=1e-6)


def test_nan_never_wins_and_equal_losses_keep_the_earlier_step():
    from saragan_amd import functional as F
    s = {k: v.cuda() for k, v in fresh(3, 40, 3).items()}
    g = torch.ones(3, 40, device='cuda')
    z0 = s['z'].clone()
    call = lambda loss, lr, t: F.latent_step_(s['z'], s['m'], s['v'], g, torch.tensor(loss, device='cuda'), s['best_loss'],  # noqa: E731
                                              s['z_best'], s['best_step'], lr, t)
    call([2.0, float('nan'), 1.0], 0.1, 1)
    assert s['best_loss'].tolist() == [2.0, float('inf'), 1.0] and s['best_step'].tolist() == [1, -1, 1]
    assert torch.equal(s['z_best'][0], z0[0]) and torch.equal(s['z_best'][1], torch.zeros(40, device='cuda'))
    z1 = s['z'].clone()
    call([2.0, 3.0, 0.5], 0.0, 2)
    assert s['best_loss'].tolist() == [2.0, 3.0, 0.5] and s['best_step'].tolist() == [1, 2, 2]
    assert torch.equal(s['z'], z1) and torch.equal(s['z_best'][0], z0[0]) and torch.equal(s['z_best'][2], z1[2])
