"""The premise of tests/test_dp_step_gpu.py, on the host in fp64: every loss of the oracle is a batch mean, so the mean of
the ranks' half-batch gradients IS the full-batch gradient and "expected = the oracle's full-batch step" is the right
reference for the averaging reducer.  That is not obvious for two terms: the wgan gradient penalty keeps the W axis (quirk Q1:
slopes [N, W] broadcast against [N, 1]; under `alternate`, [N, 1] + [N] broadcasts to [N, N]) and the logistic penalty is
gp_weight * mean(slopes^2) over the batch.  If the oracle ever gains a term that couples samples, this fails first."""
import os

import numpy as np
import pytest
import torch

from tests import dpref

FIXTURES = ['oracle_step_p3_wgan_a000.npz', 'oracle_step_p2_wgan_a060.npz', 'oracle_step_p3_logistic_a025.npz']


@pytest.mark.parametrize('world', [2, 4])
@pytest.mark.parametrize('strategy', ['simultaneous', 'alternate'])
@pytest.mark.parametrize('name', FIXTURES)
def test_mean_of_rank_gradients_is_the_full_batch_gradient(golden_dir, name, strategy, world):
    from tests.stepfix import load_step_fixture
    fx = load_step_fixture(os.path.join(golden_dir, name), torch.float64)
    for freeze in ([None, fx['freeze']] if fx['freeze'] is not None else [None]):
        # SGD with lr 0 leaves the weights alone: under `alternate` both halves of the step then see p0, on every rank
        full = dpref.oracle_run(fx, strategy, 'SGD', 1, freeze=freeze, lr=0.0)[0]['out']
        parts = [dpref.oracle_run(fx, strategy, 'SGD', 1, freeze=freeze, rank=r, world=world, lr=0.0)[0]['out'] for r in range(world)]
        for key in ('g_grads', 'd_grads'):
            assert list(full[key]) == list(parts[0][key])
            for k, ref in full[key].items():
                mean = sum(p[key][k] for p in parts) / world
                scale = float(ref.abs().max())
                assert float((mean - ref).abs().max()) <= 1e-12 * scale, (key, k, float((mean - ref).abs().max()), scale)
        for key in ('gen_loss', 'disc_loss'):
            mean = sum(float(p[key]) for p in parts) / world
            np.testing.assert_allclose(mean, float(full[key]), rtol=1e-12, atol=0)
        mean = sum(float(p['gp_loss'].mean()) for p in parts) / world
        np.testing.assert_allclose(mean, float(full['gp_loss'].mean()), rtol=1e-12, atol=0)
