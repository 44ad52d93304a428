"""python -m saragan_amd.project on the device, on the checkpoint recipe of tests/test_generate_dataset_gpu.py: phase 3,
f32, 4 x 16 x 16, the CPU oracle generator as the reference.

Tolerances.  Nothing here is compared more tightly than the oracle agrees with itself: the same quantity is evaluated by the oracle
in float64 and in float32 (float32 parameters and latents) on the inputs of the comparison, and four times the largest difference
of the two is the bound -- for d loss / d z in (a), for a loss in (b) ("the forward tolerance").  The bounds are computed from the
oracle alone, before the device's numbers are looked at, and printed with the device's figures."""
import io
import json
import os

import numpy as np
import pytest
import torch

from oracle import pgan_oracle as O
from tests import condref as CR
from tests.stepfix import BASE_SHAPE, FILTER_SPEC, KERNEL_SPEC, LATENT
from tests.test_generate_dataset_gpu import save_params

pytestmark = pytest.mark.gpu

# (c) SEED, LR: with these the float64 oracle's own run of the tool's rule (project.run with the oracle as the generator on the CPU
# twins: the five targets as the oracle makes them, 2 restarts, 30 steps) lowers every file's loss to less than half of its initial
# value: best / initial = 0.035, 0.272, 0.246, 0.187, 0.072 (seeds 0 .. 9 were tried at lr 0.2; seed 2 was the first to pass; seed 7
# starts ON the targets' latents, numpy's SeedSequence ignoring the trailing restart 0).  The device is only asked for 0.75.
PHASE, COUNT, MEAN, STD, SEED, LR, STEPS, LEVELS = 3, 5, 1024.0, 1024.0, 2, 0.2, 30, 3
NAMES = [f'{i:07d}.npy' for i in range(COUNT)]


def oracle_volumes(p, z, cond=None):
    if cond is None:
        return O.generator(p, z, 0.0, PHASE, BASE_SHAPE, 'leaky_relu', KERNEL_SPEC, FILTER_SPEC, 0.2)
    return CR.generator(p, z, cond, 0.0, PHASE, BASE_SHAPE, 'leaky_relu', KERNEL_SPEC, FILTER_SPEC, 0.2)


def torch_loss(y, x):
    """The loss per sample with torch ops (differentiable, any float type): targets x in data units."""
    r = y - (x.to(y.dtype) - MEAN) / STD
    total = 0
    for l in range(LEVELS):
        m = torch.nn.functional.avg_pool3d(r, 2 ** l) if l else r
        total = total + (m * m).flatten(1).mean(dim=1)
    return total


def oracle_loss_and_grad(p, z, x, dtype):
    """(loss [n], d sum(loss) / d z) of the oracle in `dtype`."""
    q = {k: v.to(dtype) for k, v in p.items()}
    zz = z.to(dtype).clone().requires_grad_(True)
    loss = torch_loss(oracle_volumes(q, zz), x)
    g, = torch.autograd.grad(loss.sum(), zz)
    return loss.detach().double(), g.double()


def tool(argv):
    from saragan_amd import project as P
    return P.run(P.build_parser().parse_args(argv), out=io.StringIO())


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    from saragan_amd import generate as G
    root = tmp_path_factory.mktemp('project')
    p = O.init_params(PHASE, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC, seed=4, bias_std=0.1)
    spec = root / 'spec.json'
    spec.write_text(json.dumps(dict(kernel_spec=KERNEL_SPEC, filter_spec=FILTER_SPEC)))
    model = save_params(p, str(root / 'model_3'))
    base = ['pgan', '--start_shape', str(BASE_SHAPE), '--final_shape', '(1, 4, 16, 16)', '--kernel_spec', str(spec), '--filter_spec', str(spec),
            '--network_size', 'xs', '--latent_dim', str(LATENT), '--phase', str(PHASE), '--data_mean', str(MEAN), '--data_stddev', str(STD),
            '--dtype', 'f32']
    # the targets: five volumes the generator itself makes (other latents than any the projection starts from)
    G.run(G.build_parser().parse_args(base + ['--model_path', model, '--output_dir', str(root / 'made'), '--num_samples', str(COUNT), '--seed', '7',
                                              '--batch_size', '2', '--out_dtype', 'int16']), out=io.StringIO())
    target_dir = root / 'made' / f'generated_{PHASE}'
    for n in os.listdir(target_dir):
        if not n.endswith('.npy'):
            os.remove(target_dir / n)
    vols = np.stack([np.load(target_dir / n) for n in NAMES])

    def argv(out, *more, model_path=model):
        return base + ['--model_path', model_path, '--output_dir', str(out), '--seed', str(SEED), '--steps', str(STEPS), '--lr', str(LR),
                       '--levels', str(LEVELS), '--restarts', '2', '--out_dtype', 'int16', str(target_dir), *more]
    return dict(root=root, params=p, base=base, model=model, target_dir=target_dir, vols=vols, argv=argv)


@pytest.fixture(scope='module')
def run_a(setup):
    out = setup['root'] / 'a'
    rec = tool(setup['argv'](out, '--batch_size', '2', '--residual_dir', str(out / 'resid'), '--png'))
    d = out / f'projected_{PHASE}'
    return dict(rec=rec, dir=d, out=out, latents=np.load(d / 'latents.npy'), js=json.load(open(d / 'projection.json')))


def device_generator(setup):
    from saragan_amd import project as P
    from saragan_amd.generation import RestoredGenerator
    args = P.build_parser().parse_args(setup['argv'](setup['root'] / 'unused'))
    g = RestoredGenerator(args, 'cuda')
    g(torch.zeros(2, LATENT, device='cuda'))
    g.restore(False)
    P._grad_free(g.store)
    return g


def test_a_dloss_dz_against_the_oracle(setup):
    from saragan_amd import functional as F
    from saragan_amd import project as P
    g = device_generator(setup)
    z0 = torch.from_numpy(P.latent_rows(SEED, range(COUNT), 1, LATENT))
    x = torch.from_numpy(setup['vols'])[:, None]
    l64, g64 = oracle_loss_and_grad(setup['params'], z0, x, torch.float64)
    l32, g32 = oracle_loss_and_grad(setup['params'], z0, x, torch.float32)
    tol_g, tol_l = 4 * (g32 - g64).abs().max().item(), 4 * (l32 - l64).abs().max().item()
    z = z0.cuda().requires_grad_(True)
    y = g(z, None, grad=True)
    loss, terms, grad = F.multiscale_residual_raw(y.detach(), x.cuda(), torch.arange(COUNT, dtype=torch.int32, device='cuda'), MEAN, STD, LEVELS)
    gz, = torch.autograd.grad(y, z, grad)
    err_g, err_l = (gz.double().cpu() - g64).abs().max().item(), (loss.double().cpu() - l64).abs().max().item()
    print(f'dL/dz: device - f64 {err_g:.3e}, bound 4 x (f32 - f64) = {tol_g:.3e}, largest |dL/dz| {g64.abs().max().item():.3e}; '
          f'loss: {err_l:.3e}, bound {tol_l:.3e}, largest loss {l64.max().item():.3e}')
    assert all(v.grad is None for v in g.store.vars.values())
    assert err_l <= tol_l
    assert err_g <= tol_g


def test_b_one_run_of_the_tool(setup, run_a):
    from saragan_amd import functional as F
    from saragan_amd import project as P
    js, lat, d = run_a['js'], run_a['latents'], run_a['dir']
    assert sorted(n for n in os.listdir(d) if not n.endswith('.png')) == sorted(NAMES + ['latents.npy', 'projection.json'])
    assert sorted(n for n in os.listdir(d) if n.endswith('.png')) == ['sheet_0000.png', 'sheet_0001.png', 'sheet_0002.png']
    assert open(d / 'sheet_0000.png', 'rb').read(8) == b'\x89PNG\r\n\x1a\n'
    assert lat.shape == (COUNT, LATENT) and lat.dtype == np.float32 and run_a['rec']['variables_with_grad'] == []
    x = torch.from_numpy(setup['vols'])[:, None]
    zl = torch.from_numpy(lat)
    l64, _ = oracle_loss_and_grad(setup['params'], zl, x, torch.float64)
    l32, _ = oracle_loss_and_grad(setup['params'], zl, x, torch.float32)
    tol_l = 4 * (l32 - l64).abs().max().item()
    # the loss the CPU path computes from the saved latent's oracle volume
    yo = oracle_volumes(setup['params'], zl.double()).float()
    cpu_loss, _, _ = F.multiscale_residual_raw(yo, x, list(range(COUNT)), MEAN, STD, LEVELS)
    g = device_generator(setup)
    want = F.store_volumes(g(zl.cuda()), torch.int16, scale=STD, shift=MEAN).cpu().numpy()[:, 0]
    for f in js['files']:
        i = f['index']
        print(f'{f["name"]}: best {f["best_loss"]:.6e} at step {f["best_step"]}, restart {f["restart"]}, initial {f["initial_loss"]:.6e}, '
              f'oracle at the saved latent {cpu_loss[i].item():.6e}, forward bound {tol_l:.3e}, rms {f["rms"]:.2f}')
        assert not f['failed'] and f['name'] == NAMES[i] and len(f['terms']) == LEVELS
        assert f['best_loss'] <= f['initial_loss']
        assert abs(f['best_loss'] - cpu_loss[i].item()) <= tol_l
        recon = np.load(d / f['name'])
        assert recon.dtype == np.int16 and recon.shape == (4, 16, 16)
        assert np.abs(recon.astype(np.int64) - want[i]).max() <= 1
        assert np.array_equal(np.load(run_a['out'] / 'resid' / f['name']).astype(np.int64), np.abs(setup['vols'][i].astype(np.int64) - recon))
    # another batch size: the same initial latents exactly (the rule knows no batch), the same result within (a)'s bound
    rec_b = tool(setup['argv'](setup['root'] / 'b', '--batch_size', '3'))
    lat_b = np.load(setup['root'] / 'b' / f'projected_{PHASE}' / 'latents.npy')
    assert np.array_equal(P.latent_rows(SEED, [3, 4], 2, LATENT), P.latent_rows(SEED, range(COUNT), 2, LATENT)[6:])
    z0 = torch.from_numpy(P.latent_rows(SEED, range(COUNT), 1, LATENT))
    _, g64 = oracle_loss_and_grad(setup['params'], z0, x, torch.float64)
    _, g32 = oracle_loss_and_grad(setup['params'], z0, x, torch.float32)
    tol_g = 4 * (g32 - g64).abs().max().item()
    print(f'latents of batch sizes 2 and 3 differ by {np.abs(lat - lat_b).max():.3e}, bound {tol_g:.3e}')
    assert [f['restart'] for f in rec_b['files']] == [f['restart'] for f in js['files']]
    assert all(abs(a['initial_loss'] - b['initial_loss']) <= tol_l for a, b in zip(rec_b['files'], js['files']))
    assert np.abs(lat - lat_b).max() <= tol_g


def test_c_descent(run_a):
    for f in run_a['js']['files']:
        assert f['best_loss'] < 0.75 * f['initial_loss'], f


def test_d_generate_reproduces_the_reconstructions(setup, run_a):
    from saragan_amd import generate as G
    out = setup['root'] / 'regen'
    m = G.run(G.build_parser().parse_args(setup['base'] + ['--model_path', setup['model'], '--output_dir', str(out), '--batch_size', '2',
                                                           '--out_dtype', 'int16', '--latents_path', str(run_a['dir'] / 'latents.npy')]),
              out=io.StringIO())
    assert m['latent'].endswith('latents.npy') and 'default_rng' not in m['latent'] and len(m['files']) == COUNT
    for n in NAMES:
        a, b = np.load(out / f'generated_{PHASE}' / n).astype(np.int64), np.load(run_a['dir'] / n).astype(np.int64)
        assert np.abs(a - b).max() <= 1


def test_e_conditional_checkpoint(setup):
    from saragan_amd import functional as F
    p = CR.init_params(PHASE, BASE_SHAPE, LATENT, KERNEL_SPEC, FILTER_SPEC, 3, seed=5)
    model = save_params(p, str(setup['root'] / 'cond_model_3'))
    table = np.eye(3, dtype=np.float32)[[0, 2, 1, 1, 0]] * np.float32(1.5)
    path = setup['root'] / 'labels.npy'
    np.save(path, table)
    with pytest.raises(ValueError, match='--conditioning'):
        tool(setup['argv'](setup['root'] / 'cond0', '--batch_size', '5', model_path=model))
    rec = tool(setup['argv'](setup['root'] / 'cond', '--batch_size', '3', '--conditioning_path', str(path), model_path=model))
    d = setup['root'] / 'cond' / f'projected_{PHASE}'
    lat = torch.from_numpy(np.load(d / 'latents.npy'))
    # the reconstruction is the conditional oracle's volume at the saved latent WITH the file's label row
    ref = oracle_volumes(p, lat.double(), torch.from_numpy(table).double()).numpy()[:, 0] * STD + MEAN
    for f in rec['files']:
        assert not f['failed'] and f['best_loss'] <= f['initial_loss']
        recon = np.load(d / f['name']).astype(np.float64)
        e = 2e-2 + 1e-4 * np.abs(ref[f['index']])      # tests/test_generate_dataset_gpu.py's tolerance of the generator, in data units
        assert np.abs(recon - np.trunc(np.clip(ref[f['index']], -32768, 32767))).max() <= 1 + e.max()
