"""--preview_every_nsteps inside the training loop, in the small configuration of tests/test_intensity_metrics_loop_gpu.py
(phases 2-3, 8^3 -> 16^3, base batch 8, f32): the expected files exist with the expected sizes; every PNG decodes to
tests/viewref.py's sheet of the very tensors the loop rendered (the args._preview_tap hook); the columns of consecutive sheets
come from the same latents; reals_*.png is the sheet of the first files as read from disk; a run with previews ends with the
same checkpoint bits as a run without; generate_minimal --png writes the sheet of its saved samples."""
import json
import os

import numpy as np
import pytest
import torch

from tests import viewref

pytestmark = pytest.mark.gpu

MEAN, STD = 1024.0, 1024.0
VIEWS = ('slice_d', 'slice_h', 'max_h')            # the default
WINDOW = (MEAN - STD, MEAN + 2 * STD)              # the default: the reference's clip range [-1, 2] in data units
KERNEL_SPEC = [[[3, 3, 3], [3, 3, 3]]] * 3
FILTER_SPEC = [[16, 16], [16, 8], [8, 8]]
SAMPLES, INTERP, EVERY, NIMG = 3, 4, 16, 32
PHASES = ((2, 4, (8, 8, 8)), (3, 2, (16, 16, 16)))  # (phase, its batch size 8 // 2 ** (phase - 1), the volume shape)


def _args(data, logdir, previews):
    from saragan_amd.main import build_parser, finalize_args
    argv = ['pgan', str(data) + '/', '--start_shape', '(1, 4, 4, 4)', '--final_shape', '(1, 32, 32, 32)',
            '--starting_phase', '2', '--ending_phase', '3', '--base_batch_size', '8', '--latent_dim', '16',
            '--noise_stddev', '0.01', '--mixing_nimg', '16', '--stabilizing_nimg', '16', '--loss_fn', 'logistic',
            '--gp_weight', '1', '--data_mean', str(int(MEAN)), '--data_stddev', str(int(STD)), '--logdir', str(logdir),
            '--g_lr', '1e-3', '--d_lr', '1e-3', '--checkpoint_every_nsteps', '16', '--dtype', 'f32', '--seed', '7']
    if previews:
        argv += ['--preview_every_nsteps', str(EVERY), '--preview_samples', str(SAMPLES), '--preview_interp', str(INTERP)]
    args, unknown = build_parser().parse_known_args(argv)
    assert not unknown
    args.kernel_spec, args.filter_spec = KERNEL_SPEC, FILTER_SPEC
    args._preview_tap = []
    return finalize_args(args)


@pytest.fixture(scope='module')
def dataset(tmp_path_factory):
    data = tmp_path_factory.mktemp('data')
    for z, xy in ((4, 4), (8, 8), (16, 16)):
        d = data / f'{xy}x{xy}'
        d.mkdir(parents=True)
        for i in range(20):
            rng = np.random.default_rng(1234 + i)
            np.save(d / f'{i:04d}.npy', np.clip(rng.normal(1024, 512, (z, xy, xy)), 0, 4095).astype(np.int16))
    return data


@pytest.fixture(scope='module')
def runs(dataset, tmp_path_factory):
    """The same seed twice in reproducible mode: with previews, and without."""
    import saragan_amd
    from saragan_amd.train import run_training
    out = {}
    saragan_amd.set_deterministic(True)
    try:
        for name, on in (('with', True), ('without', False)):
            args = _args(dataset, tmp_path_factory.mktemp(name), on)
            run_training(args, log_every=10 ** 6)
            out[name] = args
    finally:
        saragan_amd.set_deterministic(False)
    return out


def _points():
    """(phase, file tag) of every preview point: local_step % EVERY < batch, named by the global step after that step."""
    pts, start = [], 0
    for phase, bs, _ in PHASES:
        pts += [(phase, f'{start + local + bs:09d}') for local in range(0, NIMG, bs) if local % EVERY < bs]
        pts.append((phase, 'final'))
        start += NIMG
    return pts


def _read(path):
    with open(path, 'rb') as f:
        return viewref.decode_png(f.read())


def test_expected_files_and_sizes(runs):
    d = os.path.join(runs['with'].logdir, 'previews')
    shapes = {ph: shape for ph, _, shape in PHASES}
    want = {}
    for phase, tag in _points():
        dd, h, w = shapes[phase]
        want[f'fakes_{phase}_{tag}.png'] = (h + dd + dd, SAMPLES * w)
        want[f'interp_{phase}_{tag}.png'] = (h + dd + dd, INTERP * w)
    for phase, _, (dd, h, w) in PHASES:
        cols = int(2 ** np.floor(np.log2(np.sqrt(dd))))
        want[f'grid_fake_{phase}.png'] = (-(-dd // cols) * h, cols * w)
        want[f'reals_{phase}.png'] = (h + dd + dd, SAMPLES * w)
    assert sorted(os.listdir(d)) == sorted(want)
    assert len(_points()) == 6      # two preview points and the final sheet per phase
    for name, shape in want.items():
        img, text = _read(os.path.join(d, name))
        assert img.shape == shape, name
        assert text['phase'] == name.split('_')[-2 if name[0] in 'fi' else -1].split('.')[0] and text['seed'] == '7'
        assert text['window'] == f'{WINDOW[0]},{WINDOW[1]}' and text['views'] == ','.join(VIEWS)
        assert text['weights'] == ('none' if name.startswith('reals') else 'EMA')


def test_every_png_is_viewrefs_sheet_of_the_rendered_tensors(runs):
    args = runs['with']
    d = os.path.join(args.logdir, 'previews')
    tap = args._preview_tap
    names = [name for _, name, _, _ in tap]
    assert sorted(names) == sorted(n for n in os.listdir(d) if not n.startswith('reals')) and len(set(names)) == len(names)
    fixed = None
    for phase, name, z, chunks in tap:
        x = torch.cat(chunks).numpy()
        bs, shape = {ph: (b, s) for ph, b, s in PHASES}[phase]
        assert all(c.shape[0] <= bs for c in chunks) and x.shape[2:] == shape      # generated in chunks of the phase's batch
        img, _ = _read(os.path.join(d, name))
        if name.startswith('grid_fake'):
            assert x.shape[0] == 1 and (img == viewref.slice_grid(x[0, 0], WINDOW, STD, MEAN)).all(), name
            continue
        assert (img == viewref.sheet(x, VIEWS, WINDOW, STD, MEAN)).all(), name
        assert len(np.unique(img)) > 1, name      # not blank
        if name.startswith('fakes'):      # column i of every sheet comes from the same latent, drawn once per run
            assert z.shape == (SAMPLES, 16) and (fixed is None or torch.equal(z, fixed))
            fixed = z
        else:
            assert z.shape == (INTERP, 16) and torch.allclose(z[0], fixed[0]) and torch.allclose(z[-1], fixed[1])


def test_reals_are_the_first_files_as_read_from_disk(runs, dataset):
    d = os.path.join(runs['with'].logdir, 'previews')
    for phase, _, shape in PHASES:
        files = sorted(os.listdir(dataset / f'{shape[1]}x{shape[2]}'))[:SAMPLES]
        vols = np.stack([np.load(dataset / f'{shape[1]}x{shape[2]}' / f) for f in files])
        assert vols.dtype == np.int16
        img, _ = _read(os.path.join(d, f'reals_{phase}.png'))
        assert (img == viewref.sheet(vols, VIEWS, WINDOW)).all()


def test_weights_are_the_same_bits_with_and_without_previews(runs):
    from saragan_amd.utils import load_checkpoint
    a, b = runs['with'].logdir, runs['without'].logdir
    assert not os.path.exists(os.path.join(b, 'previews')) and runs['without']._preview_tap == []
    ckpts = sorted(f for f in os.listdir(a) if f.endswith('.npz'))
    assert ckpts == sorted(f for f in os.listdir(b) if f.endswith('.npz'))
    # the phases' final checkpoints hold the EMA shadows, the periodic ones the training weights
    assert {'model_2.npz', 'model_3.npz'} < set(ckpts) and any('ckpt' in c for c in ckpts)
    for c in ckpts:
        wa, wb = load_checkpoint(os.path.join(a, c)), load_checkpoint(os.path.join(b, c))
        assert sorted(wa) == sorted(wb)
        bad = [k for k in wa if wa[k].tobytes() != wb[k].tobytes()]
        assert not bad, (c, bad)


def test_generate_minimal_png(runs, tmp_path):
    from saragan_amd import generate_minimal as gm
    from saragan_amd.dataset import normalize_numpy
    spec = tmp_path / 'spec.json'
    spec.write_text(json.dumps(dict(kernel_spec=KERNEL_SPEC, filter_spec=FILTER_SPEC)))
    argv = ['pgan', '--start_shape', '(1, 4, 4, 4)', '--final_shape', '(1, 32, 32, 32)', '--kernel_spec', str(spec),
            '--filter_spec', str(spec), '--network_size', 'xxs', '--latent_dim', '16', '--output_dir', str(tmp_path),
            '--model_path', os.path.join(runs['with'].logdir, 'model_3'), '--num_samples', '3', '--batch_size', '2', '--phase', '3',
            '--data_mean', str(int(MEAN)), '--data_stddev', str(int(STD)), '--dtype', 'f32', '--png', '--preview_views',
            'mean_d,max_w', '--preview_zoom_d', '2', '--preview_window', '0,3000']
    out = gm.main(gm.build_parser().parse_args(argv))
    saved = np.load(out)
    img, text = _read(out[:-4] + '.png')
    x = np.asarray(normalize_numpy(saved, MEAN, STD), dtype=np.float32)
    assert (img == viewref.sheet(x, ('mean_d', 'max_w'), (0.0, 3000.0), STD, MEAN, 2)).all()
    assert img.shape == (16 + 2 * 16, saved.shape[0] * 16) and text['phase'] == '3' and len(np.unique(img)) > 1
