"""--compute_intensity_hist inside the training loop: the configuration of tests/test_sample_metrics_loop_gpu.py with
--hist_range and --hist_levels 2.  The counts are exact, so every reported value is recomputed from the very batches the
loop evaluated -- level 0 with tests/histref.py from the kept batches, level 1 from the pyramid tensors the accumulator
built -- and compared with ==, as are the printed lines.  A second run without the flag reports nothing new; the command
line is run once over two directories of int16 volumes."""
import numpy as np
import pytest

from tests import histref

pytestmark = pytest.mark.gpu

KEYS = ('intensity_ks', 'intensity_w1', 'intensity_gap')
LO, HI = 0, 4095
MEAN, STD = 1024.0, 1024.0


def _args(data, logdir, hist):
    from saragan_amd.main import build_parser, finalize_args
    argv = ['pgan', str(data) + '/', '--start_shape', '(1, 4, 4, 4)', '--final_shape', '(1, 32, 32, 32)',
            '--starting_phase', '2', '--ending_phase', '3', '--base_batch_size', '8', '--latent_dim', '16',
            '--noise_stddev', '0.01', '--mixing_nimg', '16', '--stabilizing_nimg', '16', '--loss_fn', 'logistic',
            '--gp_weight', '1', '--data_mean', str(int(MEAN)), '--data_stddev', str(int(STD)), '--logdir', str(logdir),
            '--g_lr', '1e-3', '--d_lr', '1e-3', '--checkpoint_every_nsteps', '1000000', '--dtype', 'f32',
            '--calc_metrics', '--compute_psnrs', '--metrics_every_nsteps', '16', '--num_metric_samples', '4',
            '--metrics_batch_size', '2', '--validation_fraction', '0.2', '--test_fraction', '0.1']
    if hist:
        argv += ['--compute_intensity_hist', '--hist_range', f'{LO},{HI}', '--hist_levels', '2']
    args, unknown = build_parser().parse_known_args(argv)
    assert not unknown
    args.kernel_spec = [[[3, 3, 3], [3, 3, 3]]] * 3
    args.filter_spec = [[16, 16], [16, 8], [8, 8]]
    args._metric_tap = []
    args._metric_hists = []
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


def _expected(kept, pyramids):
    """The three lists from the kept (real, fake) batches and the per-batch [real pyramid, fake pyramid] tensors."""
    from saragan_amd.metrics.intensity_metrics import histogram_distances
    half = (HI - LO) // 2
    counts = [[np.zeros(HI - LO + 1, np.int64), np.zeros(HI - LO + 1, np.int64)],
              [np.zeros(2 * half + 1, np.int64), np.zeros(2 * half + 1, np.int64)]]
    assert len(pyramids) == 2 * len(kept)
    for b, (real, fake) in enumerate(kept):
        for side, x in enumerate((real, fake)):
            counts[0][side] += histref.hist(x.astype(np.float32), LO, HI, STD, MEAN, pooled=True)[0]
            pyr = pyramids[2 * b + side]
            assert len(pyr) == 2 and pyr[0].shape == x.shape and pyr[1].shape[2:] == tuple(e // 2 for e in x.shape[2:])
            counts[1][side] += histref.hist(pyr[0], -half, half, STD, 0.0, pooled=True)[0]
    m = {k: [] for k in KEYS}
    for r, f in counts:
        assert r.sum() == f.sum() == sum(k[0].size for k in kept)
        d = histref.distances(r, f)
        assert d == {k: histogram_distances(r, f)[k] for k in d}
        m['intensity_ks'].append(d['ks'])
        m['intensity_w1'].append(d['w1'])
        m['intensity_gap'].append(d['max_density_gap'])
    return m


def test_intensity_metrics_in_the_training_loop(dataset, tmp_path, capsys):
    from saragan_amd.metrics.intensity_metrics import format_lines
    from saragan_amd.train import run_training
    args = _args(dataset, tmp_path / 'log', True)
    assert args.hist_range == (LO, HI)
    run_training(args, log_every=10 ** 6)
    text = capsys.readouterr().out
    tap, hists = args._metric_tap, args._metric_hists
    assert len(tap) == len(hists) == 12
    lines = [ln for ln in text.splitlines() if ln.startswith('Intensity')]
    assert len(lines) == 3 * 12
    for i, ((ph, tag, m, kept), (hph, htag, rec)) in enumerate(zip(tap, hists)):
        assert (ph, tag) == (hph, htag)
        assert rec[-1] == 2                                     # both levels exist at 8^3 and at 16^3
        want = _expected(kept, rec[:-1])
        for k in KEYS:
            assert m[k] == want[k], (ph, tag, k)
        assert lines[3 * i:3 * i + 3] == format_lines(want), (ph, tag)
        assert 'psnr' in m                                      # the per-batch metrics are still there
        assert 0.0 < m['intensity_ks'][0] <= 1.0                # an untrained generator does not match the data


def test_without_the_flag_nothing_new_is_reported(dataset, tmp_path, capsys):
    from saragan_amd.train import run_training
    args = _args(dataset, tmp_path / 'log', False)
    run_training(args, log_every=10 ** 6)
    text = capsys.readouterr().out
    assert len(args._metric_tap) == 12
    for _, _, m, _ in args._metric_tap:
        assert not set(m) & set(KEYS) and 'psnr' in m
    assert all(rec == [] for _, _, rec in args._metric_hists)
    assert 'Intensity' not in text and 'intensity' not in text


def test_command_line_over_two_directories(tmp_path, capsys):
    from saragan_amd.metrics import intensity_metrics as IM
    rng = np.random.default_rng(9)
    sets = {}
    for name, centre in (('real', 1000), ('fake', 1100)):
        (tmp_path / name).mkdir()
        vols = np.clip(rng.normal(centre, 400, (5, 4, 8, 8)), -200, 4300).astype(np.int16)
        for i, v in enumerate(vols):
            np.save(tmp_path / name / f'{i:03d}.npy', v)
        sets[name] = vols
    m = IM.main([str(tmp_path / 'real'), str(tmp_path / 'fake'), '--range', '0,4095', '--batch', '2', '--scale', '1.5',
                 '--shift', '-100'])
    out = capsys.readouterr().out
    hr = histref.hist(sets['real'], 0, 4095, 1.5, -100.0, pooled=True)
    hf = histref.hist(sets['fake'], 0, 4095, 1.5, -100.0, pooled=True)
    d = histref.distances(hr, hf)
    assert m == {'intensity_ks': [d['ks']], 'intensity_w1': [d['w1']], 'intensity_gap': [d['max_density_gap']]}
    assert [ln for ln in out.splitlines() if ln.startswith('Intensity')] == IM.format_lines(m)
    assert '5 real and 5 generated volumes of shape (4, 8, 8)' in out
    with pytest.raises(SystemExit, match='--range'):
        IM.main([str(tmp_path / 'real'), str(tmp_path / 'fake'), '--range', '9,1'])
