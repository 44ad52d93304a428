"""--compute_mmd / --compute_nn_accuracy / --compute_precision_recall inside the training loop: the configuration of
tests/test_metrics_loop_gpu.py plus the three flags.  Every pooled evaluation's distance matrix is checked against the
direct fp64 distances of the very batches the loop used, and every reported value against tests/nnref.py evaluated ON
THAT RECORDED MATRIX (the generator's outputs are not known in advance, so no ordering margin can be promised for them:
the reductions are checked exactly on the matrix the kernel produced, the matrix within its rounding bound).  A second run
without the flags reports none of the new keys."""
import numpy as np
import pytest

from tests import nnref

pytestmark = pytest.mark.gpu

NEW_KEYS = ('mmd', 'nn_accuracy', 'nn_accuracy_real', 'nn_accuracy_fake', 'precision', 'recall')


def _args(data, logdir, sample_flags):
    from saragan_amd.main import build_parser, finalize_args
    argv = ['pgan', str(data) + '/', '--start_shape', '(1, 4, 4, 4)', '--final_shape', '(1, 32, 32, 32)',
            '--starting_phase', '2', '--ending_phase', '3', '--base_batch_size', '8', '--latent_dim', '16',
            '--noise_stddev', '0.01', '--mixing_nimg', '16', '--stabilizing_nimg', '16', '--loss_fn', 'logistic',
            '--gp_weight', '1', '--data_mean', '1024', '--data_stddev', '1024', '--logdir', str(logdir),
            '--g_lr', '1e-3', '--d_lr', '1e-3', '--checkpoint_every_nsteps', '1000000', '--dtype', 'f32',
            '--calc_metrics', '--compute_FID', '--compute_swds', '--compute_ssims', '--compute_psnrs', '--compute_mses',
            '--compute_nrmses', '--metrics_every_nsteps', '16', '--num_metric_samples', '4', '--metrics_batch_size', '2',
            '--validation_fraction', '0.2', '--test_fraction', '0.1']
    if sample_flags:
        argv += ['--compute_mmd', '--compute_nn_accuracy', '--compute_precision_recall', '--pr_k', '3']
    args, unknown = build_parser().parse_known_args(argv)
    assert not unknown
    args.kernel_spec = [[[3, 3, 3], [3, 3, 3]]] * 3
    args.filter_spec = [[16, 16], [16, 8], [8, 8]]
    args._metric_tap = []
    args._metric_sets = []
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


def test_sample_metrics_in_the_training_loop(dataset, tmp_path, capsys):
    from saragan_amd import _lib
    from saragan_amd.train import run_training
    args = _args(dataset, tmp_path / 'log', True)
    run_training(args, log_every=10 ** 6)
    text = capsys.readouterr().out
    chunk = int(_lib.load().sg_pairwise_sqdist_chunk())
    tap, sets = args._metric_tap, list(args._metric_sets)
    assert len(tap) == 12
    assert 'MMD^2: ' in text and '1-NN accuracy (total real fake): ' in text and 'Precision / recall (k=3): ' in text
    # the 2-sample test subset: n = 2 < k + 1, once per phase
    assert text.count('Precision / recall (k=3) is switched off for this evaluation: 2 samples per set, it needs 4') == 2
    assert len(sets) == 12          # MMD and 1-NN accuracy run at n = 2 too
    for (ph, tag, m, kept), (sph, stag, n, D) in zip(tap, sets):
        assert (ph, tag) == (sph, stag)
        real = np.concatenate([r for r, _ in kept]).astype(np.float32)
        fake = np.concatenate([f for _, f in kept]).astype(np.float32)
        assert n == real.shape[0] == fake.shape[0] == {'loop': 4, 'loop_EMA': 4, 'test': 2, 'validation': 4}[tag]
        Z = np.concatenate([real, fake]).reshape(2 * n, -1)
        assert D.shape == (2 * n, 2 * n) and D.dtype == np.float64
        err = np.abs(D - nnref.sqdist(Z))
        assert (err <= nnref.sqdist_bound(Z, Z, chunk)).all(), (ph, tag, err.max())
        assert np.array_equal(D, D.T) and not D.diagonal().any()
        assert abs(m['mmd'] - nnref.mmd2(D, n)) <= 1e-12, (ph, tag)
        assert (m['nn_accuracy'], m['nn_accuracy_real'], m['nn_accuracy_fake']) == \
            tuple(float(x) for x in nnref.nn_accuracy(D, n)), (ph, tag)
        if tag == 'test':
            assert 'precision' not in m and 'recall' not in m
        else:
            assert (m['precision'], m['recall']) == tuple(float(x) for x in nnref.precision_recall(D, n, 3)), (ph, tag)
        assert 'psnr' in m and 'mse' in m and 'nrmse' in m            # the per-batch metrics are still there


def test_without_the_flags_nothing_new_is_reported(dataset, tmp_path, capsys):
    from saragan_amd.train import run_training
    args = _args(dataset, tmp_path / 'log', False)
    run_training(args, log_every=10 ** 6)
    text = capsys.readouterr().out
    assert len(args._metric_tap) == 12 and args._metric_sets == []
    for _, _, m, _ in args._metric_tap:
        assert not set(m) & set(NEW_KEYS)
        assert 'psnr' in m
    for word in ('MMD', '1-NN', 'Precision / recall', 'switched off', 'sample metrics took'):
        assert word not in text
