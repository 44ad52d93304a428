"""Host side of the download-free sample metrics (saragan_amd/metrics/sample_metrics.py): the three reductions over a
squared-distance matrix are plain torch and run on CPU f64 tensors here, against the loop-by-definition restatement in
tests/nnref.py; the new flags; save_metrics with the flags off; the command line's shape check."""
import numpy as np
import pytest
import torch

from tests import nnref

K = 3


def _matrix(R, F):
    return nnref.sqdist(np.concatenate([R, F]).astype(np.float64))


def _check_against_nnref(D, n, k=K):
    from saragan_amd.metrics import sample_metrics as SM
    Dt = torch.as_tensor(D, dtype=torch.float64)
    got_nn, got_pr = SM.nn_accuracy(Dt, n), SM.precision_recall(Dt, n, k)
    assert all(isinstance(x, float) for x in got_nn + got_pr)
    assert got_nn == tuple(float(x) for x in nnref.nn_accuracy(D, n))
    assert got_pr == tuple(float(x) for x in nnref.precision_recall(D, n, k))
    return got_nn, got_pr


def test_random_matrix_matches_the_definitions():
    from saragan_amd.metrics import sample_metrics as SM
    R, F = nnref.seed1_sets()
    D = _matrix(R, F)
    (tot, real, fake), (prec, rec) = _check_against_nnref(D, 24)
    # the figures the fp64 pipeline gives for this data
    assert (round(tot, 3), round(real, 3), round(fake, 3)) == (0.708, 0.458, 0.958)
    assert (round(prec, 3), round(rec, 3)) == (0.958, 0.292)
    Dt = torch.as_tensor(D)
    got = SM.mmd2(Dt, 24)
    assert isinstance(got, float) and abs(got - nnref.mmd2(D, 24)) <= 1e-12
    assert abs(SM.mmd2(Dt, 24, sigma2=7.5) - nnref.mmd2(D, 24, sigma2=7.5)) <= 1e-12
    m = SM.metrics_from_matrix(Dt, 24, K)
    assert sorted(m) == ['mmd', 'nn_accuracy', 'nn_accuracy_fake', 'nn_accuracy_real', 'precision', 'recall']
    assert (m['nn_accuracy'], m['nn_accuracy_real'], m['nn_accuracy_fake']) == (tot, real, fake)
    assert (m['precision'], m['recall'], m['mmd']) == (prec, rec, got)


def test_identical_sets():
    R, _ = nnref.seed1_sets()
    F = R[np.random.default_rng(5).permutation(24)]
    (_, _, fake), (prec, rec) = _check_against_nnref(_matrix(R, F), 24)
    assert prec == 1.0 and rec == 1.0
    assert fake == 0.0          # every fake's nearest other point is the real it copies (distance 0)


def test_far_apart_clusters():
    from saragan_amd.metrics import sample_metrics as SM
    R, F = nnref.seed1_sets()
    D = _matrix(R, F + 100.0)
    (tot, real, fake), (prec, rec) = _check_against_nnref(D, 24)
    assert (tot, real, fake) == (1.0, 1.0, 1.0) and (prec, rec) == (0.0, 0.0)
    got = SM.mmd2(torch.as_tensor(D), 24)
    assert got > 0 and abs(got - nnref.mmd2(D, 24)) <= 1e-12


def test_ties_resolve_to_the_lowest_index():
    from saragan_amd.metrics import sample_metrics as SM
    # points on a line: 0, 2 | 1, 3, then a far pair | pair so that n = 4 >= k + 1
    R = np.array([[0.0], [2.0], [50.0], [60.0]])
    F = np.array([[1.0], [3.0], [55.0], [65.0]])
    D = _matrix(R, F)
    n = 4
    # real 1 (at 2) is 1 away from fake 0 (index 4) and fake 1 (index 5): 4 wins.  fake 0 (at 1) is 1 away from real 0
    # (index 0) and real 1 (index 1): 0 wins.  real 2 (50) is 5 from fake 2 (index 6) only; fake 2 (55) is 5 from real 2
    # (index 2) and real 3 (index 3): 2 wins.
    assert [nnref.nearest_other(D, i) for i in range(2 * n)] == [4, 4, 6, 6, 0, 1, 2, 3]
    _check_against_nnref(D, n)
    assert SM.nn_accuracy(torch.as_tensor(D), n) == (0.0, 0.0, 0.0)
    # a tie between a same-label and an other-label neighbour: the decision depends on the index order alone
    R2, F2 = np.array([[0.0], [1.0], [20.0], [30.0]]), np.array([[-1.0], [40.0], [50.0], [60.0]])
    D2 = _matrix(R2, F2)
    assert nnref.nearest_other(D2, 0) == 1          # real 1 (index 1) and fake 0 (index 4) are both 1 away from real 0
    _check_against_nnref(D2, 4)
    # ties ON a radius count as inside (<=)
    _check_against_nnref(D, n, k=1)
    _check_against_nnref(D, n, k=2)


def test_too_few_samples_raise():
    from saragan_amd.metrics import sample_metrics as SM
    R, F = nnref.seed1_sets()
    D = torch.as_tensor(_matrix(R[:3], F[:3]))
    with pytest.raises(ValueError):
        SM.precision_recall(D, 3, k=3)              # n = k
    assert len(SM.precision_recall(D, 3, k=2)) == 2
    with pytest.raises(ValueError):
        SM.mmd2(torch.zeros(2, 2, dtype=torch.float64), 1)
    with pytest.raises(ValueError):
        SM.nn_accuracy(D, 4)                        # not the [2n, 2n] matrix of n = 4
    with pytest.raises(RuntimeError, match='GPU only'):
        SM.pairwise_sqdist(torch.zeros(4, 8))


def test_parser_takes_the_flags():
    from saragan_amd.main import build_parser
    from saragan_amd.metrics.save_metrics import get_compute_metrics_dict
    base = ['pgan', '/data/', '--start_shape', '(1, 4, 4, 4)', '--final_shape', '(1, 32, 32, 32)', '--starting_phase', '2',
            '--ending_phase', '3', '--latent_dim', '16', '--noise_stddev', '0.01']
    args, unknown = build_parser().parse_known_args(base)
    assert not unknown
    assert (args.compute_mmd, args.compute_nn_accuracy, args.compute_precision_recall, args.pr_k) == (False, False, False, 3)
    flags = get_compute_metrics_dict(args)
    assert not any(flags.values()) and {'compute_mmd', 'compute_nn_accuracy', 'compute_precision_recall'} <= set(flags)
    args, unknown = build_parser().parse_known_args(base + ['--compute_mmd', '--compute_nn_accuracy',
                                                            '--compute_precision_recall', '--pr_k', '5'])
    assert not unknown
    assert (args.compute_mmd, args.compute_nn_accuracy, args.compute_precision_recall, args.pr_k) == (True, True, True, 5)
    flags = get_compute_metrics_dict(args)
    assert flags['compute_mmd'] and flags['compute_nn_accuracy'] and flags['compute_precision_recall']
    assert not flags['compute_swds']


class _Subset:
    """What save_metrics uses of a NumpyPathDataset."""

    def __init__(self, files):
        self.scratch_files, self.last_labels, self.at = files, None, 0

    def batch(self, n):
        out = np.stack([np.load(f) for f in self.scratch_files[self.at:self.at + n]])[:, None].astype(np.float32)
        self.at += n
        return out


class _Sess:
    def run(self, what, feed_dict=None):
        return what()


def test_save_metrics_with_the_flags_off(tmp_path, monkeypatch, capsys):
    """None of the three flags: nothing is retained or launched, the printed text and the keys are what they were."""
    from saragan_amd.metrics import save_metrics as SMod
    files = []
    for i in range(4):
        np.save(tmp_path / f'{i}.npy', np.full((4, 4, 4), float(i)))
        files.append(str(tmp_path / f'{i}.npy'))

    def boom(*a, **k):
        raise AssertionError('the pooled evaluation ran with its flags off')
    monkeypatch.setattr(SMod.SM, 'pairwise_sqdist', boom)
    monkeypatch.setattr(SMod, '_sample_set_metrics', boom)
    gen = lambda: torch.zeros(2, 1, 4, 4, 4)
    flags = SMod.get_compute_metrics_dict(type('A', (), {'compute_FID': True})())
    kept, sets = [], []
    m = SMod.save_metrics(None, _Sess(), _Subset(files), gen, 2, 1, 0, 4, False, False, flags, 4, None, None, True, keep=kept,
                          keep_sets=sets)
    text = capsys.readouterr().out
    assert m == {} and sets == [] and len(kept) == 2
    assert 'FID is NOT computed' in text
    for word in ('MMD', '1-NN', 'Precision', 'switched off', 'skipped'):
        assert word not in text


def test_cli_refuses_unequal_shapes(tmp_path):
    from saragan_amd.metrics import sample_metrics as SM
    a, b = tmp_path / 'real', tmp_path / 'fake'
    a.mkdir()
    b.mkdir()
    for i in range(5):
        np.save(a / f'{i}.npy', np.zeros((4, 8, 8), np.float32))
        np.save(b / f'{i}.npy', np.zeros((4, 8, 4), np.float32))
    with pytest.raises(SystemExit, match='differ in shape'):
        SM.main([str(a), str(b)])
    np.save(b / '9.npy', np.zeros((2, 2, 2), np.float32))
    with pytest.raises(SystemExit, match='different shapes'):
        SM.main([str(a), str(b)])
    with pytest.raises(SystemExit):
        SM.main([str(a), str(tmp_path / 'real'), '--data_mean', '1'])       # --data_mean without --data_stddev
