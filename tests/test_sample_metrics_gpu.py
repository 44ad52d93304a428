"""get_sample_metrics end to end on the GPU against the fp64 pipeline of tests/nnref.py, on data whose every discrete
decision (which point is nearest, which side of a radius a distance falls) is separated by more than 10 x the kernel's
rounding bound: the discrete statistics must then be EQUAL, and MMD^2 within the bound's image under the Gaussian kernel."""
import numpy as np
import pytest
import torch

from tests import nnref

pytestmark = pytest.mark.gpu


def test_command_line_on_two_directories(tmp_path, capsys):
    """The seed-1 sets as two directories of .npy volumes, one more fake than reals (min(count) is used), with a
    normalisation that is exact in f32 (x / 2 on data scaled by 2): the printed lines and the returned values."""
    from saragan_amd.metrics import sample_metrics as SM
    R, F = nnref.seed1_sets()
    for name, X in (('real', R), ('fake', np.concatenate([F, F[:1]]))):
        (tmp_path / name).mkdir()
        for i, x in enumerate(X):
            np.save(tmp_path / name / f'{i:03d}.npy', (2.0 * x).reshape(2, 3, 4))
    m = SM.main([str(tmp_path / 'real'), str(tmp_path / 'fake'), '--k', '3', '--data_mean', '0', '--data_stddev', '2'])
    text = capsys.readouterr().out
    D = nnref.sqdist(np.concatenate([R, F]))
    assert (m['nn_accuracy'], m['nn_accuracy_real'], m['nn_accuracy_fake']) == tuple(float(x) for x in nnref.nn_accuracy(D, 24))
    assert (m['precision'], m['recall']) == tuple(float(x) for x in nnref.precision_recall(D, 24, 3))
    assert '24 real and 24 generated volumes of shape (2, 3, 4)' in text
    assert f"MMD^2: {m['mmd']:.6g}" in text and '1-NN accuracy (total real fake): 0.7083 0.4583 0.9583' in text
    assert 'Precision / recall (k=3): 0.9583 / 0.2917' in text


def test_seed1_sets_end_to_end():
    from saragan_amd import _lib
    from saragan_amd.metrics import sample_metrics as SM
    R, F = nnref.seed1_sets()
    n, k = 24, 3
    Z = np.concatenate([R, F])
    D = nnref.sqdist(Z)
    bound = float(nnref.sqdist_bound(Z, Z, int(_lib.load().sg_pairwise_sqdist_chunk())).max())
    nn_gap, rad_gap = nnref.deciding_gaps(D, n, k)
    # a condition on the input, not a tolerance: no rounding within the bound can move a decision
    assert nn_gap > 10 * bound and rad_gap > 10 * bound, (nn_gap, rad_gap, bound)
    shape = (24, 1, 2, 3, 4)
    kept = []
    m = SM.get_sample_metrics(torch.as_tensor(R.reshape(shape), device='cuda'), torch.as_tensor(F.reshape(shape), device='cuda'),
                              k=k, keep=kept)
    assert sorted(m) == ['mmd', 'nn_accuracy', 'nn_accuracy_fake', 'nn_accuracy_real', 'precision', 'recall']
    assert all(isinstance(x, float) for x in m.values())
    assert len(kept) == 1 and kept[0].shape == (48, 48) and kept[0].dtype == np.float64
    assert (np.abs(kept[0] - D) <= nnref.sqdist_bound(Z, Z, int(_lib.load().sg_pairwise_sqdist_chunk()))).all()
    want_nn, want_pr = nnref.nn_accuracy(D, n), nnref.precision_recall(D, n, k)
    assert (m['nn_accuracy'], m['nn_accuracy_real'], m['nn_accuracy_fake']) == tuple(float(x) for x in want_nn)
    assert (m['precision'], m['recall']) == tuple(float(x) for x in want_pr)
    assert [round(float(x), 3) for x in want_nn] == [0.708, 0.458, 0.958] and [round(float(x), 3) for x in want_pr] == [0.958, 0.292]
    sigma2 = D[:n, :n].sum() / (n * (n - 1))
    want_mmd = nnref.mmd2(D, n)
    print(f'seed-1 sets: bound {bound:.3e}, gaps {nn_gap:.4f} {rad_gap:.4f}, MMD^2 {m["mmd"]:.9f} (fp64 {want_mmd:.9f}), '
          f'|err| {abs(m["mmd"] - want_mmd):.3e}, max |D err| {np.abs(kept[0] - D).max():.3e}')
    assert abs(m['mmd'] - want_mmd) <= 3 * bound / sigma2
