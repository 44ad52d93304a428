"""Host side of the intensity-histogram metrics (saragan_amd/metrics/intensity_metrics.py): the three distances on count
vectors against the loops of tests/histref.py, the flags, save_metrics with the flag off, the argument checks of
functional.intensity_hist that run without a device, and the reference's statistic on the golden case."""
import os

import numpy as np
import pytest
import torch

from tests import histref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'kms_reference.npz')
BASE = ['pgan', '/data/', '--start_shape', '(1, 4, 4, 4)', '--final_shape', '(1, 32, 32, 32)', '--starting_phase', '2',
        '--ending_phase', '3', '--latent_dim', '16', '--noise_stddev', '0.01']


def test_distances_against_the_loops():
    from saragan_amd.metrics.intensity_metrics import histogram_distances
    rng = np.random.default_rng(0)
    for bins in (1, 2, 7, 64, 300):
        for _ in range(5):
            r = rng.integers(0, 10 ** int(rng.integers(1, 10)), bins + 1)
            f = rng.integers(0, 10 ** int(rng.integers(1, 10)), bins + 1)
            r[int(rng.integers(0, bins))] += 1      # no empty side
            f[int(rng.integers(0, bins))] += 1
            got, want = histogram_distances(r, f), histref.distances(r, f)
            for key in ('ks', 'w1', 'max_density_gap'):
                assert got[key] == want[key], (bins, key)      # both are the correctly rounded exact rational
            assert (got['nan_real'], got['nan_fake']) == (int(r[-1]), int(f[-1]))
    # device-shaped input: [1, bins + 1] tensors
    a, b = torch.tensor([[3, 1, 0, 9]]), torch.tensor([[1, 1, 2, 0]])
    assert histogram_distances(a, b)['ks'] == histref.distances(a.numpy(), b.numpy())['ks']


def test_identical_disjoint_and_shifted():
    from saragan_amd.metrics.intensity_metrics import histogram_distances
    rng = np.random.default_rng(1)
    h = rng.integers(0, 10 ** 9, 101)
    d = histogram_distances(h, h)
    assert (d['ks'], d['w1'], d['max_density_gap']) == (0.0, 0.0, 0.0)
    d = histogram_distances(h, 3 * h)                # the same distribution from three times the samples
    assert (d['ks'], d['w1'], d['max_density_gap']) == (0.0, 0.0, 0.0)
    left, right = np.zeros(41, np.int64), np.zeros(41, np.int64)
    left[:10], right[25:40] = rng.integers(1, 1000, 10), rng.integers(1, 1000, 15)
    assert histogram_distances(left, right)['ks'] == 1.0
    for shift in (1, 7, 30):
        base = np.zeros(200, np.int64)
        base[20:120] = rng.integers(0, 10 ** 6, 100)
        moved = np.roll(base, shift)
        moved[-1] = base[-1] = 5                     # (the NaN column does not move and does not count)
        assert histogram_distances(base, moved)['w1'] == float(shift)
        assert histogram_distances(base, 7 * moved)['w1'] == float(shift)


def test_nan_column_and_empty_side():
    from saragan_amd.metrics.intensity_metrics import histogram_distances
    d = histogram_distances([1, 1, 0, 40], [0, 1, 1, 2])
    assert (d['nan_real'], d['nan_fake']) == (40, 2)
    assert d['ks'] == 0.5 and d['w1'] == 1.0 and d['max_density_gap'] == 0.5
    with pytest.raises(ValueError, match='finite'):
        histogram_distances([0, 0, 0, 9], [1, 2, 3, 0])
    with pytest.raises(ValueError, match='finite'):
        histogram_distances([1, 2, 3, 0], [0, 0, 0, 0])
    with pytest.raises(ValueError):
        histogram_distances([1, 2, 3], [1, 2, 3, 4])
    with pytest.raises(ValueError):
        histogram_distances([0.5, 1.0], [1.0, 2.0])      # counts are integers


def test_format_lines_and_levels():
    from saragan_amd.metrics import intensity_metrics as IM
    m = {'intensity_ks': [0.25, 0.5], 'intensity_w1': [12.5, 1.0], 'intensity_gap': [0.125, 0.0]}
    assert IM.format_lines(m) == ['Intensity KS (per level): 0.25 0.5', 'Intensity W1 (per level, data units): 12.5 1',
                                  'Intensity max density gap (per level): 0.125 0']
    assert IM.format_lines({}) == []
    assert IM.usable_levels((2, 1, 8, 16, 16), 3) == 3 and IM.usable_levels((2, 1, 4, 16, 16), 4) == 3
    assert IM.usable_levels((2, 1, 3, 16, 16), 2) == 1 and IM.usable_levels((5, 7), 1) == 1
    acc = IM.IntensityAccumulator(0, 65, levels=2)
    assert acc.level_range(0) == (0, 65) and acc.level_range(1) == (-32, 32)
    assert IM.parse_range('-1024,3071') == (-1024, 3071)
    for bad in ('5', '5,5', '9,1', 'a,b'):
        with pytest.raises(ValueError):
            IM.parse_range(bad)
    with pytest.raises(ValueError):
        IM.IntensityAccumulator(5, 5)


def test_parser_takes_the_flags():
    from saragan_amd.main import build_parser, finalize_hist_args
    from saragan_amd.metrics.save_metrics import get_compute_metrics_dict
    args, unknown = build_parser().parse_known_args(BASE)
    assert not unknown
    assert (args.compute_intensity_hist, args.hist_range, args.hist_levels) == (False, None, 1)
    flags = get_compute_metrics_dict(args)
    assert 'compute_intensity_hist' in flags and not any(flags.values())
    assert finalize_hist_args(args).hist_range is None          # off: nothing is asked for
    args, unknown = build_parser().parse_known_args(BASE + ['--compute_intensity_hist', '--hist_range=-1024,3071',
                                                            '--hist_levels', '3'])
    assert not unknown
    finalize_hist_args(args)
    assert (args.compute_intensity_hist, args.hist_range, args.hist_levels) == (True, (-1024, 3071), 3)
    assert get_compute_metrics_dict(args)['compute_intensity_hist']
    args, _ = build_parser().parse_known_args(BASE + ['--compute_intensity_hist'])
    with pytest.raises(SystemExit, match='--hist_range'):
        finalize_hist_args(args)
    for bad in ('7', '9,1', '0,100000', 'x,y'):
        args, _ = build_parser().parse_known_args(BASE + ['--compute_intensity_hist', '--hist_range', bad])
        with pytest.raises(SystemExit, match='--hist_range'):
            finalize_hist_args(args)
    args, _ = build_parser().parse_known_args(BASE + ['--compute_intensity_hist', '--hist_range', '0,10', '--hist_levels', '0'])
    with pytest.raises(SystemExit, match='--hist_levels'):
        finalize_hist_args(args)


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


def test_save_metrics_with_the_flag_off(tmp_path, monkeypatch, capsys):
    """compute_intensity_hist off, called positionally with the signature it always had: no accumulator is built, nothing
    is launched or printed, no key is added."""
    from saragan_amd.metrics import save_metrics as SMod
    files = []
    for i in range(4):
        np.save(tmp_path / f'{i}.npy', np.full((4, 4, 4), float(i)))
        files.append(str(tmp_path / f'{i}.npy'))

    def boom(*a, **k):
        raise AssertionError('the intensity histograms ran with their flag off')
    monkeypatch.setattr(SMod.IM, 'IntensityAccumulator', boom)
    monkeypatch.setattr(SMod.IM, 'histogram_distances', boom)
    monkeypatch.setattr(SMod.IM.F, 'intensity_hist', boom)
    gen = lambda: torch.zeros(2, 1, 4, 4, 4)
    flags = SMod.get_compute_metrics_dict(type('A', (), {'compute_FID': True})())
    assert flags['compute_intensity_hist'] is False
    kept = []
    m = SMod.save_metrics(None, _Sess(), _Subset(files), gen, 2, 1, 0, 4, False, False, flags, 4, None, None, True, keep=kept)
    text = capsys.readouterr().out
    assert m == {} and len(kept) == 2
    assert 'Intensity' not in text and 'intensity' not in text
    # on, without a range: refused by name before anything runs
    flags['compute_intensity_hist'] = True
    with pytest.raises(ValueError, match='hist_range'):
        SMod.save_metrics(None, _Sess(), _Subset(files), gen, 2, 1, 0, 4, False, False, flags, 4, None, None, True)


def test_argument_errors_on_cpu_tensors():
    from saragan_amd import _lib
    from saragan_amd import functional as F
    x = torch.zeros(2, 3, 4)
    with pytest.raises(ValueError, match='device tensor'):
        F.intensity_hist(x, 0, 8)
    with pytest.raises(ValueError, match='device tensor'):
        F.intensity_hist(x, 0, 8, out=torch.zeros(2, 9, dtype=torch.int64), accumulate=True)
    for bad in (x.to(torch.float64), x.to(torch.int32), x.to(torch.int64), x > 0, np.zeros((2, 3), np.float32)):
        with pytest.raises(TypeError):
            F.intensity_hist(bad, 0, 8)
    with pytest.raises(ValueError, match='contiguous'):
        F.intensity_hist(x.transpose(0, 2), 0, 8)
    with pytest.raises(ValueError, match='contiguous'):
        F.intensity_hist(torch.zeros(()), 0, 8)
    for lo, hi in ((8, 8), (9, 1)):
        with pytest.raises(ValueError, match='empty'):
            F.intensity_hist(x, lo, hi)
    with pytest.raises(ValueError, match='at most'):
        F.intensity_hist(x, -5, _lib.INTENSITY_HIST_MAX_BINS - 4)
    with pytest.raises(ValueError, match='32-bit'):
        F.intensity_hist(x, 2 ** 31 - 5, 2 ** 31 + 5)
    with pytest.raises(ValueError, match='finite'):
        F.intensity_hist(x, 0, 8, scale=float('inf'))
    for out in (torch.zeros(2, 9), torch.zeros(2, 8, dtype=torch.int64), torch.zeros(1, 9, dtype=torch.int64),
                torch.zeros(9, 2, dtype=torch.int64).t(), np.zeros((2, 9), np.int64)):
        with pytest.raises(ValueError, match='out must be'):
            F.intensity_hist(x, 0, 8, out=out)
    with pytest.raises(ValueError, match='out must be'):
        F.intensity_hist(x, 0, 8, pooled=True, out=torch.zeros(2, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match='accumulate'):
        F.intensity_hist(x, 0, 8, accumulate=True)
    assert _lib.INTENSITY_HIST_MAX_BINS >= 4096


def test_the_reference_s_statistic_on_the_golden_case():
    """tests/golden/kms_reference.npz (tools/make_golden_kms.py): the reference's kolmogorov_smirnov_distance is the largest
    gap between the MEANS of n per-volume densities; from pooled counts it is one division, so the two differ by the
    reference's n + 3 roundings of values <= 1: 4 n 2^-53 absolute."""
    from saragan_amd.metrics.intensity_metrics import histogram_distances
    g = np.load(GOLDEN)
    assert sorted(g.files) == ['clip_range', 'fake', 'intercept', 'real', 'value']
    lo, hi = (int(v) for v in g['clip_range'])
    ic = float(g['intercept'])
    real, fake = g['real'], g['fake']
    n = real.shape[0]
    assert lo >= 0 and real.dtype == fake.dtype == np.float32
    for x in (real, fake):      # every volume attains both clip bounds: np.histogram's automatic range is the fixed grid
        col = histref.columns(x.reshape(n, -1), lo, hi, ic, ic)
        assert (col.min(axis=1) == 0).all() and (histref.mapped(x, ic, ic).reshape(n, -1).max(axis=1) >= hi).all()
        assert (histref.mapped(x, ic, ic).reshape(n, -1).min(axis=1) < lo + 1).all()
    hr, hf = histref.hist(real, lo, hi, ic, ic, pooled=True), histref.hist(fake, lo, hi, ic, ic, pooled=True)
    bound = 4 * n * 2.0 ** -53
    assert abs(histref.distances(hr, hf)['max_density_gap'] - float(g['value'])) <= bound
    assert abs(histogram_distances(hr, hf)['max_density_gap'] - float(g['value'])) <= bound
