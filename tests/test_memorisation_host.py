"""The CPU path of the memorisation audit (metrics/memorisation.py --device cpu; table_ops.sqdist_exact / nearest_rows on CPU
tensors) against the numpy int64 restatement of its definitions in tests/memref.py.  Every comparison of a distance is ==."""
import json
import os

import numpy as np
import pytest
import torch

from tests import memref


def _run(tmp_path, name, extra=(), dtype=np.int16, holdout=False):
    from saragan_amd.metrics import memorisation
    train, fakes, hold = memref.planted(dtype)
    base = tmp_path / f'data_{np.dtype(dtype).name}'
    if not base.exists():
        memref.write_dir(str(base / 'train'), train, 'train')
        memref.write_dir(str(base / 'fake'), fakes, 'fake')
        memref.write_dir(str(base / 'holdout'), hold, 'real')
    report = str(tmp_path / f'{name}.json')
    argv = [str(base / 'train'), str(base / 'fake'), '--device', 'cpu', '--report', report] + list(extra)
    if holdout:
        argv += ['--holdout_dir', str(base / 'holdout')]
    returned = memorisation.main(argv)
    with open(report) as f:
        written = json.load(f)
    assert memref.strip(written) == memref.strip(json.loads(json.dumps(returned)))
    return written, (train, fakes, hold)


@pytest.mark.parametrize('dtype', ['uint8', 'int8', 'int16', 'uint16'])
def test_sqdist_exact_cpu_is_the_definition(dtype):
    rng = np.random.default_rng(3)
    info = np.iinfo(dtype)
    a = rng.integers(info.min, info.max + 1, size=(5, 3, 7)).astype(dtype)
    b = rng.integers(info.min, info.max + 1, size=(9, 3, 7)).astype(dtype)
    a[0], b[0] = info.min, info.max
    from saragan_amd import functional as F
    got = F.sqdist_exact(torch.from_numpy(a), torch.from_numpy(b))
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), memref.sqdist(a, b))
    sym = F.sqdist_exact(torch.from_numpy(a)).numpy()
    assert np.array_equal(sym, memref.sqdist(a, a)) and np.array_equal(sym, sym.T) and not sym.diagonal().any()


def test_sqdist_exact_rejects_what_it_cannot_take():
    from saragan_amd import functional as F
    x = torch.zeros((2, 4), dtype=torch.int16)
    with pytest.raises(TypeError):
        F.sqdist_exact(x.float())
    with pytest.raises(TypeError):
        F.sqdist_exact(x, x.to(torch.uint8))
    with pytest.raises(ValueError):
        F.sqdist_exact(x, torch.zeros((2, 5), dtype=torch.int16))
    with pytest.raises(ValueError):
        F.sqdist_exact(x[:, ::2])


def test_nearest_rows_cpu_ties_tails_chunks_and_own_id():
    from saragan_amd import functional as F
    rng = np.random.default_rng(5)
    d = rng.integers(0, 4, size=(6, 11)).astype(np.int64)      # many repeated values
    d[np.arange(6), np.arange(6)] = 0
    for k in (1, 3, 16):
        for skip in (False, True):
            want_d, want_i = memref.nearest(d, k, skip_self=skip)
            results = []
            for step in (1, 3, 11):
                best = None
                for at in range(0, 11, step):
                    part = torch.from_numpy(np.ascontiguousarray(d[:, at:at + step]))
                    best = F.nearest_rows(part, k, r_base=at, q_ids=torch.arange(6) if skip else None, best=best)
                results.append(best)
                for i in range(6):
                    n = len(want_d[i])
                    assert best[0][i, :n].tolist() == want_d[i] and best[1][i, :n].tolist() == want_i[i]
                    assert (best[0][i, n:] == 2 ** 63 - 1).all() and (best[1][i, n:] == -1).all()
            assert all(torch.equal(r[0], results[0][0]) and torch.equal(r[1], results[0][1]) for r in results)
    with pytest.raises(ValueError):
        F.nearest_rows(torch.zeros((2, 2), dtype=torch.int64), 17)
    with pytest.raises(ValueError):
        F.nearest_rows(torch.zeros((2, 2), dtype=torch.int64), 0)


def test_planted_copies_are_found_and_the_report_is_the_definition(tmp_path):
    rep, (train, fakes, hold) = _run(tmp_path, 'base', holdout=True)
    names = [f'train_{i:04d}.npy' for i in range(memref.N_TRAIN)]
    want, loo = memref.expected_rows(fakes, train, 3, names)
    assert rep['exact'] is True and rep['dtype'] == 'int16' and rep['voxels'] == 256 and rep['shape'] == list(memref.SHAPE)
    assert rep['pooled']['duplicates'] == 1
    f0, f1 = rep['fakes'][0], rep['fakes'][1]
    assert f0['duplicate'] and not f0['authentic'] and f0['nearest'][0] == names[memref.COPY_OF] and f0['d2'][0] == 0
    assert not f1['duplicate'] and not f1['authentic'] and f1['nearest'][0] == names[memref.NOISY_OF] and f1['d2'][0] == 256
    for i, (got, exp) in enumerate(zip(rep['fakes'], want)):
        assert got['file'] == f'fake_{i:04d}.npy'
        assert {k: v for k, v in got.items() if k != 'file'} == exp, i
    assert [t['loo'] for t in rep['train']] == loo
    assert [t['file'] for t in rep['train']] == names
    bad = sum(not r['authentic'] for r in want)
    assert rep['pooled']['unauthentic'] == bad and rep['pooled']['authentic_share'] == 1.0 - bad / memref.N_FAKE
    hwant, _ = memref.expected_rows(hold, train, 3, names)
    assert [{k: v for k, v in r.items() if k != 'file'} for r in rep['holdout']] == hwant
    assert rep['pooled']['holdout_unauthentic'] == sum(not r['authentic'] for r in hwant)
    z = memref.midrank_z([r['d2'][0] for r in want], [r['d2'][0] for r in hwant])
    assert abs(rep['pooled']['data_copying_z'] - z) <= 1e-12 * abs(z)
    assert rep['worst'][0] == 'fake_0000.npy' and rep['worst'][1] == 'fake_0001.npy'
    assert 'definition' in rep and rep['arguments']['k'] == 3


def test_mann_whitney_z_with_ties():
    from saragan_amd.metrics.memorisation import mann_whitney_z
    x, y = [0, 3, 3, 7, 9, 9, 9], [3, 4, 9, 9, 12]
    z = memref.midrank_z(x, y)
    assert abs(mann_whitney_z(x, y) - z) <= 1e-12 * abs(z)
    assert mann_whitney_z([1, 2], [3, 4, 5]) < 0 < mann_whitney_z([3, 4, 5], [1, 2])


def test_chunking_does_not_change_the_report(tmp_path):
    base, _ = _run(tmp_path, 'c40_q12', ['--chunk', '40', '--query_block', '12'], holdout=True)
    for chunk in (1, 7, 40):
        for block in (1, 12):
            rep, _ = _run(tmp_path, f'c{chunk}_q{block}', ['--chunk', str(chunk), '--query_block', str(block)], holdout=True)
            assert memref.strip(rep) == memref.strip(base), (chunk, block)


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_unsigned_directories(tmp_path, dtype):
    rep, (train, fakes, _) = _run(tmp_path, 'u', ['--k', '2'], dtype=np.dtype(dtype))
    want, loo = memref.expected_rows(fakes, train, 2, [f'train_{i:04d}.npy' for i in range(memref.N_TRAIN)])
    assert rep['exact'] is True and rep['dtype'] == dtype
    assert [{k: v for k, v in r.items() if k != 'file'} for r in rep['fakes']] == want
    assert [t['loo'] for t in rep['train']] == loo and rep['pooled']['duplicates'] >= 1


def test_float32_directory_is_marked_inexact(tmp_path, capsys):
    rep, (train, fakes, _) = _run(tmp_path, 'f', dtype=np.float32)
    assert rep['exact'] is False and rep['dtype'] == 'float32'
    assert 'not exact' in capsys.readouterr().out
    assert rep['fakes'][0]['nearest'][0] == f'train_{memref.COPY_OF:04d}.npy' and rep['fakes'][0]['duplicate']
    assert rep['fakes'][1]['nearest'][0] == f'train_{memref.NOISY_OF:04d}.npy' and not rep['fakes'][1]['authentic']
    d = ((fakes[3].astype(np.float64) - train.astype(np.float64)) ** 2).reshape(memref.N_TRAIN, -1).sum(1)
    assert rep['fakes'][3]['nearest_index'][0] == int(d.argmin())
    assert rep['fakes'][3]['d2'][0] == pytest.approx(d.min(), rel=1e-12)


def test_limits(tmp_path):
    rep, (train, fakes, _) = _run(tmp_path, 'lim', ['--max_queries', '4', '--max_train', '9', '--k', '16'])
    want, loo = memref.expected_rows(fakes[:4], train[:9], 16, [f'train_{i:04d}.npy' for i in range(9)])
    assert [{k: v for k, v in r.items() if k != 'file'} for r in rep['fakes']] == want      # k > files: 9 entries a row
    assert len(rep['fakes'][0]['d2']) == 9 and [t['loo'] for t in rep['train']] == loo


def test_bad_directories_are_errors_before_anything_is_written(tmp_path):
    from saragan_amd.metrics import memorisation
    train, fakes, _ = memref.planted()
    good_t, good_f = memref.write_dir(str(tmp_path / 't'), train, 'train'), memref.write_dir(str(tmp_path / 'f'), fakes, 'fake')
    other_shape = memref.write_dir(str(tmp_path / 's'), np.zeros((3, 4, 8, 4), np.int16), 'fake')
    other_dtype = memref.write_dir(str(tmp_path / 'd'), fakes.astype(np.uint16), 'fake')
    mixed_shape = memref.write_dir(str(tmp_path / 'ms'), fakes[:2], 'fake')
    np.save(os.path.join(mixed_shape, 'fake_9999.npy'), np.zeros((4, 8, 9), np.int16))
    mixed_dtype = memref.write_dir(str(tmp_path / 'md'), fakes[:2], 'fake')
    np.save(os.path.join(mixed_dtype, 'fake_9999.npy'), np.zeros(memref.SHAPE, np.int8))
    empty = str(tmp_path / 'e')
    os.makedirs(empty)
    report = str(tmp_path / 'never.json')
    for t, f in ((good_t, other_shape), (good_t, other_dtype), (good_t, mixed_shape), (good_t, mixed_dtype), (good_t, empty),
                 (empty, good_f), (mixed_shape, good_f)):
        with pytest.raises(SystemExit) as e:
            memorisation.main([t, f, '--device', 'cpu', '--report', report])
        assert 'memorisation:' in str(e.value)
        assert not os.path.exists(report) and not os.path.exists(os.path.join(f, 'memorisation.json'))
    with pytest.raises(SystemExit):
        memorisation.main([good_t, good_f, '--device', 'cpu', '--report', report, '--k', '17'])
    with pytest.raises(SystemExit):      # the sheet is drawn on the device
        memorisation.main([good_t, good_f, '--device', 'cpu', '--report', report, '--png', str(tmp_path / 'p.png')])
    assert not os.path.exists(report)
