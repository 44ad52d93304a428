"""python -m saragan_amd.metrics.memorisation on the GPU (sg_sqdist_exact + sg_topk_merge, the training set streamed through
pinned buffers) against the numpy int64 restatement of its definitions in tests/memref.py and against its own CPU path."""
import json
import os
import struct

import numpy as np
import pytest
import torch

from tests import memref

pytestmark = pytest.mark.gpu

NAMES = [f'train_{i:04d}.npy' for i in range(memref.N_TRAIN)]


@pytest.fixture(scope='module')
def data(tmp_path_factory):
    """The planted int16 directories, written once, with the arrays they hold."""
    base = tmp_path_factory.mktemp('memorisation')
    train, fakes, hold = memref.planted(np.int16)
    dirs = {'train': memref.write_dir(str(base / 'train'), train, 'train'), 'fake': memref.write_dir(str(base / 'fake'), fakes, 'fake'),
            'holdout': memref.write_dir(str(base / 'holdout'), hold, 'real'), 'base': base}
    return dirs, (train, fakes, hold)


def _run(dirs, name, extra=(), device='cuda', holdout=True):
    from saragan_amd.metrics import memorisation
    report = str(dirs['base'] / f'{name}.json')
    argv = [dirs['train'], dirs['fake'], '--device', device, '--report', report] + list(extra)
    if holdout:
        argv += ['--holdout_dir', dirs['holdout']]
    memorisation.main(argv)
    with open(report) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def base_report(data):
    return _run(data[0], 'base')


def _rows(rows):
    return [{k: v for k, v in r.items() if k != 'file'} for r in rows]


def test_planted_copies_and_every_entry_of_the_report(data, base_report):
    rep, (train, fakes, hold) = base_report, data[1]
    want, loo = memref.expected_rows(fakes, train, 3, NAMES)
    assert rep['exact'] is True and rep['dtype'] == 'int16' and rep['voxels'] == 256
    assert rep['pooled']['duplicates'] == 1
    f0, f1 = rep['fakes'][0], rep['fakes'][1]
    assert f0['duplicate'] and not f0['authentic'] and f0['nearest'][0] == NAMES[memref.COPY_OF] and f0['d2'][0] == 0
    assert not f1['duplicate'] and not f1['authentic'] and f1['nearest'][0] == NAMES[memref.NOISY_OF] and f1['d2'][0] == 256
    assert _rows(rep['fakes']) == want      # the independent fakes' rows too, entry for entry
    assert [t['loo'] for t in rep['train']] == loo and [t['file'] for t in rep['train']] == NAMES
    bad = sum(not r['authentic'] for r in want)
    assert rep['pooled']['unauthentic'] == bad and rep['pooled']['authentic_share'] == 1.0 - bad / memref.N_FAKE
    hwant, _ = memref.expected_rows(hold, train, 3, NAMES)
    assert _rows(rep['holdout']) == hwant
    assert rep['pooled']['holdout_unauthentic'] == sum(not r['authentic'] for r in hwant)
    z = memref.midrank_z([r['d2'][0] for r in want], [r['d2'][0] for r in hwant])
    assert abs(rep['pooled']['data_copying_z'] - z) <= 1e-12 * abs(z)
    assert rep['worst'][:2] == ['fake_0000.npy', 'fake_0001.npy']
    assert set(rep['seconds']) == {'read', 'upload', 'distances', 'topk', 'total'}


def test_cpu_and_device_write_the_same_report(data, base_report):
    assert memref.strip(_run(data[0], 'cpu', device='cpu')) == memref.strip(base_report)


@pytest.mark.parametrize('chunk', [1, 7, 40])
@pytest.mark.parametrize('block', [1, 12])
def test_chunking_does_not_change_the_report(data, base_report, chunk, block):
    rep = _run(data[0], f'c{chunk}_q{block}', ['--chunk', str(chunk), '--query_block', str(block)])
    assert memref.strip(rep) == memref.strip(base_report)


def test_png_sheet(data):
    from saragan_amd import preview
    png = str(data[0]['base'] / 'pairs.png')
    rep = _run(data[0], 'png', ['--png', png, '--png_pairs', '3', '--window=-1024,2047'], holdout=False)
    with open(png, 'rb') as f:
        raw = f.read()
    assert raw[:8] == b'\x89PNG\r\n\x1a\n' and raw[12:16] == b'IHDR'
    w, h, depth, colour = struct.unpack('>IIBB', raw[16:26])
    tops, heights, col_w = preview.sheet_layout(memref.SHAPE, preview.parse_views(preview.DEFAULT_VIEWS))
    assert (w, h, depth, colour) == (2 * 3 * col_w, sum(heights), 8, 0)
    assert b'fake_0000.npy|' + NAMES[memref.COPY_OF].encode() in raw and len(rep['worst']) == 3
    # the copy's two columns are the same pixels
    import zlib
    at, idat = 8, b''
    while at < len(raw):
        n, kind = struct.unpack('>I4s', raw[at:at + 8])
        if kind == b'IDAT':
            idat += raw[at + 8:at + 8 + n]
        at += 12 + n
    img = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, w + 1)[:, 1:]
    assert np.array_equal(img[:, :col_w], img[:, col_w:2 * col_w]) and img.max() > 0


@pytest.mark.parametrize('dtype', ['uint16', 'uint8'])
def test_unsigned_directories(tmp_path, dtype):
    train, fakes, _ = memref.planted(np.dtype(dtype))
    dirs = {'train': memref.write_dir(str(tmp_path / 'train'), train, 'train'),
            'fake': memref.write_dir(str(tmp_path / 'fake'), fakes, 'fake'), 'base': tmp_path}
    rep = _run(dirs, 'u', ['--k', '2', '--chunk', '16'], holdout=False)
    want, loo = memref.expected_rows(fakes, train, 2, NAMES)
    assert rep['exact'] is True and rep['dtype'] == dtype
    assert _rows(rep['fakes']) == want and [t['loo'] for t in rep['train']] == loo
    assert os.path.exists(str(tmp_path / 'u.json'))


def test_float32_directory_takes_the_f32_path(tmp_path, capsys):
    train, fakes, _ = memref.planted(np.float32)
    dirs = {'train': memref.write_dir(str(tmp_path / 'train'), train, 'train'),
            'fake': memref.write_dir(str(tmp_path / 'fake'), fakes, 'fake'), 'base': tmp_path}
    rep = _run(dirs, 'f', ['--chunk', '16'], holdout=False)
    assert rep['exact'] is False and 'not exact' in capsys.readouterr().out
    assert rep['fakes'][0]['nearest'][0] == NAMES[memref.COPY_OF] and rep['fakes'][1]['nearest'][0] == NAMES[memref.NOISY_OF]
    assert not rep['fakes'][1]['authentic']
    d = ((fakes[3].astype(np.float64) - train.astype(np.float64)) ** 2).reshape(memref.N_TRAIN, -1).sum(1)
    assert rep['fakes'][3]['nearest_index'][0] == int(d.argmin())
    # |a|^2 + |b|^2 - 2 a.b with f32 chains of at most 1024 terms: 2 gamma_n (|a|^2 + |b|^2), n = 256 (tests/test_pdist_gpu.py)
    norms = float((fakes[3].astype(np.float64) ** 2).sum() + (train[int(d.argmin())].astype(np.float64) ** 2).sum())
    assert abs(rep['fakes'][3]['d2'][0] - d.min()) <= 2 * (256 * 2.0 ** -24 / (1 - 256 * 2.0 ** -24)) * norms


def test_bad_directories_are_errors_before_anything_is_written(data, tmp_path):
    from saragan_amd.metrics import memorisation
    dirs, (train, fakes, _) = data
    other_shape = memref.write_dir(str(tmp_path / 's'), np.zeros((3, 4, 8, 4), np.int16), 'fake')
    mixed_dtype = memref.write_dir(str(tmp_path / 'md'), fakes[:2], 'fake')
    np.save(os.path.join(mixed_dtype, 'fake_9999.npy'), np.zeros(memref.SHAPE, np.int8))
    empty = str(tmp_path / 'e')
    os.makedirs(empty)
    report = str(tmp_path / 'never.json')
    for f in (other_shape, mixed_dtype, empty):
        with pytest.raises(SystemExit):
            memorisation.main([dirs['train'], f, '--report', report, '--png', str(tmp_path / 'never.png')])
        assert os.listdir(tmp_path / 'e') == [] and not os.path.exists(report) and not os.path.exists(str(tmp_path / 'never.png'))
