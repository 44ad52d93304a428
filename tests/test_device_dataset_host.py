"""Host logic of the device-resident dataset, on CPU buffers: the position draws behind batch_paths /
batch_mpi_paths, ResidentLoader against PinnedPrefetcher bit for bit (functional.gather_rows' numpy path performs the prefetcher's
two f32 operations in its order), make_loader's choice and its notice, DeviceTable's accounting and its refusals."""
import numpy as np
import pytest
import torch

FILE_DTYPES = ['uint8', 'int16', 'uint16', 'float16', 'float32', 'float64']


def _volume(dtype, seed, shape=(3, 5, 7)):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind in 'iu':
        info = np.iinfo(dtype)
        return rng.integers(info.min, min(info.max, 4095) + 1, shape).astype(dtype)
    return rng.normal(1024, 512, shape).astype(dtype)


def _make_table(d, dtype, nfiles=12, fortran=3, shape=(3, 5, 7)):
    d.mkdir(parents=True)
    for i in range(nfiles):
        v = _volume(dtype, 100 + i, shape)
        np.save(d / f'{i:04d}.npy', np.asfortranarray(v) if i == fortran else v)
    return str(d) + '/'


def _dataset(path, seed, labels=False, **kw):
    from saragan_amd.dataset import NumpyPathDataset
    ds = NumpyPathDataset(path, None, False, True, seed=seed, **kw)
    if labels:
        ds.set_labels(np.arange(len(ds) * 3, dtype=np.float32).reshape(len(ds), 3) / 7)
    return ds


@pytest.mark.parametrize('seed', [0, 3])
def test_positions_name_the_files_batch_paths_draws(tmp_path, seed):
    path = _make_table(tmp_path / '8x8', 'int16', nfiles=10)
    a, b = _dataset(path, seed, labels=True), _dataset(path, seed, labels=True)
    for _ in range(9):                                       # 9 x 3 of 10 files: two refills
        pos, paths = a.batch_positions(3), b.batch_paths(3)
        assert [a.scratch_files[i] for i in pos] == paths
        assert np.array_equal(a.last_labels, b.last_labels) and np.array_equal(a.last_labels, a.labels[pos])
    for rank in (0, 1):                                      # the _mpi_ pair: column `rank` of the global draw
        a, b = (_dataset(path, seed, labels=True, rank=rank, world_size=2) for _ in range(2))
        for _ in range(6):                                   # 6 x (2 x 2) of 10
            pos, paths = a.batch_mpi_positions(2), b.batch_mpi_paths(2)
            assert len(pos) == 2 and [a.scratch_files[i] for i in pos] == paths
            assert np.array_equal(a.last_labels, b.last_labels)
    small = _make_table(tmp_path / '4x4', 'int16', nfiles=5)
    a, b = _dataset(small, seed), _dataset(small, seed)
    twice = 0
    for _ in range(4):                                       # a batch larger than the table: a file may come twice in one batch
        pos, paths = a.batch_positions(8), b.batch_paths(8)
        assert len(pos) == 8 and [a.scratch_files[i] for i in pos] == paths
        twice += len(set(pos)) < len(pos)
    assert twice == 4                                        # 8 draws of 5 files


@pytest.mark.parametrize('norm', [None, (1024, 1024)], ids=['raw', 'normalised'])
@pytest.mark.parametrize('dtype', FILE_DTYPES)
def test_resident_loader_equals_the_prefetcher_bit_for_bit(tmp_path, dtype, norm):
    from saragan_amd.dataset import PinnedPrefetcher, ResidentLoader
    path = _make_table(tmp_path / 'vol', dtype)              # 12 files, file 3 Fortran-ordered
    mean, std = norm if norm else (None, None)
    a, b = _dataset(path, 4, labels=True), _dataset(path, 4, labels=True)
    res = ResidentLoader(a, 4, False, mean, std, device='cpu')
    want_dtype = dtype if dtype != 'float64' else 'float32'  # the file's own dtype; others are converted once, at load
    assert res.table.volumes.dtype == getattr(torch, want_dtype) and tuple(res.table.volumes.shape) == (12, 1, 3, 5, 7)
    pin = PinnedPrefetcher(b, 4, False, mean, std, device='cpu')
    try:
        for _ in range(10):
            x, y = res.next(), pin.next()
            assert x.dtype == torch.float32 and tuple(x.shape) == (4, 1, 3, 5, 7)
            assert np.array_equal(x.numpy(), y.numpy())
            assert np.array_equal(res.labels.numpy(), pin.labels.numpy())
    finally:
        pin.close()
        res.close()


def test_make_loader_choices(tmp_path, capsys):
    from saragan_amd.dataset import DeviceTable, PinnedPrefetcher, ResidentLoader, make_loader
    path = _make_table(tmp_path / 'vol', 'int16')
    need = DeviceTable.estimate_bytes(_dataset(path, 0))
    capsys.readouterr()
    off = make_loader(_dataset(path, 0), 4, False, 1024, 1024, 'cpu', 0)
    assert type(off) is PinnedPrefetcher and 'device dataset' not in capsys.readouterr().out      # today's behaviour, silently
    off.close()
    small = make_loader(_dataset(path, 0), 4, False, 1024, 1024, 'cpu', (need - 1) / 2 ** 30)
    out = capsys.readouterr().out
    assert type(small) is PinnedPrefetcher
    notice = [ln for ln in out.splitlines() if 'device dataset' in ln]
    assert len(notice) == 1 and str(need) in notice[0] and str(need - 1) in notice[0]             # one line, both figures
    small.close()
    fits = make_loader(_dataset(path, 0), 4, False, 1024, 1024, 'cpu', (need + 1) / 2 ** 30)
    assert type(fits) is ResidentLoader and 'device dataset' not in capsys.readouterr().out
    assert fits.table.nbytes == need
    fits.close()


def test_estimate_bytes_is_files_times_volume_plus_labels(tmp_path):
    from saragan_amd.dataset import DeviceTable
    ds = _dataset(_make_table(tmp_path / 'a', 'int16'), 0)
    assert DeviceTable.estimate_bytes(ds) == 12 * (3 * 5 * 7) * 2
    ds = _dataset(_make_table(tmp_path / 'b', 'uint8', nfiles=7), 0, labels=True)
    assert DeviceTable.estimate_bytes(ds) == 7 * 105 * 1 + 7 * 3 * 4
    assert DeviceTable(ds, 'cpu').nbytes == DeviceTable.estimate_bytes(ds)
    ds = _dataset(_make_table(tmp_path / 'c', 'float64', nfiles=4), 0)                            # held as f32
    assert DeviceTable.estimate_bytes(ds) == 4 * 105 * 4


@pytest.mark.parametrize('what', ['shape', 'dtype'])
def test_a_mismatched_file_is_named(tmp_path, what):
    from saragan_amd.dataset import DeviceTable
    path = _make_table(tmp_path / 'vol', 'int16', nfiles=6)
    odd = _volume('int16', 1, (3, 5, 8)) if what == 'shape' else _volume('uint16', 1)
    np.save(tmp_path / 'vol' / '0004.npy', odd)
    with pytest.raises(ValueError, match='0004.npy'):
        DeviceTable(_dataset(path, 0), 'cpu')


def test_a_position_outside_the_table_is_refused_on_the_host():
    from saragan_amd import functional as F
    table = torch.from_numpy(_volume('int16', 0, (5, 4)))
    assert np.array_equal(F.gather_rows(table, [4, 0, 4]).numpy(), table.numpy()[[4, 0, 4]].astype(np.float32))
    for bad in ([0, 5], [-1], np.array([2, 7]), torch.tensor([1, -3])):
        with pytest.raises(ValueError, match='outside the table'):
            F.gather_rows(table, bad)
    with pytest.raises(ValueError):
        F.gather_rows(table, [0], mean=1.0)
