"""GPU tests of the device-resident dataset: sg_gather_rows against numpy with no tolerance on both of its
kernels, its 64-bit row offsets at the smallest table where 32-bit ones fail, its guards; ResidentLoader against
PinnedPrefetcher on the device; and the training loop with and without --device_dataset_gib, bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NP_DTYPES = {'u8': np.uint8, 'i8': np.int8, 'i16': np.int16, 'u16': np.uint16, 'f16': np.float16, 'f32': np.float32}
ROW_ELEMS = [1, 16, 105, 1024, 1031]      # 16 / 1024: the 16-byte kernel; 1, 105, 1031: rows or base off 16 bytes, the element kernel
ROWS = 9
INDICES = {1: [3], 5: [7, 2, 8, 2, 0]}    # out of order, one duplicate


def _values(dtype, shape, seed):
    rng = np.random.default_rng(seed)
    dtype = np.dtype(dtype)
    if dtype.kind in 'iu':
        info = np.iinfo(dtype)
        return rng.integers(info.min, info.max + 1, shape).astype(dtype)
    return (rng.normal(0, 1, shape) * 10.0 ** rng.integers(-3, 4, shape)).astype(dtype)


def _host(table, idx, norm):
    """The prefetcher's arithmetic: convert, then np.subtract and np.divide with np.float32 scalars, in place."""
    out = np.empty((len(idx),) + table.shape[1:], dtype=np.float32)
    np.copyto(out, table[idx], casting='unsafe')
    if norm is not None:
        np.subtract(out, np.float32(norm[0]), out=out)
        np.divide(out, np.float32(norm[1]), out=out)
    return out


@pytest.mark.parametrize('norm', [None, (1024, 1024), (0.3, 7)], ids=['raw', 'pow2', 'inexact'])
@pytest.mark.parametrize('name', list(NP_DTYPES))
def test_gather_rows_equals_numpy_bit_for_bit(name, norm):
    from saragan_amd import functional as F
    mean, std = norm if norm is not None else (None, None)
    for row_elems in ROW_ELEMS:
        alloc = _values(NP_DTYPES[name], (ROWS + 1, row_elems), 17 * row_elems)
        table = torch.from_numpy(alloc).cuda()[1:]      # one row into its allocation: the base is misaligned for 105 and 1031
        assert table.is_contiguous() and table.data_ptr() % 16 == (row_elems * alloc.itemsize) % 16
        for n, idx in INDICES.items():
            want = torch.from_numpy(_host(alloc[1:], idx, norm))
            got = F.gather_rows(table, idx, mean, std)                                                   # host positions
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, row_elems)
            assert torch.equal(got.cpu(), want), (name, row_elems, n, norm)
            dev = torch.tensor(idx, dtype=torch.int32, device='cuda')                                   # device positions, out=
            out = torch.full((n, row_elems), -1.0, device='cuda')
            assert F.gather_rows(table, dev, mean, std, out=out) is out
            assert torch.equal(out.cpu(), want), (name, row_elems, n, norm)


def test_row_offsets_are_64_bit():
    """u8 [2^20 + 8, 4096]: 4 GiB + 32 KiB, never filled; the last 8 rows start past 2^32 bytes."""
    from saragan_amd import functional as F
    rows, row_elems = (1 << 20) + 8, 4096
    table = torch.empty((rows, row_elems), dtype=torch.uint8, device='cuda')
    last = _values(np.uint8, (8, row_elems), 5)
    table[rows - 8:] = torch.from_numpy(last).cuda()
    order = [5, 0, 7, 2, 6, 1, 4, 3]
    got = F.gather_rows(table, [rows - 8 + k for k in order])
    assert torch.equal(got.cpu(), torch.from_numpy(last[order].astype(np.float32)))
    del table, got
    torch.cuda.empty_cache()


def _raw(table_ptr, sdt, rows, row_elems, idx, n, out, norm=0, mean=0.0, std=1.0):
    from saragan_amd import _lib
    return _lib.load().sg_gather_rows(C.c_void_p(table_ptr), sdt, rows, row_elems, C.c_void_p(idx.data_ptr()), n,
                                      C.c_void_p(out.data_ptr()), norm, mean, std,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize('row_elems', [16, 105], ids=['vector', 'element'])
def test_an_index_outside_the_table_gives_nan_rows(row_elems):
    from saragan_amd import _lib
    table = torch.from_numpy(_values(np.int16, (ROWS, row_elems), 1)).cuda()
    idx = torch.tensor([-1, ROWS, 4], dtype=torch.int32, device='cuda')
    out = torch.zeros((3, row_elems), device='cuda')
    assert _raw(table.data_ptr(), _lib.SG_SRC_I16, ROWS, row_elems, idx, 3, out, 1, 1024.0, 1024.0) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out[:2]).all()
    assert torch.equal(out[2].cpu(), torch.from_numpy(_host(table.cpu().numpy(), [4], (1024, 1024))[0]))


def test_bad_host_arguments_return_a_status():
    from saragan_amd import _lib
    table = torch.zeros((4, 16), dtype=torch.int16, device='cuda')
    idx = torch.zeros(2, dtype=torch.int32, device='cuda')
    out = torch.zeros((2, 16), device='cuda')
    assert _raw(table.data_ptr(), _lib.SG_SRC_I16, 4, 16, idx, 2, out) == 0
    assert _raw(0, _lib.SG_SRC_I16, 4, 16, idx, 2, out) != 0              # null table
    assert _raw(table.data_ptr(), _lib.SG_SRC_I16, 4, 16, idx, -1, out) != 0
    assert _raw(table.data_ptr(), 6, 4, 16, idx, 2, out) != 0             # unknown dtype codes
    assert _raw(table.data_ptr(), -1, 4, 16, idx, 2, out) != 0
    assert _raw(table.data_ptr(), _lib.SG_SRC_I16, 4, 0, idx, 2, out) != 0
    torch.cuda.synchronize()


def _files(d, nfiles=12, shape=(4, 16, 16)):
    d.mkdir(parents=True)
    for i in range(nfiles):
        np.save(d / f'{i:04d}.npy', _values(np.int16, shape, 50 + i))
    return str(d) + '/'


def _dataset(path, **kw):
    from saragan_amd.dataset import NumpyPathDataset
    ds = NumpyPathDataset(path, None, False, True, seed=6, **kw)
    return ds.set_labels(np.arange(len(ds) * 3, dtype=np.float32).reshape(len(ds), 3) / 7)


def test_resident_loader_equals_the_prefetcher_on_the_device(tmp_path):
    from saragan_amd.dataset import PinnedPrefetcher, ResidentLoader
    path = _files(tmp_path / '16x16')
    res = ResidentLoader(_dataset(path, rank=1, world_size=2), 4, True, 1024, 1024, 'cuda:0')
    pin = PinnedPrefetcher(_dataset(path, rank=1, world_size=2), 4, True, 1024, 1024, 'cuda:0')
    try:
        assert res.table.volumes.dtype == torch.int16 and res.table.volumes.is_cuda
        for _ in range(6):
            x, y = res.next(), pin.next()
            assert x.is_cuda and tuple(x.shape) == (4, 1, 4, 16, 16)
            assert torch.equal(x, y) and torch.equal(res.labels, pin.labels)
    finally:
        pin.close()
        res.close()


def test_a_batch_stays_valid_until_the_call_after_the_next(tmp_path):
    from saragan_amd.dataset import ResidentLoader
    res = ResidentLoader(_dataset(_files(tmp_path / '16x16')), 4, False, 1024, 1024, 'cuda:0')
    try:
        held = []                                                         # (tensor, labels, clones taken at the call)
        for k in range(8):
            x = res.next()
            held.append((x, res.labels, x.clone(), res.labels.clone()))
            if k:                                                         # call k - 1's tensors across call k
                px, pl, cx, cl = held[k - 1]
                assert torch.equal(px, cx) and torch.equal(pl, cl)
        assert any(not torch.equal(h[0], h[2]) for h in held[:-2])        # (the ring does come round: buffers are reused)
    finally:
        res.close()


# ---- the training loop: the data and arguments of tests/test_train_gpu.py -------------------------------------------------------
def _args(data, logdir, **kw):
    from saragan_amd.main import build_parser, finalize_args
    argv = ['pgan', str(data) + '/', '--start_shape', '(1, 1, 4, 4)', '--final_shape', '(1, 4, 16, 16)',
            '--starting_phase', '1', '--ending_phase', '2', '--base_batch_size', '4', '--latent_dim', '16',
            '--noise_stddev', '0.01', '--mixing_nimg', '16', '--stabilizing_nimg', '16', '--loss_fn', 'wgan',
            '--gp_weight', '10', '--data_mean', '1024', '--data_stddev', '1024', '--logdir', str(logdir),
            '--g_lr', '1e-3', '--d_lr', '1e-3', '--checkpoint_every_nsteps', '1000000', '--dtype', 'f32']
    args, _ = build_parser().parse_known_args(argv)
    args.kernel_spec = [[[1, 3, 3], [1, 3, 3]], [[1, 3, 3], [3, 3, 3]], [[3, 3, 3], [3, 3, 3]]]
    args.filter_spec = [[16, 16], [16, 8], [8, 8]]
    for k, v in kw.items():
        setattr(args, k, v)
    return finalize_args(args)


def _make_data(root):
    for ph, (z, xy) in enumerate([(1, 4), (2, 8), (4, 16)], 1):
        d = root / f'{xy}x{xy}'
        d.mkdir(parents=True)
        for i in range(12):
            rng = np.random.default_rng(1234 + i)
            v = np.clip(rng.normal(1024, 512, (z, xy, xy)), 0, 4095).astype(np.int16)
            np.save(d / f'{i:04d}.npy', v)


def _train(data, logdir, gib, monkeypatch):
    """Phases 1-2, three steps each, in the reproducible mode -> (losses per phase, final variables, loader types per phase)."""
    import saragan_amd
    import saragan_amd.train as T
    made = []
    make = T.make_loader

    def recording(*a, **kw):
        made.append(make(*a, **kw))
        return made[-1]

    monkeypatch.setattr(T, 'make_loader', recording)
    saragan_amd.set_deterministic(True)
    try:
        out = T.run_training(_args(data, logdir, device_dataset_gib=gib), max_steps_per_phase=3)
    finally:
        saragan_amd.set_deterministic(False)
    losses = [(out['stats'][p]['d_loss'], out['stats'][p]['g_loss']) for p in (1, 2)]
    variables = {k: v.detach().cpu().numpy() for k, v in out['store'].vars.items()}
    return losses, variables, [type(m).__name__ for m in made]


@pytest.fixture(scope='module')
def streamed_run(tmp_path_factory):
    root = tmp_path_factory.mktemp('device_dataset')
    _make_data(root / 'data')
    with pytest.MonkeyPatch.context() as mp:
        losses, variables, kinds = _train(root / 'data', root / 'log0', 0, mp)
    assert kinds == ['PinnedPrefetcher'] * 2 and np.isfinite(losses).all()
    return root, losses, variables


@pytest.mark.parametrize('gib,kind', [(1, 'ResidentLoader'), (1e-9, 'PinnedPrefetcher')], ids=['resident', 'over_budget'])
def test_training_is_identical_with_the_resident_table(streamed_run, monkeypatch, gib, kind):
    root, losses0, variables0 = streamed_run
    losses, variables, kinds = _train(root / 'data', root / f'log_{kind}', gib, monkeypatch)
    assert kinds == [kind] * 2
    assert losses == losses0
    assert set(variables) == set(variables0)
    for k, v in variables0.items():
        np.testing.assert_array_equal(variables[k], v, err_msg=k)
