"""sg_multiscale_residual against the CPU path, bit for bit: the loss, the per-level terms and the gradient.  The CPU
path itself is pinned to an independent float64 statement in tests/test_project_host.py.  NaNs (a position outside the table) are
compared as NaNs, whatever their payload."""
import numpy as np
import pytest
import torch

from tests import projref as R

pytestmark = pytest.mark.gpu

SHAPES = [((1, 4, 8, 8), 3, 3),            # one cube per sample
          ((1, 2, 6, 10), 2, 2),           # cube counts that are no powers of two, ragged edge-8 cubes
          ((1, 8, 16, 48), 4, 2),          # several cubes per sample, the aligned path
          ((1, 3, 5, 7), 1, 3),            # the element path
          ((2, 4, 8, 8), 2, 2),            # two channels
          ((1, 16, 24, 136), 4, 2)]        # more than one strip of eight cubes along w, more than one block
LAM = [1.0, 0.7, 1.3, 0.9]


def F():
    from saragan_amd import functional
    return functional


def same(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.dtype in (torch.bfloat16, torch.float16):
        a, b = a.float(), b.float()      # (exact)
    return a.shape == b.shape and np.array_equal(a.numpy(), b.numpy(), equal_nan=True)


def check(y, table, pos, mean, stddev, levels, lam, idx=None):
    want = F().multiscale_residual_raw(y, table, pos, mean, stddev, levels, lam)
    got = F().multiscale_residual_raw(y.cuda(), table.cuda(), pos if idx is None else idx, mean, stddev, levels, lam)
    for name, a, b in zip(('loss', 'terms', 'grad'), got, want):
        assert a.dtype == b.dtype and same(a, b), name
    assert got[2].stride() == y.stride()
    return got


# (with one channel channels_last_3d is the same memory as NCDHW: the two-channel shape takes both formats)
@pytest.mark.parametrize('shape,levels,n,channels_last', [s + (False,) for s in SHAPES] + [((2, 4, 8, 8), 2, 2, True), ((3, 3, 5, 7), 1, 2, True)])
def test_shapes_bit_for_bit(shape, levels, n, channels_last):
    y = R.make_y(n, shape, torch.bfloat16, 1, channels_last=channels_last)
    table = R.make_table(4, shape, torch.int16, 1)
    check(y, table, np.arange(n) % 4, 1000.0, 500.0, levels, LAM[:levels])


def test_the_library_agrees_on_its_limit():
    from saragan_amd import _lib
    assert _lib.load().sg_multiscale_residual_max_levels() == _lib.SG_MSR_DEVICE_LEVELS
    y, table = R.make_y(1, (1, 16, 16, 16), torch.float32, 0).cuda(), R.make_table(1, (1, 16, 16, 16), torch.uint8, 0).cuda()
    with pytest.raises(ValueError, match='levels <= 4 on the device'):
        F().multiscale_residual_raw(y, table, [0], levels=5)


def test_empty_batch():
    y, table = R.make_y(0, (1, 4, 8, 8), torch.float32, 0).cuda(), R.make_table(2, (1, 4, 8, 8), torch.int16, 0).cuda()
    loss, terms, grad = F().multiscale_residual_raw(y, table, [], levels=3)
    assert loss.shape == (0,) and terms.shape == (0, 3) and grad.shape == y.shape


@pytest.mark.parametrize('tdt', R.TABLE_DTYPES)
@pytest.mark.parametrize('ydt', R.Y_DTYPES)
def test_every_type_pair(tdt, ydt):
    shape = (1, 4, 8, 8)
    check(R.make_y(3, shape, ydt, 2), R.make_table(4, shape, tdt, 2), [3, 0, 2], 3.0, 2.0, 3, LAM[:3])


def test_repeated_descending_and_outside_positions():
    shape = (1, 4, 8, 8)
    y, table = R.make_y(6, shape, torch.float16, 3), R.make_table(4, shape, torch.uint16, 3)
    pos = np.array([3, 3, 2, 0, 4, -1])
    idx = torch.tensor(pos, dtype=torch.int32, device='cuda')
    loss, terms, grad = check(y, table, pos, 100.0, 50.0, 3, LAM[:3], idx=idx)
    assert torch.isnan(loss[4:]).all() and torch.isnan(terms[4:]).all() and torch.isnan(grad[4:].float()).all()
    assert torch.isfinite(loss[:4]).all() and torch.isfinite(grad[:4].float()).all()


@pytest.mark.parametrize('ydt,tdt', [(torch.bfloat16, torch.int16), (torch.float32, torch.uint8), (torch.float16, torch.float32)])
def test_views_one_element_past_a_boundary_and_guards(ydt, tdt):
    shape, n, levels = (1, 8, 16, 48), 2, 4
    y, table = R.make_y(n, shape, ydt, 4), R.make_table(2, shape, tdt, 4)
    want = F().multiscale_residual_raw(y, table, [1, 0], 3.0, 2.0, levels, LAM)

    def shifted(t, by, fill):
        buf = torch.full((t.numel() + 16,), fill, dtype=t.dtype, device='cuda')
        view = buf[by:by + t.numel()].view(t.shape)
        view.copy_(t)
        return buf, view

    for by_y, by_t, by_g in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (0, 0, 0)):
        _, yv = shifted(y, by_y, 7)
        _, tv = shifted(table, by_t, 7)
        gbuf, gv = shifted(torch.zeros_like(y), by_g, 7)
        got = F().multiscale_residual_raw(yv, tv, [1, 0], 3.0, 2.0, levels, LAM, out=gv)
        assert got[2].data_ptr() == gv.data_ptr()
        for a, b in zip(got, want):
            assert same(a, b), (by_y, by_t, by_g)
        guard = torch.cat([gbuf[:by_g], gbuf[by_g + y.numel():]]).float()
        assert (guard == 7).all(), (by_y, by_t, by_g)


def test_values_on_which_a_fused_multiply_add_would_differ():
    """Level 0's squares are exact in f64 (24 x 24 bits); from level 1 on m * m, and every k * m of the gradient, has more than 53
    bits, so a product fused into the following sum keeps bits the definition rounds away.  Values with full mantissas (float32
    targets, odd weights, a count that is no power of two) make nearly every such pair differ; the numpy twin never fuses."""
    shape = (3, 4, 12, 20)
    y, table = R.make_y(2, shape, torch.float32, 9), R.make_table(3, shape, torch.float32, 9)
    rng = np.random.default_rng(9)
    y = y * torch.from_numpy(rng.uniform(0.5, 1.5, y.shape).astype(np.float32))
    check(y, table, [2, 1], 0.37, 1.7, 3, [0.9, 1.1, 1.3])
    check(y.contiguous(memory_format=torch.channels_last_3d), table, [2, 1], 0.37, 1.7, 3, [0.9, 1.1, 1.3])


def test_two_calls_give_the_same_bits():
    shape = (1, 16, 24, 136)
    y, table = R.make_y(3, shape, torch.bfloat16, 5).cuda(), R.make_table(3, shape, torch.int16, 5).cuda()
    idx = torch.tensor([2, 2, 0], dtype=torch.int32, device='cuda')
    a = F().multiscale_residual_raw(y, table, idx, 1000.0, 500.0, 4, LAM)
    b = F().multiscale_residual_raw(y, table, idx, 1000.0, 500.0, 4, LAM)
    assert all(same(p, q) for p, q in zip(a, b))


def test_backward_delivers_the_same_gradient():
    shape = (1, 8, 16, 48)
    y, table = R.make_y(2, shape, torch.bfloat16, 6).cuda(), R.make_table(2, shape, torch.int16, 6).cuda()
    _, _, grad = F().multiscale_residual_raw(y, table, [0, 1], 1000.0, 500.0, 4, LAM)
    yg = y.clone().requires_grad_(True)
    loss, terms = F().multiscale_residual(yg, table, [0, 1], 1000.0, 500.0, 4, LAM)
    loss.sum().backward()
    assert torch.equal(yg.grad, grad) and not terms.requires_grad


def test_one_launch_past_two_to_the_31_elements():
    """bf16 y, u8 targets, levels 1, 17 samples of 2^27 voxels that share ONE target row: y = t + k_i, so r = k_i everywhere, every
    partial sum is an integer below 2^53, loss_i = terms_i = k_i^2 and every gradient element is bf16(2 k_i / 2^27), in closed form."""
    n, shape = 17, (1, 32, 2048, 2048)
    vox = int(np.prod(shape))
    assert n * vox > 2 ** 31
    need = n * vox * 2 * 2 + vox * 5 + n * (vox // 512) * 8 + (1 << 30)      # y, grad; the target and its f32 image; workspace; slack
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    gen = torch.Generator(device='cuda').manual_seed(3)
    table = torch.randint(0, 101, (1,) + shape, dtype=torch.uint8, device='cuda', generator=gen)
    k = torch.arange(n, dtype=torch.float32) - 3      # -3 .. 13: t + k stays an integer below 256, exact in bf16
    y = torch.empty((n,) + shape, dtype=torch.bfloat16, device='cuda')
    t = table[0].float()
    for i in range(n):
        y[i] = (t + k[i].item()).to(torch.bfloat16)
    del t
    idx = torch.zeros(n, dtype=torch.int32, device='cuda')
    loss, terms, grad = F().multiscale_residual_raw(y, table, idx, 0.0, 1.0, 1, [1.0])
    assert torch.equal(loss.cpu(), k * k) and torch.equal(terms.cpu()[:, 0], (k * k).double())
    want = (2.0 * k.double() / vox).to(torch.bfloat16)      # (2 k / 2^27 has few bits: exact)
    assert torch.equal(want.double(), 2.0 * k.double() / vox)
    for i in range(n):
        assert bool((grad[i] == want[i].item()).all()), i
