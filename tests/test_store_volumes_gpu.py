"""sg_store_volumes on the device against functional.store_volumes' numpy twin, bit for bit, statistics included:
every source and output type and both roundings, at shapes that reach the piece kernel (whole 16-byte loads and stores), its
misaligned head, the element kernel and the transposition of a channels-last source; edge values; a set on which a fused
multiply-add would differ; and one launch whose element count passes 2^31."""
import numpy as np
import pytest
import torch

from tests import svref

pytestmark = pytest.mark.gpu

# (n, c, d, h, w), what it reaches
SHAPES = [((3, 1, 3, 5, 7), 'element kernel: rows of 105 elements'),
          ((2, 1, 2, 33, 67), 'element kernel over several blocks: rows of 4422 elements'),
          ((2, 1, 4, 8, 16), 'piece kernel: rows of 512 elements'),
          ((3, 1, 16, 32, 32), 'piece kernel over several blocks'),
          ((2, 2, 3, 5, 8), 'two channels'),
          ((0, 1, 4, 8, 16), 'an empty batch')]


def F():
    from saragan_amd import functional
    return functional


def same(got, ref):
    got = [g.cpu() for g in got]
    assert got[0].dtype == ref[0].dtype and got[0].shape == ref[0].shape and got[0].is_contiguous()
    assert np.array_equal(got[0].numpy(), ref[0].numpy(), equal_nan=True), np.argwhere(got[0].numpy() != ref[0].numpy())[:4]
    assert np.array_equal(got[1].numpy(), ref[1].numpy()), (got[1], ref[1])


@pytest.mark.parametrize('rounding', ['trunc', 'rint'])
@pytest.mark.parametrize('out', ['i16', 'u16', 'u8', 'f32'])
@pytest.mark.parametrize('src', ['f32', 'bf16'])
def test_device_equals_the_numpy_twin(src, out, rounding):
    scale, shift, clip = svref.CONFIG[out]
    lo, hi = clip if clip else (0, 65535)
    kw = dict(scale=scale, shift=shift, clip=clip, rounding=rounding, stats=True)
    for seed, (shape, what) in enumerate(SHAPES):
        x = svref.make_input(src, shape, scale, shift, lo, hi, seed=seed)
        ref = F().store_volumes(x, svref.T_OUT[out], **kw)
        if shape[0]:
            assert ref[1][:, 4:].sum(0).gt(0).all(), what      # below, above and nan all occur
        same(F().store_volumes(x.cuda(), svref.T_OUT[out], **kw), ref)
        if shape[1] > 1:                                       # the same values in channels-last memory: transposed on the way
            cl = x.cuda().contiguous(memory_format=torch.channels_last_3d)
            assert not cl.is_contiguous()
            same(F().store_volumes(cl, svref.T_OUT[out], **kw), ref)


@pytest.mark.parametrize('out', ['i16', 'u8', 'f32'])
@pytest.mark.parametrize('src', ['f32', 'bf16', 'f16'])
def test_views_one_element_off_alignment(src, out):
    """Source and output both start one element behind a 16-byte boundary: the piece kernel with its head and tail.  Only the
    source does: no common head, the element kernel."""
    scale, shift, clip = svref.CONFIG[out]
    shape = (3, 1, 4, 8, 16)
    count = int(np.prod(shape))
    x = svref.make_input(src, shape, scale, shift, *clip, seed=9)
    kw = dict(scale=scale, shift=shift, clip=clip, rounding='rint', stats=True)
    ref = F().store_volumes(x, svref.T_OUT[out], **kw)
    xbuf = torch.zeros(count + 1, device='cuda', dtype=x.dtype)
    xbuf[1:] = x.reshape(-1).cuda()
    xv = xbuf[1:].view(shape)
    assert xv.data_ptr() % 16 == xv.element_size() and xv.is_contiguous()
    fill = 77
    obuf = torch.full((count + 2,), fill, device='cuda', dtype=svref.T_OUT[out])
    ov = obuf[1:-1].view(shape)
    got = F().store_volumes(xv, svref.T_OUT[out], out=ov, **kw)
    assert got[0] is ov
    same(got, ref)
    assert obuf[0].item() == fill and obuf[-1].item() == fill      # nothing written in front of the view or behind it
    same(F().store_volumes(xv, svref.T_OUT[out], **kw), ref)       # an aligned output: no common head


@pytest.mark.parametrize('src', ['f32', 'bf16'])
def test_exact_ties_and_bounds(src):
    """scale 1, shift 0: the ties k + 0.5, the bounds and their neighbours reach the kernel exactly as they are written."""
    vals = svref.edge_values(svref.T_SRC[src], 1.0, 0.0, -100, 100)
    x = vals.repeat(3 * 128 // vals.numel() + 1)[:3 * 128].reshape(3, 1, 2, 8, 8)
    for out, clip in (('i16', (-100, 100)), ('u8', (0, 100)), ('u16', (0, 100)), ('f32', (-100.0, 100.0)), ('f32', None)):
        for rounding in ('trunc', 'rint'):
            kw = dict(clip=clip, rounding=rounding, stats=True)
            ref = F().store_volumes(x, svref.T_OUT[out], **kw)
            same(F().store_volumes(x.cuda(), svref.T_OUT[out], **kw), ref)
    tr = F().store_volumes(x.cuda(), torch.int16, rounding='trunc').cpu().reshape(-1)
    ri = F().store_volumes(x.cuda(), torch.int16, rounding='rint').cpu().reshape(-1)
    t = x.float().reshape(-1)
    at = lambda v: int((t == v).nonzero()[0])      # noqa: E731
    assert [tr[at(v)].item() for v in (-2.5, -1.5, -0.5, 0.5, 1.5, 2.5)] == [-2, -1, 0, 0, 1, 2]
    assert [ri[at(v)].item() for v in (-2.5, -1.5, -0.5, 0.5, 1.5, 2.5)] == [-2, -2, 0, 0, 2, 2]


def test_two_rounded_operations_not_a_fused_one():
    x, scale, shift, two, fused = svref.fma_sensitive()
    assert (two != fused).any()                                  # (constructed and shown on the CPU: test_store_volumes_host.py)
    xt = torch.from_numpy(x).reshape(2, 1, 4, 16, 32)
    got = F().store_volumes(xt.cuda(), torch.float32, scale=scale, shift=shift).cpu().numpy().reshape(-1)
    assert np.array_equal(got, two)
    # where the two results straddle an integer the stored integer would move as well
    ref = F().store_volumes(xt, torch.int16, scale=scale, shift=shift, rounding='trunc', stats=True)
    same(F().store_volumes(xt.cuda(), torch.int16, scale=scale, shift=shift, rounding='trunc', stats=True), ref)
    odd = torch.from_numpy(x[:4095]).reshape(3, 1, 5, 7, 39).cuda()      # rows of 1365 elements: the element kernel
    assert np.array_equal(F().store_volumes(odd, torch.float32, scale=scale, shift=shift).cpu().numpy().reshape(-1), two[:4095])


def test_two_calls_give_identical_statistics():
    x = svref.make_input('bf16', (4, 1, 16, 64, 64), 1024.0, 1024.0, 0, 65535, seed=2).cuda()
    a = F().store_volumes(x, torch.uint16, scale=1024.0, shift=1024.0, stats=True)
    b = F().store_volumes(x, torch.uint16, scale=1024.0, shift=1024.0, stats=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert a[1][:, 4:].sum().item() > 0
    none = F().store_volumes(x, torch.uint16, scale=1024.0, shift=1024.0)      # without statistics: the same volumes
    assert torch.equal(none.view(torch.int16), a[0].view(torch.int16))


def test_more_than_2_to_31_elements():
    """Two rows of 2^30 + 2^20 bf16 elements to uint8: 2^31 + 2^21 in all, so the second row's offsets pass 2^31.  Each row repeats a
    period of 2^20 elements made on the device 1025 times: its sums and counts are 1025 times the period's."""
    period, reps = 1 << 20, 1025
    scale, shift, clip = svref.CONFIG['u8']
    g = torch.Generator(device='cuda').manual_seed(11)
    base = torch.randn(2, period, device='cuda', generator=g) * 1.4
    base[:, ::4099] = float('nan')
    base[:, 5::8191] = float('inf')
    base = base.to(torch.bfloat16)
    x = torch.empty(2, reps, period, device='cuda', dtype=torch.bfloat16)
    x.copy_(base[:, None, :])
    x = x.view(2, 1, reps, 1024, 1024)
    assert x.numel() > 2 ** 31
    kw = dict(scale=scale, shift=shift, clip=clip, rounding='rint', stats=True)
    out, st = F().store_volumes(x, torch.uint8, **kw)
    ref, rst = F().store_volumes(base.cpu().view(2, 1, 1, 1024, 1024), torch.uint8, **kw)
    row = out.view(2, -1)[1]
    assert torch.equal(row[:period].cpu(), ref[1].reshape(-1)) and torch.equal(row[-period:].cpu(), ref[1].reshape(-1))
    assert torch.equal(out.view(2, -1)[0][-period:].cpu(), ref[0].reshape(-1))
    want = rst.clone()
    want[:, [0, 1, 4, 5, 6]] *= reps
    assert torch.equal(st.cpu(), want), (st, want)
    assert (want[:, 4:] > 0).all() and not torch.equal(want[0], want[1])
