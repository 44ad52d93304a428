"""tests/wgref.py on the CPU: the shifted-slice fp64 weight gradient equals torch's fp64 autograd of conv3d bit for bit on
integer data (both are exact there), masked_dy decodes the sign words as the C ABI documents them, and the exactness range
check refuses a case whose sums could pass 2^24."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import wgref as R

CASES = [
    # n, cin, cout, (d, h, w), kernel, ups
    (2, 5, 7, (4, 5, 6), (3, 3, 3), False),
    (1, 8, 3, (3, 7, 5), (1, 3, 3), False),      # ragged extents
    (3, 4, 6, (2, 3, 9), (1, 1, 1), False),
    (2, 3, 4, (5, 5, 5), (5, 5, 5), False),
    (1, 2, 3, (3, 5, 6), (3, 1, 1), False),
    (1, 2, 3, (3, 5, 6), (1, 1, 3), False),
    (1, 2, 2, (2, 3, 4), (7, 7, 7), False),      # taps that only ever meet padding
    (2, 6, 5, (4, 6, 2), (3, 3, 3), True),       # x at half resolution
    (1, 3, 3, (2, 2, 8), (1, 3, 3), True),
]


@pytest.mark.parametrize('case', CASES, ids=[f'{c[1]}to{c[2]}at{"x".join(map(str, c[3]))}k{"".join(map(str, c[4]))}{"ups" if c[5] else ""}' for c in CASES])
def test_wgrad_ref_equals_fp64_autograd_bit_for_bit(case):
    n, cin, cout, sp, k, ups = case
    xs = tuple(v // 2 for v in sp) if ups else sp
    x = R.int_data((n, cin, *xs), 11, torch.float64)
    dy = R.int_data((n, cout, *sp), 12, torch.float64)
    assert x.permute(0, 2, 3, 4, 1).is_contiguous() and float(x.abs().max()) == 3 and torch.equal(x, x.round())
    w = torch.zeros((cout, cin, *k), dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = TF.conv3d(R.up2(x) if ups else x, w, b, padding=tuple(v // 2 for v in k))
    gw, gb = torch.autograd.grad(y, [w, b], dy)
    dw, db = R.wgrad_ref(x, dy, k, ups=ups)
    assert dw.dtype == torch.float64 and dw.shape == (*k, cin, cout)
    assert torch.equal(dw, gw.permute(2, 3, 4, 1, 0))
    assert torch.equal(db, gb)
    # and an f32 running sum of the products in a shuffled order is that same integer: the claim the GPU tests rest on
    R.assert_exact_range(9, 1, n * sp[0] * sp[1] * sp[2])
    xf = (R.up2(x) if ups else x).permute(0, 2, 3, 4, 1).reshape(-1, cin)
    centre = (dw[k[0] // 2, k[1] // 2, k[2] // 2, 0, 0], xf[:, 0] * dy.permute(0, 2, 3, 4, 1).reshape(-1, cout)[:, 0])
    prod = centre[1].numpy().astype(np.float32)
    np.random.default_rng(3).shuffle(prod)
    acc = np.float32(0)
    for p in prod:
        acc = np.float32(acc + p)
    assert float(acc) == float(centre[0])


def test_masked_dy_on_a_hand_written_example():
    # fine tensor 1 x 33 channels x 2 x 2 x 2: two sign words per voxel; dy_half is one voxel
    n, c, sp = 1, 33, (2, 2, 2)
    dy_half = torch.arange(1, c + 1, dtype=torch.float64).view(1, c, 1, 1, 1)
    words = torch.zeros((8, 2), dtype=torch.int32)
    words[0, 0] = 0b101            # voxel (0,0,0): channels 0 and 2
    words[3, 0] = -2 ** 31         # voxel (0,1,1): channel 31 (the word's sign bit)
    words[5, 1] = 1                # voxel (1,0,1): channel 32, the second word
    words[7, 1] = 2                # a bit beyond the channel count: ignored
    got = R.masked_dy(dy_half, words, 0.25, 0.125, (n, c, *sp))
    want = 0.125 * dy_half.expand(1, c, 2, 2, 2).clone()
    want[0, 0, 0, 0, 0] *= 0.25
    want[0, 2, 0, 0, 0] *= 0.25
    want[0, 31, 0, 1, 1] *= 0.25
    want[0, 32, 1, 0, 1] *= 0.25
    assert torch.equal(got, want)
    assert int(R.mask_bits(words, n, c, sp).sum()) == 4


def test_exact_range_refuses_a_case_that_is_too_large():
    R.assert_exact_range(9, 1, 2 * 4 * 128 * 128)            # 1.2 M against 16.8 M
    R.assert_exact_range(9 * 0.125, 0.125 * 0.25, 466_000)   # the masked gather: 36 units per term
    with pytest.raises(AssertionError):
        R.assert_exact_range(9, 1, 2 ** 24 // 9 + 1)
    with pytest.raises(AssertionError):
        R.assert_exact_range(9 * 0.125, 0.125 * 0.25, 467_000)


def test_scaled_is_one_f32_rounding_and_one_add():
    s = torch.tensor([3.0, -5461.0, 1234567.0], dtype=torch.float64)
    got = R.scaled(s, 0.37)
    want = [np.float32(0.37) * np.float32(v) for v in s.tolist()]
    assert got.dtype == torch.float32 and got.tolist() == [float(v) for v in want]
    pre = torch.tensor([1.0, 2.0, -7.0])
    acc = R.scaled(s, 0.37, prefill=pre)
    assert acc.tolist() == [float(np.float32(p) + v) for p, v in zip(pre.tolist(), want)]
    with pytest.raises(AssertionError):
        R.scaled(torch.tensor([2.0 ** 24 + 1], dtype=torch.float64), 0.25)
