"""Helpers shared by tests/test_wgrad_exact_gpu.py and tests/test_wgref_host.py: integer-valued inputs for which every f32
sum of the weight-gradient kernels (csrc/wgrad.hip, csrc/small.hip, csrc/subpix.hip) is exact, and a plain fp64 restatement
(torch / numpy) of the weight and bias gradient they compute.

Why integers: the kernels multiply bf16 / f32 inputs and add the products in f32 (MFMA, FMA, atomics, slabs).  With x and dy
integers in [-3, 3] every product and every partial sum is an integer below 9 * (terms per sum); while that stays below
2^24 nothing is rounded anywhere, so the finished sum has the same bits in ANY order of accumulation and an fp64 reference
is the exact value: the comparison is torch.equal, and one lost, doubled or misplaced term changes the integer.
assert_exact_range() makes the 2^24 condition a checked one per case.  Nothing here touches the GPU."""
import numpy as np
import torch

LIMIT = 2 ** 24      # integers up to here are exact in f32


def int_data(shape, seed, dtype, lo=-3, hi=3):
    """Integers in [lo, hi] as a `dtype` tensor on the CPU; 5-D shapes (NCDHW) are NDHWC-contiguous, as cl() makes them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int32).to(dtype)
    return x.contiguous(memory_format=torch.channels_last_3d) if x.dim() == 5 else x.contiguous()


def assert_exact_range(max_term, unit, terms):
    """Every term of a sum is a multiple of `unit` no larger than max_term, and there are `terms` of them: the sum and all
    of its partial sums, in units, stay below 2^24, so f32 addition is exact in any order."""
    assert max_term / unit * terms < LIMIT, (f'{terms} terms of up to {max_term} in units of {unit}: partial sums may pass 2^24, '
                                             f'the case is too large to be exact in f32')


def up2(t):
    """Nearest x2 of an NCDHW tensor (upscale3d, networks/ops.py:265-273)."""
    return t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)


def wgrad_ref(x, dy, k, ups=False):
    """dw[kd,kh,kw,cin,cout] = sum_v x[v + tap - pad] (x) dy[v] and db[cout] = sum_v dy[v] in fp64 (stride 1, 'SAME', zeros
    outside): x padded once, then one [V, cin]^T @ [V, cout] product per tap over the shifted slice.  x, dy: NCDHW (any
    memory format, any dtype, any device); ups: x is the half-resolution tensor, nearest x2 first."""
    x, dy = x.double(), dy.double()
    if ups:
        x = up2(x)
    n, cin, d, h, w = x.shape
    cout = dy.shape[1]
    assert dy.shape == (n, cout, d, h, w), (x.shape, dy.shape)
    pd, ph, pw = k[0] // 2, k[1] // 2, k[2] // 2
    xp = torch.zeros((n, d + 2 * pd, h + 2 * ph, w + 2 * pw, cin), dtype=torch.float64, device=x.device)
    xp[:, pd:pd + d, ph:ph + h, pw:pw + w] = x.permute(0, 2, 3, 4, 1)
    dyv = dy.permute(0, 2, 3, 4, 1).reshape(-1, cout)
    dw = torch.empty((k[0], k[1], k[2], cin, cout), dtype=torch.float64, device=x.device)
    # (a product that reduces over 2^18 .. 2^20 voxels into 32 x 64 outputs keeps a GPU's fp64 GEMM on a handful of tiles: the
    # voxels are cut into up to 256 equal slabs, one batched product, and the slabs summed -- the same exact value)
    nvox = dyv.shape[0]
    slabs = 1
    while slabs < 256 and nvox % (2 * slabs) == 0 and nvox // (2 * slabs) >= 1024:
        slabs *= 2
    dys = dyv.reshape(slabs, -1, cout)
    for a in range(k[0]):
        for b in range(k[1]):
            for c in range(k[2]):
                xs = xp[:, a:a + d, b:b + h, c:c + w].reshape(slabs, -1, cin)
                dw[a, b, c] = torch.bmm(xs.transpose(1, 2), dys).sum(0)
    return dw, dyv.sum(0)


def mask_bits(words, n, c, sp):
    """bool [n,c,d,h,w]: bit (ch % 32) of sign word [n*d*h*w][ch // 32] -- the layout sg_conv3d_wgrad_bias_up_masked documents
    for mask_bits (include/saragan_hip.h; F_bits of tests/test_kernels_gpu.py decodes the same words)."""
    wv = words.reshape(n, *sp, (c + 31) // 32).long() & 0xFFFFFFFF
    ch = torch.arange(c, device=words.device)
    return ((wv[..., ch // 32] >> (ch % 32)) & 1).permute(0, 4, 1, 2, 3).bool()


def masked_dy(dy_half, bits, slope, gain, shape):
    """gain * where(bit, slope, 1) * nearest-x2(dy_half) in fp64, NCDHW: the effective dy of sg_conv3d_wgrad_bias_up_masked.
    shape = (n, cout, d, h, w) of the FINE tensor; bits: int32 words [n*d*h*w][cout / 32]."""
    n, c, d, h, w = shape
    m = mask_bits(bits, n, c, (d, h, w))
    up = up2(dy_half.double())
    assert up.shape == tuple(shape), (up.shape, shape)
    return gain * torch.where(m, torch.full_like(up, slope), torch.ones_like(up)) * up


def scaled(total, coef, prefill=None):
    """What the finalize kernels store for an exact f32 sum: np.float32(coef) * np.float32(sum), one rounding (__fmul_rn);
    with SG_WGRAD_ACCUMULATE one np.float32 add onto `prefill` after it (__fadd_rn).  Returns an f32 tensor."""
    s = total.detach().cpu().numpy()
    s32 = s.astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s), 'the sum itself is not an f32 value'
    out = np.float32(coef) * s32
    assert out.dtype == np.float32
    if prefill is not None:
        out = prefill.detach().cpu().numpy().astype(np.float32) + out
    return torch.from_numpy(np.ascontiguousarray(out))
