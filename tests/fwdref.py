"""Helpers shared by tests/test_conv_fwd_exact_gpu.py and tests/test_fwdref_host.py: a plain fp64 restatement (torch) of what
sg_conv3d_fwd and the sub-pixel up-convolution entry points compute -- forward, data gradient and the epilogues that stay exact
-- for the integer-valued inputs of tests/wgref.py.

Why it is exact: x and w are integers in [-3, 3] and coef a power of two, so coef * w is a bf16 (and f32) value, every product
is a multiple of coef and every partial sum a multiple of coef below 9 * taps * cin * coef: while that stays below 2^24 units
(wgref.assert_exact_range, checked per case) nothing is rounded anywhere in the f32 accumulation, whatever the tiling, chunk
order, K split or addend pass.  The f32 accumulator then holds the value this file computes, an f32 output must EQUAL it and a
bf16 output must equal it rounded ONCE to nearest-even (expected()).  Sums above 256 units of a bf16 ulp make every odd multiple
a rounding tie (bf16_ties counts them), so torch.equal also pins the rounding mode and that there is one rounding, not two.

Layouts: activations NCDHW tensors (any memory format), weights DHWIO [kd][kh][kw][cin][cout].  Nothing here touches the GPU;
every function computes on the device its arguments live on."""
import torch

from tests.wgref import up2


def conv_taps(x, w, lo, ups=False):
    """y[v, co] = sum over taps t and ci of x[v + t - lo, ci] * w[t, ci, co], zeros outside, in fp64: x padded once, then one
    [V, cin] @ [cin, cout] product per tap over the shifted slice.  lo = (k // 2 per dimension) is the stride-1 'SAME'
    convolution; ups: x is the half-resolution tensor, nearest x2 first.  Returns NCDHW fp64."""
    x, w = x.double(), w.double()
    if ups:
        x = up2(x)
    n, cin, d, h, wd = x.shape
    k = w.shape[:3]
    cout = w.shape[4]
    assert w.shape[3] == cin, (x.shape, w.shape)
    hi = [k[i] - 1 - lo[i] for i in range(3)]
    assert min(lo) >= 0 and min(hi) >= 0, (lo, k)
    xp = torch.zeros((n, d + lo[0] + hi[0], h + lo[1] + hi[1], wd + lo[2] + hi[2], cin), dtype=torch.float64, device=x.device)
    xp[:, lo[0]:lo[0] + d, lo[1]:lo[1] + h, lo[2]:lo[2] + wd] = x.permute(0, 2, 3, 4, 1)
    y = torch.zeros((n * d * h * wd, cout), dtype=torch.float64, device=x.device)
    for a in range(k[0]):
        for b in range(k[1]):
            for c in range(k[2]):
                y += xp[:, a:a + d, b:b + h, c:c + wd].reshape(-1, cin) @ w[a, b, c]
    return y.reshape(n, d, h, wd, cout).permute(0, 4, 1, 2, 3)


def conv_ref(x, w, ups=False):
    """conv3d(x, w) (stride 1, 'SAME'), or conv3d(upscale3d(x), w) with ups."""
    return conv_taps(x, w, [s // 2 for s in w.shape[:3]], ups=ups)


def flip_transpose(w):
    """The data-gradient filter of w [kd][kh][kw][I][O]: mirrored in the taps, transposed in (I, O) -- what
    sg_conv3d_pack_weights(transpose_flip = 1) packs."""
    return w.flip(0, 1, 2).transpose(3, 4).contiguous()


def dgrad_ref(gy, w, ups=False):
    """Gradient of conv_ref(x, w, ups) for x, given the output gradient gy: the same function on the flipped, transposed filter,
    followed with ups by the 2x2x2 block sum (the adjoint of the nearest x2)."""
    g = conv_ref(gy, flip_transpose(w))
    return block_sum(g, (2, 2, 2)) if ups else g


def block_sum(y, f):
    n, c, d, h, w = y.shape
    return y.reshape(n, c, d // f[0], f[0], h // f[1], f[1], w // f[2], f[2]).sum((3, 5, 7))


def subpixel_class_ref(x, w2, par):
    """One parity class of the sub-pixel form through sg_conv3d_fwd (kd = kh = kw = 2, tap_off = par): tap t of a dimension
    reads input offset t - 1 + par.  Returns the LOW-resolution class image [n, cout, d, h, w] (the kernel scatters it to the
    voxels 2 v + out_off of the fine tensor)."""
    return conv_taps(x, w2, [1 - p for p in par])


def subpixel_weights(w, par):
    """The summed 2x2x2 filter of parity class par of conv3d(upscale3d(x), w): per dimension, parity 0 taps {w0, w1 + w2},
    parity 1 taps {w0 + w1, w2} (include/saragan_hip.h, sg_conv_epilogue.out_scale)."""
    w = w.double()
    for dim, p in enumerate(par):
        a, b, c = w.select(dim, 0), w.select(dim, 1), w.select(dim, 2)
        w = torch.stack([a, b + c] if p == 0 else [a + b, c], dim)
    return w


def bias_act(y, bias=None, slope=None):
    """y + bias[c], then LeakyReLU (v >= 0 ? v : v * slope) when slope is given."""
    if bias is not None:
        y = y + bias.double().to(y.device).reshape(1, -1, 1, 1, 1)
    if slope is not None:
        y = torch.where(y >= 0, y, y * slope)
    return y


def sign_words(t):
    """Sign words of an NCDHW tensor (include/saragan_hip.h: uint32 words[nvox][ceil(c / 32)], bit j of word k = (t[v][32 k + j]
    < 0), bits of channels >= c zero) as int32 [nvox, ceil(c / 32)]."""
    t = t.permute(0, 2, 3, 4, 1)
    c = t.shape[-1]
    nw = (c + 31) // 32
    neg = torch.zeros((*t.shape[:-1], nw * 32), dtype=torch.int64, device=t.device)
    neg[..., :c] = (t < 0).to(torch.int64)
    words = (neg.reshape(-1, nw, 32) << torch.arange(32, device=t.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def word_bits(words, n, c, sp):
    """bool NCDHW: the bit of each element in sign words [n * d * h * w][ceil(c / 32)] (the inverse of sign_words)."""
    wv = words.reshape(n, *sp, (c + 31) // 32).long() & 0xFFFFFFFF
    ch = torch.arange(c, device=words.device)
    return ((wv[..., ch // 32] >> (ch % 32)) & 1).permute(0, 4, 1, 2, 3).bool()


def apply_mask(y, words, slope):
    """y * (bit ? slope : 1): sg_conv_epilogue.mask_bits, applied last."""
    n, c, d, h, w = y.shape
    return torch.where(word_bits(words.to(y.device), n, c, (d, h, w)), y * slope, y)


def masked_gather(x_half, words, slope, gain):
    """in_gain * where(bit, in_mask_slope, 1) * upscale3d(x_half): what the masked gather reads (sg_conv_epilogue.in_mask_bits;
    words are those of the FINE tensor)."""
    up = up2(x_half.double())
    n, c, d, h, w = up.shape
    return gain * torch.where(word_bits(words.to(up.device), n, c, (d, h, w)), up * slope, up)


POOL_BLOCK = {1: (2, 1, 2), 2: (1, 2, 2), 3: (2, 2, 2)}


def pool_mean(y, mode):
    """sg_conv_epilogue.pool: the mean over 2 (D) x 1 x 2 (W) blocks (1), 1 x 2 (H) x 2 (W) blocks (2) or 2 x 2 x 2 blocks (3)."""
    f = POOL_BLOCK[mode]
    return block_sum(y, f) / (f[0] * f[1] * f[2])


def pixel_norm(y, eps):
    """(y * rsqrt(mean_c(y^2) + eps), the rsqrt factor [n, 1, d, h, w]) in fp64."""
    s = torch.rsqrt((y * y).mean(1, keepdim=True) + eps)
    return y * s, s


def rgb_head(y_stored, rgb_w, rgb_bias):
    """sg_conv_epilogue.rgb_out: sum_c y[c] * rgb_w[c] + rgb_bias over y AS STORED (rounded to the storage type)."""
    out = (y_stored.double() * rgb_w.double().to(y_stored.device).reshape(1, -1, 1, 1, 1)).sum(1, keepdim=True)
    return out + (float(rgb_bias) if rgb_bias is not None else 0.0)


def expected(ref, dtype):
    """The one rounding of the store: fp64 -> f32 is exact for these sums (asserted), f32 -> bf16 is round-to-nearest-even."""
    f = ref.float()
    assert torch.equal(f.double(), ref), 'the exact value is not an f32 value: the case is outside the exact range'
    return f.to(dtype)


def bf16_ties(ref):
    """How many entries of an exact fp64 tensor lie exactly half way between two bf16 values (8 significant bits): the entries
    where round-to-nearest-even differs from round-half-away, and where a second rounding could show."""
    f = ref.float()
    assert torch.equal(f.double(), ref)
    bits = f.contiguous().view(torch.int32)
    return int(((bits & 0xFFFF) == 0x8000).sum())


def bf16_ulp(ref):
    """The spacing of bf16 values at |ref| (fp64, elementwise; normal range)."""
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)
