"""Helpers shared by tests/test_elementwise_gpu.py, tests/test_optim_kernels_gpu.py and tests/test_optim_rules_host.py: the
rnd / cl / close helpers of tests/test_kernels_gpu.py and plain fp64 restatements (torch / numpy on the CPU) of the
element-wise, reduction and optimiser operations of csrc/elementwise.hip and csrc/optim.hip.  Nothing here touches the GPU
except dev() / cl() / unaligned()."""
import numpy as np
import torch

DT = [torch.float32, torch.bfloat16]
SLOPE = 0.2


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def tol(dtype):
    return (1e-4, 1e-5) if dtype == torch.float32 else (1e-2, 1e-2)


def rnd(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g, dtype=torch.float64)
    return x.to(dtype).to(torch.float64)   # value representable in `dtype`


def cl(x, dtype):
    x = x.to(dtype).to(dev())
    return x.contiguous(memory_format=torch.channels_last_3d) if x.dim() == 5 else x.contiguous()


def close(got, ref, dtype, what='', tols=None):
    got = got.detach().double().cpu().numpy()
    ref = ref.detach().double().cpu().numpy()
    rt, at = tols or tol(dtype)
    scale = max(1e-30, float(np.abs(ref).max()))
    np.testing.assert_allclose(got, ref, rtol=rt, atol=at * scale, err_msg=what)


def elems16(dtype):
    """Elements of `dtype` in one 16-byte piece (E of csrc/elementwise.hip)."""
    return 16 // torch.empty((), dtype=dtype).element_size()


def unaligned(x, dtype):
    """x (fp64, NCDHW or 2-D, values representable in dtype) as an NDHWC device tensor whose base address is one element
    past a 16-byte boundary: numel + E elements are allocated and the contiguous view starting at element 1 is returned."""
    e = elems16(dtype)
    buf = torch.zeros(x.numel() + e, dtype=dtype, device=dev())
    flat = buf[1:1 + x.numel()]
    if x.dim() == 5:
        n, c, d, h, w = x.shape
        flat.copy_(x.permute(0, 2, 3, 4, 1).reshape(-1).to(dtype))
        v = flat.view(n, d, h, w, c).permute(0, 4, 1, 2, 3)
        assert v.is_contiguous(memory_format=torch.channels_last_3d)
    else:
        flat.copy_(x.reshape(-1).to(dtype))
        v = flat.view(x.shape)
    assert v.data_ptr() % 16 != 0
    return v


def sum_rtol(k):
    """Relative bound of an f32 sum of k terms in any order against the fp64 sum of the same terms, doubled
    (k * 2^-24 is the first-order worst case, so 4 k 2^-24 with the factor 2 of safety), never below the f32 tolerance."""
    return max(1e-4, 4.0 * k * 2.0 ** -24)


def assert_sum_close(got, ref, abs_terms, k, what=''):
    """got: f32 sums from a kernel; ref / abs_terms: fp64 sums of the terms and of their absolute values."""
    got = got.detach().double().cpu().numpy()
    ref = np.asarray(ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else ref)
    at = np.asarray(abs_terms.detach().double().cpu().numpy() if torch.is_tensor(abs_terms) else abs_terms)
    err = np.abs(got - ref)
    lim = sum_rtol(k) * at + 1e-30
    bad = err > lim
    assert not bad.any(), (what, int(bad.sum()), float((err / lim).max()))


# ---------------------------------------------------------------------------------------------------
# sign words (include/saragan_hip.h): int32 [n, d, h, w, ceil(c / 32)], bit j of word k = (t[.., 32 k + j] < 0)
# ---------------------------------------------------------------------------------------------------
def sign_words_np(t):
    """numpy packing of `t < 0` for an NCDHW (or [N, F]) tensor / array -> int32 array [n, d, h, w, ceil(c/32)]."""
    a = t.detach().cpu().double().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)
    if a.ndim == 2:
        a = a[:, :, None, None, None]
    a = np.moveaxis(a, 1, -1)
    c = a.shape[-1]
    nw = (c + 31) // 32
    neg = np.zeros((*a.shape[:-1], nw * 32), dtype=np.uint8)
    neg[..., :c] = a < 0
    bits = np.packbits(neg.reshape(*a.shape[:-1], nw, 32), axis=-1, bitorder='little')     # 4 bytes per word, low byte first
    return np.ascontiguousarray(bits).view('<u4').reshape(*a.shape[:-1], nw).view(np.int32)


def sign_words_dev(t):
    return torch.from_numpy(sign_words_np(t).copy()).to(dev())


def lrelu_mask(m, slope=SLOPE):
    """The LeakyReLU backward factor of an activation (or pre-activation) m: slope where m < 0, else 1."""
    return torch.where(m < 0, slope, 1.0).to(torch.float64)


# ---------------------------------------------------------------------------------------------------
# element-wise references, fp64, NCDHW
# ---------------------------------------------------------------------------------------------------
def pn_scale(x, eps=1e-8):
    return torch.rsqrt(torch.mean(x * x, dim=1, keepdim=True) + eps)


def pn_bwd(gy, y, scale):
    """dx = scale * (gy - y * mean_c(gy * y)) with the GIVEN y and scale (sg_pixel_norm_bwd's inputs)."""
    return scale * (gy - y * torch.mean(gy * y, dim=1, keepdim=True))


def up_nn(x, factors):
    for dim, f in zip((2, 3, 4), factors):
        if f != 1:
            x = x.repeat_interleave(f, dim)
    return x


def down_sum(x, factors):
    n, c, d, h, w = x.shape
    fd, fh, fw = factors
    return x.reshape(n, c, d // fd, fd, h // fh, fh, w // fw, fw).sum(dim=(3, 5, 7))


def tri_up(x):
    return torch.nn.functional.interpolate(x, scale_factor=2, mode='trilinear', align_corners=False)


def tri_up_adj(g):
    n, c, d, h, w = g.shape
    x = torch.zeros((n, c, d // 2, h // 2, w // 2), dtype=torch.float64, requires_grad=True)
    (gx,) = torch.autograd.grad(tri_up(x), x, g)
    return gx


def mbstd_grad_input(shape, seed, dtype, boost=32.0):
    """A gradient for minibatch_stddev's output whose statistic channel is large and of one sign, so that the term of the
    backward that comes through the statistic is as large as the pass-through term (a power of two keeps bf16 values)."""
    g = rnd(shape, seed, dtype)
    g[:, -1] = g[:, -1].abs() * boost
    return g


# ---------------------------------------------------------------------------------------------------
# optimiser rules (include/saragan_hip.h), fp64, on tensors; g is the gradient AFTER gscale
# ---------------------------------------------------------------------------------------------------
def adam_rule(p, g, m, v, lr_t, b1, b2, eps=1e-8):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - lr_t * m / (torch.sqrt(v) + eps), m, v


def sgd_rule(p, g, lr):
    return p - lr * g


def momentum_rule(p, g, a, lr, h, nesterov):
    a = h * a + g
    return (p - (lr * g + lr * h * a) if nesterov else p - lr * a), a


def adadelta_rule(p, g, a, a2, lr, h, eps):
    a = h * a + (1 - h) * g * g
    u = torch.sqrt(a2 + eps) * torch.rsqrt(a + eps) * g
    return p - lr * u, a, h * a2 + (1 - h) * u * u


def ema_rule(shadow, p, decay):
    return shadow - (1 - decay) * (shadow - p)


def f32_vec(n, seed, scale=1.0):
    """n fp64 values representable in f32."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g, dtype=torch.float64) * scale).float().double()
