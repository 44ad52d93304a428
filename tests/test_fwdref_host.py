"""tests/fwdref.py -- the fp64 references of tests/test_conv_fwd_exact_gpu.py -- checked on the CPU, bit for bit, against fp64
torch.nn.functional.conv3d, autograd and oracle/pgan_oracle.py (integer inputs: every one of these is exact, so any two correct
formulations agree to the last bit), and the tie condition the GPU file relies on for its seeds."""
import pytest
import torch
import torch.nn.functional as TF

from oracle import pgan_oracle as O
from tests import fwdref as R
from tests import wgref as W

F64 = torch.float64


def _torch_conv(x, w):
    """stride-1 'SAME' cross-correlation of NCDHW x with a DHWIO filter."""
    return TF.conv3d(x, w.permute(4, 3, 0, 1, 2), padding=[s // 2 for s in w.shape[:3]])


CASES = [(2, 5, 7, (3, 5, 6), (3, 3, 3)), (1, 8, 3, (1, 6, 8), (1, 3, 3)), (2, 4, 6, (2, 3, 4), (1, 1, 1)), (1, 3, 4, (4, 6, 5), (5, 3, 1))]


@pytest.mark.parametrize('n,cin,cout,sp,k', CASES)
def test_forward_and_data_gradient_equal_conv3d_and_autograd(n, cin, cout, sp, k):
    x = W.int_data((n, cin, *sp), 1, F64).requires_grad_(True)
    w = W.int_data((*k, cin, cout), 2, F64) * 0.25
    gy = W.int_data((n, cout, *sp), 3, F64)
    y = _torch_conv(x, w)
    assert torch.equal(R.conv_ref(x.detach(), w), y.detach())
    (gx,) = torch.autograd.grad(y, [x], gy)
    assert torch.equal(R.dgrad_ref(gy, w), gx)
    # what sg_conv3d_pack_weights(transpose_flip = 1) is handed: the filter of the layer whose gradient this is, [k][k][k][O][I]
    # seen from the data-gradient convolution (cin = O channels of gy in, cout = I channels out)
    assert torch.equal(R.conv_ref(gy, R.flip_transpose(w)), gx)


@pytest.mark.parametrize('n,cin,cout,sp,k', [(2, 5, 7, (4, 6, 8), (3, 3, 3)), (1, 8, 3, (2, 6, 8), (1, 3, 3))])
def test_gathered_form_equals_conv3d_of_the_upscaled_input(n, cin, cout, sp, k):
    half = tuple(v // 2 for v in sp)
    x = W.int_data((n, cin, *half), 4, F64).requires_grad_(True)
    w = W.int_data((*k, cin, cout), 5, F64) * 0.5
    gy = W.int_data((n, cout, *sp), 6, F64)
    y = _torch_conv(O.upscale3d(x), w)
    assert torch.equal(R.conv_ref(x.detach(), w, ups=True), y.detach())
    (gx,) = torch.autograd.grad(y, [x], gy)
    assert torch.equal(R.dgrad_ref(gy, w, ups=True), gx)
    assert torch.equal(W.up2(x.detach()), O.upscale3d(x.detach()))


def test_subpixel_decomposition():
    """Each parity class of conv3d(upscale3d(x), w) is the 2x2x2 convolution of x with the summed filter, read at tap_off = parity;
    the oracle's own sub-pixel form agrees; the sub-pixel data gradient is the adjoint."""
    n, cin, cout, sp = 2, 6, 5, (3, 4, 5)
    x = W.int_data((n, cin, *sp), 7, F64)
    w = W.int_data((3, 3, 3, cin, cout), 8, F64)
    full = R.conv_ref(x, w, ups=True)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                cls = R.subpixel_class_ref(x, R.subpixel_weights(w, (a, b, c)), (a, b, c))
                assert torch.equal(cls, full[:, :, a::2, b::2, c::2]), (a, b, c)
    coef = O.runtime_coef(w.shape, 'linear')
    assert torch.allclose(O.conv3d_upscaled_subpixel(x, w, 'linear'), full * coef, rtol=1e-13, atol=1e-12)
    gy = W.int_data((n, cout, *(2 * v for v in sp)), 9, F64)
    gx = R.dgrad_ref(gy, w, ups=True)
    assert float((gx * x).sum()) == float((gy * full).sum())      # <A^T gy, x> = <gy, A x>, exact in integers


def test_epilogues_equal_the_oracle():
    n, c, sp = 2, 40, (4, 6, 8)
    y = W.int_data((n, c, *sp), 10, F64) * 0.25
    b = W.int_data((c,), 11, F64)
    assert torch.equal(R.bias_act(y, b, 0.25), O.act(O.apply_bias(y, b), 'leaky_relu', 0.25))
    assert torch.equal(R.bias_act(y, b, None), O.apply_bias(y, b))
    pn, s = R.pixel_norm(y, 1e-8)
    assert torch.equal(pn, O.pixel_norm(y, 1e-8))
    assert torch.equal(s, torch.rsqrt((y * y).mean(1, keepdim=True) + 1e-8))
    assert torch.equal(R.pool_mean(y, 3), O.downscale3d(y))
    # pool = 1 / 2 are the first stage of the same mean (include/saragan_hip.h): the other pair finishes it
    assert torch.equal(R.block_sum(R.pool_mean(y, 1), (1, 2, 1)) / 2, O.downscale3d(y))
    assert torch.equal(R.block_sum(R.pool_mean(y, 2), (2, 1, 1)) / 2, O.downscale3d(y))
    assert R.pool_mean(y, 1).shape == (n, c, sp[0] // 2, sp[1], sp[2] // 2)
    assert R.pool_mean(y, 2).shape == (n, c, sp[0], sp[1] // 2, sp[2] // 2)


def test_sign_words_masks_and_masked_gather():
    n, c, sp = 2, 40, (2, 4, 6)
    t = W.int_data((n, c, *sp), 12, F64)
    words = R.sign_words(t)
    assert words.shape == (n * 2 * 4 * 6, 2) and words.dtype == torch.int32
    # a direct statement of the layout: bit j of word (v, k) = (t[v][32 k + j] < 0); channels >= c give zero bits
    tv = t.permute(0, 2, 3, 4, 1).reshape(-1, c)
    for v, k in ((0, 0), (5, 1), (95, 0), (95, 1)):
        want = sum(1 << j for j in range(32) if 32 * k + j < c and tv[v, 32 * k + j] < 0)
        assert (int(words[v, k]) & 0xFFFFFFFF) == want
    bits = R.word_bits(words, n, c, sp)
    assert torch.equal(bits, t < 0)
    assert torch.equal(bits, W.mask_bits(words, n, c, sp))
    assert torch.equal(R.apply_mask(t, words, 0.25), torch.where(t < 0, t * 0.25, t))
    # the masked gather is the backward of downscale3d(leaky_relu(.)): autograd on that composition
    fine = W.int_data((n, c, 4, 8, 12), 13, F64).requires_grad_(True)
    g_half = W.int_data((n, c, 2, 4, 6), 14, F64)
    out = O.downscale3d(O.act(fine, 'leaky_relu', 0.25))
    (g_fine,) = torch.autograd.grad(out, [fine], g_half)
    fw = R.sign_words(fine.detach())
    assert torch.equal(R.masked_gather(g_half, fw, 0.25, 0.125), g_fine)
    assert torch.equal(R.masked_gather(g_half, fw, 0.25, 0.125), W.masked_dy(g_half, fw, 0.25, 0.125, fine.shape))


def test_rgb_head_and_the_one_rounding():
    y = (W.int_data((1, 32, 2, 3, 4), 15, F64) * 0.25).to(torch.bfloat16)
    rw = W.int_data((32,), 16, torch.float32)
    want = TF.conv3d(y.double(), rw.double().reshape(1, 32, 1, 1, 1)) + 2.0
    assert torch.equal(R.rgb_head(y, rw, 2.0), want)
    # 257 = 0x101 lies half way between the bf16 values 256 and 258: nearest-even gives 256, and 259 gives 260
    ref = torch.tensor([257.0, 259.0, 256.0, 64.25, 64.75, -257.0, 3.0], dtype=F64)
    assert R.expected(ref, torch.bfloat16).tolist() == [256.0, 260.0, 256.0, 64.0, 65.0, -256.0, 3.0]
    assert R.bf16_ties(ref) == 5
    assert torch.equal(R.expected(ref, torch.float32).double(), ref)
    with pytest.raises(AssertionError):
        R.expected(torch.tensor([2.0 ** 24 + 1], dtype=F64), torch.float32)
    assert R.bf16_ulp(torch.tensor([1.0, 1.5, 2.0, 300.0], dtype=F64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0]


def _cost(c):
    return c.n * c.sp[0] * c.sp[1] * c.sp[2] * c.cin * c.cout * c.k[0] * c.k[1] * c.k[2]


def _tie_cases():
    from tests import test_conv_fwd_exact_gpu as G
    return [c for c in G.ROUTES if c.tie]


def test_every_kernel_family_has_a_tie_case():
    fams = {c.kernel.split('<')[0].split(' (')[0] for c in _tie_cases()}
    assert {'conv_fwd', 'conv_fwd2', 'conv_fwd3r', 'conv_fwd3s', 'conv_fwd3p', 'conv_fwd3p16', 'conv_fwd3w', 'conv_fwd4', 'conv_fwd5',
            'conv_gemm', 'pw_fwd_small_cout', 'dense_small_m'} <= fams, fams
    assert any(c.kernel.endswith('x2 (K split)') for c in _tie_cases()) and any(c.kernel == 'conv_gemm (K split)' for c in _tie_cases())


@pytest.mark.parametrize('c', _tie_cases(), ids=[c.id for c in _tie_cases()])
def test_tie_condition_holds_for_the_chosen_seeds(c):
    """The GPU file's bf16 cases marked tie=True, with their own seeds: the exact reference holds outputs that lie half way between
    two bf16 values (and passes the exact-range condition), so torch.equal against fwdref.expected pins round-to-nearest-even and
    one rounding.  Of the large cases the leading corner of the output (1 sample, 2 planes, 8 rows) is computed here: the same
    values the whole reference holds there, which test_cropped_reference_is_the_corner_of_the_whole_one checks."""
    from tests import test_conv_fwd_exact_gpu as G
    plain = not (c.ups or c.mask or c.in_gain is not None or c.par is not None)
    d = G.case_reference(c, torch.device('cpu'), crop=(1, 2, 8) if plain and _cost(c) >= 2e8 else None)
    ties = R.bf16_ties(d['ref'])
    want = R.expected(d['ref'], torch.bfloat16)
    assert ties > 0, c.id
    # at a tie truncation and nearest-even differ wherever the kept mantissa is odd: the comparison can tell them apart
    trunc = (d['ref'].float().view(torch.int32) & ~0xFFFF).view(torch.float32).to(torch.bfloat16)
    assert not torch.equal(trunc, want)


def test_cropped_reference_is_the_corner_of_the_whole_one():
    from tests import test_conv_fwd_exact_gpu as G
    for c in (G.Case('a', '', 2, 6, 5, (5, 11, 7), bias=True, act=True), G.Case('b', '', 2, 6, 5, (4, 12, 6), flip=True, pool=2),
              G.Case('c', '', 3, 4, 5, (1, 9, 6), k=G.K133), G.Case('d', '', 2, 6, 5, (2, 6, 7))):
        whole = G.case_reference(c, torch.device('cpu'))['ref']
        part = G.case_reference(c, torch.device('cpu'), crop=(1, 2, 8))['ref']
        assert part.shape[2] >= 1 and part.shape[3] >= 3
        assert torch.equal(part, whole[:1, :, :part.shape[2], :part.shape[3]]), c.id


def _sub_tie_cases():
    from tests import test_conv_fwd_exact_gpu as G
    return [c for c in G.SUBPIX if not c.pn and (c.dgrad or c.cin >= 32)]


@pytest.mark.parametrize('c', _sub_tie_cases(), ids=[c.id for c in _sub_tie_cases()])
def test_tie_condition_holds_for_the_subpixel_cases(c):
    """The sub-pixel cases whose GPU test asserts a tie (forward from 32 input channels on, every data gradient): first sample."""
    from tests import test_conv_fwd_exact_gpu as G
    ref = G.sub_reference(c, torch.device('cpu'), samples=1)[4]
    assert R.bf16_ties(ref) > 0, c.id
