"""Helpers shared by tests/test_autograd_exact_gpu.py and tests/test_agref_host.py: a plain fp64 restatement (torch, on the
device of its arguments) of the forward, backward and backward-of-backward of the discriminator's autograd nodes
(saragan_amd/functional.py: _Conv, _ConvBiasAct with LeakyReLU, _ConvBiasActPool, _PooledDgradGather, _Wgrad, _BiasActBwd, _Up,
_Down), built from tests/fwdref.py and tests/wgref.py, the integer data of the cases and their range assertions.

Why node-level references can be exact.  For a fixed LeakyReLU mask every node is linear in its input and linear in its filter.
With integer x, filter, bias and gy, a slope of 1/4 and the gains 1/8, 1/2 and 4, each first-order result is ONE kernel deep (or
a mask / up-scale pass, exact in bf16 for these values, followed by one kernel): gx is the exact value rounded once
(fwdref.expected), gw is wgref.scaled(sum, coef), gb the exact sum.  Second order differentiates <gx, v> for a free integer v
instead of sum(gx^2): by bilinearity the derivative for gy is the node's forward map applied to v and the derivative for w the
weight gradient of (v, masked gy) -- neither reads the rounded gx, so every operand of every second-order kernel is a free
integer tensor again.

Pairs (producer -> consumer) store one intermediate between two kernels.  It is kept bf16-exact by construction -- the
consumer's filter has at most NNZ entries of +-1 per input channel, the producer's (where v travels forward through it) at most
NNZ per output channel -- and stored() asserts that, so a route that rounds the intermediate once more, or not at all, computes
the same value and every route must EQUAL the reference.

Filters: the kernels round coef * w to the compute dtype when they pack.  In bf16 the variable is q / coef in f32 (q small
integers): the packed value is exactly q for any coef (q_over_coef asserts it), and the gradient for the variable is
wgref.scaled(sum, coef).  In f32 the variable is q itself and coef a power of two.

Layouts as in fwdref: activations NCDHW, filters DHWIO.  Nothing here touches the GPU by itself."""
import numpy as np
import torch

from tests import fwdref as R
from tests import wgref as W

BF, F32 = torch.bfloat16, torch.float32
SLOPE = 0.25          # a power of two: M * g is exact
NNZ = 4               # non-zero +-1 entries per channel of a sparse filter
K333, K111 = (3, 3, 3), (1, 1, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# data
# ---------------------------------------------------------------------------------------------------------------------------
def ints(shape, seed, dtype, density=1.0):
    """Integers in [-3, 3] (wgref.int_data); with density < 1 each entry is kept with that probability (same generator
    family: seed + 7919 draws the keep mask), the others are zero."""
    x = W.int_data(shape, seed, dtype)
    if density < 1.0:
        g = torch.Generator().manual_seed(seed + 7919)
        keep = torch.rand(tuple(shape), generator=g) < density
        x = x * keep.to(x.dtype) + 0      # (+ 0: no negative zeros)
        x = x.contiguous(memory_format=torch.channels_last_3d) if x.dim() == 5 else x.contiguous()
    return x


def dense_filter(k, cin, cout, seed):
    """Integer filter in [-3, 3], f32 DHWIO (contiguous)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-3, 4, (*k, cin, cout), generator=g, dtype=torch.int32).float().contiguous()


def sparse_filter(k, cin, cout, seed, per):
    """f32 DHWIO filter with exactly NNZ entries of +-1 per input channel (per = 'in': its data gradient sums at most NNZ
    terms per element) or per output channel (per = 'out': its forward does), zeros elsewhere."""
    g = torch.Generator().manual_seed(seed)
    taps = k[0] * k[1] * k[2]
    rows, cols = (cin, taps * cout) if per == 'in' else (cout, taps * cin)
    m = torch.zeros((rows, cols))
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:NNZ]
        m[r, idx] = (torch.randint(0, 2, (NNZ,), generator=g) * 2 - 1).float()
    if per == 'in':
        w = m.reshape(cin, *k, cout).permute(1, 2, 3, 0, 4)
    else:
        w = m.reshape(cout, *k, cin).permute(1, 2, 3, 4, 0)
    return w.contiguous()


def q_over_coef(q, coef, dtype):
    """The variable whose packed image is exactly q: bf16 -- q / coef in f32 (the pack multiplies by float(coef) in f32 and
    rounds to bf16: asserted to give q back); f32 -- q itself, coef must be a power of two."""
    if dtype == F32:
        m, _ = np.frexp(coef)
        assert m == 0.5, 'f32 cases need a power-of-two coef'
        return q.clone()
    w = (q.double() / coef).float()
    packed = torch.from_numpy(w.numpy() * np.float32(coef)).to(BF)
    assert torch.equal(packed.float(), q), 'coef * (q / coef) does not round to q in bf16'
    return w


# ---------------------------------------------------------------------------------------------------------------------------
# range and representability
# ---------------------------------------------------------------------------------------------------------------------------
def quantum(t):
    """The largest power of two (<= 1) that divides every entry of an exact fp64 tensor (multiples of 2^-15 at the finest)."""
    v = t.double() * 32768.0
    r = v.round()
    assert bool((v == r).all()), 'not a multiple of 2^-15'
    r = r.abs().long()
    low = r & -r                                   # the lowest set bit of each entry, 0 for a zero
    low = low[low != 0]
    return min(1.0, int(low.min()) / 32768.0) if low.numel() else 1.0


def assert_conv_range(x, q, terms=None):
    """sum over taps and input channels of x * q: every partial sum stays below 2^24 units (the analytic bound:
    max|x| * max|q| per term, taps * cin terms)."""
    x, q = x.double(), q.double()
    unit = quantum(x) * quantum(q)
    if terms is None:
        terms = q.shape[0] * q.shape[1] * q.shape[2] * q.shape[3]
    W.assert_exact_range(float(x.abs().max()) * float(q.abs().max()), unit, terms)


def assert_wgrad_range(x, dy):
    """sum over voxels of x[v + tap] (x) dy[v]: the analytic bound where it suffices, else the data-derived one,
    max|x| * max_co sum_v |dy[v, co]| / unit < 2^24 (it bounds every partial sum of every output in any order)."""
    x, dy = x.double(), dy.double()
    unit = quantum(x) * quantum(dy)
    mx, md = float(x.abs().max()), float(dy.abs().max())
    nvox = dy.numel() // dy.shape[1]
    if mx * md / unit * nvox < W.LIMIT:
        W.assert_exact_range(mx * md, unit, nvox)
        return 'analytic'
    col = float(dy.abs().sum((0, 2, 3, 4)).max())
    assert mx * col / unit < W.LIMIT, (f'max|x| {mx} * max_co sum_v |dy| {col} / unit {unit} = {mx * col / unit:.3g} passes 2^24: '
                                       f'the case is too large (or too dense) to be exact in f32')
    return 'data'


def stored(t, dtype):
    """An intermediate tensor as the route stores it: must be representable in `dtype` (so that a route which rounds it, and
    one which keeps it in registers, hold the same value)."""
    s = t.float().to(dtype)
    assert torch.equal(s.double(), t), f'an intermediate is not representable in {dtype}: the pair is not exact by construction'
    return t


# ---------------------------------------------------------------------------------------------------------------------------
# nodes.  q is the EFFECTIVE filter (coef * variable, integer valued), words are int32 sign words (fwdref.sign_words)
# ---------------------------------------------------------------------------------------------------------------------------
def cba_forward(x, q, b, slope=SLOPE):
    """leaky_relu(conv3d(x, q) + b): (pre-activation, y, sign words of the pre-activation)."""
    assert_conv_range(x, q, q.shape[0] * q.shape[1] * q.shape[2] * q.shape[3] + 1)
    pre = R.bias_act(R.conv_ref(x, q), b)
    return pre, R.bias_act(pre, None, slope), R.sign_words(pre)


def masked(g, words, slope=SLOPE):
    """M * g: the LeakyReLU backward (and its own backward) for the stage with these sign words."""
    return R.apply_mask(g.double(), words, slope) if words is not None else g.double()


def conv_backward(x, q, g):
    """(gx, sum_w, sum_b) of conv3d(x, q) + b for the output gradient g (already masked): the data gradient, and the RAW sums
    sum_v x (x) g, sum_v g -- the gradient for the variable is wgref.scaled(sum_w, coef)."""
    assert_conv_range(g, q, q.shape[0] * q.shape[1] * q.shape[2] * q.shape[4])
    assert_wgrad_range(x, g)
    sw, sb = W.wgrad_ref(x, g, tuple(q.shape[:3]))
    return R.dgrad_ref(g, q), sw, sb


def conv_backward2(q, g, v):
    """Backward of gx = conv'(g, q) contracted with v: (the gradient for g = conv3d(v, q), the raw weight sum of (v, g))."""
    assert_conv_range(v, q)
    assert_wgrad_range(v, g)
    sw, _ = W.wgrad_ref(v, g, tuple(q.shape[:3]))
    return R.conv_ref(v, q), sw


def pool_forward(x, q, b, slope=SLOPE):
    """downscale3d(leaky_relu(conv3d(x, q) + b)): (pre-activation, the exact 2x2x2 mean, sign words)."""
    pre, a, words = cba_forward(x, q, b, slope)
    return pre, R.pool_mean(a, 3), words


def pooled_gradient(gy, words, shape, slope=SLOPE):
    """M * upscale3d(gy) / 8 at full resolution (wgref.masked_dy): the gradient of downscale3d(leaky_relu(.))."""
    return W.masked_dy(gy, words, slope, 0.125, shape)


def pool_backward2(q, words, gy, v, shape, slope=SLOPE):
    """Backward of gx = conv'(M * upscale3d(gy) / 8, q) contracted with v: (for gy: the 2x2x2 mean of M * conv3d(v, q), the
    full-resolution M * conv3d(v, q) it is the mean of, the raw weight sum of (v, M * upscale3d(gy) / 8))."""
    assert_conv_range(v, q)
    full = masked(R.conv_ref(v, q), words, slope)
    g = pooled_gradient(gy, words, shape, slope)
    assert_wgrad_range(v, g)
    sw, _ = W.wgrad_ref(v, g, tuple(q.shape[:3]))
    return R.pool_mean(full, 3), full, sw


# ---------------------------------------------------------------------------------------------------------------------------
# the case table of tests/test_autograd_exact_gpu.py (checked on the host by tests/test_agref_host.py)
# ---------------------------------------------------------------------------------------------------------------------------
class Case:
    """kind: 'cba' (_ConvBiasAct alone / with a pre-masking consumer / with one pre-masking and one plain consumer), 'wgrad'
    (_Wgrad.backward), 'pw' (from_rgb), 'pool' (_ConvBiasActPool and the gradient penalty's routes through it).
    n, cin, cout, sp: the node's input.  density: of the non-zeros of the output gradient at this shape."""

    def __init__(self, cid, kind, dtype, n, cin, cout, sp, variant='alone', coef=0.25, density=1.0, seed=0):
        self.id, self.kind, self.dtype, self.n, self.cin, self.cout, self.sp = cid, kind, dtype, n, cin, cout, tuple(sp)
        self.variant, self.coef, self.density, self.seed = variant, coef, density, seed

    def __repr__(self):
        return self.id


def _dn(dt):
    return 'bf16' if dt == BF else 'f32'


HE_32 = 1.3859292911256331 / (27 * 32) ** 0.5      # the network's own he_std of a 3x3x3 filter on 32 channels: gain / sqrt(fan_in), not a power of two

CBA_CASES = [Case(f'cba_{v}_{_dn(dt)}_{ci}to{co}', 'cba', dt, 2, ci, co, sp, variant=v, coef=(0.25 if dt == F32 else HE_32), seed=100 + 10 * i + j)
             for i, v in enumerate(('alone', 'premask', 'mixed')) for dt in (BF, F32)
             for j, (ci, co, sp) in enumerate(((8, 16, (2, 4, 8)), (32, 32, (2, 8, 32))))]
WGRAD_CASES = [Case(f'wgrad_{_dn(dt)}', 'wgrad', dt, 2, 8, 16, (2, 4, 8), coef=0.5, seed=200 + i) for i, dt in enumerate((BF, F32))]
PW_CASES = [Case(f'pw_{_dn(dt)}', 'pw', dt, 2, 1, 32, (4, 8, 32), coef=(0.5 if dt == F32 else 1.3859292911256331), seed=300 + i)
            for i, dt in enumerate((BF, F32))]
# the volume of test_pooled_backward_gather_on_ragged_volumes with both a ragged H (126 is no multiple of the 4-row tile) and an odd
# D / 2 (3 tile steps); 2^18 <= voxels < 2^20, so the forward runs pool mode 2 and the double backward the generic route
POOL_CASES = [Case('pool_ragged', 'pool', BF, 4, 32, 64, (6, 126, 256), coef=HE_32, density=0.2, seed=400),
              Case('pool_2p20', 'pool', BF, 1, 32, 64, (4, 512, 512), coef=HE_32, density=0.15, seed=410)]
# the forward's pool modes (functional._pool_mode): variant = (mode the epilogue runs, switch that forces it or None)
POOLFWD_CASES = [Case('poolfwd_mode3', 'poolfwd', BF, 1, 32, 64, (4, 512, 512), variant=(3, None), coef=HE_32, seed=500),
                 Case('poolfwd_mode1_by_switch', 'poolfwd', BF, 1, 32, 64, (4, 512, 512), variant=(1, '_NO_POOL3'), coef=HE_32, seed=501),
                 Case('poolfwd_mode1_16_channels', 'poolfwd', BF, 1, 16, 64, (4, 512, 512), variant=(1, None), coef=HE_32, seed=502),
                 Case('poolfwd_mode2', 'poolfwd', BF, 1, 64, 64, (4, 256, 256), variant=(2, None), coef=HE_32, seed=503)]
# from_rgb -> discriminator_block through networks.ops: one volume that engages pool mode 3 and the fused from_rgb backward (2^20
# voxels, W a multiple of 32) and one at which nothing is fused.  density: of the pooled gradient (entries of +-1), set by the
# data-derived bound of the filter gradients over 2^20 voxels in units of 1/512
BLOCK_CASES = [Case('block_fused', 'block', BF, 1, 1, 64, (4, 512, 512), density=0.003, seed=600),
               Case('block_tiny', 'block', BF, 2, 1, 64, (2, 4, 8), density=1.0, seed=601)]
CASES = CBA_CASES + WGRAD_CASES + PW_CASES + POOL_CASES + POOLFWD_CASES + BLOCK_CASES


def coefs(c):
    """(producer, consumer, second consumer): the network's own He constant and two more that are no powers of two in bf16 (the
    variable is q / coef), powers of two in f32 (the variable is q)."""
    return (c.coef, 0.043, 0.0721) if c.dtype == BF else (c.coef, 0.5, 0.125)


def effective(c, d):
    """The filters of the reference are the EFFECTIVE ones: q in bf16 (the variable is q / coef), coef * q in f32 (the variable is q,
    coef a power of two)."""
    if c.dtype == F32:
        for key, k in zip(('q1', 'q2', 'q3'), coefs(c)):
            if key in d:
                d[key] = d[key] * k
    return d


def cba_data(c):
    """CPU tensors of a 'cba' case: x, gy(s), v, effective filters q*, biases.  The producer's filter is dense for the node
    alone and sparse per output channel in the pairs (v travels forward through it into a stored tensor); the consumers' filters
    are sparse per input channel (their data gradient is the stored intermediate)."""
    s = c.seed * 100
    shp = (c.n, c.cin, *c.sp)
    oshp = (c.n, c.cout, *c.sp)
    d = {'x': ints(shp, s, c.dtype), 'v': ints(shp, s + 1, c.dtype), 'b1': W.int_data((c.cout,), s + 2, F32)}
    if c.variant == 'alone':
        d['q1'] = dense_filter(K333, c.cin, c.cout, s + 3)
        d['gy'] = ints(oshp, s + 4, c.dtype)
    else:
        d['q1'] = sparse_filter(K333, c.cin, c.cout, s + 3, 'out')
        d['q2'] = sparse_filter(K333, c.cout, c.cout, s + 5, 'in')
        d['gy'] = ints(oshp, s + 4, c.dtype)
        if c.variant == 'mixed':
            d['q3'] = sparse_filter(K333, c.cout, c.cout, s + 6, 'in')
            d['gy3'] = ints(oshp, s + 7, c.dtype)
    return d


def cba_reference(c, d):
    """The exact results of a 'cba' case from its data (tensors on any device).  Keys: y, words, gx, sw1, sb1 [, y2, sw2, y3,
    sw3] first order; g_gy, s2w1 [, s2w2, g_gy3, s2w3] for <gx, v>."""
    x, v, q1, b1, gy = d['x'].double(), d['v'].double(), d['q1'].double(), d['b1'].double(), d['gy'].double()
    pre, h, words = cba_forward(x, q1, b1)
    out = {'words': words}
    if c.variant == 'alone':
        g = masked(gy, words)
        out['y'] = h
        out['gx'], out['sw1'], out['sb1'] = conv_backward(x, q1, g)
        t, out['s2w1'] = conv_backward2(q1, g, v)
        out['g_gy'] = masked(t, words)
        return out
    hs = R.expected(h, c.dtype).double()       # the consumers read the producer's output as stored
    out['y'] = h
    q2 = d['q2'].double()
    assert_conv_range(hs, q2)
    out['y2'] = R.conv_ref(hs, q2)
    gh, out['sw2'], _ = conv_backward(hs, q2, gy)
    if c.variant == 'mixed':
        q3, gy3 = d['q3'].double(), d['gy3'].double()
        assert_conv_range(hs, q3)
        out['y3'] = R.conv_ref(hs, q3)
        gh3, out['sw3'], _ = conv_backward(hs, q3, gy3)
        stored(gh, c.dtype), stored(gh3, c.dtype)
        gh = gh + gh3
    g = stored(masked(stored(gh, c.dtype), words), c.dtype)      # the stored intermediate: before and after the mask
    out['gx'], out['sw1'], out['sb1'] = conv_backward(x, q1, g)
    # <gx, v>: v goes forward through the producer's filter, is masked (stored), then through the consumers' filters
    t, out['s2w1'] = conv_backward2(q1, g, v)
    t = stored(masked(stored(t, c.dtype), words), c.dtype)
    out['g_gy'], out['s2w2'] = conv_backward2(q2, gy, t)[0], W.wgrad_ref(t, gy, K333)[0]
    assert_wgrad_range(t, gy)
    if c.variant == 'mixed':
        out['g_gy3'], out['s2w3'] = R.conv_ref(t, q3), W.wgrad_ref(t, gy3, K333)[0]
        assert_wgrad_range(t, gy3)
    return out


def wgrad_data(c):
    s = c.seed * 100
    return {'x': ints((c.n, c.cin, *c.sp), s, c.dtype), 'dy': ints((c.n, c.cout, *c.sp), s + 1, c.dtype),
            'u': dense_filter(K333, c.cin, c.cout, s + 2)}


def wgrad_reference(c, d):
    """dw = coef * sum_v x (x) dy; <dw, u> differentiated: for x the data gradient of dy with the filter coef * u, for dy the
    convolution of x with it (coef a power of two: coef * u packs exactly)."""
    x, dy, u = d['x'].double(), d['dy'].double(), d['u'].double()
    assert_wgrad_range(x, dy)
    sw, sb = W.wgrad_ref(x, dy, K333)
    qu = u * c.coef
    assert_conv_range(dy, qu, 27 * c.cout)
    assert_conv_range(x, qu)
    return {'sw': sw, 'sb': sb, 'gx': R.dgrad_ref(dy, qu), 'gdy': R.conv_ref(x, qu)}


def pw_data(c):
    """from_rgb (1x1x1, one image channel -> cout) followed by a 3x3x3 cout -> cout convolution (sparse per input channel)."""
    s = c.seed * 100
    return {'x': ints((c.n, 1, *c.sp), s, c.dtype), 'q1': dense_filter(K111, 1, c.cout, s + 1), 'b1': W.int_data((c.cout,), s + 2, F32),
            'gy': ints((c.n, c.cout, *c.sp), s + 3, c.dtype), 'q2': sparse_filter(K333, c.cout, c.cout, s + 4, 'in'),
            'gy2': ints((c.n, c.cout, *c.sp), s + 5, c.dtype)}


def pw_reference(c, d):
    """alone: (gx, sw1, sb1) for gy on from_rgb's output.  pair: the same for gy2 on the consumer's output, whose data gradient
    (masked by from_rgb's sign words) is the intermediate -- stored by the plain route, never written by the fused one."""
    x, q1, b1, gy, q2, gy2 = (d[k].double() for k in ('x', 'q1', 'b1', 'gy', 'q2', 'gy2'))
    pre, h, words = cba_forward(x, q1, b1)
    out = {'y': h, 'words': words}
    out['gx'], out['sw1'], out['sb1'] = conv_backward(x, q1, masked(gy, words))
    hs = R.expected(h, c.dtype).double()
    assert_conv_range(hs, q2)
    out['y2'] = R.conv_ref(hs, q2)
    gh, out['sw2'], _ = conv_backward(hs, q2, gy2)
    g = stored(masked(stored(gh, c.dtype), words), c.dtype)
    out['pgx'], out['psw1'], out['psb1'] = conv_backward(x, q1, g)
    return out


def pool_data(c, crop=None, keys=('x', 'v', 'gy', 'q', 'b', 'a_in')):
    """The 32 -> 64 layer with downscale3d: dense x and v, the pooled gy at the case's density, a dense integer filter, an integer bias and
    the sign words of an (unrelated) input stage.  crop = (d, h, w): the leading corner of that extent of every tensor; keys:
    only these tensors (each has a seed of its own)."""
    s = c.seed * 100
    sp = c.sp
    half = tuple(e // 2 for e in sp)
    make = {'x': lambda: ints((c.n, c.cin, *sp), s, c.dtype), 'v': lambda: ints((c.n, c.cin, *sp), s + 1, c.dtype),
            'gy': lambda: ints((c.n, c.cout, *half), s + 2, c.dtype, c.density), 'q': lambda: dense_filter(K333, c.cin, c.cout, s + 3),
            'b': lambda: W.int_data((c.cout,), s + 4, F32), 'a_in': lambda: ints((c.n, c.cin, *sp), s + 5, c.dtype)}
    d = {k: make[k]() for k in keys}
    if crop is not None:
        cd, ch, cw = crop
        for k in ('x', 'v', 'a_in'):
            d[k] = d[k][:, :, :cd, :ch, :cw].contiguous(memory_format=torch.channels_last_3d)
        d['gy'] = d['gy'][:, :, :cd // 2, :ch // 2, :cw // 2].contiguous(memory_format=torch.channels_last_3d)
    return d


def pool_reference(c, d, in_mask):
    """Exact results of a 'pool' case.  First order (gy on the pooled output): y, words, gx [masked by the input stage's words],
    sw, sb.  <gx, v>: g_gy (the pooled forward map on [M_in *] v), g_full (its full-resolution form, what the generic route
    stores before the masked block sum), s2w."""
    x, v, gy, q, b = (d[k].double() for k in ('x', 'v', 'gy', 'q', 'b'))
    shape = (x.shape[0], q.shape[4], *x.shape[2:])
    pre, y, words = pool_forward(x, q, b)
    out = {'y': y, 'words': words, 'pre': pre}
    g = pooled_gradient(gy, words, shape)
    gx, out['sw'], out['sb'] = conv_backward(x, q, g)
    w_in = R.sign_words(d['a_in']) if in_mask else None
    out['in_words'] = w_in
    out['gx'] = masked(gx, w_in)
    vv = masked(v, w_in)       # the output mask of gx, pulled back onto v (exact: v * 1/4)
    out['g_gy'], out['g_full'], out['s2w'] = pool_backward2(q, words, gy, vv, shape)
    return out


def poolfwd_data(c, crop=None):
    """_ConvBiasActPool forward: dense x, a filter that is sparse per OUTPUT channel (|pre-activation| <= 3 * NNZ + 3 = 15, so the
    4-voxel means modes 1 and 2 store are multiples of 1/16 below 16: bf16 values) and an integer bias."""
    s = c.seed * 100
    d = {'x': ints((c.n, c.cin, *c.sp), s, c.dtype), 'q': sparse_filter(K333, c.cin, c.cout, s + 1, 'out'), 'b': W.int_data((c.cout,), s + 2, F32)}
    if crop is not None:
        d['x'] = d['x'][:, :, :crop[0], :crop[1], :crop[2]].contiguous(memory_format=torch.channels_last_3d)
    return d


def poolfwd_reference(c, d):
    """y: the exact 2x2x2 mean (the caller rounds it once); words: of the pre-activation.  The 4-voxel means of modes 1 and 2 are
    asserted to be bf16 values, so the route that stores them and pools the remaining pairs holds the same y."""
    pre, y, words = pool_forward(d['x'].double(), d['q'].double(), d['b'].double())
    a = R.bias_act(pre, None, SLOPE)
    for mode in (1, 2):
        stored(R.pool_mean(a, mode), c.dtype)
    return {'y': y, 'words': words}


def both_sparse_filter(k, cin, cout, seed):
    """f32 DHWIO filter with exactly NNZ entries of +-1 per input channel AND NNZ * cin / cout per output channel (cout a multiple
    of cin): input channel ci feeds the output channels r * ci + j (mod cout), j < NNZ, r = cout / cin, each through a random tap."""
    g = torch.Generator().manual_seed(seed)
    r = cout // cin
    assert r * cin == cout and NNZ * cin % cout == 0
    w = torch.zeros((*k, cin, cout))
    for ci in range(cin):
        for j in range(NNZ):
            tap = [int(torch.randint(0, s, (1,), generator=g)) for s in k]
            w[tap[0], tap[1], tap[2], ci, (r * ci + j) % cout] = float(int(torch.randint(0, 2, (1,), generator=g)) * 2 - 1)
    return w.contiguous()


def block_data(c, crop=None):
    """from_rgb (1 -> 32, dense) -> conv_1 (32 -> 32) -> conv_2 (32 -> 64) -> downscale3d: the image x, the free image v, the
    pooled gradient gy (entries of +-1 at the case's density), filters that are sparse per input AND per output channel (the
    gradients travel backward, v forward, through stored tensors) and integer biases."""
    s = c.seed * 100
    half = tuple(e // 2 for e in c.sp)
    d = {'x': ints((c.n, 1, *c.sp), s, c.dtype), 'v': ints((c.n, 1, *c.sp), s + 1, c.dtype),
         'gy': W.int_data((c.n, 64, *half), s + 2, c.dtype, -1, 1), 'q0': dense_filter(K111, 1, 32, s + 3), 'b0': W.int_data((32,), s + 4, F32),
         'q1': both_sparse_filter(K333, 32, 32, s + 5), 'b1': W.int_data((32,), s + 6, F32),
         'q2': both_sparse_filter(K333, 32, 64, s + 7), 'b2': W.int_data((64,), s + 8, F32)}
    if c.density < 1.0:
        g = torch.Generator().manual_seed(s + 9)
        keep = torch.rand(tuple(d['gy'].shape), generator=g) < c.density
        d['gy'] = (d['gy'] * keep.to(c.dtype) + 0).contiguous(memory_format=torch.channels_last_3d)
    if crop is not None:
        cd, ch, cw = crop
        for k in ('x', 'v'):
            d[k] = d[k][:, :, :cd, :ch, :cw].contiguous(memory_format=torch.channels_last_3d)
        d['gy'] = d['gy'][:, :, :cd // 2, :ch // 2, :cw // 2].contiguous(memory_format=torch.channels_last_3d)
    return d


def block_reference(c, d):
    """Exact results of a 'block' case.  Forward: y (the exact pooled mean), a2 (the full-resolution activation the unfused route
    stores first).  First order for gy on y: gx and (sw*, sb*) of the three layers.  <gx, v>: g_gy, g_full (the full-resolution
    M2 * conv_2(t1) the unfused route stores first) and s2w*.  Every tensor stored between two kernels is asserted representable."""
    x, v, gy = d['x'].double(), d['v'].double(), d['gy'].double()
    q0, q1, q2 = d['q0'].double(), d['q1'].double(), d['q2'].double()
    dt = c.dtype
    _, h0, w0 = cba_forward(x, q0, d['b0'].double())
    stored(h0, dt)
    _, h1, w1 = cba_forward(h0, q1, d['b1'].double())
    stored(h1, dt)
    pre2, a2, w2 = cba_forward(h1, q2, d['b2'].double())
    out = {'y': R.pool_mean(a2, 3), 'a2': a2, 'words': (w0, w1, w2)}
    shape = tuple(a2.shape)
    del pre2, a2
    g2 = pooled_gradient(gy, w2, shape)
    gh1, out['sw2'], out['sb2'] = conv_backward(h1, q2, g2)
    gh1 = stored(masked(stored(gh1, dt), w1), dt)
    gh0, out['sw1'], out['sb1'] = conv_backward(h0, q1, gh1)
    gh0 = stored(masked(stored(gh0, dt), w0), dt)
    out['gx'], out['sw0'], out['sb0'] = conv_backward(x, q0, gh0)
    t0, out['s2w0'] = conv_backward2(q0, gh0, v)
    t0 = stored(masked(stored(t0, dt), w0), dt)
    t1, out['s2w1'] = conv_backward2(q1, gh1, t0)
    t1 = stored(masked(stored(t1, dt), w1), dt)
    full, out['s2w2'] = conv_backward2(q2, g2, t1)
    out['g_full'] = masked(full, w2)
    out['g_gy'] = R.pool_mean(out['g_full'], 3)
    return out
