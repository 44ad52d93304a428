"""Every forward / data-gradient route of sg_conv3d_fwd (csrc/conv3d.hip, conv3p.hip, conv3w.hip, gemm.hip, small.hip) and the
sub-pixel up-convolution entry points (csrc/subpix.hip) on inputs for which every f32 sum is exact: x and w are integers in
[-3, 3] and coef a power of two, so each product and each partial sum is a multiple of coef below 9 x taps x cin x coef < 2^24
units whatever the tiling, chunk order, K split or addend pass, and the fp64 reference of tests/fwdref.py is the exact value.

f32 routes must store that value; bf16 routes must store it rounded ONCE, to nearest-even (fwdref.expected): the assertion is
torch.equal.  With 27 x 32 terms the sums have a standard deviation of about 120 units, so many outputs lie above 256 units,
where every odd multiple is a rounding tie: the comparison therefore pins the rounding mode and that there is one rounding (not
a bf16 store before the bias, the activation or a pooled mean).  Cases marked tie=True assert on the host that their reference
holds at least one such tie, so the property is checked and not assumed.  (pw_fwd_small_cin sums at most 4 products, 36 units,
and cannot tie.  conv_small_fwd (<= 144 terms) and the 6-channel conv_fwd cases (162 terms) could reach 256 units but with a
standard deviation of about 50 units do not in these tensors: they carry no such mark; conv_fwd has its tie case behind
SG_FWD_V1=1.)

Exact epilogues are part of the exact comparison: integer bias, LeakyReLU and masks with slope 0.25, sign words (compared with
fwdref.sign_words), the fused nearest-x2 gather, the masked gather (slope 0.25, power-of-two gain), x_plane_channels = 32 and the
pooled means (4 or 8 exact values, exact in f32, one rounding: include/saragan_hip.h states the mean of the UNROUNDED
activation).  pixel_norm uses an rsqrt: those cases are compared under a derived bound (see test_pixel_norm_within_derived_bound).

Each case names the launch constant or dispatch condition it crosses and asserts the kernel that ran by name (sg_prof_enable /
sg_prof_collect, forward launches are profile kind 0 -- the sub-pixel entry points too, prof.hip / subpix.hip:654,973): a case
that silently lands on another route fails.  y is pre-filled with a sentinel, workspaces with 0xFF bytes.

Template instantiations the chooser builds but cannot reach at any shape:
  conv_fwd2<T,2,4,4>: gc = 4 is never chosen for the 2 x 4 register tile (conv3d.hip: `!(mtw == 2 && ntb == 4)`), the macro
    maps it to <T,2,2,4>.
  conv_fwd<T,1,*>: the v1 kernel is never launched with MTW = 1 (`if (!v2 && mtw == 1) continue`).
Every other instantiation of conv_fwd, conv_fwd2, conv_fwd3r and conv_fwd4 has a case."""
import ctypes as C
import functools

import pytest
import torch

from tests import fwdref as R
from tests import gref as G
from tests import wgref as W

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
K333, K133, K111, K222 = (3, 3, 3), (1, 3, 3), (1, 1, 1), (2, 2, 2)
SENTINEL = 7.5
SG_EINVAL, SG_EALIGN, SG_EUNSUPPORTED = -1, -3, -4


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _libs():
    from saragan_amd import _lib
    return _lib, _lib.load()


def _dt(dtype):
    from saragan_amd import _lib
    return _lib.SG_BF16 if dtype == BF else _lib.SG_F32


def _fwd_kernels(_lib, lib):
    """Names of the forward launches (profile kind 0) that succeeded since sg_prof_enable(1)."""
    ents = (_lib.ProfEntry * 16)()
    cnt = C.c_int32(0)
    lib.sg_prof_collect(ents, 16, C.byref(cnt))
    return sorted({ents[i].kernel.decode() for i in range(cnt.value) if ents[i].kind == 0})


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _garbage(nbytes):
    return torch.full((max(int(nbytes), 16),), 255, dtype=torch.uint8, device=dev())


def _ndhwc(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


class Case:
    """One call of sg_conv3d_fwd.  (n, cin, cout, sp, k, ups) are the fields of sg_conv_shape (sp the OUTPUT extent); flip: the
    weights are packed with transpose_flip = 1 from a [k][k][k][cout][cin] filter and the reference is the data gradient.
    bias / act / mask / sign / pool / pn: the epilogue.  in_gain: the masked gather.  xpl: x_plane_channels = 32.  ws: hand the
    call the workspace sg_conv3d_fwd_workspace asks for.  par: one sub-pixel parity class (k = 2x2x2, out_scale = 2): tap_off = par,
    written at the voxels 2 v + out_off (out_off = par unless given)."""

    def __init__(self, cid, kernel, n, cin, cout, sp, k=K333, dt=BF, flip=False, ups=False, env=None, coef=0.25, bias=False, act=False,
                 mask=False, sign=False, pool=0, pn=False, in_gain=None, xpl=False, ws=True, par=None, out_off=None, tie=False):
        self.id, self.kernel, self.n, self.cin, self.cout, self.sp, self.k, self.dt = cid, kernel, n, cin, cout, tuple(sp), tuple(k), dt
        self.flip, self.ups, self.env, self.coef, self.bias, self.act, self.mask, self.sign = flip, ups, env or {}, coef, bias, act, mask, sign
        self.pool, self.pn, self.in_gain, self.xpl, self.ws, self.par, self.tie = pool, pn, in_gain, xpl, ws, par, tie
        self.out_off = par if out_off is None else out_off

    def key(self):
        return (self.n, self.cin, self.cout, self.sp, self.k, self.dt, self.flip, self.ups, self.coef, self.bias, self.act, self.mask,
                self.sign, self.pool, self.pn, self.in_gain, self.par)

    def out_sp(self):
        if self.par is not None:
            return tuple(2 * v for v in self.sp)
        f = R.POOL_BLOCK.get(self.pool, (1, 1, 1))
        return tuple(v // q for v, q in zip(self.sp, f))


def case_reference(c, device, crop=None):
    """Inputs and the exact fp64 result of case c on `device`: dict with x, w (f32 DHWIO as the pack call reads it), bias, mask,
    in_mask (int32 words), pre (the value before mask / pool / pixel norm: sign words are taken from it) and ref.
    crop = (samples, planes, rows): the reference of that leading corner of the output only, computed from the corner of x it
    depends on (plain cases without gather or masks: what the CPU check of the tie condition needs of the large cases)."""
    seed = 3000 + 7 * c.cin + 3 * c.cout + c.sp[0] + 5 * c.sp[1] + 11 * c.sp[2] + c.n + 13 * len(c.k) * c.k[0]
    fine = c.sp
    xin = tuple(v // 2 for v in fine) if c.ups else fine
    x = W.int_data((c.n, c.cin, *xin), seed, c.dt).to(device)
    wshape = (*c.k, c.cout, c.cin) if c.flip else (*c.k, c.cin, c.cout)
    w = W.int_data(wshape, seed + 1, F32).contiguous().to(device)      # (int_data lays 5-D tensors out NDHWC: DHWIO here)
    g = torch.Generator().manual_seed(seed + 2)
    out = {'x': x, 'w': w, 'bias': None, 'mask': None, 'in_mask': None}
    weff = (R.flip_transpose(w) if c.flip else w).double() * c.coef
    if crop is not None:
        assert not (c.ups or c.mask or c.in_gain is not None or c.par is not None)
        cn, cd, ch = crop
        x = x[:cn, :, :cd + c.k[0] // 2, :ch + c.k[1] // 2]
    unit, top, terms = c.coef, 9 * c.coef, c.k[0] * c.k[1] * c.k[2] * c.cin
    if c.in_gain is not None:
        nw = (c.cin + 31) // 32
        out['in_mask'] = torch.randint(-2 ** 31, 2 ** 31 - 1, (c.n * fine[0] * fine[1] * fine[2], nw), generator=g, dtype=torch.int32).to(device)
        y = R.conv_ref(R.masked_gather(x, out['in_mask'], 0.25, c.in_gain), weff)
        unit, top = unit * c.in_gain * 0.25, top * c.in_gain
    elif c.par is not None:
        y = R.subpixel_class_ref(x, weff, c.par)
    else:
        y = R.conv_ref(x, weff, ups=c.ups)
    if crop is not None:      # the last plane / row of the corner saw zeros where the tensor goes on: drop what depends on them
        y = y[:, :, :min(cd, c.sp[0]), :min(ch, c.sp[1])]
    if c.bias:
        out['bias'] = torch.randint(-3, 4, (c.cout,), generator=g).float().to(device)
        terms += 1
    y = R.bias_act(y, out['bias'], 0.25 if c.act else None)
    unit = unit * (0.25 if c.act else 1.0)
    out['pre'] = y
    if c.mask:
        out['mask'] = torch.randint(-2 ** 31, 2 ** 31 - 1, (c.n * fine[0] * fine[1] * fine[2], (c.cout + 31) // 32), generator=g,
                                    dtype=torch.int32).to(device)
        y = R.apply_mask(y, out['mask'], 0.25)
        unit *= 0.25
    if c.pool:
        y = R.pool_mean(y, c.pool)
        f = R.POOL_BLOCK[c.pool]
        unit, terms = unit / (f[0] * f[1] * f[2]), terms * f[0] * f[1] * f[2]
    W.assert_exact_range(top, unit, terms)
    out['ref'] = y
    return out


class _ByKey:
    """lru_cache key: cases that differ only in id / env / expected kernel share inputs and reference."""
    def __init__(self, c):
        self.c, self.k = c, c.key()

    def __hash__(self):
        return hash(self.k)

    def __eq__(self, o):
        return self.k == o.k


@functools.lru_cache(maxsize=6)
def _cached(bk):
    return case_reference(bk.c, dev())


def _case_data(c):
    return _cached(_ByKey(c))


@pytest.fixture(scope='module', autouse=True)
def _release_case_data():
    """The cached inputs and references live on the device: released when the module is done."""
    yield
    _cached.cache_clear()
    torch.cuda.empty_cache()


def _shape(c):
    _lib, _ = _libs()
    return _lib.ConvShape(c.n, *c.sp, c.cin, c.cout, *c.k, 1 if c.ups else 0)


def _pack(c, w, shp=None):
    _lib, lib = _libs()
    shp = shp or _shape(c)
    nb = lib.sg_conv3d_packed_bytes(C.byref(shp), _dt(c.dt))
    assert nb > 0
    wp = _garbage(nb)
    _lib.check(lib.sg_conv3d_pack_weights(w.data_ptr(), c.coef, 1 if c.flip else 0, wp.data_ptr(), C.byref(shp), _dt(c.dt), _stream()), 'pack')
    return wp


def _x_buffer(c, x):
    """x as the call reads it: NDHWC, or with x_plane_channels = 32 the 32-channel groups as separate NDHWC tensors in a row."""
    if not c.xpl:
        return _ndhwc(x)
    return torch.cat([_ndhwc(x[:, i:i + 32]).permute(0, 2, 3, 4, 1).reshape(-1) for i in range(0, c.cin, 32)])


def _launch(c, d, tweak=None, y=None):
    """One sg_conv3d_fwd for case c on the data d; returns (rc, kernel names, y NCDHW view, sign words, pn_scale)."""
    _lib, lib = _libs()
    shp, dt = _shape(c), _dt(c.dt)
    wp = _pack(c, d['w'])
    xb = _x_buffer(c, d['x'])
    if y is None:
        y = _ndhwc(torch.full((c.n, c.cout, *c.out_sp()), SENTINEL, dtype=c.dt, device=dev()))
    nvox = c.n * c.sp[0] * c.sp[1] * c.sp[2] * (8 if c.par is not None else 1)
    signs = torch.full((nvox, (c.cout + 31) // 32), 0x5A5A5A5A, dtype=torch.int32, device=dev()) if c.sign else None
    scale = torch.full((nvox,), SENTINEL, dtype=F32, device=dev()) if c.pn else None
    ep = _lib.ConvEpilogue()
    if d['bias'] is not None:
        ep.bias = d['bias'].data_ptr()
    ep.act, ep.slope = (1, 0.25) if c.act else (0, 0.0)
    if c.pn:
        ep.pixel_norm, ep.eps, ep.pn_scale = 1, 1e-8, scale.data_ptr()
    if d['mask'] is not None:
        ep.mask_bits, ep.mask_slope = d['mask'].data_ptr(), 0.25
    if signs is not None:
        ep.sign_out = signs.data_ptr()
    if c.par is not None:
        ep.out_scale = 2
        ep.out_off = (C.c_int32 * 3)(*c.out_off)
        ep.tap_off = (C.c_int32 * 3)(*c.par)
    ep.pool = c.pool
    ws = None
    if c.ws:
        nb = lib.sg_conv3d_fwd_workspace(C.byref(shp), dt)
        if nb:
            ws = _garbage(nb)
            ep.workspace, ep.workspace_bytes = ws.data_ptr(), ws.numel()
    if c.xpl:
        ep.x_plane_channels = 32
    if d['in_mask'] is not None:
        ep.in_mask_bits, ep.in_mask_slope, ep.in_gain = d['in_mask'].data_ptr(), 0.25, c.in_gain
    if tweak:
        tweak(ep)
    lib.sg_prof_enable(1)
    try:
        rc = lib.sg_conv3d_fwd(xb.data_ptr(), wp.data_ptr(), y.data_ptr(), C.byref(shp), C.byref(ep), dt, _stream())
        torch.cuda.synchronize()
        names = _fwd_kernels(_lib, lib)
    finally:
        lib.sg_prof_enable(0)
    return rc, names, y, signs, scale


def _assert_equal(cid, got, want, what='y'):
    if not torch.equal(got, want):
        bad = (got != want)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{cid}: {what} differs in {int(bad.sum())} of {bad.numel()} entries, first at {idx}: '
                             f'{float(got[tuple(idx)])!r} != {float(want[tuple(idx)])!r}')


def _run_exact(c, sg_env):
    _lib, _ = _libs()
    d = _case_data(c)
    if c.env:
        sg_env(**c.env)
    rc, names, y, signs, _ = _launch(c, d)
    _lib.check(rc, c.id)
    assert names == [c.kernel], (c.id, names)
    want = R.expected(d['ref'], c.dt)
    if c.tie:
        assert c.dt == BF and R.bf16_ties(d['ref']) > 0, f'{c.id}: the reference holds no bf16 rounding tie'
    if c.par is not None:      # the voxels 2 v + out_off hold the class image, every other voxel its sentinel
        a, b, e = c.out_off
        _assert_equal(c.id, y[:, :, a::2, b::2, e::2], want, 'class voxels')
        rest = y.clone()
        rest[:, :, a::2, b::2, e::2] = SENTINEL
        assert bool((rest == SENTINEL).all()), f'{c.id}: a voxel of another parity class was written'
    else:
        _assert_equal(c.id, y, want)
    if c.sign:
        assert c.par is None
        _assert_equal(c.id, signs, R.sign_words(d['pre']), 'sign words')


# ----------------------------------------------------------------------------------------------------------------------
# conv_fwd3w (conv3w.hip:887): bf16, 3x3x3, cin = 32, cout % 32 = 0, D >= 2, H >= 8, W % 32 = 0.  Columns of 16 (H) x 32 (W):
# ncol = n * cdiv(H, 16) * (W / 32); gx = (256 / ntile) / 8 * 8; with ncol < gx the columns are cut along D into segments of
# L = max(4, cdiv(D, cdiv(gx, ncol))) rounded up to even planes, and gx shrinks to the items there are.
# ----------------------------------------------------------------------------------------------------------------------
FWD3W = [
    Case('3w_minimum', 'conv_fwd3w<bf16,32->32>', 1, 32, 32, (2, 8, 32), tie=True),            # D = 2, H = 8: the smallest shape it takes
    Case('3w_H7_declines', 'conv_fwd2<bf16,1,1,2>', 1, 32, 32, (2, 7, 32)),                   # H < 8: 56 voxels, one 128-voxel tile per slice
    # D = 10 in segments of L = 4: three, the last half filled; H = 24: a 16-row block and an 8-row one; W = 96: a column with a
    # neighbour on both sides
    Case('3w_D10_H24_W96', 'conv_fwd3w<bf16,32->32>', 1, 32, 32, (10, 24, 96), tie=True),
    Case('3w_D5_H20_W64_cout96', 'conv_fwd3w<bf16,32->32>', 2, 32, 96, (5, 20, 64), tie=True),  # odd D, three blockIdx.y slices, one W seam
    # ncol = 1 * 8 * 8 = 64 = gx at cout 128 (ntile 4): whole columns, no D segments
    Case('3w_ncol_equals_gx', 'conv_fwd3w<bf16,32->32>', 1, 32, 128, (2, 128, 256), tie=True),
    Case('3w_dgrad', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (5, 20, 64), flip=True, tie=True),
    Case('3w_dgrad_mask', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (5, 20, 64), flip=True, mask=True),
    Case('3w_bias_act_sign', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (5, 20, 64), bias=True, act=True, sign=True),
    Case('3w_bias', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (5, 20, 64), bias=True, coef=1.0, tie=True),
    Case('3w_pool1', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (6, 20, 64), bias=True, act=True, pool=1),
    Case('3w_pool1_sign', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (6, 20, 64), bias=True, act=True, pool=1, sign=True),
    Case('3w_pool1_mask', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (6, 20, 64), flip=True, pool=1, mask=True),
    Case('3w_pool3', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (6, 20, 64), bias=True, act=True, pool=3),
    Case('3w_pool3_sign', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (6, 20, 64), bias=True, act=True, pool=3, sign=True),
    Case('3w_pool3_mask', 'conv_fwd3w<bf16,32->32>', 2, 32, 64, (6, 20, 64), flip=True, pool=3, mask=True),
]

# ----------------------------------------------------------------------------------------------------------------------
# conv_fwd3s<GC> (launch_fwd3s): bf16, 3x3x3, cin <= 32, tiles 2 x 4 x 32, D >= 4, W % 32 = 0, cout % 32 = 0 and at least
# gx = (256 / ntile) / 8 * 8 column pairs: n * cdiv(cdiv(H, 4), 2) * (W / 32) >= gx.  cout 128: gx = 64.  cin 32 is conv_fwd3w's
# unless H < 8 or SG_FWD3S_16=0; cin 24 reaches <2> (the second chunk half filled), cin 16 reaches <1>.
# ----------------------------------------------------------------------------------------------------------------------
FWD3S = [
    Case('3s2_engaging_edge', 'conv_fwd3s<bf16,2>', 1, 24, 128, (4, 64, 256), tie=True),       # 8 pairs x 8 = 64 = gx
    Case('3s2_one_column_fewer', 'conv_fwd2<bf16,2,2,2>', 1, 24, 128, (4, 64, 224)),          # 8 x 7 = 56 < gx; 224 tiles x 2 slice pairs >= 384
    Case('3s2_D5_H62_W96', 'conv_fwd3s<bf16,2>', 1, 24, 128, (5, 174, 96), tie=True),         # nTd = 3, last H tile 2 rows, nTw = 3: 22 x 3 = 66
    Case('3s1_engaging_edge', 'conv_fwd3s<bf16,1>', 1, 16, 128, (4, 64, 256), tie=True),
    Case('3s1_D5_H62_W64', 'conv_fwd3s<bf16,1>', 2, 16, 128, (5, 126, 64), bias=True, act=True, sign=True),   # 2 x 16 x 2 = 64
    Case('3s2_no_3w', 'conv_fwd3s<bf16,2>', 1, 32, 128, (4, 64, 256), env={'SG_FWD3S_16': 0}, tie=True),
    Case('3s2_dgrad_mask', 'conv_fwd3s<bf16,2>', 1, 24, 128, (4, 64, 256), flip=True, mask=True),
    Case('3s2_pool1_sign', 'conv_fwd3s<bf16,2>', 1, 24, 128, (4, 64, 256), bias=True, act=True, pool=1, sign=True),
    Case('3s2_pool1', 'conv_fwd3s<bf16,2>', 1, 24, 128, (4, 64, 256), bias=True, act=True, pool=1),
    Case('3s1_dgrad', 'conv_fwd3s<bf16,1>', 1, 16, 128, (4, 64, 256), flip=True, tie=True),
    # block means of M * conv(x), the double backward of a pooled LeakyReLU layer (GC = 2 only: conv3d.hip:1773)
    Case('3s2_pool1_dgrad_mask', 'conv_fwd3s<bf16,2>', 1, 24, 128, (4, 64, 256), flip=True, pool=1, mask=True),
]

# ----------------------------------------------------------------------------------------------------------------------
# 64 -> 32 at 3x3x3 with the workspace: conv_fwd3p16 / conv_fwd3p (conv3p.hip:883; npair = n * cdiv(cdiv(H, 4), 2) * (W / 32) >= 8,
# D >= 2), else the two-pass K split of conv_fwd3s<2> (D >= 4 and 256 column pairs), else the streamed kernels.
# ----------------------------------------------------------------------------------------------------------------------
P64 = [
    # (D = 4: sg_conv3d_fwd_workspace offers the workspace from D >= 4, and without one the layer is not split at all)
    Case('3p16_eight_pairs', 'conv_fwd3p16<bf16,64->32>', 1, 64, 32, (4, 32, 64), tie=True),    # 4 x 2 = 8 pairs: gx = 8
    Case('3p_eight_pairs', 'conv_fwd3p<bf16,64->32>', 1, 64, 32, (4, 32, 64), env={'SG_FWD3P_16': 0}, tie=True),
    Case('3p16_six_pairs', 'conv_fwd2<bf16,1,1,2>', 1, 64, 32, (4, 24, 64)),                   # 3 x 2 = 6 pairs: gx = 0, declines
    Case('3p16_D5_H30_W96', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (5, 30, 96), bias=True, act=True, sign=True),
    Case('3p_D5_H30_W96', 'conv_fwd3p<bf16,64->32>', 2, 64, 32, (5, 30, 96), bias=True, act=True, sign=True, env={'SG_FWD3P_16': 0}),
    Case('3p16_dgrad_mask', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (5, 30, 96), flip=True, mask=True),
    Case('3p16_ups', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, tie=True),
    Case('3p_ups_sign', 'conv_fwd3p<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, bias=True, act=True, sign=True, env={'SG_FWD3P_16': 0}),
    Case('3p16_in_mask', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, in_gain=0.125),
    Case('3p16_in_mask_mask', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, in_gain=1.0, mask=True),
    Case('3p_dgrad_mask', 'conv_fwd3p<bf16,64->32>', 2, 64, 32, (5, 30, 96), flip=True, mask=True, env={'SG_FWD3P_16': 0}),
    Case('3p_ups', 'conv_fwd3p<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, env={'SG_FWD3P_16': 0}, tie=True),
    Case('3p_in_mask', 'conv_fwd3p<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, in_gain=0.125, env={'SG_FWD3P_16': 0}),
    Case('3p_in_mask_mask', 'conv_fwd3p<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, in_gain=1.0, mask=True, env={'SG_FWD3P_16': 0}),
    # the K split: 8 x 4 x 8 = 256 column pairs = gx (ntile 1)
    Case('x2_engaging_edge', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, tie=True),
    Case('x2_one_sample_fewer', 'conv_fwd4<bf16,2,1,3,3,3>', 7, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}),   # 224 pairs; 896 tiles
    Case('x2_planes', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), xpl=True, tie=True),
    Case('x2_bias_act_sign', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (5, 30, 256), env={'SG_FWD_NO_3P': 1}, bias=True, act=True, sign=True),
    Case('x2_dgrad_mask', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, flip=True, mask=True),
    Case('x2_ups', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, ups=True),
    Case('x2_ups_sign', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, ups=True, bias=True, act=True, sign=True),
    Case('x2_in_mask_mask', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, ups=True, in_gain=0.125, mask=True),
    Case('x2_in_mask', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, ups=True, in_gain=1.0),
]

# ----------------------------------------------------------------------------------------------------------------------
# conv_fwd3r<T,2,GC,KD,KH,KW> (launch_fwd3r): >= 512 tiles of 256 voxels.  bf16 3x3x3 shapes stay off conv_fwd3w / conv_fwd3s with
# W = 40 (32-wide tiles, the second 8 wide); f32 has no sliding-halo kernel.  GC = nchunk: bf16 cin 32 | 16, f32 cin 16 | 8.
# All eight instantiations.
# ----------------------------------------------------------------------------------------------------------------------
FWD3R = [
    Case('3r_f32_333_gc2_512_tiles', 'conv_fwd3r<f32,2,2,3,3,3>', 2, 16, 32, (16, 64, 64), dt=F32),
    Case('3r_f32_333_496_tiles', 'conv_fwd2<f32,2,1,2>', 2, 16, 32, (16, 62, 64), dt=F32),       # one H tile row fewer: 496 < 512
    Case('3r_f32_333_gc1', 'conv_fwd3r<f32,2,1,3,3,3>', 2, 8, 40, (16, 64, 64), dt=F32, bias=True, act=True, sign=True),
    Case('3r_bf16_333_gc2_W40', 'conv_fwd3r<bf16,2,2,3,3,3>', 2, 32, 32, (16, 64, 40), tie=True),
    Case('3r_bf16_333_gc1_W40', 'conv_fwd3r<bf16,2,1,3,3,3>', 2, 16, 64, (16, 64, 40), flip=True, mask=True),
    Case('3r_bf16_133_gc2', 'conv_fwd3r<bf16,2,2,1,3,3>', 8, 32, 32, (1, 128, 128), k=K133, tie=True),
    Case('3r_bf16_133_gc1', 'conv_fwd3r<bf16,2,1,1,3,3>', 8, 16, 32, (1, 128, 128), k=K133, bias=True, act=True, sign=True),
    Case('3r_f32_133_gc2', 'conv_fwd3r<f32,2,2,1,3,3>', 8, 16, 32, (1, 128, 128), k=K133, dt=F32),
    Case('3r_f32_133_gc1', 'conv_fwd3r<f32,2,1,1,3,3>', 8, 8, 32, (1, 128, 128), k=K133, dt=F32, flip=True, mask=True),
    Case('3r_bf16_133_480_tiles', 'conv_fwd2<bf16,2,1,2>', 8, 32, 32, (1, 120, 128), k=K133),      # 8 x 15 x 4 tiles of 1 x 8 x 32 < 512
    Case('3r_bf16_133_W96', 'conv_fwd3r<bf16,2,2,1,3,3>', 11, 32, 32, (1, 128, 96), k=K133, tie=True),   # nTw = 3: 11 x 16 x 3 = 528 tiles
    Case('3r_f32_333_W96', 'conv_fwd3r<f32,2,2,3,3,3>', 2, 16, 32, (16, 64, 96), dt=F32),             # nTw = 3: 768 tiles
]

# ----------------------------------------------------------------------------------------------------------------------
# conv_fwd5 (launch_fwd5): bf16, 3x3x3, cin % 16 = 0, cout % 64 = 0, 256-voxel tiles 32 wide with even TH, ntiles >= 2 gx with
# gx = (256 / (cout / 64)) / 8 * 8.  48 input channels are three chunks: neither conv_fwd3s nor conv_fwd3r has that form.
# ----------------------------------------------------------------------------------------------------------------------
FWD5 = [
    Case('5_engaging_edge', 'conv_fwd5<bf16,2,2,3,3,3>', 1, 48, 256, (8, 32, 128), tie=True),      # 128 tiles = 2 gx, gx = 64
    Case('5_96_tiles', 'conv_fwd2<bf16,2,2,2>', 1, 48, 256, (8, 32, 96)),                         # 96 < 128; 96 x 4 slice pairs = 384 blocks
    Case('5_ragged', 'conv_fwd5<bf16,2,2,3,3,3>', 1, 48, 256, (9, 30, 160), bias=True, act=True, sign=True),
    Case('5_dgrad_mask', 'conv_fwd5<bf16,2,2,3,3,3>', 1, 48, 256, (8, 32, 128), flip=True, mask=True),
    Case('5_pool2', 'conv_fwd5<bf16,2,2,3,3,3>', 1, 48, 256, (8, 32, 128), bias=True, act=True, pool=2),
    Case('5_pool2_sign', 'conv_fwd5<bf16,2,2,3,3,3>', 1, 48, 256, (8, 32, 128), bias=True, act=True, pool=2, sign=True),
    Case('5_pool2_dgrad', 'conv_fwd5<bf16,2,2,3,3,3>', 1, 64, 256, (8, 32, 128), flip=True, pool=2, tie=True),
]

# ----------------------------------------------------------------------------------------------------------------------
# conv_fwd4<T,2,NTB,KD,KH,KW> (launch_fwd4) with SG_FWD4_GX=8: ntiles >= 2 gx = 16 (1x3x3: 4 gx = 32).  NTB = 2 where cout > 32 and
# the tile is 32 wide with even TH (or 16 wide with TH % 4 = 0: the RS = 2 form, same name); one sub-pixel parity class is the
# 2x2x2 form with out_scale = 2.
# ----------------------------------------------------------------------------------------------------------------------
G8 = {'SG_FWD4_GX': 8}
FWD4 = [
    Case('4_333_ntb2_16_tiles', 'conv_fwd4<bf16,2,2,3,3,3>', 1, 48, 64, (4, 32, 32), env=G8, tie=True),
    Case('4_333_15_tiles', 'conv_fwd2<bf16,1,1,2>', 1, 48, 64, (4, 30, 32), env=G8),
    Case('4_333_ntb1', 'conv_fwd4<bf16,2,1,3,3,3>', 1, 48, 32, (5, 30, 64), env=G8, bias=True, act=True, sign=True),
    Case('4_333_ntb2_ragged_cout96', 'conv_fwd4<bf16,2,2,3,3,3>', 2, 40, 96, (5, 30, 64), env=G8, flip=True, mask=True),
    Case('4_333_no_wres', 'conv_fwd4<bf16,2,2,3,3,3>', 1, 48, 64, (4, 32, 32), env={'SG_FWD4_GX': 8, 'SG_FWD4_NO_WRES': 1}, tie=True),
    Case('4_333_w16', 'conv_fwd4<bf16,2,2,3,3,3>', 4, 48, 64, (4, 16, 16), env=G8, tie=True),       # tiles 2 x 8 x 16: the RS = 2 form
    Case('4_333_ups', 'conv_fwd4<bf16,2,2,3,3,3>', 1, 48, 64, (4, 32, 32), env=G8, ups=True, tie=True),
    Case('4_133_ntb2_32_tiles', 'conv_fwd4<bf16,2,2,1,3,3>', 1, 48, 64, (1, 64, 128), k=K133, env=G8, tie=True),
    Case('4_133_ntb1', 'conv_fwd4<bf16,2,1,1,3,3>', 1, 48, 32, (1, 64, 128), k=K133, env=G8, bias=True, act=True, sign=True),
    Case('4_f32_333_ntb2', 'conv_fwd4<f32,2,2,3,3,3>', 1, 20, 64, (4, 32, 32), dt=F32, env=G8),     # 20 channels: the third chunk half filled
    Case('4_f32_333_ntb1', 'conv_fwd4<f32,2,1,3,3,3>', 1, 24, 32, (4, 32, 32), dt=F32, env=G8, flip=True, mask=True),
    Case('4_f32_133_ntb2', 'conv_fwd4<f32,2,2,1,3,3>', 1, 24, 64, (1, 64, 128), k=K133, dt=F32, env=G8),
    Case('4_f32_133_ntb1', 'conv_fwd4<f32,2,1,1,3,3>', 1, 24, 32, (1, 64, 128), k=K133, dt=F32, env=G8, bias=True, act=True, sign=True),
    Case('4_333_W96', 'conv_fwd4<bf16,2,2,3,3,3>', 1, 48, 64, (4, 32, 96), env=G8, tie=True),        # nTw = 3: 48 tiles
    Case('4_333_batch_folded', 'conv_fwd4<bf16,2,1,3,3,3>', 64, 48, 64, (2, 4, 8), env=G8, tie=True),   # 64 voxels a sample: TN = 4, 16 tiles
    Case('4_133_28_tiles', 'conv_fwd2<bf16,1,1,2>', 1, 48, 64, (1, 56, 128), k=K133, env=G8),         # 7 x 4 = 28 < 4 gx = 32
    # tap_off and out_off are separate fields: the class image of taps (0, 1, 1) scattered to the voxels of class (1, 0, 0)
    Case('4_222_tap_011_out_100', 'conv_fwd4<bf16,2,2,2,2,2>', 1, 64, 64, (4, 32, 32), k=K222, env=G8, par=(0, 1, 1), out_off=(1, 0, 0), tie=True),
    Case('4_222_class_010_ntb2', 'conv_fwd4<bf16,2,2,2,2,2>', 1, 64, 64, (4, 32, 32), k=K222, env=G8, par=(0, 1, 0), coef=1.0, tie=True),
    Case('4_222_class_101_ntb1', 'conv_fwd4<bf16,2,1,2,2,2>', 1, 64, 32, (4, 32, 32), k=K222, env=G8, par=(1, 0, 1), bias=True, act=True),
    Case('4_f32_222_class_111_ntb2', 'conv_fwd4<f32,2,2,2,2,2>', 1, 32, 64, (4, 32, 32), k=K222, dt=F32, env=G8, par=(1, 1, 1)),
    Case('4_f32_222_class_000_ntb1', 'conv_fwd4<f32,2,1,2,2,2>', 1, 32, 32, (4, 32, 32), k=K222, dt=F32, env=G8, par=(0, 0, 0), bias=True, act=True),
]

# ----------------------------------------------------------------------------------------------------------------------
# conv_fwd2<T,MTW,NTB,GC> and conv_fwd<T,2,NTB>: the register tile (MTW x 128 voxels, NTB 32-channel slices) is the first of
# (2,4) (2,2) (2,1) (1,2) (1,1) with >= 384 blocks, else the one with the most blocks (the first of equals); NTB = 4 needs three
# slices, NTB = 2 two.  GC = 4 with >= 4 chunks and <= 9 taps (not on 2 x 4), else 2 with >= 2 chunks, else 1.  conv_fwd: cin * es
# no multiple of 16, or SG_FWD_V1=1.  SG_FWD_NO_V3 / NO_V4 / NO_V5 keep the persistent kernels off the large shapes.
# Every reachable instantiation is in the table: 2 x 14 of conv_fwd2, 2 x 3 of conv_fwd.
# ----------------------------------------------------------------------------------------------------------------------
NOP = {'SG_FWD_NO_V3': 1, 'SG_FWD_NO_V4': 1, 'SG_FWD_NO_V5': 1}
# (MTW, NTB): n, cout, 3x3x3 extent, 1x3x3 extent, switches
_TILE = {
    (1, 1): (2, 32, (4, 8, 8), (1, 16, 16), None),        # 4 tiles of 128 voxels against 2 of 256
    (2, 1): (1, 32, (2, 4, 8), (1, 8, 8), None),          # 64 voxels: one tile either way, and (2,1) comes first
    (2, 2): (24, 64, (4, 32, 32), (1, 64, 64), NOP),      # 24 x 16 tiles of 256 = 384 blocks of two slices
    (2, 4): (24, 128, (4, 32, 32), (1, 64, 64), NOP),     # 384 blocks of four slices
    (1, 2): (25, 96, (4, 8, 32), (1, 32, 32), NOP),       # three slices: (2,1) has 100 x 3 = 300 blocks, (1,2) 200 x 2 = 400
}
_EPI = [dict(), dict(bias=True, act=True, sign=True), dict(flip=True, mask=True)]
FWD2 = []
for _dt_ in (BF, F32):
    _t, _ch = ('bf16', 16) if _dt_ == BF else ('f32', 8)
    for (_m, _n), (_nb, _co, _sp3, _sp1, _env) in _TILE.items():
        for _gc in (1, 2, 4):
            if _gc == 4 and (_m, _n) == (2, 4):
                continue
            # GC = 1: one chunk; 2: a whole and a half-filled chunk; 4: four chunks under 9 taps
            _cin = {1: _ch, 2: _ch + _ch // 2, 4: 4 * _ch}[_gc]
            FWD2.append(Case(f'2_{_t}_{_m}{_n}_gc{_gc}', f'conv_fwd2<{_t},{_m},{_n},{_gc}>', _nb, _cin, _co, _sp1 if _gc == 4 else _sp3,
                             k=K133 if _gc == 4 else K333, dt=_dt_, env=_env, tie=(_dt_ == BF and _gc > 1), **_EPI[len(FWD2) % 3]))
FWD2 += [
    Case('2_11_gc2_ragged', 'conv_fwd2<bf16,1,1,2>', 2, 24, 40, (3, 5, 7)),
    Case('2_21_gc1_batch_folded', 'conv_fwd2<bf16,2,1,1>', 4, 16, 32, (2, 4, 4)),                  # TN = 4 (128 voxels in all)
    Case('1_bf16_cin6', 'conv_fwd<bf16,2,1>', 2, 6, 10, (3, 5, 7), bias=True, act=True, sign=True),   # 105 voxels a sample: TN = 2
    Case('1_bf16_batch_folded', 'conv_fwd<bf16,2,1>', 4, 6, 10, (2, 4, 4)),                          # 32 voxels a sample: TN = 4
    Case('1_f32_cin3', 'conv_fwd<f32,2,1>', 2, 3, 10, (3, 5, 7), dt=F32, flip=True, mask=True),
    Case('1_bf16_v1_switch', 'conv_fwd<bf16,2,1>', 1, 32, 32, (2, 4, 8), env={'SG_FWD_V1': 1}, tie=True),
    Case('1_bf16_ntb2', 'conv_fwd<bf16,2,2>', 24, 6, 40, (4, 32, 32)),                             # 384 tiles, two slices
    Case('1_bf16_ntb4', 'conv_fwd<bf16,2,4>', 24, 6, 72, (4, 32, 32), flip=True, mask=True),       # three slices: cout >= 65
    Case('1_f32_ntb2', 'conv_fwd<f32,2,2>', 24, 3, 40, (4, 32, 32), dt=F32, bias=True, act=True, sign=True),
    Case('1_f32_ntb4', 'conv_fwd<f32,2,4>', 24, 3, 72, (4, 32, 32), dt=F32),
]

# ----------------------------------------------------------------------------------------------------------------------
# conv_gemm (gemm_plan, gemm.hip:277): bf16, cin >= 64, cout % 64 = 0, H, W <= 16.  1x3x3 on volumes of <= 128 voxels with
# cin >= 128: tiles of 256 voxels over the folded batch, K split while tiles x ks < 192.  3x3x3 at 16 x 16 planes with
# n d 256 <= 8192.  conv_small_fwd (sg_small_eligible): D = 1, 1x3x3, channels in {4, 8, 16}, n h w >= 65536.
# Pointwise: pw_fwd_small_cin (cin <= 4), pw_fwd_small_cout (cout <= 4), dense_small_m (<= 128 voxels, >= 64 chunks).
# ----------------------------------------------------------------------------------------------------------------------
OTHER = [
    Case('gemm_133_192_tiles', 'conv_gemm', 384, 128, 128, (2, 8, 8), k=K133, tie=True),              # 384 / 2 samples per tile = 192
    Case('gemm_133_191_tiles', 'conv_gemm (K split)', 382, 128, 128, (2, 8, 8), k=K133, tie=True),
    Case('gemm_133_ksplit_bias_act_sign', 'conv_gemm (K split)', 3, 128, 192, (2, 8, 8), k=K133, bias=True, act=True, sign=True),
    Case('gemm_133_ksplit_dgrad_mask', 'conv_gemm (K split)', 5, 192, 128, (1, 4, 4), k=K133, flip=True, mask=True),
    Case('gemm_333_ksplit', 'conv_gemm (K split)', 2, 64, 64, (3, 16, 16), tie=True),
    Case('gemm_333_ksplit_ups', 'conv_gemm (K split)', 1, 64, 64, (4, 16, 16), ups=True, bias=True, act=True, sign=True),
    Case('gemm_no_workspace_declines', 'conv_fwd2<bf16,1,1,2>', 2, 64, 64, (3, 16, 16), ws=False),
    Case('small_bf16', 'conv_small_fwd<bf16>', 1, 16, 8, (1, 256, 256), k=K133, bias=True, act=True, sign=True),
    Case('small_f32', 'conv_small_fwd<f32>', 1, 8, 16, (1, 256, 256), k=K133, dt=F32, flip=True, mask=True),
    Case('small_bf16_4to16', 'conv_small_fwd<bf16>', 2, 4, 16, (1, 128, 256), k=K133),
    Case('small_one_row_fewer', 'conv_fwd2<bf16,1,1,1>', 1, 16, 8, (1, 254, 256), k=K133),          # 65024 voxels < 65536
    Case('pw_cin1_bf16', 'pw_fwd_small_cin<bf16>', 2, 1, 32, (3, 5, 7), k=K111, bias=True, act=True, sign=True),
    Case('pw_cin3_f32', 'pw_fwd_small_cin<f32>', 2, 3, 16, (3, 5, 7), k=K111, dt=F32, bias=True),
    Case('pw_cin2_bf16_two_trips', 'pw_fwd_small_cin<bf16>', 1, 2, 64, (4, 40, 64), k=K111, mask=True),
    Case('pw_cin4_bf16', 'pw_fwd_small_cin<bf16>', 2, 4, 128, (3, 5, 7), k=K111),
    Case('pw_cout1_bf16', 'pw_fwd_small_cout<bf16>', 2, 512, 1, (3, 5, 7), k=K111, bias=True, tie=True),
    Case('pw_cout3_f32', 'pw_fwd_small_cout<f32>', 2, 32, 3, (3, 5, 7), k=K111, dt=F32, flip=True),
    Case('dense_small_m_bf16', 'dense_small_m<bf16>', 5, 1024, 96, (1, 1, 1), k=K111, bias=True, act=True, tie=True),
    Case('dense_small_m_f32', 'dense_small_m<f32>', 128, 512, 40, (1, 1, 1), k=K111, dt=F32),
    Case('dense_small_m_129_voxels', 'conv_fwd2<bf16,1,1,4>', 129, 1024, 96, (1, 1, 1), k=K111, tie=True),   # nvox > 128
]

ROUTES = FWD3W + FWD3S + P64 + FWD3R + FWD5 + FWD4 + FWD2 + OTHER
assert len({c.id for c in ROUTES}) == len(ROUTES)


@pytest.mark.parametrize('c', ROUTES, ids=[c.id for c in ROUTES])
def test_route_is_exact(c, sg_env):
    _run_exact(c, sg_env)


# ----------------------------------------------------------------------------------------------------------------------
# pixel_norm: inside the bound tests/gref.py derives above pn_check (shared with tests/test_autograd_gen_exact_gpu.py).
# ----------------------------------------------------------------------------------------------------------------------
PN = [
    Case('pn_3w', 'conv_fwd3w<bf16,32->32>', 2, 32, 32, (5, 20, 64), bias=True, act=True, sign=True, pn=True),
    Case('pn_3p16', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (5, 30, 96), bias=True, act=True, pn=True),
    Case('pn_3p', 'conv_fwd3p<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, bias=True, act=True, sign=True, pn=True, env={'SG_FWD3P_16': 0}),
    Case('pn_x2', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, bias=True, act=True, sign=True, pn=True),
    Case('pn_5', 'conv_fwd5<bf16,2,2,3,3,3>', 2, 48, 64, (16, 64, 64), bias=True, act=True, pn=True),           # 512 tiles = 2 gx, gx = 256
    Case('pn_4', 'conv_fwd4<bf16,2,2,3,3,3>', 1, 48, 64, (4, 32, 32), env=G8, bias=True, act=True, sign=True, pn=True),
    Case('pn_2_f32', 'conv_fwd2<f32,2,1,2>', 1, 12, 24, (2, 4, 8), dt=F32, bias=True, act=True, pn=True),
    Case('pn_2_bf16', 'conv_fwd2<bf16,1,2,2>', 2, 24, 40, (3, 5, 7), bias=True, act=True, sign=True, pn=True),   # both slices in the block
    Case('pn_1_bf16', 'conv_fwd<bf16,2,1>', 2, 6, 10, (3, 5, 7), bias=True, act=True, sign=True, pn=True),
    Case('pn_3r_f32', 'conv_fwd3r<f32,2,2,3,3,3>', 2, 16, 32, (16, 64, 64), dt=F32, bias=True, act=True, pn=True),
    Case('pn_3s', 'conv_fwd3s<bf16,2>', 8, 24, 32, (4, 32, 256), bias=True, act=True, sign=True, pn=True),         # 256 column pairs = gx
    Case('pn_small', 'conv_small_fwd<bf16>', 1, 16, 8, (1, 256, 256), k=K133, bias=True, act=True, pn=True),
    # the remaining PN / PN|SIGN entries of the launchers' epilogue tables
    Case('pn_3w_no_sign', 'conv_fwd3w<bf16,32->32>', 2, 32, 32, (5, 20, 64), bias=True, act=True, pn=True),
    Case('pn_5_sign', 'conv_fwd5<bf16,2,2,3,3,3>', 2, 48, 64, (16, 64, 64), bias=True, act=True, sign=True, pn=True),
    Case('pn_3s_no_sign', 'conv_fwd3s<bf16,2>', 8, 24, 32, (4, 32, 256), bias=True, act=True, pn=True),
    Case('pn_x2_no_sign', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, bias=True, act=True, pn=True),
    Case('pn_x2_ups', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, ups=True, bias=True, act=True, pn=True),
    Case('pn_x2_ups_sign', 'conv_fwd3s<bf16,2> x2 (K split)', 8, 64, 32, (4, 32, 256), env={'SG_FWD_NO_3P': 1}, ups=True, bias=True, act=True,
         sign=True, pn=True),
    Case('pn_3p16_sign', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (5, 30, 96), bias=True, act=True, sign=True, pn=True),
    Case('pn_3p16_ups', 'conv_fwd3p16<bf16,64->32>', 2, 64, 32, (6, 28, 64), ups=True, bias=True, act=True, pn=True),
]


_pn_check = G.pn_check


@pytest.mark.parametrize('c', PN, ids=[c.id for c in PN])
def test_pixel_norm_within_derived_bound(c, sg_env):
    _lib, _ = _libs()
    d = _case_data(c)
    if c.env:
        sg_env(**c.env)
    rc, names, y, signs, scale = _launch(c, d)
    _lib.check(rc, c.id)
    assert names == [c.kernel], (c.id, names)
    _pn_check(c.id, y, scale, d['pre'], c.dt, c.cout)
    if c.sign:      # the signs of bias + act, which the positive factor does not change
        _assert_equal(c.id, signs, R.sign_words(d['pre']), 'sign words')


def test_rgb_head_on_the_stored_pixel_normed_output():
    """rgb_out (conv3w.hip:585-610): sum_c y[c] * rgb_w[c] + rgb_bias over y AS STORED, so the reference is taken from the bf16 y the
    same call wrote (itself under the pixel-norm bound).  y is pixel-normed, so the sum belongs with the tolerance cases: 32 exact
    products (integer rgb_w) added by 8 FMAs per lane, 2 quad additions and the bias add, 11 roundings of partial sums no larger
    than sum |y rgb_w| + |b|, then the one bf16 rounding."""
    _lib, _ = _libs()
    c = Case('rgb_3w', 'conv_fwd3w<bf16,32->32>', 2, 32, 32, (5, 20, 64), bias=True, act=True, sign=True, pn=True)
    d = _case_data(c)
    g = torch.Generator().manual_seed(9)
    rgb_w = torch.randint(-3, 4, (32,), generator=g).float().to(dev())
    rgb_b = torch.tensor([2.0], device=dev())
    rgb = torch.full((c.n, 1, *c.sp), SENTINEL, dtype=BF, device=dev())
    rc, names, y, signs, scale = _launch(c, d, _set(rgb_w=rgb_w.data_ptr(), rgb_bias=rgb_b.data_ptr(), rgb_out=rgb.data_ptr()))
    _lib.check(rc, c.id)
    assert names == [c.kernel], names
    _pn_check(c.id, y, scale, d['pre'], BF, 32)
    _assert_equal(c.id, signs, R.sign_words(d['pre']), 'sign words')
    ref = R.rgb_head(y, rgb_w, 2.0)
    bound = G.rgb_bound(y, rgb_w, 2.0, ref)
    err = (rgb.double() - ref).abs()
    assert bool((err <= bound).all())


# ----------------------------------------------------------------------------------------------------------------------
# Sub-pixel up-convolution (subpix.hip): s is the LOW-resolution shape; tiles of 256 low-resolution voxels, 2 x 4 x 32, 2 x 8 x 16
# or 4 x 8 x 8, the volume in whole tiles.  The packers sum up to 8 integer weights times coef before the one bf16 rounding: at
# most 24 units, exact.  upconv_subpixel_fwd: the persistent kernel; <one tile per block> behind SG_DBG_FLAGS=64; <2 N tiles> is
# pixel_norm over 64 channels.  upconv_subpixel_dgrad: cin % 64 = 0, cout % 16 = 0, tiles 2 x 4 x 32 or 2 x 8 x 16.
# ----------------------------------------------------------------------------------------------------------------------
class Sub:
    def __init__(self, cid, kernel, n, cin, cout, sp, env=None, bias=False, act=False, sign=False, pn=False, dgrad=False):
        self.id, self.kernel, self.n, self.cin, self.cout, self.sp, self.env = cid, kernel, n, cin, cout, tuple(sp), env or {}
        self.bias, self.act, self.sign, self.pn, self.dgrad = bias, act, sign, pn, dgrad


SUBPIX = [
    Sub('sub_one_tile', 'upconv_subpixel_fwd', 1, 16, 32, (2, 4, 32)),
    Sub('sub_seams_all_round', 'upconv_subpixel_fwd', 2, 48, 96, (6, 12, 96), bias=True, act=True, sign=True),    # 3 x 3 x 3 tiles
    Sub('sub_w16', 'upconv_subpixel_fwd', 2, 64, 32, (4, 16, 16)),                                                # tiles 2 x 8 x 16
    Sub('sub_w8', 'upconv_subpixel_fwd', 3, 32, 64, (8, 8, 8), bias=True, act=True, sign=True),                   # tiles 4 x 8 x 8
    Sub('sub_one_tile_per_block', 'upconv_subpixel_fwd<one tile per block>', 2, 48, 96, (4, 8, 64), env={'SG_DBG_FLAGS': 64},
        bias=True, act=True, sign=True),
    Sub('sub_pn32', 'upconv_subpixel_fwd', 2, 64, 32, (4, 8, 64), bias=True, act=True, sign=True, pn=True),
    Sub('sub_pn64_two_tiles', 'upconv_subpixel_fwd<2 N tiles>', 2, 32, 64, (4, 8, 64), bias=True, act=True, sign=True, pn=True),
    Sub('subdg_one_tile', 'upconv_subpixel_dgrad', 1, 64, 16, (2, 4, 32), dgrad=True),
    Sub('subdg_seams_all_round', 'upconv_subpixel_dgrad', 2, 128, 48, (6, 12, 96), dgrad=True),                   # two 64-channel parts
    Sub('subdg_w16', 'upconv_subpixel_dgrad', 3, 64, 32, (4, 16, 16), dgrad=True),
]


SUB_COEF = 0.25


def sub_reference(c, device, samples=None):
    """(x, gy, w, bias, exact fp64 result) of sub-pixel case c on `device`: the forward's bias + act output, or for a dgrad
    case the gradient for x.  samples: the reference of the first samples only (samples are independent)."""
    seed = 5000 + 7 * c.cin + 3 * c.cout + c.sp[0] + 5 * c.sp[1] + 11 * c.sp[2] + c.n
    fine = tuple(2 * v for v in c.sp)
    w = W.int_data((3, 3, 3, c.cin, c.cout), seed + 1, F32).contiguous().to(device)
    if c.dgrad:
        gy = W.int_data((c.n, c.cout, *fine), seed, BF).to(device)
        return None, gy, w, None, R.dgrad_ref(gy[:samples], w.double() * SUB_COEF, ups=True)
    x = W.int_data((c.n, c.cin, *c.sp), seed, BF).to(device)
    g = torch.Generator().manual_seed(seed + 2)
    bias = torch.randint(-3, 4, (c.cout,), generator=g).float().to(device) if c.bias else None
    return x, None, w, bias, R.bias_act(R.conv_ref(x[:samples], w.double() * SUB_COEF, ups=True), bias, 0.25 if c.act else None)


@pytest.mark.parametrize('c', SUBPIX, ids=[c.id for c in SUBPIX])
def test_subpixel_route_is_exact(c, sg_env):
    """conv3d(upscale3d(x)) and its data gradient in sub-pixel form against the plain formulation: the 27-tap convolution of the
    nearest-x2 input, and the 2x2x2 block sum of the flipped-filter convolution of the fine gradient (both exact here).  At
    32 input channels the 8 x 8 x 32 products of a fine voxel's sum reach well past 256 units: ties asserted."""
    _lib, lib = _libs()
    coef = SUB_COEF
    fine = tuple(2 * v for v in c.sp)
    x, gy, w, bias, ref = sub_reference(c, dev())
    shp = _lib.ConvShape(c.n, *c.sp, c.cin, c.cout, 3, 3, 3, 0)
    if c.env:
        sg_env(**c.env)
    W.assert_exact_range(9 * coef, coef * 0.25, 27 * 8 * max(c.cin, c.cout) + 1)
    if c.dgrad:
        assert lib.sg_upconv3d_subpixel_dgrad_supported(C.byref(shp), _lib.SG_BF16)
        wp = _garbage(lib.sg_upconv3d_subpixel_dgrad_packed_bytes(C.byref(shp), _lib.SG_BF16))
        _lib.check(lib.sg_upconv3d_subpixel_dgrad_pack(w.data_ptr(), coef, wp.data_ptr(), C.byref(shp), _lib.SG_BF16, _stream()), 'pack')
        gx = _ndhwc(torch.full((c.n, c.cin, *c.sp), SENTINEL, dtype=BF, device=dev()))
        lib.sg_prof_enable(1)
        try:
            rc = lib.sg_upconv3d_subpixel_dgrad(_ndhwc(gy).data_ptr(), wp.data_ptr(), gx.data_ptr(), C.byref(shp), _lib.SG_BF16, _stream())
            torch.cuda.synchronize()
            names = _fwd_kernels(_lib, lib)
        finally:
            lib.sg_prof_enable(0)
        _lib.check(rc, c.id)
        assert names == [c.kernel], (c.id, names)
        assert R.bf16_ties(ref) > 0, f'{c.id}: the reference holds no bf16 rounding tie'
        _assert_equal(c.id, gx, R.expected(ref, BF), 'gx')
        return
    assert lib.sg_upconv3d_subpixel_supported(C.byref(shp), _lib.SG_BF16)
    pre = ref
    wp = _garbage(lib.sg_upconv3d_subpixel_packed_bytes(C.byref(shp), _lib.SG_BF16))
    _lib.check(lib.sg_upconv3d_subpixel_pack(w.data_ptr(), coef, wp.data_ptr(), C.byref(shp), _lib.SG_BF16, _stream()), 'pack')
    y = _ndhwc(torch.full((c.n, c.cout, *fine), SENTINEL, dtype=BF, device=dev()))
    nvox = c.n * fine[0] * fine[1] * fine[2]
    signs = torch.full((nvox, c.cout // 32), 0x5A5A5A5A, dtype=torch.int32, device=dev()) if c.sign else None
    scale = torch.full((nvox,), SENTINEL, dtype=F32, device=dev()) if c.pn else None
    ep = _lib.ConvEpilogue()
    if bias is not None:
        ep.bias = bias.data_ptr()
    ep.act, ep.slope = (1, 0.25) if c.act else (0, 0.0)
    if c.pn:
        ep.pixel_norm, ep.eps, ep.pn_scale = 1, 1e-8, scale.data_ptr()
    if signs is not None:
        ep.sign_out = signs.data_ptr()
    lib.sg_prof_enable(1)
    try:
        rc = lib.sg_upconv3d_subpixel_fwd(_ndhwc(x).data_ptr(), wp.data_ptr(), y.data_ptr(), C.byref(shp), C.byref(ep), _lib.SG_BF16, _stream())
        torch.cuda.synchronize()
        names = _fwd_kernels(_lib, lib)
    finally:
        lib.sg_prof_enable(0)
    _lib.check(rc, c.id)
    assert names == [c.kernel], (c.id, names)
    if c.pn:
        _pn_check(c.id, y, scale, pre, BF, c.cout)
    else:
        if c.cin >= 32:
            assert R.bf16_ties(pre) > 0, f'{c.id}: the reference holds no bf16 rounding tie'
        _assert_equal(c.id, y, R.expected(pre, BF))
    if c.sign:
        _assert_equal(c.id, signs, R.sign_words(pre), 'sign words')


def test_pack_weights_batch_writes_the_bytes_of_the_single_calls():
    """sg_conv3d_pack_weights_batch on three layers (one with the second, 16x16x32 fragment image of conv_fwd3w, one packed with
    transpose_flip, one small-channel layer with its f32 tail): byte for byte what three sg_conv3d_pack_weights calls write."""
    _lib, lib = _libs()
    cases = [Case('a', '', 1, 32, 64, (4, 16, 32)), Case('b', '', 1, 40, 24, (3, 5, 7), flip=True, coef=0.5),
             Case('c', '', 1, 16, 8, (1, 256, 256), k=K133)]
    ws = [W.int_data((*c.k, c.cout, c.cin) if c.flip else (*c.k, c.cin, c.cout), 70 + i, F32).contiguous().to(dev()) for i, c in enumerate(cases)]
    single = [_pack(c, w) for c, w in zip(cases, ws)]
    batch = [_garbage(s.numel()) for s in single]
    n = len(cases)
    shapes = (_lib.ConvShape * n)(*[_shape(c) for c in cases])
    rc = lib.sg_conv3d_pack_weights_batch(n, (C.c_void_p * n)(*[w.data_ptr() for w in ws]), (C.c_float * n)(*[c.coef for c in cases]),
                                          (C.c_int * n)(*[1 if c.flip else 0 for c in cases]), (C.c_void_p * n)(*[b.data_ptr() for b in batch]),
                                          shapes, _lib.SG_BF16, _stream())
    _lib.check(rc, 'batch')
    torch.cuda.synchronize()
    for c, s, b in zip(cases, single, batch):
        nb = lib.sg_conv3d_packed_bytes(C.byref(_shape(c)), _lib.SG_BF16)
        assert torch.equal(s[:nb], b[:nb]), c.id


# ----------------------------------------------------------------------------------------------------------------------
# Refusals: the return code, no launch, and y (pre-filled with the sentinel) as it was.
# ----------------------------------------------------------------------------------------------------------------------
def _refused(c, code, tweak=None, shift=None):
    """shift: 'x' | 'wp' | 'y' -- that base pointer moved by one element (2 bytes: not 16-byte aligned)."""
    _lib, lib = _libs()
    d = case_reference(c, dev())
    if shift is None:
        rc, names, y, _, _ = _launch(c, d, tweak)
    else:
        shp, dt = _shape(c), _dt(c.dt)
        wp = _pack(c, d['w'])
        xb = _ndhwc(d['x'])
        y = _ndhwc(torch.full((c.n, c.cout, *c.sp), SENTINEL, dtype=c.dt, device=dev()))
        ptr = {'x': xb.data_ptr(), 'wp': wp.data_ptr(), 'y': y.data_ptr()}
        ptr[shift] += 2
        ep = _lib.ConvEpilogue()
        lib.sg_prof_enable(1)
        try:
            rc = lib.sg_conv3d_fwd(ptr['x'], ptr['wp'], ptr['y'], C.byref(shp), C.byref(ep), dt, _stream())
            torch.cuda.synchronize()
            names = _fwd_kernels(_lib, lib)
        finally:
            lib.sg_prof_enable(0)
    assert rc == code, (c.id, rc)
    assert names == [], (c.id, names)
    assert bool((y == SENTINEL).all()), f'{c.id}: a refused call wrote to y'


PLAIN = dict(n=1, cin=32, cout=32, sp=(4, 8, 32))


@pytest.mark.parametrize('which', ['x', 'wp', 'y'])
def test_refuses_a_misaligned_base(which):
    _refused(Case(f'misaligned_{which}', '', **PLAIN), SG_EALIGN, shift=which)


def _set(**kv):
    def tweak(ep):
        for k, v in kv.items():
            setattr(ep, k, v)
    return tweak


@pytest.mark.parametrize('delta', [-1, 1])
def test_refuses_another_struct_size(delta):
    _lib, _ = _libs()
    _refused(Case('struct_size', '', **PLAIN), SG_EINVAL, _set(struct_size=C.sizeof(_lib.ConvEpilogue) + delta))


@pytest.mark.parametrize('pool,dt,code', [(-1, BF, SG_EINVAL), (4, BF, SG_EINVAL), (1, F32, SG_EUNSUPPORTED), (2, F32, SG_EUNSUPPORTED),
                                          (3, F32, SG_EUNSUPPORTED)])
def test_refuses_pool_out_of_range_or_in_f32(pool, dt, code):
    _refused(Case('pool', '', dt=dt, **PLAIN), code, _set(pool=pool))


def test_refuses_a_masked_gather_whose_gain_is_no_power_of_two():
    c = Case('in_gain', '', 2, 64, 32, (6, 28, 64), ups=True, in_gain=0.125)
    _refused(c, SG_EUNSUPPORTED, _set(in_gain=0.3))


def test_refuses_a_masked_gather_on_a_layer_that_is_not_64_to_32():
    c = Case('in_mask_32to32', '', 2, 32, 32, (6, 28, 64), ups=True, in_gain=0.125)
    _refused(c, SG_EUNSUPPORTED)


def test_refuses_rgb_out_with_cin_other_than_32():
    c = Case('rgb_cin64', '', 1, 64, 32, (4, 8, 32), bias=True, act=True, sign=True, pn=True)
    rgb_w = torch.ones(32, device=dev())
    rgb = torch.full((4 * 8 * 32,), SENTINEL, dtype=BF, device=dev())
    _refused(c, SG_EUNSUPPORTED, _set(rgb_w=rgb_w.data_ptr(), rgb_out=rgb.data_ptr()))
    assert bool((rgb == SENTINEL).all())


@pytest.mark.parametrize('field', ['tap_off', 'out_off'])
def test_refuses_a_subpixel_offset_of_two(field):
    c = Case(field, '', 1, 64, 32, (4, 32, 32), k=K222, par=(0, 1, 0), env=G8)
    _refused(c, SG_EINVAL, _set(**{field: (C.c_int32 * 3)(0, 2, 0)}))


@pytest.mark.parametrize('xpl,code', [(16, SG_EINVAL), (64, SG_EINVAL), (32, SG_EUNSUPPORTED)])
def test_refuses_x_plane_channels_other_than_0_or_32_and_32_off_the_two_pass_path(xpl, code):
    """32 on a 32 -> 32 layer is a valid request that only the 64 -> 32 K split implements: SG_EUNSUPPORTED."""
    _refused(Case('xpl', '', **PLAIN), code, _set(x_plane_channels=xpl))


def test_refuses_pixel_norm_over_more_than_four_cout_tiles():
    scale = torch.zeros(4 * 8 * 32, device=dev())
    _refused(Case('pn_160', '', 1, 32, 160, (4, 8, 32)), SG_EINVAL, _set(pixel_norm=1, eps=1e-8, pn_scale=scale.data_ptr()))


@pytest.mark.parametrize('sp,cin', [((2, 4, 12), 16), ((3, 4, 32), 16), ((2, 4, 32), 24)])
def test_subpixel_forward_refuses_a_shape_it_does_not_tile(sp, cin):
    """W = 12 is none of the tile widths, D = 3 is no whole number of 2-plane tiles, 24 channels are no whole chunks."""
    _lib, lib = _libs()
    shp = _lib.ConvShape(1, *sp, cin, 32, 3, 3, 3, 0)
    assert not lib.sg_upconv3d_subpixel_supported(C.byref(shp), _lib.SG_BF16)
    x = W.int_data((1, cin, *sp), 1, BF).to(dev())
    wp = _garbage(max(lib.sg_upconv3d_subpixel_packed_bytes(C.byref(shp), _lib.SG_BF16), 16))
    y = _ndhwc(torch.full((1, 32, *(2 * v for v in sp)), SENTINEL, dtype=BF, device=dev()))
    ep = _lib.ConvEpilogue()
    lib.sg_prof_enable(1)
    try:
        rc = lib.sg_upconv3d_subpixel_fwd(_ndhwc(x).data_ptr(), wp.data_ptr(), y.data_ptr(), C.byref(shp), C.byref(ep), _lib.SG_BF16, _stream())
        torch.cuda.synchronize()
        names = _fwd_kernels(_lib, lib)
    finally:
        lib.sg_prof_enable(0)
    assert rc == SG_EUNSUPPORTED and names == [], (rc, names)
    assert bool((y == SENTINEL).all())
