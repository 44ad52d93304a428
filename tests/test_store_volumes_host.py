"""Host side of functional.store_volumes: the numpy twin against the reference's own expression and against direct
recomputations, its edge cases, every argument error, and the header against the ctypes binding.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tests import svref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def store(x, kind, **kw):
    from saragan_amd import functional as F
    return F.store_volumes(x, svref.T_OUT[kind] if isinstance(kind, str) else kind, **kw)


def test_twin_equals_the_reference_expression():
    """generate.py:149 of the reference: (np.clip(x, -1, 2) * 1024).astype(np.int16), for finite float32 input."""
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((3, 1, 4, 9, 11)) * 1.5).astype(np.float32)
    x.reshape(-1)[:12] = [-1.0, 2.0, np.nextafter(np.float32(-1), np.float32(-2)), np.nextafter(np.float32(2), np.float32(3)), 0.0, -0.0,
                          1e30, -1e30, 3.4e38, -3.4e38, 0.99951171875, -0.00048828125]
    got = store(torch.from_numpy(x), 'i16', scale=1024.0, shift=0.0, clip=(-1024, 2048), rounding='trunc')
    ref = (np.clip(x, -1, 2) * 1024).astype(np.int16)
    assert got.dtype == torch.int16 and got.shape == x.shape
    assert np.array_equal(got.numpy(), ref)
    assert ref.min() == -1024 and ref.max() == 2048


def test_ties_and_negative_values():
    t = np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5, -2.75, -0.25, 0.25, 2.75, -0.0, 0.0], np.float32)
    x = torch.from_numpy(t).reshape(1, 1, 1, 1, -1)
    tr = store(x, 'i16', rounding='trunc').numpy().reshape(-1)
    ri = store(x, 'i16', rounding='rint').numpy().reshape(-1)
    assert tr.tolist() == [-2, -1, 0, 0, 1, 2, 3, -2, 0, 0, 2, 0, 0]                 # toward zero, as .astype
    assert ri.tolist() == [-2, -2, 0, 0, 2, 2, 4, -3, 0, 0, 3, 0, 0]                 # ties to even
    # an unsigned type clips the negative ones first: nothing wraps
    assert store(x, 'u8', rounding='rint').numpy().reshape(-1).tolist() == [0, 0, 0, 0, 2, 2, 4, 0, 0, 0, 3, 0, 0]
    # scale and shift: two float32 roundings, then the tie
    got = store(torch.tensor([0.00048828125, -0.99951171875]).reshape(1, 1, 1, 1, 2), 'u16', scale=1024.0, shift=1024.0, rounding='rint')
    assert got.numpy().reshape(-1).tolist() == [1024, 0]                              # 1024.5 -> 1024 (even), 0.5 -> 0


@pytest.mark.parametrize('out', ['i16', 'u16', 'u8', 'f32'])
def test_nan_and_infinities_and_their_counts(out):
    x = torch.tensor([np.nan, np.inf, -np.inf, 1e10, -1e10, 5.0, np.nan, 7.25]).reshape(2, 1, 1, 1, 4)
    clip = {'i16': (-100, 100), 'u16': (2, 100), 'u8': (2, 100), 'f32': (-100.5, 100.5)}[out]
    got, st = store(x, out, clip=clip, stats=True)
    lo, hi = clip
    g = got.numpy().reshape(2, 4)
    if out == 'f32':
        assert np.isnan(g[0, 0]) and np.isnan(g[1, 2]) and g[0, 0].view(np.uint32) == 0x7FC00000
        assert g[0, 1:].tolist() == [hi, lo, hi] and g[1, [0, 1, 3]].tolist() == [lo, 5.0, 7.25]
        assert st[:, :4].eq(0).all()
    else:
        assert g.tolist() == [[lo, hi, lo, hi], [lo, 5, lo, 7]]                         # a NaN is stored as lo
        assert st[:, :4].tolist() == [[2 * lo + 2 * hi, 2 * lo * lo + 2 * hi * hi, lo, hi], [2 * lo + 12, 2 * lo * lo + 74, lo, 7]]
    assert st[:, 4:].tolist() == [[1, 2, 1], [1, 0, 1]]                                 # below, above, nan
    # without a clip float32 keeps the infinities; they count as neither below nor above
    if out == 'f32':
        got, st = store(x, out, stats=True)
        assert got.numpy().reshape(-1)[1:5].tolist() == [np.inf, -np.inf, 1e10, -1e10] and st[:, 4:].tolist() == [[0, 0, 1], [0, 0, 1]]


@pytest.mark.parametrize('src', ['f32', 'bf16', 'f16'])
@pytest.mark.parametrize('out', ['i16', 'u16', 'u8', 'f32'])
def test_statistics_against_a_direct_recomputation(src, out):
    scale, shift, clip = svref.CONFIG[out]
    lo, hi = clip if clip else (0, 65535)
    x = svref.make_input(src, (3, 2, 3, 5, 7), scale, shift, lo, hi, seed=3)
    for rounding in ('trunc', 'rint'):
        got, st = store(x, out, scale=scale, shift=shift, clip=clip, rounding=rounding, stats=True)
        # the definition once more, element by element in float32
        with np.errstate(over='ignore', invalid='ignore'):
            t = x.float().numpy() * np.float32(scale) + np.float32(shift)
        nan, below, above = np.isnan(t), t < np.float32(lo), t > np.float32(hi)
        assert nan.any() and below.any() and above.any() and (~(nan | below | above)).any()
        u = np.clip(np.where(nan, np.float32(lo), t), np.float32(lo), np.float32(hi))
        if out == 'f32':
            ref = np.where(nan, np.float32(np.nan), u)
        else:
            ref = (np.rint(u) if rounding == 'rint' else np.trunc(u)).astype(got.numpy().dtype)
        assert np.array_equal(got.numpy(), ref, equal_nan=True)
        assert np.array_equal(st.numpy(), svref.recompute_stats(ref, below, above, nan))
    if out != 'f32':
        tr, ri = (store(x, out, scale=scale, shift=shift, clip=clip, rounding=r).numpy() for r in ('trunc', 'rint'))
        assert (tr != ri).any()


def test_layouts_buffers_and_empty_batches():
    x = svref.make_input('f32', (2, 3, 3, 4, 5), 64.0, 100.0, 3, 250)
    ref = store(x, 'u8', scale=64.0, shift=100.0, clip=(3, 250))
    cl = x.contiguous(memory_format=torch.channels_last_3d)
    assert not cl.is_contiguous()
    got = store(cl, 'u8', scale=64.0, shift=100.0, clip=(3, 250))
    assert got.is_contiguous() and torch.equal(got, ref)                                   # transposed to NCDHW on the way
    buf = torch.zeros(2, 3, 3, 4, 5, dtype=torch.uint8)
    assert store(x, 'u8', scale=64.0, shift=100.0, clip=(3, 250), out=buf) is buf and torch.equal(buf, ref)
    got, st = store(torch.zeros(0, 1, 2, 2, 2), 'i16', stats=True)
    assert got.shape == (0, 1, 2, 2, 2) and got.dtype == torch.int16 and st.shape == (0, 7)
    # the default clip is the type's range
    wide = torch.tensor([-1e6, 1e6, 70000.0, -40000.0]).reshape(1, 1, 1, 1, 4)
    assert store(wide, 'i16').reshape(-1).tolist() == [-32768, 32767, 32767, -32768]
    assert store(wide, 'u16').reshape(-1).tolist() == [0, 65535, 65535, 0]
    assert store(wide, 'u8').reshape(-1).tolist() == [0, 255, 255, 0]
    assert store(wide, 'f32').reshape(-1).tolist() == [-1e6, 1e6, 70000.0, -40000.0]


def test_a_fused_multiply_add_would_differ():
    """The set the GPU test runs: a fused x * scale + shift rounds differently from the two operations on some of it."""
    x, scale, shift, two, fused = svref.fma_sensitive()
    differ = two != fused
    assert 0 < differ.sum() < x.size
    got = store(torch.from_numpy(x).reshape(1, 1, 1, 1, -1), 'f32', scale=scale, shift=shift).numpy().reshape(-1)
    assert np.array_equal(got, two) and (got != fused).any()


def test_argument_errors():
    x = torch.zeros(2, 1, 2, 3, 4)
    with pytest.raises(TypeError, match='expected a tensor'):
        store(np.zeros((1, 1, 2, 2, 2), np.float32), 'i16')
    with pytest.raises(TypeError, match='sources are'):
        store(x.double(), 'i16')
    with pytest.raises(TypeError, match='sources are'):
        store(x.to(torch.int16), 'i16')
    with pytest.raises(TypeError, match='out_dtype is'):
        store(x, torch.int32)
    with pytest.raises(TypeError, match='out_dtype is'):
        store(x, torch.float16)
    with pytest.raises(ValueError, match=r'expected \[n, c, d, h, w\]'):
        store(x[0], 'i16')
    with pytest.raises(ValueError, match='at least one channel'):
        store(torch.zeros(2, 0, 2, 3, 4), 'i16')
    with pytest.raises(ValueError, match='contiguous or channels_last_3d'):
        store(torch.zeros(2, 2, 2, 3, 8)[..., ::2], 'i16')
    with pytest.raises(ValueError, match='rounding is'):
        store(x, 'i16', rounding='floor')
    for bad in (float('inf'), float('nan')):
        with pytest.raises(ValueError, match='not finite'):
            store(x, 'i16', scale=bad)
    with pytest.raises(ValueError, match=r'clip is \(lo, hi\)'):
        store(x, 'i16', clip=(1, 2, 3))
    for clip in ((0.5, 3), (0, float('nan')), (0, float('inf'))):
        with pytest.raises(ValueError, match='are integers'):
            store(x, 'i16', clip=clip)
    for out, clip in (('i16', (5, 4)), ('i16', (-32769, 0)), ('i16', (0, 32768)), ('u16', (-1, 5)), ('u16', (0, 65536)), ('u8', (0, 256)),
                      ('u8', (-1, 0))):
        with pytest.raises(ValueError, match='empty or outside'):
            store(x, out, clip=clip)
    for clip in ((2.0, 1.0), (float('nan'), 1.0), (0.0, float('nan'))):
        with pytest.raises(ValueError, match='is empty'):
            store(x, 'f32', clip=clip)
    for buf in (torch.zeros(2, 1, 2, 3, 4, dtype=torch.uint16), torch.zeros(2, 1, 2, 3, 5, dtype=torch.int16),
                torch.zeros(2, 1, 2, 3, 8, dtype=torch.int16)[..., ::2], np.zeros((2, 1, 2, 3, 4), np.int16)):
        with pytest.raises(ValueError, match='out must be'):
            store(x, 'i16', out=buf)


def test_library_refuses_bad_arguments_before_any_launch():
    """The C entry checks its arguments before it touches the device: SG_EINVAL / SG_EALIGN come back without a GPU."""
    import ctypes as C
    from saragan_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 15) & ~15
    F32, BF16, I16, U16, U8 = _lib.SG_SRC_F32, _lib.SG_SRC_BF16, _lib.SG_SRC_I16, _lib.SG_SRC_U16, _lib.SG_SRC_U8

    def call(x=a, dt=F32, cl=0, n=1, c=1, d=2, h=2, w=2, scale=1.0, shift=0.0, lo=0.0, hi=10.0, rounding=0, odt=I16, out=a + 1024,
             stats=None):
        return lib.sg_store_volumes(x, dt, cl, n, c, d, h, w, scale, shift, lo, hi, rounding, odt, out, stats, None)

    EINVAL, EALIGN = -1, -3
    assert call(n=-1) == EINVAL and call(c=0) == EINVAL and call(d=-1) == EINVAL and call(w=-2) == EINVAL
    assert call(dt=I16) == EINVAL and call(dt=9) == EINVAL and call(odt=BF16) == EINVAL and call(odt=_lib.SG_SRC_I8) == EINVAL
    assert call(rounding=2) == EINVAL and call(scale=float('inf')) == EINVAL and call(scale=float('nan')) == EINVAL
    assert call(lo=3.0, hi=2.0) == EINVAL and call(lo=float('nan')) == EINVAL and call(hi=float('nan')) == EINVAL
    assert call(lo=0.5) == EINVAL and call(hi=32768.0) == EINVAL and call(lo=-32769.0) == EINVAL
    assert call(odt=U16, lo=-1.0) == EINVAL and call(odt=U16, hi=65536.0) == EINVAL and call(odt=U8, hi=256.0) == EINVAL
    assert call(odt=F32, lo=float('-inf'), hi=float('inf'), n=0) == 0                    # float32 bounds may be infinite
    assert call(x=None) == EINVAL and call(out=None) == EINVAL
    assert call(n=2 ** 40, d=2 ** 20, h=2 ** 20, w=2 ** 20) == EINVAL                    # the element count overflows
    assert call(x=a + 2) == EALIGN and call(dt=BF16, x=a + 1) == EALIGN and call(out=a + 1025) == EALIGN
    assert call(stats=a + 2052) == EALIGN
    assert call(n=0) == 0 and call(d=0) == 0 and call(n=0, x=None, out=None) == 0        # nothing to do: nothing launched


def test_header_binding_and_build_agree():
    from saragan_amd import _lib, build
    import ctypes as C
    hdr = open(os.path.join(ROOT, 'include', 'saragan_hip.h')).read()
    m = re.search(r'int sg_store_volumes\((.*?)\);', hdr, re.S)
    params = [p.strip() for p in m.group(1).split(',')]
    restype, argtypes = _lib.SIGNATURES['sg_store_volumes']
    assert restype is C.c_int and len(argtypes) == len(params) == 17
    kinds = {'const void*': C.c_void_p, 'void*': C.c_void_p, 'int64_t*': C.c_void_p, 'sg_stream_t': C.c_void_p, 'sg_src_dtype': C.c_int,
             'int32_t': C.c_int32, 'int64_t': C.c_int64, 'float': C.c_float}
    for p, a in zip(params, argtypes):
        assert kinds[p.rsplit(' ', 1)[0]] is a, p
    assert re.search(r'SG_ROUND_TRUNC = 0, SG_ROUND_RINT = 1', hdr) and (_lib.SG_ROUND_TRUNC, _lib.SG_ROUND_RINT) == (0, 1)
    assert 'export.hip' in build.SOURCES and '-ffp-contract=off' in build.FILE_FLAGS['export.hip']
    assert '`sg_store_volumes`' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    usage = build.resource_usage()['export.hip']
    assert sum('store_volumes' in k for k in usage) == 24
    for k, v in usage.items():
        assert v['vgpr_spill'] == 0 and v['scratch_bytes'] == 0, (k, v)
