"""Host side of the dataset pyramid: functional.block_pyramid's numpy path against tests/pyrref.py with ==, the
anchors against the original's pad_to / crop_to, argument errors, the prepare_data tool end to end on the CPU, and the header
against the ctypes binding.  No GPU."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pyrref
from tests.test_render_view_gpu import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_OUT = {'u16': torch.uint16, 'i16': torch.int16, 'f32': torch.float32}
N_OUT = {'u16': np.uint16, 'i16': np.int16, 'f32': np.float32}
INT_SRC = ('u8', 'i8', 'i16', 'u16')


def pyramid(x, target, levels, out='u16', **kw):
    from saragan_amd import functional as F
    return F.block_pyramid(x, target, levels, out_dtype=T_OUT[out], **kw)


def same(got, ref):
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        g = g.cpu().numpy()
        assert g.shape == r.shape and g.dtype == r.dtype, (i, g.shape, r.shape, g.dtype, r.dtype)
        assert np.array_equal(g, r, equal_nan=True), (i, np.argwhere(g != r)[:4])


@pytest.mark.parametrize('name', INT_SRC + ('f16', 'f32'))
@pytest.mark.parametrize('mode', ('mean', 'max'))
def test_numpy_path_every_dtype_mode_and_output(name, mode):
    """(3, 5, 9, 13) into (8, 8, 16): D and W padded by an odd amount, H cropped."""
    x = make(name, (3, 5, 9, 13))
    ic = {'u8': 7, 'i8': -100, 'i16': -1024, 'u16': 0, 'f16': -3.5, 'f32': 100.25}[name]
    for out in (('u16', 'i16', 'f32') if name in INT_SRC else ('f32',)):
        for levels in (1, 2, 3):
            same(pyramid(x, (8, 8, 16), levels, out, reduce=mode, intercept=ic),
                 pyrref.pyramid(x.numpy(), (8, 8, 16), levels, mode, ic, out_dtype=N_OUT[out]))


def test_numpy_path_sign_clip_wide_sums_and_stats():
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.integers(-1030, -1018, (2, 8, 8, 16)).astype(np.int16))      # means around 0: both signs, halves
    kw = dict(intercept=-1024, clip=(-2000, 2000))
    got, st = pyramid(x, (8, 8, 16), 4, 'i16', stats=True, **kw)
    ref = pyrref.pyramid(x.numpy(), (8, 8, 16), 4, out_dtype=np.int16, **kw)
    same(got, ref)
    assert (ref[1] < 0).any() and np.array_equal(st.numpy(), pyrref.stats(ref))
    big = torch.full((1, 32, 32, 32), 65535, dtype=torch.uint16)
    same(pyramid(big, (32, 32, 32), 6, 'f32', intercept=-65535), pyrref.pyramid(big.numpy(), (32, 32, 32), 6, intercept=-65535,
                                                                             out_dtype=np.float32))
    got = pyramid(big, (32, 32, 32), 6, 'i16', intercept=-65535)
    assert all((g.numpy() == 32767).all() for g in got)
    hot = torch.from_numpy(rng.integers(0, 2, (1, 4, 8, 8)).astype(np.uint16) * 6000)      # exceeds the clip at level 0 only
    same(pyramid(hot, (4, 8, 8), 3, 'u16', clip=(0, 3072)), pyrref.pyramid(hot.numpy(), (4, 8, 8), 3, clip=(0, 3072)))


@pytest.mark.parametrize('source,target', [((5, 9, 13), (8, 8, 16)), ((4, 8, 16), (8, 16, 32)), ((9, 17, 33), (8, 16, 32)),
                                           ((6, 10, 12), (5, 7, 12)), ((1, 1, 1), (4, 4, 4))])
def test_anchors_are_pad_to_and_crop_to(source, target):
    """Odd and even differences, short and long axes: the offsets reproduce np.pad + crop, voxel for voxel."""
    from saragan_amd import functional as F
    x = np.arange(1, 1 + np.prod(source), dtype=np.int16).reshape(source)
    for anchor in [('center',) * 3, ('start',) * 3, ('end',) * 3, ('end', 'center', 'start')]:
        off = F.pyramid_offsets(source, target, anchor)
        want = pyrref.window(x, target, 0, anchor)
        got = np.zeros(target, np.int16)
        for t in np.ndindex(*target):
            s = tuple(ti + o for ti, o in zip(t, off))
            if all(0 <= si < ext for si, ext in zip(s, source)):
                got[t] = x[s]
        assert np.array_equal(got, want), (anchor, off)
        same(pyramid(torch.from_numpy(x[None]), target, 1, 'i16', anchor=anchor),
             pyrref.pyramid(x[None], target, 1, out_dtype=np.int16, anchor=anchor))
    d = target[0] - source[0]
    if d > 0:
        assert F.pyramid_offsets(source, target)[0] == -(d // 2)
    else:
        assert F.pyramid_offsets(source, target)[0] == source[0] // 2 - target[0] // 2


def test_argument_errors():
    x = make('i16', (1, 4, 8, 8))
    with pytest.raises(TypeError):
        pyramid(x.numpy(), (4, 8, 8), 1)
    with pytest.raises(TypeError):
        pyramid(x.to(torch.int32), (4, 8, 8), 1)
    with pytest.raises(TypeError):
        pyramid(x.to(torch.bfloat16), (4, 8, 8), 1, 'f32')
    with pytest.raises(TypeError):
        pyramid(make('f32', (1, 4, 8, 8)), (4, 8, 8), 1, 'u16')      # a float source with an integer output
    with pytest.raises(TypeError):
        from saragan_amd import functional as F
        F.block_pyramid(x, (4, 8, 8), 1, out_dtype=torch.uint8)
    for bad in (dict(target=(4, 8)), dict(target=(4, 8, 6), levels=3), dict(levels=0), dict(levels=7, target=(64, 64, 64)), dict(reduce='median'),
                dict(anchor=('middle',) * 3), dict(anchor=('center',) * 2), dict(clip=(5, 4)), dict(clip=(-1, 10)),
                dict(clip=(0, 70000)), dict(intercept=2 ** 31), dict(pad_value=0.5), dict(out='f32', stats=True)):
        kw = dict(target=(4, 8, 8), levels=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            pyramid(x, kw.pop('target'), kw.pop('levels'), **kw)
    with pytest.raises(ValueError):
        pyramid(x[0], (4, 8, 8), 1)
    with pytest.raises(ValueError):
        pyramid(x[:, :, :, ::2], (4, 8, 4), 1)


# ---- the tool
SIX = [('a0', (5, 17, 18)), ('a1', (9, 14, 20)), ('a2', (5, 17, 18)), ('b0', (9, 14, 20)), ('b1', (5, 17, 18)), ('c0', (9, 14, 20))]
TOOL_ARGS = ['--final_shape', '8,16,16', '--start_shape', '2,4,4', '--intercept=-1024', '--clip=0,3000', '--batch', '2']


def write_six(src):
    """Six small int16 files of two shapes (both pad and crop against 8 x 16 x 16), CT-like values."""
    os.makedirs(src, exist_ok=True)
    for k, (name, shape) in enumerate(SIX):
        np.save(os.path.join(src, name + '.npy'), make('i16', (1,) + shape, seed=k)[0].numpy())


def run_tool(*args):
    return subprocess.run([sys.executable, '-m', 'saragan_amd.prepare_data', *args], cwd=ROOT, capture_output=True, text=True)


def test_tool_end_to_end_on_the_cpu(tmp_path):
    from saragan_amd.dataset import NumpyPathDataset
    src, dst = str(tmp_path / 'src'), str(tmp_path / 'dst')
    write_six(src)
    r = run_tool(src, dst, *TOOL_ARGS, '--device', 'cpu')
    assert r.returncode == 0, r.stderr
    assert 'padded 6 / cropped 6 / files 6' in r.stdout
    stats = json.load(open(os.path.join(dst, 'stats.json')))
    assert 'definition' in stats and len(stats['levels']) == 3
    sources = [np.load(os.path.join(src, n + '.npy')) for n, _ in SIX]
    for i, lv in enumerate(stats['levels']):
        size = 16 >> i
        d = os.path.join(dst, f'{size}x{size}')
        assert lv['directory'] == f'{size}x{size}' and sorted(os.listdir(d)) == sorted(n + '.npy' for n, _ in SIX)
        ds = NumpyPathDataset(d + '/', None, copy_files=False, is_correct_phase=True, seed=1)
        assert len(ds) == 6 and tuple(ds.shape) == (1, 8 >> i, size, size) and ds.dtype == np.uint16
        written = np.stack([np.load(os.path.join(d, n + '.npy')) for n, _ in SIX])
        for k, vol in enumerate(sources):      # every file is the reference's level of its own source
            ref = pyrref.pyramid(vol[None], (8, 16, 16), 3, intercept=-1024, clip=(0, 3000))[i][0]
            assert np.array_equal(written[k], ref)
        w = written.astype(np.float64)
        assert lv['files'] == 6 and lv['shape'] == [8 >> i, size, size] and lv['dtype'] == 'uint16'
        assert lv['min'] == int(written.min()) and lv['max'] == int(written.max())
        assert abs(lv['mean'] - w.mean()) <= 1e-12 * abs(w.mean()) and abs(lv['stddev'] - w.std()) <= 1e-12 * w.std()
    flags = re.search(r'--data_mean (\S+) --data_stddev (\S+)', r.stdout)
    assert float(flags.group(1)) == stats['levels'][0]['mean'] and float(flags.group(2)) == stats['levels'][0]['stddev']
    # a second run without --overwrite fails before writing anything
    before = {os.path.join(dp, p): os.path.getmtime(os.path.join(dp, p)) for dp, _, fs in os.walk(dst) for p in fs}
    os.remove(os.path.join(dst, '4x4', 'c0.npy'))
    r2 = run_tool(src, dst, *TOOL_ARGS, '--device', 'cpu')
    assert r2.returncode != 0 and 'exists' in r2.stderr and not os.path.exists(os.path.join(dst, '4x4', 'c0.npy'))
    assert all(os.path.getmtime(os.path.join(dp, p)) == before[os.path.join(dp, p)] for dp, _, fs in os.walk(dst) for p in fs)
    assert run_tool(src, dst, *TOOL_ARGS, '--device', 'cpu', '--overwrite').returncode == 0
    assert os.path.exists(os.path.join(dst, '4x4', 'c0.npy'))


def test_tool_names_the_axis_that_does_not_fit(tmp_path):
    src = str(tmp_path / 'src')
    write_six(src)
    r = run_tool(src, str(tmp_path / 'dst'), '--final_shape', '8,16,16', '--start_shape', '2,4,8', '--device', 'cpu')
    assert r.returncode != 0 and 'axis W' in r.stderr and not os.path.exists(tmp_path / 'dst')
    r = run_tool(src, str(tmp_path / 'dst'), '--final_shape', '8,16,16', '--start_shape', '3,4,4', '--device', 'cpu')
    assert r.returncode != 0 and 'axis D' in r.stderr


# ---- the header and the binding
def _ctype_of(arg):
    arg = arg.strip()
    if '*' in arg:
        return 'pp' if 'void* const*' in arg else 'p'
    return {'int32_t': 'i32', 'int64_t': 'i64', 'float': 'f', 'sg_src_dtype': 'int', 'sg_stream_t': 'p', 'int': 'int'}[arg.split()[0]]


def test_header_and_binding_agree_on_the_pyramid_entries():
    from saragan_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'saragan_hip.h')).read()
    names = {'p': C.c_void_p, 'pp': C.POINTER(C.c_void_p), 'i32': C.c_int32, 'i64': C.c_int64, 'f': C.c_float, 'int': C.c_int}
    for fn in ('sg_block_pyramid',):
        m = re.search(r'\bint\s+' + fn + r'\s*\(([^)]*)\)\s*;', header)
        assert m, f'{fn} is not declared by the header'
        kinds = [_ctype_of(a) for a in m.group(1).replace('\n', ' ').split(',')]
        restype, argtypes = _lib.SIGNATURES[fn]
        assert restype is C.c_int and list(argtypes) == [names[k] for k in kinds], fn
    assert re.search(r'#define\s+SG_PYRAMID_LEVELS_PER_LAUNCH\s+6\b', header) and _lib.SG_PYRAMID_LEVELS_PER_LAUNCH == 6
    assert re.search(r'SG_PYR_MEAN\s*=\s*0\s*,\s*SG_PYR_MAX\s*=\s*1', header) and (_lib.SG_PYR_MEAN, _lib.SG_PYR_MAX) == (0, 1)
    from saragan_amd import build
    assert 'pyramid.hip' in build.SOURCES and '-ffp-contract=off' in build.FILE_FLAGS['pyramid.hip']
