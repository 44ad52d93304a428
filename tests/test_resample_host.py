"""Host side of the resampler: functional.resample_volume's numpy twin against scipy in f64 and against dense
per-axis matrices built here from the definition, the exact cases, zero-weight taps, argument errors, the header against the ctypes
binding, and the prepare_data tool with --spacing end to end on the CPU.  No GPU.

The bound.  Every weight is an f64 weight rounded once to f32: a relative error of at most 2^-24.  A voxel's coefficient is a
product of three such weights, 3 * 2^-24 relative to first order, and the coefficients are a convex combination (they are >= 0 and
sum to 1), so the result is off by at most 3 * 2^-24 * max|x|; a fourth unit covers the f64 rounding of both sides."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import pyrref
from tests.test_pyramid_host import SIX, TOOL_ARGS, run_tool, write_six
from tests.test_render_view_gpu import make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_OUT = {'u16': torch.uint16, 'i16': torch.int16, 'f32': torch.float32}
INT_SRC = ('u8', 'i8', 'i16', 'u16')
ALL_SRC = INT_SRC + ('f16', 'f32')
STEPS, STARTS = (2.4, 0.9765625, -0.7), (0.0, 0.0, 44.0)
SHAPE, OUT = (11, 23, 45), (7, 26, 70)      # the last planes, rows and columns of OUT lie outside the source


def resample(x, out_shape, step, start, **kw):
    from saragan_amd import functional as F
    if 'out' in kw:
        kw['out_dtype'] = T_OUT[kw.pop('out')]
    return F.resample_volume(x, out_shape, step, start, **kw)


def coords(out_shape=OUT, step=STEPS, start=STARTS):
    return [s0 + np.arange(o, dtype=np.float64) * st for o, st, s0 in zip(out_shape, step, start)]


def inside_mask(shape, cs):
    ins = [(c >= -0.5) & (c <= s - 0.5) for c, s in zip(cs, shape)]
    return ins[0][:, None, None] & ins[1][None, :, None] & ins[2][None, None, :]


def bound(x):
    return 4.0 * 2.0 ** -24 * float(np.abs(x.astype(np.float64)).max())


# ---- 1: the twin against scipy
def test_linear_against_scipy_map_coordinates():
    from scipy.ndimage import map_coordinates
    x = make('i16', (1,) + SHAPE)
    a = x.numpy()[0].astype(np.float64)
    cs = coords()
    grid = np.meshgrid(*cs, indexing='ij')
    ref = map_coordinates(a, grid, order=1, mode='nearest')
    ins = inside_mask(SHAPE, cs)
    assert ins.any() and not ins.all() and not ins[-1].any() and not ins[:, -1].any() and not ins[:, :, -1].any()
    tol = bound(a)
    got = resample(x, OUT, STEPS, STARTS, fill=-1000, out='f32').numpy()[0]
    err = np.abs(got.astype(np.float64) - ref)[ins].max()
    print(f'linear f32 against scipy: max error {err:.3e}, bound {tol:.3e}')
    assert got.dtype == np.float32 and err <= tol
    assert (got[~ins] == -1000.0).all()
    for out, lo, hi in (('i16', -32768, 32767), ('u16', 0, 65535)):
        q = resample(x, OUT, STEPS, STARTS, fill=-1000, out=out).numpy()[0]
        err = np.abs(q.astype(np.float64) - np.clip(ref, lo, hi))[ins].max()
        print(f'linear {out} against scipy: max error {err:.3e}, bound {0.5 + tol:.3e}')
        assert q.dtype == np.dtype({'i16': np.int16, 'u16': np.uint16}[out]) and err <= 0.5 + tol
        assert (q[~ins] == max(-1000, lo)).all()
    assert resample(x, OUT, STEPS, STARTS).dtype == torch.int16      # the default follows the source


# ---- 2: exact cases
@pytest.mark.parametrize('name', ALL_SRC)
def test_identity_and_flip_return_the_source(name):
    x = make(name, (2, 5, 6, 9))
    outs = ('u16', 'i16', 'f32') if name in INT_SRC else ('f32',)
    for mode in ('nearest', 'linear', 'antialias'):
        for out in outs:
            want = x.numpy().astype(np.float64)
            if out != 'f32':
                want = np.clip(want, *{'u16': (0, 65535), 'i16': (-32768, 32767)}[out])
            got = resample(x, (5, 6, 9), (1, 1, 1), (0, 0, 0), mode=mode, out=out)
            assert got.dtype == T_OUT[out] and np.array_equal(got.numpy().astype(np.float64), want), (mode, out)
            got = resample(x, (5, 6, 9), (-1, -1, -1), (4, 5, 8), mode=mode, out=out)
            assert np.array_equal(got.numpy().astype(np.float64), np.flip(want, axis=(1, 2, 3))), (mode, out)
    default = resample(x, (5, 6, 9), (1, 1, 1), (0, 0, 0))
    assert default.dtype == {'u8': torch.uint16, 'i8': torch.int16, 'i16': torch.int16, 'u16': torch.uint16, 'f16': torch.float32,
                             'f32': torch.float32}[name]
    assert np.array_equal(default.numpy(), x.numpy().astype(default.numpy().dtype))      # the same values: the source's bits


def test_half_steps_are_exact_rationals():
    """step 0.5 with linear: the weights are 1, or 1/2 and 1/2 -- dyadic, so integer data give exact halves."""
    x = make('i16', (1, 4, 5, 7))
    a = x.numpy()[0].astype(np.float64)
    for axis in range(3):
        out_shape = list(a.shape)
        out_shape[axis] = 2 * a.shape[axis] - 1
        step = [1.0, 1.0, 1.0]
        step[axis] = 0.5
        lo = np.take(a, np.arange(out_shape[axis]) // 2, axis=axis)
        hi = np.take(a, (np.arange(out_shape[axis]) + 1) // 2, axis=axis)
        want = (lo + hi) / 2.0
        got = resample(x, out_shape, step, (0, 0, 0), out='f32').numpy()[0]
        assert np.array_equal(got.astype(np.float64), want), axis
        got = resample(x, out_shape, step, (0, 0, 0), out='i16').numpy()[0]
        assert (want != np.rint(want)).any() and np.array_equal(got.astype(np.float64), np.rint(want)), axis      # ties to even


@pytest.mark.parametrize('name', ALL_SRC)
def test_nearest_copies_values(name):
    x = make(name, (2,) + SHAPE)
    cs = coords()
    idx = [np.clip(np.floor(c + 0.5).astype(np.int64), 0, s - 1) for c, s in zip(cs, SHAPE)]
    want = x.numpy()[:, idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
    ins = inside_mask(SHAPE, cs)
    got = resample(x, OUT, STEPS, STARTS, mode='nearest', fill=3).numpy()
    assert np.array_equal(got[:, ins], want[:, ins].astype(got.dtype)) and (got[:, ~ins] == 3).all()


# ---- 3: antialias against dense matrices built from the definition
def dense_triangle(S, O, step, start):
    """[O, S]: row o holds the normalised triangle of half-width max(1, |step|) around start + o * step, edge voxels repeated."""
    m = np.zeros((O, S), np.float64)
    k = max(1.0, abs(step))
    for o in range(O):
        c = start + o * step
        taps = range(int(np.ceil(c - k)), int(np.floor(c + k)) + 1)
        w = np.array([max(0.0, 1.0 - abs(i - c) / k) for i in taps])
        w = w / w.sum()
        for i, wi in zip(taps, w):
            m[o, min(max(i, 0), S - 1)] += wi
    return m


def test_antialias_against_dense_matrices():
    from saragan_amd import functional as F
    x = make('i16', (2,) + SHAPE)
    a = x.numpy().astype(np.float64)
    step, start, out_shape = (2.4, 0.6, -2.4), (0.0, 0.3, 44.0), (5, 36, 18)
    mats = [dense_triangle(s, o, st, s0) for s, o, st, s0 in zip(SHAPE, out_shape, step, start)]
    ref = np.einsum('ad,bh,cw,ndhw->nabc', *mats, a)
    ins = inside_mask(SHAPE, coords(out_shape, step, start))
    assert ins.all()
    got = resample(x, out_shape, step, start, mode='antialias', out='f32').numpy()
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f'antialias f32 against the dense matrices: max error {err:.3e}, bound {bound(a):.3e}')
    assert err <= bound(a)
    q = resample(x, out_shape, step, start, mode='antialias', out='i16').numpy()
    assert np.abs(q.astype(np.float64) - ref).max() <= 0.5 + bound(a)
    # the taps themselves: 5 or 6 at step 2.4, and at step 0.6 the linear table
    _, idx, w = F.resample_taps(SHAPE[0], out_shape[0], 2.4, 0.0, 'antialias')
    assert idx.shape[1] in (5, 6) and w.dtype == np.float32 and idx.dtype == np.int32
    assert np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 6 * 2.0 ** -24
    lin, aa = F.resample_taps(SHAPE[1], 36, 0.6, 0.3, 'linear'), F.resample_taps(SHAPE[1], 36, 0.6, 0.3, 'antialias')
    assert all(np.array_equal(p, q) for p, q in zip(lin, aa)) and lin[1].shape[1] == 2


# ---- 4: zero-weight taps
@pytest.mark.parametrize('name', ('f16', 'f32'))
def test_a_zero_weight_tap_is_not_read(name):
    from saragan_amd import functional as F
    x = make(name, (1, 5, 6, 9))
    x[0, 2, 3, 4] = float('inf')
    x[0, 3, 1, 7] = float('nan')
    bad = ~np.isfinite(x.numpy()[0].astype(np.float64))
    out_shape, step, start = (9, 11, 17), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)      # even outputs sit on a voxel: weights 1 and 0
    reach = []
    for s, o, st, s0 in zip(x.shape[1:], out_shape, step, start):
        _, idx, w = F.resample_taps(s, o, st, s0, 'linear')
        m = np.zeros((o, s), bool)
        for k in range(idx.shape[1]):
            m[np.arange(o)[w[:, k] != 0], idx[w[:, k] != 0, k]] = True
        assert (w == 0).any()
        reach.append(m.astype(np.int64))
    want = np.einsum('ad,bh,cw,dhw->abc', *reach, bad.astype(np.int64)) > 0
    got = resample(x, out_shape, step, start).numpy()[0]
    assert np.array_equal(~np.isfinite(got), want) and 0 < want.sum() < want.size / 4
    assert np.isnan(got[6, 2, 14]) and got[4, 6, 8] == np.inf and np.isfinite(got[4, 6, 10])


# ---- 5: argument errors
def test_argument_errors():
    from saragan_amd import functional as F
    x = make('i16', (1, 4, 8, 8))
    ok = dict(out_shape=(4, 8, 8), step=(1, 1, 1), start=(0, 0, 0))

    def call(t=x, **over):
        kw = dict(ok)
        kw.update(over)
        return F.resample_volume(t, kw.pop('out_shape'), kw.pop('step'), kw.pop('start'), **kw)
    assert call().shape == (1, 4, 8, 8)
    for bad in (dict(t=x.numpy()), dict(t=x.to(torch.int32)), dict(t=x.to(torch.bfloat16)), dict(out_dtype=torch.uint8),
                dict(t=make('f32', (1, 4, 8, 8)), out_dtype=torch.int16), dict(t=make('f16', (1, 4, 8, 8)), out_dtype=torch.uint16)):
        with pytest.raises(TypeError):
            call(**bad)
    for bad in (dict(t=x[0]), dict(t=x[:, :, :, ::2]), dict(out_shape=(4, 8)), dict(out_shape=(4, -1, 8)), dict(step=(1, 1)),
                dict(start=(0, 0, 0, 0)), dict(step=(1, 0, 1)), dict(step=(1, float('nan'), 1)), dict(start=(0, float('inf'), 0)),
                dict(mode='cubic'), dict(mode=('linear', 'linear')), dict(fill=0.5), dict(fill=2 ** 31), dict(step=(16, 1, 1), mode='antialias'),
                dict(out_shape=(2 ** 29 + 1, 1, 1)), dict(step=1.0)):
        with pytest.raises(ValueError):
            call(**bad)
    assert call(step=(15, 1, 1), mode='antialias').shape == (1, 4, 8, 8)
    assert call(t=make('f32', (1, 4, 8, 8)), fill=0.5).dtype == torch.float32
    assert call(out_shape=(0, 8, 8)).shape == (1, 0, 8, 8) and call(t=x[:0]).shape == (0, 4, 8, 8)
    for bad in (dict(S=0), dict(O=-1), dict(step=0.0), dict(step=float('inf')), dict(start=float('nan')), dict(mode='cubic'),
                dict(step=15.5, mode='antialias'), dict(step=-16.0, mode='antialias')):
        kw = dict(S=4, O=4, step=1.0, start=0.0, mode='linear')
        kw.update(bad)
        with pytest.raises(ValueError):
            F.resample_taps(**kw)
    inside, idx, w = F.resample_taps(4, 6, 1.0, -1.0, 'linear')
    assert inside.tolist() == [False, True, True, True, True, False] and idx.min() == 0 and idx.max() == 3
    assert F.resample_taps(4, 2, 1.0, -0.5, 'nearest')[0].tolist() == [True, True]      # c = -0.5 and S - 0.5 are inside
    assert F.resample_taps(4, 2, 4.0, -0.5, 'nearest')[0].tolist() == [True, True]


# ---- 6: the header and the binding
def test_header_and_binding_agree_on_the_resample_entry():
    from saragan_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'saragan_hip.h')).read()
    m = re.search(r'\bint\s+sg_resample_axes\s*\(([^)]*)\)\s*;', header)
    assert m, 'sg_resample_axes is not declared by the header'
    names = {'int32_t': C.c_int32, 'int64_t': C.c_int64, 'float': C.c_float, 'sg_src_dtype': C.c_int, 'sg_stream_t': C.c_void_p}
    kinds = [C.c_void_p if '*' in a else names[a.split()[0]] for a in m.group(1).replace('\n', ' ').split(',')]
    restype, argtypes = _lib.SIGNATURES['sg_resample_axes']
    assert restype is C.c_int and list(argtypes) == kinds
    assert re.search(r'#define\s+SG_RESAMPLE_MAX_TAPS\s+32\b', header) and _lib.SG_RESAMPLE_MAX_TAPS == 32
    assert 'resample.hip' in build.SOURCES and '-ffp-contract=off' in build.FILE_FLAGS['resample.hip']


# ---- 8: the tool
FOUR_ARGS = ['--final_shape', '8,16,16', '--levels', '2', '--intercept=-1024', '--clip=0,3000', '--batch', '2', '--spacing', '3,1.25,1.25',
             '--orient', 'positive']
TARGET = (3.0, 1.25, 1.25)


def write_four(src):
    """Two NRRD files of different spacings, a third whose array axes are (z, -x, y) of the world, and a `.npy` with its spacing in
    a table.  Returns {stem: (array, directions or None, spacing)} and the table's path."""
    from saragan_amd import nrrd_io
    os.makedirs(src, exist_ok=True)
    vols = {}
    a = make('i16', (1, 6, 14, 16), seed=1)[0].numpy()
    nrrd_io.write(os.path.join(src, 'a.nrrd'), a, (3.0, 1.0, 1.0), origin=(-10.0, 5.0, 0.0))
    vols['a'] = (a, ((0, 0, 3.0), (0, 1.0, 0), (1.0, 0, 0)), (3.0, 1.0, 1.0))
    b = make('i16', (1, 7, 16, 18), seed=2)[0].numpy()
    nrrd_io.write(os.path.join(src, 'b.nhdr'), b, (2.5, 0.8, 0.8), encoding='raw', data_file='b.raw')
    vols['b'] = (b, None, (2.5, 0.8, 0.8))
    c = make('i16', (1, 5, 20, 15), seed=3)[0].numpy()
    dirs = ((0.0, 0.0, 2.0), (-0.9, 0.0, 0.0), (0.0, 0.9, 0.0))
    nrrd_io.write(os.path.join(src, 'c.nrrd'), c, None, directions=dirs, endian='big')
    vols['c'] = (c, dirs, tuple(float(np.sqrt(sum(q * q for q in v))) for v in dirs))      # the lengths, as the reader takes them
    d = make('i16', (1, 9, 12, 12), seed=4)[0].numpy()
    np.save(os.path.join(src, 'd.npy'), d)
    vols['d'] = (d, None, (1.5, 1.5, 1.5))
    table = os.path.join(src, 'spacing.csv')
    with open(table, 'w') as f:
        f.write('# name,sd,sh,sw\nd.npy,1.5,1.5,1.5\n')
    return vols, table


def expected_level0(arr, dirs, spacing, interp='linear'):
    """block_pyramid(resample_volume(...)) of one source, the orientation worked out here."""
    from saragan_amd import functional as F
    perm, flip = (0, 1, 2), (False,) * 3
    if dirs is not None:
        world = [int(np.argmax(np.abs(v))) for v in dirs]
        perm = tuple(world.index(2 - t) for t in range(3))
        flip = tuple(dirs[p][2 - t] < 0 for t, p in enumerate(perm))
    vol = np.ascontiguousarray(arr.transpose(perm))
    old = [spacing[p] for p in perm]
    out_shape = [int(np.ceil(s * (o / n))) for s, o, n in zip(vol.shape, old, TARGET)]
    step = [-(n / o) if f else n / o for o, n, f in zip(old, TARGET, flip)]
    start = [s - 1.0 if f else 0.0 for s, f in zip(vol.shape, flip)]
    r = F.resample_volume(torch.from_numpy(vol[None]), out_shape, step, start, mode=interp, fill=-1024)
    return F.block_pyramid(r, (8, 16, 16), 2, intercept=-1024, clip=(0, 3000)), vol.shape, old, out_shape


def test_tool_resamples_four_sources_on_the_cpu(tmp_path):
    src, dst = str(tmp_path / 'src'), str(tmp_path / 'dst')
    vols, table = write_four(src)
    r = run_tool(src, dst, *FOUR_ARGS, '--spacing_table', table, '--device', 'cpu')
    assert r.returncode == 0, r.stderr
    assert 'files 4 / discarded 0' in r.stdout
    stats = json.load(open(os.path.join(dst, 'stats.json')))
    rec = stats['resample']
    assert rec['spacing'] == list(TARGET) and rec['interp'] == 'linear' and rec['grid'] == 'itk' and rec['orient'] == 'positive'
    assert [f['name'] for f in rec['files']] == ['a.npy', 'b.npy', 'c.npy', 'd.npy']
    flipped = False
    for entry, (stem, (arr, dirs, spacing)) in zip(rec['files'], sorted(vols.items())):
        (lv0, lv1), shape, old, out_shape = expected_level0(arr, dirs, spacing)
        assert entry['source_shape'] == list(shape) and entry['resampled_shape'] == out_shape
        assert np.allclose(entry['source_spacing'], old, rtol=1e-12)
        assert np.array_equal(np.load(os.path.join(dst, '16x16', stem + '.npy')), lv0[0].numpy()), stem
        assert np.array_equal(np.load(os.path.join(dst, '8x8', stem + '.npy')), lv1[0].numpy()), stem
        flipped = flipped or shape != arr.shape
    assert flipped      # c.nrrd was permuted
    assert sorted(os.listdir(os.path.join(dst, '16x16'))) == ['a.npy', 'b.npy', 'c.npy', 'd.npy']


def test_tool_oblique_files_and_duplicate_stems(tmp_path):
    from saragan_amd import nrrd_io
    src, dst = str(tmp_path / 'src'), str(tmp_path / 'dst')
    _, table = write_four(src)
    s = 0.5 ** 0.5
    nrrd_io.write(os.path.join(src, 'e.nrrd'), make('i16', (1, 6, 8, 8))[0].numpy(), None,
                  directions=((0.0, 0.0, 3.0), (-s, s, 0.0), (s, s, 0.0)))
    r = run_tool(src, dst, *FOUR_ARGS, '--spacing_table', table, '--device', 'cpu')
    assert r.returncode != 0 and 'e.nrrd' in r.stderr and 'oblique' in r.stderr and not os.path.exists(dst)
    r = run_tool(src, dst, *FOUR_ARGS, '--spacing_table', table, '--device', 'cpu', '--skip_unsupported')
    assert r.returncode == 0, r.stderr
    assert 'files 4 / discarded 1' in r.stdout and 'e.nrrd' in r.stdout
    assert sorted(os.listdir(os.path.join(dst, '16x16'))) == ['a.npy', 'b.npy', 'c.npy', 'd.npy']
    assert json.load(open(os.path.join(dst, 'stats.json')))['resample']['discarded'] == 1
    # two sources with one stem: refused before anything is written
    np.save(os.path.join(src, 'a.npy'), make('i16', (1, 6, 14, 16))[0].numpy())
    dst2 = str(tmp_path / 'dst2')
    r = run_tool(src, dst2, *FOUR_ARGS, '--spacing_table', table, '--device', 'cpu', '--skip_unsupported')
    assert r.returncode != 0 and 'a.npy' in r.stderr and 'a.nrrd' in r.stderr and not os.path.exists(dst2)
    # a source without a spacing, and flags that need --spacing
    os.remove(os.path.join(src, 'a.npy'))
    r = run_tool(src, dst2, *FOUR_ARGS, '--device', 'cpu', '--skip_unsupported')
    assert r.returncode != 0 and 'd.npy' in r.stderr and 'spacing' in r.stderr and not os.path.exists(dst2)
    r = run_tool(src, dst2, '--final_shape', '8,16,16', '--levels', '2', '--interp', 'nearest', '--device', 'cpu')
    assert r.returncode != 0 and '--spacing' in r.stderr


def test_tool_reads_nrrd_without_resampling(tmp_path):
    """Without --spacing an NRRD source is its array: the tree equals the one of the same arrays as `.npy`."""
    from saragan_amd import nrrd_io
    one, two = str(tmp_path / 'one'), str(tmp_path / 'two')
    write_six(one)
    os.makedirs(two)
    for k, (name, _) in enumerate(SIX):
        arr = np.load(os.path.join(one, name + '.npy'))
        if k % 2:
            nrrd_io.write(os.path.join(two, name + '.nrrd'), arr, (2.5, 0.7, 0.7), encoding=('raw', 'gzip')[k % 4 == 1])
        else:
            np.save(os.path.join(two, name + '.npy'), arr)
    trees = []
    for src, dst in ((one, str(tmp_path / 'd1')), (two, str(tmp_path / 'd2'))):
        r = run_tool(src, dst, *TOOL_ARGS, '--device', 'cpu')
        assert r.returncode == 0, r.stderr
        trees.append({os.path.relpath(os.path.join(dp, f), dst): open(os.path.join(dp, f), 'rb').read()
                      for dp, _, fs in os.walk(dst) for f in fs})
    assert trees[0] == trees[1] and len(trees[0]) == 3 * len(SIX) + 1


def test_tool_without_the_new_flags_writes_what_it_wrote(tmp_path):
    src, dst = str(tmp_path / 'src'), str(tmp_path / 'dst')
    write_six(src)
    r = run_tool(src, dst, *TOOL_ARGS, '--device', 'cpu')
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == 'padded 6 / cropped 6 / files 6' and len(lines) == 3
    assert re.fullmatch(r'seconds per volume: load \S+, upload \S+, kernel \S+, download \S+, save \S+ \(cpu\)', lines[1])
    text = open(os.path.join(dst, 'stats.json')).read()
    stats = json.loads(text)
    assert list(stats) == ['definition', 'reduce', 'intercept', 'pad_value', 'clip', 'anchor', 'levels']
    assert text == json.dumps(stats, indent=1) + '\n'
    for i in range(3):
        for name, _ in SIX:
            vol = np.load(os.path.join(src, name + '.npy'))
            ref = pyrref.pyramid(vol[None], (8, 16, 16), 3, intercept=-1024, clip=(0, 3000))[i][0]
            got = np.load(os.path.join(dst, f'{16 >> i}x{16 >> i}', name + '.npy'))
            assert got.dtype == ref.dtype and np.array_equal(got, ref)
