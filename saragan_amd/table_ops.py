"""Reads of typed device tables: batches gathered from a resident dataset (dataset.ResidentLoader),
voxel-intensity histograms (metrics/intensity_metrics.py), rendered views (preview.py), the
dataset pyramid of full-size volumes (prepare_data.py) and its resampler -- and the one write:
typed volumes stored from the generator's output (generate.py).  Also the exact squared distances between typed
integer rows and the running k nearest of the memorisation audit (metrics/memorisation.py), and the multi-scale
residual loss of the projection with the update of its latents (project.py), and the shell-binned power
spectrum of typed volumes (metrics/spectrum_metrics.py).  Re-exported by functional."""
import math

import torch

from . import _lib
from ._launch import _ptr, _stream
from ._lib import check

# ---- batches from a resident table: out[i] = f32(table[idx[i]]), optionally normalised
SRC_DT = {torch.uint8: _lib.SG_SRC_U8, torch.int8: _lib.SG_SRC_I8, torch.int16: _lib.SG_SRC_I16, torch.uint16: _lib.SG_SRC_U16,
          torch.float16: _lib.SG_SRC_F16, torch.float32: _lib.SG_SRC_F32}


def check_positions(positions, rows):
    """Host table positions as a contiguous int32 array; ValueError if one lies outside [0, rows).  (The kernel guards itself
    as well -- such a row comes back as NaN -- but a bad draw is a bug of the caller's and is reported where it is made.)"""
    import numpy as np
    pos = np.ascontiguousarray(positions.numpy() if torch.is_tensor(positions) else positions)
    if pos.ndim != 1 or (pos.size and not np.issubdtype(pos.dtype, np.integer)):
        raise ValueError(f'gather_rows: expected a 1-D sequence of integer positions, got {pos.dtype} {pos.shape}')
    if pos.size and (int(pos.min()) < 0 or int(pos.max()) >= rows):
        bad = int(pos[(pos < 0) | (pos >= rows)][0])
        raise ValueError(f'gather_rows: position {bad} lies outside the table of {rows} rows')
    return pos.astype(np.int32, copy=False)


def gather_rows(table, idx, mean=None, stddev=None, out=None):
    """f32 [n, ...] = the rows idx of table [rows, ...] (u8 / i8 / i16 / u16 / f16 / f32), converted exactly and, with mean and
    stddev, normalised as (x - mean) / stddev in two correctly rounded f32 operations: the bits np.subtract / np.divide with
    np.float32 scalars give (sg_gather_rows, one launch).  idx: host positions (a sequence, an array or a CPU tensor: validated,
    then uploaded) or an int32 tensor on the table's device (used as it is: a position outside the table gives a NaN row).
    out: an f32 buffer of the result's shape to write into.  A CPU table takes the same two numpy operations in the same order."""
    if (mean is None) != (stddev is None):
        raise ValueError('gather_rows: give both mean and stddev, or neither')
    if table.dtype not in SRC_DT:
        raise TypeError(f'gather_rows: tables are uint8, int8, int16, uint16, float16 or float32, got {table.dtype}')
    if table.dim() < 1 or not table.is_contiguous():
        raise ValueError('gather_rows: expected a contiguous [rows, ...] table')
    rows = table.shape[0]
    on_device = torch.is_tensor(idx) and idx.is_cuda
    if on_device:
        if not table.is_cuda or idx.device != table.device or idx.dtype != torch.int32 or idx.dim() != 1 or not idx.is_contiguous():
            raise ValueError('gather_rows: device positions are a contiguous 1-D int32 tensor on the table\'s device')
    else:
        pos = check_positions(idx, rows)
    n = idx.shape[0] if on_device else pos.shape[0]
    shape = (n,) + tuple(table.shape[1:])
    if out is not None and (tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != table.device
                            or not out.is_contiguous()):
        raise ValueError(f'gather_rows: out must be a contiguous float32 {shape} tensor on {table.device}')
    if not table.is_cuda:
        import numpy as np
        res = np.empty(shape, dtype=np.float32)
        np.copyto(res, table.numpy()[pos], casting='unsafe')
        if mean is not None:
            np.subtract(res, np.float32(mean), out=res)
            np.divide(res, np.float32(stddev), out=res)
        res = torch.from_numpy(res)
        return res if out is None else out.copy_(res)
    lib = _lib.load()
    if not on_device:
        idx = torch.from_numpy(pos).to(table.device)
    if out is None:
        out = torch.empty(shape, device=table.device, dtype=torch.float32)
    row_elems = table.numel() // rows if rows else max(1, math.prod(table.shape[1:]))
    check(lib.sg_gather_rows(_ptr(table), SRC_DT[table.dtype], rows, row_elems, _ptr(idx), n, _ptr(out),
                             0 if mean is None else 1, 0.0 if mean is None else float(mean), 1.0 if mean is None else float(stddev),
                             _stream()), 'sg_gather_rows')
    return out


# ---- voxel-intensity histograms
HIST_DT = dict(SRC_DT)
HIST_DT[torch.bfloat16] = _lib.SG_SRC_BF16


def intensity_hist(x, lo, hi, scale=1.0, shift=0.0, pooled=False, out=None, accumulate=False):
    """int64 [rows, hi - lo + 1] counts of x [n, ...] (u8 / i8 / i16 / u16 / f16 / bf16 / f32, contiguous, on the device) in the
    unit-wide bins of [lo, hi] after t = x * scale + shift, two correctly rounded f32 operations (sg_intensity_hist, one
    launch): column min(floor(t) - lo, hi - lo - 1), values under lo in the first bin and values from hi on in the last (the top
    edge is closed), NaN in the extra last column -- so every row sums to its element count.  pooled=False: one row per
    sample; pooled=True: one row for the whole batch.  out: an int64 buffer of the result's shape; accumulate=True adds to it
    instead of overwriting it."""
    if not torch.is_tensor(x):
        raise TypeError(f'intensity_hist: expected a tensor, got {type(x).__name__}')
    if x.dtype not in HIST_DT:
        raise TypeError(f'intensity_hist: inputs are uint8, int8, int16, uint16, float16, bfloat16 or float32, got {x.dtype}')
    if x.dim() < 1 or not x.is_contiguous():
        raise ValueError('intensity_hist: expected a contiguous [n, ...] tensor')
    lo, hi = int(lo), int(hi)
    if hi <= lo:
        raise ValueError(f'intensity_hist: the range [{lo}, {hi}] is empty')
    bins = hi - lo
    if bins > _lib.INTENSITY_HIST_MAX_BINS:
        raise ValueError(f'intensity_hist: {bins} bins, at most {_lib.INTENSITY_HIST_MAX_BINS} fit the kernel\'s LDS image')
    if lo < -2 ** 31 or hi > 2147483520:      # (the largest int32 a float32 holds)
        raise ValueError(f'intensity_hist: the range [{lo}, {hi}] does not fit 32-bit integers that float32 can bound')
    if not math.isfinite(float(scale)):
        raise ValueError(f'intensity_hist: scale {scale} is not finite')
    n = x.shape[0]
    rows, row_elems = (1, x.numel()) if pooled else (n, x.numel() // n if n else math.prod(x.shape[1:]))
    shape = (rows, bins + 1)
    if out is None:
        if accumulate:
            raise ValueError('intensity_hist: accumulate=True needs the buffer to add to (out)')
    elif (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != torch.int64 or out.device != x.device
          or not out.is_contiguous()):
        raise ValueError(f'intensity_hist: out must be a contiguous int64 {shape} tensor on {x.device}')
    if not x.is_cuda:
        raise ValueError('intensity_hist: the input is a device tensor (there is no CPU path)')
    lib = _lib.load()
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=torch.int64)
    with torch.cuda.device(x.device):
        check(lib.sg_intensity_hist(_ptr(x), HIST_DT[x.dtype], rows, row_elems, float(scale), float(shift), lo, bins, _ptr(out),
                                    1 if accumulate else 0, _stream()), 'sg_intensity_hist')
    return out


# ---- sample previews: one view of every sample of a batch, rendered into a u8 canvas
VIEW_MODES = {'slice': _lib.SG_VIEW_SLICE, 'max': _lib.SG_VIEW_MAX, 'mean': _lib.SG_VIEW_MEAN}
VIEW_AXES = {'d': 0, 'h': 1, 'w': 2}


def view_volumes(x):
    """(x, (n, d, h, w, c)): the NDHWC reading of a batch for render_view -- [n, d, h, w]; [n, 1, d, h, w] in either memory format
    (with one channel NCDHW and NDHWC are the same memory); or [n, d, h, w, c]."""
    if not torch.is_tensor(x):
        raise TypeError(f'render_view: expected a tensor, got {type(x).__name__}')
    if x.dtype not in HIST_DT:
        raise TypeError(f'render_view: inputs are uint8, int8, int16, uint16, float16, bfloat16 or float32, got {x.dtype}')
    if x.dim() == 4:
        n, d, h, w = x.shape
        c = 1
    elif x.dim() == 5 and x.shape[1] == 1:      # (a second axis of size 1 always reads as the channel axis of NCDHW)
        n, _, d, h, w = x.shape
        c = 1
        if not x.is_contiguous() and x.is_contiguous(memory_format=torch.channels_last_3d):
            x = x.permute(0, 2, 3, 4, 1)      # the same memory, contiguous as [n, d, h, w, 1]
    elif x.dim() == 5:
        n, d, h, w, c = x.shape
    else:
        raise ValueError(f'render_view: expected [n, d, h, w], [n, 1, d, h, w] or [n, d, h, w, c], got {tuple(x.shape)}')
    if not x.is_contiguous():
        raise ValueError('render_view: expected a contiguous tensor')
    return x, (n, d, h, w, c)


def view_tile(dims, axis, zoom=(1, 1)):
    """(rows, columns) of one sample's tile: the two axes that remain, in their original order, times the zoom."""
    d, h, w = dims
    rows, cols = ((h, w), (d, w), (d, h))[axis]
    return rows * zoom[0], cols * zoom[1]


def render_view(x, axis, mode, index=None, window=(-1.0, 2.0), scale=1.0, shift=0.0, zoom=(1, 1), channel=0, canvas=None,
                origin=(0, 0), grid_cols=None, pitch=None):
    """u8 [canvas_h, canvas_w]: one view of every sample of x ([n, d, h, w], [n, 1, d, h, w] or [n, d, h, w, c]; u8 / i8 / i16 /
    u16 / f16 / bf16 / f32, contiguous, on the device), one launch (sg_render_view).  axis: the collapsed axis, 0 = D, 1 = H,
    2 = W (or 'd' / 'h' / 'w'); mode 'slice' (plane `index`, default the middle one, extent // 2), 'max' or 'mean'.  The
    grey level of v is floor(clamp(((v * scale + shift) - lo) * inv, 0, 255) + 0.5) in f32, inv = f32(255 / (hi - lo)), window =
    (lo, hi) in data units.  zoom = (rows, columns): integer nearest repeat.  Sample i's tile starts at origin + (i // grid_cols *
    pitch[0], i % grid_cols * pitch[1]); grid_cols defaults to n (one row of tiles) and pitch to the tile's size.  canvas: a u8
    tensor to draw into (pixels outside the tiles keep their values); None: a zeroed one that just holds the tiles."""
    x, (n, d, h, w, c) = view_volumes(x)
    axis = VIEW_AXES.get(axis, axis)
    if axis not in (0, 1, 2):
        raise ValueError(f'render_view: axis is 0 (D), 1 (H) or 2 (W), got {axis!r}')
    if mode not in VIEW_MODES:
        raise ValueError(f'render_view: mode is slice, max or mean, got {mode!r}')
    extent = (d, h, w)[axis]
    if mode == 'slice':
        index = extent // 2 if index is None else int(index)
        if extent and not 0 <= index < extent:
            raise ValueError(f'render_view: slice {index} lies outside the axis of {extent} planes')
    elif index is not None:
        raise ValueError(f'render_view: index belongs to slices, not to {mode}')
    lo, hi = float(window[0]), float(window[1])
    if not (math.isfinite(lo) and math.isfinite(hi)) or hi <= lo:
        raise ValueError(f'render_view: the window [{lo}, {hi}] is empty or not finite')
    if not math.isfinite(float(scale)):
        raise ValueError(f'render_view: scale {scale} is not finite')
    zoom = (int(zoom[0]), int(zoom[1]))
    if zoom[0] < 1 or zoom[1] < 1:
        raise ValueError(f'render_view: zooms are integers >= 1, got {zoom}')
    if not 0 <= int(channel) < c:
        raise ValueError(f'render_view: channel {channel} of {c}')
    tile = view_tile((d, h, w), axis, zoom)
    grid_cols = max(n, 1) if grid_cols is None else int(grid_cols)
    if grid_cols < 1:
        raise ValueError(f'render_view: grid_cols {grid_cols} < 1')
    pitch = tile if pitch is None else (int(pitch[0]), int(pitch[1]))
    origin = (int(origin[0]), int(origin[1]))
    down, across = (n - 1) // grid_cols + 1 if n else 0, min(n, grid_cols)
    if min(origin) < 0 or (down > 1 and pitch[0] < tile[0]) or (across > 1 and pitch[1] < tile[1]):
        raise ValueError(f'render_view: origin {origin} is negative or pitch {pitch} is smaller than the tile {tile}')
    need = (origin[0] + (down - 1) * pitch[0] + tile[0], origin[1] + (across - 1) * pitch[1] + tile[1]) if n else (0, 0)
    if canvas is None:
        shape = need
    elif (not torch.is_tensor(canvas) or canvas.dim() != 2 or canvas.dtype != torch.uint8 or canvas.device != x.device
          or not canvas.is_contiguous()):
        raise ValueError(f'render_view: canvas must be a contiguous 2-D uint8 tensor on {x.device}')
    else:
        shape = tuple(canvas.shape)
        if need[0] > shape[0] or need[1] > shape[1]:
            raise ValueError(f'render_view: the tiles end at {need}, outside the canvas {shape}')
    if not x.is_cuda:
        raise ValueError('render_view: the input is a device tensor (there is no CPU path)')
    lib = _lib.load()
    if canvas is None:
        canvas = torch.zeros(shape, device=x.device, dtype=torch.uint8)
    import numpy as np
    lo32, hi32 = np.float32(lo), np.float32(hi)      # the window as the kernel holds it
    if not hi32 > lo32:
        raise ValueError(f'render_view: the window [{lo}, {hi}] is empty in float32')
    inv = float(np.float32(255.0 / (float(hi32) - float(lo32))))
    with torch.cuda.device(x.device):
        check(lib.sg_render_view(_ptr(x), HIST_DT[x.dtype], n, d, h, w, c, int(channel), axis, VIEW_MODES[mode],
                                 index if mode == 'slice' else 0, zoom[0], zoom[1], float(scale), float(shift), float(lo32),
                                 float(hi32), inv, _ptr(canvas), shape[0], shape[1], origin[0], origin[1], grid_cols, pitch[0],
                                 pitch[1], _stream()), 'sg_render_view')
    return canvas


# ---- the per-phase dataset pyramid: pad / crop to the target, subtract the intercept, block-reduce by 2, 4, ..., clip, cast
PYR_MODES = {'mean': _lib.SG_PYR_MEAN, 'max': _lib.SG_PYR_MAX}
PYR_ANCHORS = ('center', 'start', 'end')
PYR_OUT_DT = {torch.uint16: _lib.SG_SRC_U16, torch.int16: _lib.SG_SRC_I16, torch.float32: _lib.SG_SRC_F32}
_PYR_RANGE = {torch.uint16: (0, 65535), torch.int16: (-32768, 32767), torch.float32: (-2 ** 31, 2 ** 31 - 1)}
_PYR_SCALAR_MAX = 2 ** 30      # |intercept|, |pad_value| of integer sources: x - intercept stays a 32-bit integer
_PYR_EXTENT_MAX = 2 ** 29


def pyramid_offsets(source, target, anchor=('center',) * 3):
    """Per axis the source index of target index 0.  'center' is the original's pad_to / crop_to: a short axis gets
    floor((T - S) / 2) voxels in front, a long one starts at S // 2 - T // 2; 'start': offset 0 (pad and crop at the end); 'end':
    pad in front and crop from the front."""
    if isinstance(anchor, str):
        anchor = (anchor,) * 3
    if len(anchor) != 3 or any(a not in PYR_ANCHORS for a in anchor):
        raise ValueError(f'block_pyramid: anchor is center, start or end per axis, got {anchor!r}')
    off = []
    for s, t, a in zip(source, target, anchor):
        if a == 'start':
            off.append(0)
        elif a == 'end':
            off.append(s - t)
        else:
            off.append(-((t - s) // 2) if s < t else s // 2 - t // 2)
    return tuple(off)


def _pyramid_numpy(x, target, off, levels, mode, intercept, pad, lo, hi, out_dtype, want_stats):
    """The CPU path: the kernel's definition in numpy (windowed copy by index, integer sums, integer division toward zero)."""
    import numpy as np
    a = x.numpy()
    n, is_int = a.shape[0], a.dtype.kind in 'iu'
    out_np = {torch.uint16: np.uint16, torch.int16: np.int16, torch.float32: np.float32}[out_dtype]
    if is_int:
        v = np.full((n,) + tuple(target), pad - intercept, np.int64 if mode == 'mean' else np.int32)
    else:
        v = np.full((n,) + tuple(target), np.float32(pad) - np.float32(intercept), np.float32)
    t0 = [max(0, -o) for o in off]
    t1 = [min(t, s - o) for t, s, o in zip(target, a.shape[1:], off)]
    if all(p < q for p, q in zip(t0, t1)):
        dst = (slice(None),) + tuple(slice(p, q) for p, q in zip(t0, t1))
        src = (slice(None),) + tuple(slice(p + o, q + o) for p, q, o in zip(t0, t1, off))
        v[dst] = a[src].astype(np.int64) - intercept if is_int else a[src].astype(np.float32) - np.float32(intercept)
    if mode == 'mean':
        part = v if is_int else v.astype(np.float64)
    else:
        part = v if is_int else np.fmax(v, np.float32(-np.inf))      # (the maximum from -inf: a NaN voxel is ignored)
    outs, stats = [], np.zeros((n, levels, 4), np.int64)
    for i in range(levels):
        if i:
            d, h, w = part.shape[1:]
            cubes = part.reshape(n, d // 2, 2, h // 2, 2, w // 2, 2)
            with np.errstate(invalid='ignore'):
                part = cubes.sum(axis=(2, 4, 6)) if mode == 'mean' else cubes.max(axis=(2, 4, 6))
        if out_np is np.float32:
            with np.errstate(invalid='ignore'):
                r = (part.astype(np.float64) / np.float64(8 ** i)).astype(np.float32) if mode == 'mean' else part.astype(np.float32)
                stored = np.clip(r, np.float32(lo), np.float32(hi))
        else:
            q = part.astype(np.int64)
            if mode == 'mean' and i:
                q = np.where(q < 0, -((-q) >> (3 * i)), q >> (3 * i))      # toward zero
            stored = np.clip(q, lo, hi).astype(out_np)
            s = stored.reshape(n, -1).astype(np.int64)
            stats[:, i] = np.stack([s.sum(1), (s * s).sum(1), s.min(1), s.max(1)], axis=1)
        outs.append(torch.from_numpy(np.ascontiguousarray(stored)))
    return outs, (torch.from_numpy(stats) if want_stats else None)


def block_pyramid_launch(x, target, off, levels, mode, intercept, pad, lo, hi, out_dtype, want_stats=False):
    """One sg_block_pyramid launch on checked arguments, the window given by its offsets: (outs, stats)."""
    import ctypes as C
    lib = _lib.load()
    n = x.shape[0]
    is_int = not x.dtype.is_floating_point
    outs = [torch.empty((n,) + tuple(t >> i for t in target), device=x.device, dtype=out_dtype) for i in range(levels)]
    stats = torch.empty((n, levels, 4), device=x.device, dtype=torch.int64) if want_stats else None
    ptrs = (C.c_void_p * levels)(*[o.data_ptr() for o in outs])
    ii, ip, ilo, ihi = (int(intercept), int(pad), int(lo), int(hi)) if is_int else (0, 0, 0, 0)
    fi, fp, flo, fhi = (0.0, 0.0, 0.0, 0.0) if is_int else (float(intercept), float(pad), float(lo), float(hi))
    with torch.cuda.device(x.device):
        check(lib.sg_block_pyramid(_ptr(x), SRC_DT[x.dtype], n, x.shape[1], x.shape[2], x.shape[3], target[0], target[1], target[2],
                                   off[0], off[1], off[2], levels, PYR_MODES[mode], ii, ip, ilo, ihi, fi, fp, flo, fhi,
                                   PYR_OUT_DT[out_dtype], ptrs, _ptr(stats), _stream()), 'sg_block_pyramid')
    return outs, stats


def block_pyramid(x, target, levels, reduce='mean', intercept=0, pad_value=None, clip=None, out_dtype=torch.uint16,
                  anchor=('center',) * 3, stats=False):
    """The dataset pyramid of a batch x [n, sd, sh, sw] (u8 / i8 / i16 / u16 / f16 / f32, contiguous): a list of `levels` tensors
    [n, D >> i, H >> i, W >> i] of out_dtype (uint16, int16 or float32; float sources: float32), target = (D, H, W), every extent a
    multiple of 2 ** (levels - 1).  Every volume is padded with pad_value (None: the intercept, so the padding is 0 after the
    shift) or cropped to the target, anchored per axis (pyramid_offsets); then v = x - intercept, level i is the mean (integers:
    the exact sum divided by 8 ** i toward zero -- the bits of np.clip(block_reduce(v, 2 ** i, np.average), lo, hi).astype(T)) or
    the maximum over the 2 ** i cubes, clipped to clip = (lo, hi) (None: the output type's range).  On the device one
    sg_block_pyramid launch reads x once and writes all levels, at most six.  stats=True: also the int64 [n, levels, 4] sum, sum of squares, minimum and maximum of the stored
    values (integer out_dtype).  A CPU tensor takes a numpy path with the same integer definition."""
    if not torch.is_tensor(x):
        raise TypeError(f'block_pyramid: expected a tensor, got {type(x).__name__}')
    if x.dtype not in SRC_DT:
        raise TypeError(f'block_pyramid: sources are uint8, int8, int16, uint16, float16 or float32, got {x.dtype}')
    if out_dtype not in PYR_OUT_DT:
        raise TypeError(f'block_pyramid: out_dtype is uint16, int16 or float32, got {out_dtype}')
    is_int = not x.dtype.is_floating_point
    if not is_int and out_dtype != torch.float32:
        raise TypeError(f'block_pyramid: a {x.dtype} source takes out_dtype float32, got {out_dtype}')
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f'block_pyramid: expected a contiguous [n, d, h, w] tensor, got {tuple(x.shape)}')
    if reduce not in PYR_MODES:
        raise ValueError(f'block_pyramid: reduce is mean or max, got {reduce!r}')
    target = tuple(int(t) for t in target)
    levels = int(levels)
    if len(target) != 3 or min(target) < 0 or max(target + tuple(x.shape[1:])) > _PYR_EXTENT_MAX:
        raise ValueError(f'block_pyramid: target is (D, H, W) with extents in [0, 2^29], got {target} for a source {tuple(x.shape[1:])}')
    if not 1 <= levels <= _lib.SG_PYRAMID_LEVELS_PER_LAUNCH:
        raise ValueError(f'block_pyramid: levels is 1 .. {_lib.SG_PYRAMID_LEVELS_PER_LAUNCH}, got {levels}')
    for name, t in zip('DHW', target):
        if t % (1 << (levels - 1)):
            raise ValueError(f'block_pyramid: target {name} = {t} is not a multiple of 2^{levels - 1} for {levels} levels')
    if stats and out_dtype == torch.float32:
        raise ValueError('block_pyramid: stats are the exact integer sums of integer outputs; reduce float32 levels yourself')
    off = pyramid_offsets(x.shape[1:], target, anchor)
    pad_value = intercept if pad_value is None else pad_value
    if is_int:
        for name, s in (('intercept', intercept), ('pad_value', pad_value)):
            if int(s) != s or abs(int(s)) > _PYR_SCALAR_MAX:
                raise ValueError(f'block_pyramid: {name} of an integer source is an integer within +-2^30, got {s!r}')
        intercept, pad_value = int(intercept), int(pad_value)
        lo, hi = _PYR_RANGE[out_dtype] if clip is None else clip
        if int(lo) != lo or int(hi) != hi:
            raise ValueError(f'block_pyramid: clip bounds of an integer source are integers, got {clip!r}')
        lo, hi = int(lo), int(hi)
        if lo > hi or lo < _PYR_RANGE[out_dtype][0] or hi > _PYR_RANGE[out_dtype][1]:
            raise ValueError(f'block_pyramid: clip ({lo}, {hi}) is empty or outside {out_dtype}')
    else:
        intercept, pad_value = float(intercept), float(pad_value)
        lo, hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
        if not lo <= hi:
            raise ValueError(f'block_pyramid: clip ({lo}, {hi}) is empty')
        if not (math.isfinite(intercept) and math.isfinite(pad_value)):
            raise ValueError('block_pyramid: intercept and pad_value are finite')
    n = x.shape[0]
    if not x.is_cuda:
        outs, st = _pyramid_numpy(x, target, off, levels, reduce, intercept, pad_value, lo, hi, out_dtype, stats)
        return (outs, st) if stats else outs
    outs, st = block_pyramid_launch(x, target, off, levels, reduce, intercept, pad_value, lo, hi, out_dtype, stats)
    if stats and (n == 0 or 0 in target):      # (nothing was launched: the statistics keep their identities)
        st = torch.tensor([0, 0, 2 ** 63 - 1, -2 ** 63], device=x.device).expand(n, levels, 4).contiguous()
    return (outs, st) if stats else outs


# ---- resampling to a common voxel spacing: one tap table per axis, built here in f64; a separable f64 evaluation in table order
RESAMPLE_MODES = ('nearest', 'linear', 'antialias')
_RS_OUT_NP = {torch.uint16: 'uint16', torch.int16: 'int16', torch.float32: 'float32'}
_RS_MAX_K = 15      # the widest antialiasing triangle: 2 * 15 + 1 = 31 taps of SG_RESAMPLE_MAX_TAPS


def resample_taps(S, O, step, start, mode='linear'):
    """The tap table of one axis: (inside bool [O], index int32 [O, T], weight float32 [O, T]).  Output index o sits at the source
    coordinate c = start + o * step (numpy f64; a negative step is a flipped axis) and is inside when -0.5 <= c <= S - 0.5 (ITK's
    buffer test).  nearest: one tap floor(c + 0.5).  linear: floor(c) and floor(c) + 1 with weights 1 - f and f.  antialias: a
    triangle of half-width k = max(1, |step|) source voxels -- the T = floor(2 k) + 1 taps from ceil(c - k) on, weight
    max(0, 1 - |i - c| / k) normalised to sum 1 in f64 (taps past floor(c + k) get 0); at |step| <= 1 the triangle IS the linear
    kernel and the linear table is returned; k > 15 is a ValueError.  Indices are clamped to [0, S - 1] (the edge voxel repeats);
    weights are rounded to f32 last."""
    import numpy as np
    S, O = int(S), int(O)
    step, start = float(step), float(start)
    if mode not in RESAMPLE_MODES:
        raise ValueError(f'resample_taps: mode is nearest, linear or antialias, got {mode!r}')
    if S < 1 or O < 0:
        raise ValueError(f'resample_taps: a source extent >= 1 and an output extent >= 0, got {S} and {O}')
    if not math.isfinite(step) or step == 0.0 or not math.isfinite(start):
        raise ValueError(f'resample_taps: step is finite and not 0, start is finite, got {step!r} and {start!r}')
    k = max(1.0, abs(step))
    if mode == 'antialias':
        if k > _RS_MAX_K:
            raise ValueError(f'resample_taps: antialias spans |step| <= {_RS_MAX_K} source voxels, got {step!r}')
        if k == 1.0:
            mode = 'linear'
    c = start + np.arange(O, dtype=np.float64) * step
    inside = (c >= -0.5) & (c <= S - 0.5)
    if mode == 'nearest':
        idx = np.floor(c + 0.5)[:, None]
        w = np.ones((O, 1), np.float64)
    elif mode == 'linear':
        i0 = np.floor(c)
        f = c - i0
        idx = np.stack([i0, i0 + 1.0], axis=1)
        w = np.stack([1.0 - f, f], axis=1)
    else:
        T = int(math.floor(2.0 * k)) + 1
        idx = np.ceil(c - k)[:, None] + np.arange(T, dtype=np.float64)[None, :]
        w = np.maximum(0.0, 1.0 - np.abs(idx - c[:, None]) / k)
        w = w / w.sum(axis=1, keepdims=True)
    idx = np.clip(idx, 0, S - 1).astype(np.int32)
    return inside, idx, w.astype(np.float32)


def _pack_taps(taps):
    """(inside, index, weight) -> the int32 [1 + 2 T][O] image sg_resample_axes reads (tap-major)."""
    import numpy as np
    inside, idx, w = taps
    return np.ascontiguousarray(np.concatenate([inside.astype(np.int32)[None, :], idx.T, np.ascontiguousarray(w.T).view(np.int32)], axis=0))


def _resample_store(acc, out_np):
    import numpy as np
    if out_np == 'float32':
        with np.errstate(over='ignore', invalid='ignore'):
            return acc.astype(np.float32)
    info = np.iinfo(out_np)
    return np.clip(np.rint(acc), info.min, info.max).astype(out_np)


def _resample_numpy(x, taps, out_shape, fill, out_dtype):
    """The CPU path: the kernel's definition in numpy f64, in the same order -- vectorised over voxels, looping over taps."""
    import numpy as np
    a = x.numpy()
    out_np = _RS_OUT_NP[out_dtype]
    (ins_d, id_, wd), (ins_h, ih, wh), (ins_w, iw, ww) = taps
    od, oh, ow = out_shape
    y = np.empty((a.shape[0], od, oh, ow), out_np)
    filled = _resample_store(np.float64(fill), out_np)
    inside = ins_d[:, None, None] & ins_h[None, :, None] & ins_w[None, None, :]
    if not inside.any() or 0 in a.shape[1:]:
        y[...] = filled
        return torch.from_numpy(y)
    # the source planes some inside output plane reads with a weight that is not 0
    planes = np.unique(id_[(wd != 0) & ins_d[:, None]])
    slot = np.zeros(a.shape[1], np.int64)
    slot[planes] = np.arange(len(planes))
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(a.shape[0]):
            mid = np.empty((len(planes), oh, ow), np.float64)
            for p, d in enumerate(planes):
                v = a[s, d]
                inner = np.zeros((a.shape[2], ow), np.float64)
                for k in range(ww.shape[1]):
                    term = ww[:, k].astype(np.float64)[None, :] * v[:, iw[:, k]].astype(np.float64)
                    inner = np.where((ww[:, k] != 0)[None, :], inner + term, inner)
                m = np.zeros((oh, ow), np.float64)
                for j in range(wh.shape[1]):
                    term = wh[:, j].astype(np.float64)[:, None] * inner[ih[:, j], :]
                    m = np.where((wh[:, j] != 0)[:, None], m + term, m)
                mid[p] = m
            acc = np.zeros((od, oh, ow), np.float64)
            for i in range(wd.shape[1]):
                term = wd[:, i].astype(np.float64)[:, None, None] * mid[slot[id_[:, i]]]
                acc = np.where((wd[:, i] != 0)[:, None, None], acc + term, acc)
            y[s] = np.where(inside, _resample_store(acc, out_np), filled)
    return torch.from_numpy(y)


def resample_launch(x, packed, taps_per_axis, out_shape, fill, out_dtype):
    """One sg_resample_axes launch on checked arguments; packed: the three device tables (_pack_taps images)."""
    lib = _lib.load()
    n = x.shape[0]
    y = torch.empty((n,) + tuple(out_shape), device=x.device, dtype=out_dtype)
    is_int = not x.dtype.is_floating_point
    with torch.cuda.device(x.device):
        check(lib.sg_resample_axes(_ptr(x), SRC_DT[x.dtype], n, x.shape[1], x.shape[2], x.shape[3], out_shape[0], out_shape[1],
                                   out_shape[2], _ptr(packed[0]), taps_per_axis[0], _ptr(packed[1]), taps_per_axis[1],
                                   _ptr(packed[2]), taps_per_axis[2], int(fill) if is_int else 0, 0.0 if is_int else float(fill),
                                   PYR_OUT_DT[out_dtype], _ptr(y), _stream()), 'sg_resample_axes')
    return y


def resample_volume(x, out_shape, step, start, mode='linear', fill=0, out_dtype=None):
    """x [n, sd, sh, sw] (u8 / i8 / i16 / u16 / f16 / f32, contiguous) resampled to [n, od, oh, ow] of out_dtype (uint16, int16 or
    float32; None: int16 for signed integer sources, uint16 for unsigned, float32 for floats, which take nothing else).  Per axis,
    output index o reads the source coordinate start + o * step (step, start: one number per axis; a negative step flips) through
    the taps of resample_taps(mode) (mode: one name, or one per axis); an output voxel outside the source on any axis is `fill`
    (an integer for integer sources).  A voxel inside is the f64 sum over the d taps of wd * (the sum over the h taps of wh * (the
    sum over the w taps of ww * x)), in table order, a tap of weight 0 skipped; then one rounding to float32, or rint (ties to
    even) and a clamp to the integer type.  On the device that is one sg_resample_axes launch; a CPU tensor takes the same
    definition in numpy and gives the same bits."""
    if not torch.is_tensor(x):
        raise TypeError(f'resample_volume: expected a tensor, got {type(x).__name__}')
    if x.dtype not in SRC_DT:
        raise TypeError(f'resample_volume: sources are uint8, int8, int16, uint16, float16 or float32, got {x.dtype}')
    is_int = not x.dtype.is_floating_point
    if out_dtype is None:
        out_dtype = torch.float32 if not is_int else torch.uint16 if x.dtype in (torch.uint8, torch.uint16) else torch.int16
    if out_dtype not in PYR_OUT_DT:
        raise TypeError(f'resample_volume: out_dtype is uint16, int16 or float32, got {out_dtype}')
    if not is_int and out_dtype != torch.float32:
        raise TypeError(f'resample_volume: a {x.dtype} source takes out_dtype float32, got {out_dtype}')
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError(f'resample_volume: expected a contiguous [n, d, h, w] tensor, got {tuple(x.shape)}')
    try:
        out_shape = tuple(int(t) for t in out_shape)
        step, start = tuple(float(s) for s in step), tuple(float(s) for s in start)
    except TypeError:
        raise ValueError('resample_volume: out_shape, step and start are one number per axis (d, h, w)')
    if len(out_shape) != 3 or len(step) != 3 or len(start) != 3:
        raise ValueError(f'resample_volume: out_shape, step and start are one number per axis (d, h, w), got {out_shape}, {step}, {start}')
    if min(out_shape) < 0 or max(out_shape + tuple(x.shape[1:])) > _PYR_EXTENT_MAX:
        raise ValueError(f'resample_volume: extents lie in [0, 2^29], got {out_shape} from {tuple(x.shape[1:])}')
    modes = (mode,) * 3 if isinstance(mode, str) else tuple(mode)
    if len(modes) != 3 or any(m not in RESAMPLE_MODES for m in modes):
        raise ValueError(f'resample_volume: mode is nearest, linear or antialias (one, or one per axis), got {mode!r}')
    if is_int:
        if isinstance(fill, bool) or int(fill) != fill or abs(int(fill)) >= 2 ** 31:
            raise ValueError(f'resample_volume: fill of an integer source is a 32-bit integer, got {fill!r}')
        fill = int(fill)
    else:
        fill = float(fill)
    n = x.shape[0]
    if n == 0 or 0 in out_shape:
        return torch.empty((n,) + out_shape, device=x.device, dtype=out_dtype)
    # (an empty source axis has no voxel to tap: its table is all outside)
    taps = []
    for S, O, st, s0, m in zip(x.shape[1:], out_shape, step, start, modes):
        if S == 0:
            import numpy as np
            resample_taps(1, O, st, s0, m)      # (the argument checks)
            taps.append((np.zeros(O, bool), np.zeros((O, 1), np.int32), np.zeros((O, 1), np.float32)))
        else:
            taps.append(resample_taps(S, O, st, s0, m))
    if not x.is_cuda:
        return _resample_numpy(x, taps, out_shape, fill, out_dtype)
    packed = [torch.from_numpy(_pack_taps(t)).to(x.device) for t in taps]
    return resample_launch(x, packed, [t[1].shape[1] for t in taps], out_shape, fill, out_dtype)


# ---- typed volumes from the generator's output: de-normalise, clip, round, cast, per-sample statistics
STORE_SRC_DT = {torch.float32: _lib.SG_SRC_F32, torch.bfloat16: _lib.SG_SRC_BF16, torch.float16: _lib.SG_SRC_F16}
STORE_OUT_DT = {torch.int16: _lib.SG_SRC_I16, torch.uint16: _lib.SG_SRC_U16, torch.uint8: _lib.SG_SRC_U8, torch.float32: _lib.SG_SRC_F32}
STORE_ROUNDINGS = {'trunc': _lib.SG_ROUND_TRUNC, 'rint': _lib.SG_ROUND_RINT}
_STORE_RANGE = {torch.int16: (-32768, 32767), torch.uint16: (0, 65535), torch.uint8: (0, 255)}
_STORE_NP = {torch.int16: 'int16', torch.uint16: 'uint16', torch.uint8: 'uint8', torch.float32: 'float32'}
STORE_DEFINITION = ('t = f32(x) * f32(scale) + f32(shift), two roundings; nan = isnan(t), below = t < lo, above = t > hi; '
                    'u = lo if nan or below, hi if above, else t; stored = T(trunc(u)) or T(rint(u), ties to even) for an integer T, '
                    'NaN if nan else u for float32')


def _store_numpy(x, out_dtype, scale, shift, lo, hi, rounding, want_stats):
    """The CPU path: the kernel's definition in numpy, operation by operation."""
    import numpy as np
    a = x.float().numpy().astype(np.float32, copy=False)      # [n, c, d, h, w] by index, whatever the strides (every source converts exactly)
    n = a.shape[0]
    flo, fhi = np.float32(lo), np.float32(hi)
    with np.errstate(over='ignore', invalid='ignore'):
        t = a * np.float32(scale) + np.float32(shift)
        nan, below, above = np.isnan(t), t < flo, t > fhi
    u = np.where(nan | below, flo, np.where(above, fhi, t)).astype(np.float32)
    st = np.zeros((n, 7), np.int64)
    if out_dtype == torch.float32:
        stored = np.where(nan, np.float32(np.nan), u).astype(np.float32)
    else:
        stored = (np.rint(u) if rounding == 'rint' else np.trunc(u)).astype(_STORE_NP[out_dtype])
        if n and stored[0].size:
            s = stored.reshape(n, -1).astype(np.int64)
            st[:, :4] = np.stack([s.sum(1), (s * s).sum(1), s.min(1), s.max(1)], axis=1)
    st[:, 4:] = np.stack([m.sum(axis=(1, 2, 3, 4)) for m in (below, above, nan)], axis=1)
    return torch.from_numpy(np.ascontiguousarray(stored)), (torch.from_numpy(st) if want_stats else None)


def store_volumes(x, out_dtype, scale=1.0, shift=0.0, clip=None, rounding='trunc', stats=False, out=None):
    """A batch x [n, c, d, h, w] (f32 / bf16 / f16; contiguous, or channels_last_3d: transposed on the way) mapped back to data units
    and stored as a contiguous [n, c, d, h, w] of out_dtype (int16, uint16, uint8 or float32), one pass (sg_store_volumes).  Per
    element, exactly: t = x * scale + shift in two correctly rounded f32 operations -- numpy's x * np.float32(scale) +
    np.float32(shift); nan, below, above = isnan(t), t < lo, t > hi with clip = (lo, hi) (None: the type's range, +-inf for
    float32; integers for an integer type); u = lo where nan or below, hi where above, else t; stored = T(trunc(u)) -- the bits of
    (np.clip(x, a, b) * s).astype(T) -- or T(rint(u)), ties to even; float32: NaN where nan, else u.  stats=True: (out, int64
    [n, 7]) = the sum, sum of squares, minimum and maximum of every sample's stored values (zeros for float32), then its numbers
    of below, above and nan elements: integer sums, two calls give the same bits.  out: a contiguous buffer of the result's
    shape and type on x's device to write into.  A CPU tensor takes the same definition in numpy and gives the same bits."""
    if not torch.is_tensor(x):
        raise TypeError(f'store_volumes: expected a tensor, got {type(x).__name__}')
    if x.dtype not in STORE_SRC_DT:
        raise TypeError(f'store_volumes: sources are float32, bfloat16 or float16, got {x.dtype}')
    if out_dtype not in STORE_OUT_DT:
        raise TypeError(f'store_volumes: out_dtype is int16, uint16, uint8 or float32, got {out_dtype}')
    if x.dim() != 5:
        raise ValueError(f'store_volumes: expected [n, c, d, h, w], got {tuple(x.shape)}')
    n, c, d, h, w = x.shape
    if c < 1:
        raise ValueError(f'store_volumes: expected at least one channel, got {tuple(x.shape)}')
    channels_last = not x.is_contiguous()
    if channels_last and not x.is_contiguous(memory_format=torch.channels_last_3d):
        raise ValueError('store_volumes: expected a contiguous or channels_last_3d tensor')
    if rounding not in STORE_ROUNDINGS:
        raise ValueError(f'store_volumes: rounding is trunc or rint, got {rounding!r}')
    if not math.isfinite(float(scale)):
        raise ValueError(f'store_volumes: scale {scale} is not finite')
    if clip is not None and len(clip) != 2:
        raise ValueError(f'store_volumes: clip is (lo, hi), got {clip!r}')
    if out_dtype == torch.float32:
        lo, hi = (-math.inf, math.inf) if clip is None else (float(clip[0]), float(clip[1]))
        if not lo <= hi:
            raise ValueError(f'store_volumes: clip ({lo}, {hi}) is empty')
    else:
        lo, hi = _STORE_RANGE[out_dtype] if clip is None else clip
        if isinstance(lo, bool) or isinstance(hi, bool) or not (math.isfinite(lo) and math.isfinite(hi)) or int(lo) != lo or int(hi) != hi:
            raise ValueError(f'store_volumes: clip bounds of an integer out_dtype are integers, got {clip!r}')
        lo, hi = int(lo), int(hi)
        if lo > hi or lo < _STORE_RANGE[out_dtype][0] or hi > _STORE_RANGE[out_dtype][1]:
            raise ValueError(f'store_volumes: clip ({lo}, {hi}) is empty or outside {out_dtype}')
    shape = (n, c, d, h, w)
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != shape or out.dtype != out_dtype or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError(f'store_volumes: out must be a contiguous {out_dtype} {shape} tensor on {x.device}')
    if not x.is_cuda:
        res, st = _store_numpy(x, out_dtype, scale, shift, lo, hi, rounding, stats)
        res = res if out is None else out.copy_(res)
        return (res, st) if stats else res
    lib = _lib.load()
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=out_dtype)
    st = torch.zeros((n, 7), device=x.device, dtype=torch.int64) if stats else None      # (nothing is launched for an empty batch)
    with torch.cuda.device(x.device):
        check(lib.sg_store_volumes(_ptr(x), STORE_SRC_DT[x.dtype], 1 if channels_last else 0, n, c, d, h, w, float(scale), float(shift),
                                   float(lo), float(hi), STORE_ROUNDINGS[rounding], STORE_OUT_DT[out_dtype], _ptr(out), _ptr(st),
                                   _stream()), 'sg_store_volumes')
    return (out, st) if stats else out


# ---- exact squared distances between typed integer rows, and the running k nearest (metrics/memorisation.py)
SQDIST_DT = {torch.uint8: _lib.SG_SRC_U8, torch.int8: _lib.SG_SRC_I8, torch.int16: _lib.SG_SRC_I16, torch.uint16: _lib.SG_SRC_U16}
TOPK_MAX = 16
_I64_MAX = 2 ** 63 - 1


def _sqdist_rows(x, name):
    if not torch.is_tensor(x):
        raise TypeError(f'sqdist_exact: expected a tensor for {name}, got {type(x).__name__}')
    if x.dtype not in SQDIST_DT:
        raise TypeError(f'sqdist_exact: rows are uint8, int8, int16 or uint16, got {x.dtype} for {name}')
    if x.dim() < 1 or x.shape[0] < 1 or not x.is_contiguous():
        raise ValueError(f'sqdist_exact: expected a contiguous [m, ...] tensor with m >= 1 for {name}, got {tuple(x.shape)}')
    x = x.view(x.shape[0], -1)
    if not 1 <= x.shape[1] < 2 ** 31:
        raise ValueError(f'sqdist_exact: rows of 1 .. 2^31 - 1 elements, got {x.shape[1]} for {name}')
    return x


def sqdist_exact(q, r=None):
    """int64 [mq, mr]: out[i][j] = sum_e (q[i][e] - r[j][e])^2, exactly, for q [mq, ...] and r [mr, ...] of one integer type (u8 / i8 /
    i16 / u16; contiguous, flattened per row).  r=None: q against itself -- the upper triangle computed, mirrored, a zero diagonal.
    On the device: sg_sqdist_exact, byte-split int8 MFMAs with integer accumulation, the same bits on every call.  A CPU tensor
    takes numpy int64 arithmetic and gives the same numbers."""
    sym = r is None or r is q
    q = _sqdist_rows(q, 'q')
    r = q if sym else _sqdist_rows(r, 'r')
    if r.dtype != q.dtype:
        raise TypeError(f'sqdist_exact: q is {q.dtype} and r is {r.dtype}')
    if r.shape[1] != q.shape[1]:
        raise ValueError(f'sqdist_exact: {q.shape[1]} and {r.shape[1]} elements per row')
    if r.device != q.device:
        raise ValueError('sqdist_exact: q and r on different devices')
    mq, mr, v = q.shape[0], r.shape[0], q.shape[1]
    if not q.is_cuda:
        import numpy as np
        b = r.numpy().astype(np.int64)
        a = b if sym else q.numpy().astype(np.int64)
        res = np.empty((mq, mr), np.int64)
        for i in range(mq):
            diff = b - a[i]
            res[i] = np.einsum('jv,jv->j', diff, diff)
        return torch.from_numpy(res)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        nbytes = lib.sg_sqdist_exact_workspace(mq, mr, v)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
        out = torch.empty((mq, mr), dtype=torch.int64, device=q.device)
        check(lib.sg_sqdist_exact(_ptr(q), _ptr(r), SQDIST_DT[q.dtype], mq, mr, v, _ptr(out), _ptr(ws), nbytes, _stream()),
              'sg_sqdist_exact')
    return out


def nearest_rows(d, k, r_base=0, q_ids=None, best=None):
    """(best_d, best_id), int64 [mq, k]: per row of d [mq, mr] (int64 distances to the candidates r_base .. r_base + mr - 1) the k
    nearest so far, ascending by (distance, id) -- equal distances go to the lower id, so cutting the candidates into calls
    differently changes nothing.  best: the pair an earlier call returned, merged into in place; None: a fresh pair, INT64_MAX / -1
    (an entry that stays so is empty: fewer than k candidates).  q_ids: int64 [mq]; row i skips the candidate whose id is
    q_ids[i] (leave-one-out of a set against itself).  On the device one sg_topk_merge launch; a CPU tensor takes numpy."""
    if not torch.is_tensor(d) or d.dtype != torch.int64 or d.dim() != 2 or d.shape[0] < 1 or d.shape[1] < 1 or not d.is_contiguous():
        raise ValueError('nearest_rows: d is a contiguous int64 [mq, mr] tensor with mq, mr >= 1')
    k, r_base = int(k), int(r_base)
    if not 1 <= k <= TOPK_MAX:
        raise ValueError(f'nearest_rows: k is 1 .. {TOPK_MAX}, got {k}')
    if r_base < 0:
        raise ValueError(f'nearest_rows: r_base {r_base} < 0')
    mq, mr = d.shape
    if q_ids is not None and (not torch.is_tensor(q_ids) or q_ids.dtype != torch.int64 or tuple(q_ids.shape) != (mq,)
                              or q_ids.device != d.device or not q_ids.is_contiguous()):
        raise ValueError(f'nearest_rows: q_ids is a contiguous int64 [{mq}] tensor on {d.device}')
    if best is None:
        best = (torch.full((mq, k), _I64_MAX, dtype=torch.int64, device=d.device),
                torch.full((mq, k), -1, dtype=torch.int64, device=d.device))
    best_d, best_id = best
    for b in (best_d, best_id):
        if not torch.is_tensor(b) or b.dtype != torch.int64 or tuple(b.shape) != (mq, k) or b.device != d.device or not b.is_contiguous():
            raise ValueError(f'nearest_rows: best is a pair of contiguous int64 [{mq}, {k}] tensors on {d.device}')
    if not d.is_cuda:
        import numpy as np
        ids = np.broadcast_to(np.arange(r_base, r_base + mr, dtype=np.int64), (mq, mr))
        cd, ci = np.concatenate([best_d.numpy(), d.numpy()], axis=1), np.concatenate([best_id.numpy(), ids], axis=1)
        if q_ids is not None:
            own = np.concatenate([np.zeros((mq, k), bool), ids == q_ids.numpy()[:, None]], axis=1)
            cd, ci = np.where(own, _I64_MAX, cd), np.where(own, -1, ci)
        empty = ci < 0
        for i in range(mq):
            order = np.lexsort((ci[i], cd[i], empty[i]))[:k]      # the empty entries last, then by (distance, id)
            best_d[i], best_id[i] = torch.from_numpy(cd[i][order]), torch.from_numpy(ci[i][order])
        return best_d, best_id
    lib = _lib.load()
    with torch.cuda.device(d.device):
        check(lib.sg_topk_merge(_ptr(d), mq, mr, r_base, _ptr(q_ids), k, _ptr(best_d), _ptr(best_id), _stream()), 'sg_topk_merge')
    return best_d, best_id


# ---- projection onto the generator: the multi-scale residual loss with its gradient, and the latents' update
PROJECT_LEVELS_MAX = 6
PROJECT_DEFINITION = (
    't = (f32(x) - mean) / stddev, two roundings as gather_rows; r = f32(y) - t, one rounding; S_0 = f64(r), S_l(B) of a cube of edge '
    '2^l = the sum of its eight children in the octree\'s order: the w pairs, then the h pairs, then the d pair; m_l = S_l * 8^-l; '
    'Q_l = m_l^2 carried up the same tree to the edge-8 cubes that tile the volume from its origin (children outside count as +0), '
    'the cubes added along w, those sums along h, those over (channel, d) in index order, each sum sequential from its first '
    'element; terms_l = total / N_l with N_l = c d h w / 8^l; loss = f32(lambda_0 terms_0 + lambda_1 terms_1 + ...) in f64 and this '
    'order; grad = k_0 r + (k_1 m_1 + (k_2 m_2 + ...)) in f64 from the coarsest level down, k_l = lambda_l * (2 / N_l) / 8^l, rounded '
    'once to y\'s type (bf16 / f16 through an f32 rounded to odd)')
LATENT_STEP_DEFINITION = (
    'if loss < best_loss (never for NaN, not for an equal loss): best_loss = loss, z_best = z, best_step = step; then unless lr == 0, '
    'in f32 and operation by operation: m = b1 m + (1 - b1) g; v = b2 v + ((1 - b2) g) g; z = z - (lr (m / c1)) / (sqrt(v / c2) + eps), '
    'c_j = f32(1 - f64(b_j) ** step); then with sphere: z = f32(f64(z) * (sqrt(L) / sqrt(s))), s = the f64 sum of z_k^2 as 64 partial '
    'sums over k = j, j + 64, ... in increasing k added pairwise 32, 16, ..., 1 apart (a row with s = 0, NaN or inf is left alone)')
_LAMBDA_CACHE = {}


def _msr_weights(weights, levels):
    import numpy as np
    lam = np.ones(levels, np.float32) if weights is None else np.asarray(
        weights.detach().cpu().numpy() if torch.is_tensor(weights) else weights, dtype=np.float64)
    if lam.shape != (levels,) or not np.all(np.isfinite(lam)) or np.any(lam < 0):
        raise ValueError(f'multiscale_residual: weights are {levels} finite numbers >= 0, got {weights!r}')
    return lam.astype(np.float32)


def msr_coefficients(lam, shape, levels):
    """k_l = lambda_l * (2 / N_l) / 8^l as Python floats (f64), N_l = c d h w / 8^l: the factors of the gradient."""
    n0 = float(math.prod(shape))
    return [float(lam[l]) * (2.0 / (n0 / 8.0 ** l)) / 8.0 ** l for l in range(levels)]


def _round_once(g, dtype):
    """The f64 array g rounded ONCE to dtype: float32 directly; bfloat16 / float16 through a float32 rounded to odd (the truncated
    value with its last bit set when anything was cut off), after which the rounding to nearest even is the only one."""
    import numpy as np
    with np.errstate(over='ignore', invalid='ignore'):
        f = g.astype(np.float32)
        if dtype == torch.float32:
            return torch.from_numpy(np.ascontiguousarray(f))
        back = f.astype(np.float64)
        rz = np.where(np.abs(back) > np.abs(g), np.nextafter(f, np.float32(0)), f).astype(np.float32)
        bits = rz.view(np.uint32) | (back != g).astype(np.uint32)
        odd = np.ascontiguousarray(bits).view(np.float32)
        if dtype == torch.float16:
            return torch.from_numpy(odd.astype(np.float16))
    return torch.from_numpy(odd).to(torch.bfloat16)


def _octree_up(a):
    a = a[..., 0::2] + a[..., 1::2]
    a = a[..., 0::2, :] + a[..., 1::2, :]
    return a[..., 0::2, :, :] + a[..., 1::2, :, :]


def _seq_sum_last(a):
    acc = a[..., 0]
    for k in range(1, a.shape[-1]):
        acc = acc + a[..., k]
    return acc


def _msr_numpy(y, table, pos, mean, stddev, levels, lam):
    """The CPU path: PROJECT_DEFINITION in numpy, operation by operation.  (loss f32 [n], terms f64 [n, levels], grad like y)."""
    import numpy as np
    yf = y.float().numpy().astype(np.float32, copy=False)      # by index, whatever the strides (every type converts exactly)
    n, c, d, h, w = yf.shape
    rows = table.shape[0]
    ks = msr_coefficients(lam, (c, d, h, w), levels)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        t = np.full(yf.shape, np.nan, np.float32)
        valid = (pos >= 0) & (pos < rows)
        if valid.any():
            x = np.empty((int(valid.sum()), c, d, h, w), np.float32)
            np.copyto(x, table.numpy()[pos[valid]], casting='unsafe')
            np.subtract(x, np.float32(mean), out=x)
            np.divide(x, np.float32(stddev), out=x)
            t[valid] = x
        r = yf - t
        S, means, terms = r.astype(np.float64), [], np.empty((n, levels), np.float64)
        for l in range(levels):
            if l:
                S = _octree_up(S)
            m = S * 0.125 ** l
            means.append(m)
            q = m * m
            # (levels 5 and 6, which only this path takes, carry to cubes of the coarsest level's edge instead of 8)
            carry = max(3, levels - 1)
            edge = 1 << (carry - l)      # cells of level l along the edge of a carry cube
            pad = [(0, 0), (0, 0)] + [(0, -s % edge) for s in q.shape[2:]]
            q = np.pad(q, pad)
            for _ in range(carry - l):
                q = _octree_up(q)
            total = _seq_sum_last(_seq_sum_last(q))      # along w, then along h: [n, c, nd8]
            total = _seq_sum_last(total.reshape(n, -1))
            terms[:, l] = total / (float(c * d * h * w) / 8.0 ** l)
        acc = np.float64(lam[0]) * terms[:, 0]
        for l in range(1, levels):
            acc = acc + np.float64(lam[l]) * terms[:, l]
        loss = acc.astype(np.float32)
        g = ks[levels - 1] * means[levels - 1]
        for l in range(levels - 2, -1, -1):
            g = ks[l] * means[l] + g.repeat(2, axis=2).repeat(2, axis=3).repeat(2, axis=4)
        grad = _round_once(np.ascontiguousarray(g), y.dtype)
    if not y.is_contiguous():
        grad = grad.contiguous(memory_format=torch.channels_last_3d)
    return torch.from_numpy(loss), torch.from_numpy(terms), grad


def multiscale_residual_raw(y, table, idx, mean=0.0, stddev=1.0, levels=3, weights=None, out=None):
    """(loss f32 [n], terms f64 [n, levels], grad): the multi-scale residual loss between y [n, c, d, h, w] (f32 / bf16 / f16;
    contiguous or channels_last_3d) and the rows idx of table [rows, c, d, h, w] (u8 / i8 / i16 / u16 / f16 / f32, contiguous, in its
    stored type), normalised as gather_rows does, and d loss[i] / d y[i] in y's type and memory format -- PROJECT_DEFINITION, exactly:
    two calls give the same bits, and a CPU tensor takes the same definition in numpy and gives them too.  idx: int32 [n] on y's
    device, or host positions (uploaded); repeats are allowed; a position outside the table gives a NaN loss, NaN terms and NaN
    gradients for that sample.  levels: 1 .. 6 on the CPU, 1 .. 4 on the device (two launches: sg_multiscale_residual); every extent a
    multiple of 2^(levels - 1).  weights: `levels` numbers >= 0 (host values; None: ones).  out: a buffer for grad, of y's shape,
    type, strides and device.  No autograd: multiscale_residual has it."""
    if not torch.is_tensor(y) or not torch.is_tensor(table):
        raise TypeError('multiscale_residual: y and table are tensors')
    if y.dtype not in STORE_SRC_DT:
        raise TypeError(f'multiscale_residual: y is float32, bfloat16 or float16, got {y.dtype}')
    if table.dtype not in SRC_DT:
        raise TypeError(f'multiscale_residual: tables are uint8, int8, int16, uint16, float16 or float32, got {table.dtype}')
    if y.dim() != 5 or y.shape[1] < 1 or min(y.shape[2:]) < 1:
        raise ValueError(f'multiscale_residual: expected y [n, c, d, h, w] with no empty extent, got {tuple(y.shape)}')
    channels_last = not y.is_contiguous()
    if channels_last and not y.is_contiguous(memory_format=torch.channels_last_3d):
        raise ValueError('multiscale_residual: expected a contiguous or channels_last_3d y')
    if table.dim() != 5 or tuple(table.shape[1:]) != tuple(y.shape[1:]) or not table.is_contiguous():
        raise ValueError(f'multiscale_residual: expected a contiguous table [rows, {", ".join(str(s) for s in y.shape[1:])}], got '
                         f'{tuple(table.shape)}')
    if table.device != y.device:
        raise ValueError('multiscale_residual: y and table on different devices')
    levels = int(levels)
    if not 1 <= levels <= PROJECT_LEVELS_MAX:
        raise ValueError(f'multiscale_residual: levels is 1 .. {PROJECT_LEVELS_MAX}, got {levels}')
    for name, s in zip('dhw', y.shape[2:]):
        if s % (1 << (levels - 1)):
            raise ValueError(f'multiscale_residual: {name} = {s} is not a multiple of 2^{levels - 1} for {levels} levels')
    if not (math.isfinite(float(mean)) and math.isfinite(float(stddev))) or float(stddev) == 0.0:
        raise ValueError(f'multiscale_residual: mean and stddev are finite and stddev is not 0, got {mean!r} and {stddev!r}')
    lam = _msr_weights(weights, levels)
    if out is not None and (not torch.is_tensor(out) or out.shape != y.shape or out.dtype != y.dtype or out.device != y.device
                            or out.stride() != y.stride()):
        raise ValueError(f'multiscale_residual: out must be a {y.dtype} {tuple(y.shape)} tensor with y\'s strides on {y.device}')
    n, c, d, h, w = y.shape
    import numpy as np
    if torch.is_tensor(idx) and idx.is_cuda:
        if idx.device != y.device or idx.dtype != torch.int32 or tuple(idx.shape) != (n,) or not idx.is_contiguous():
            raise ValueError(f'multiscale_residual: device positions are a contiguous int32 [{n}] tensor on y\'s device')
    else:
        pos = np.ascontiguousarray(idx.numpy() if torch.is_tensor(idx) else idx)
        if pos.shape != (n,) or (pos.size and not np.issubdtype(pos.dtype, np.integer)):
            raise ValueError(f'multiscale_residual: expected {n} integer positions, got {pos.dtype} {pos.shape}')
        pos = pos.astype(np.int64)
        if y.is_cuda:
            idx = torch.from_numpy(np.clip(pos, -1, 2 ** 31 - 1).astype(np.int32)).to(y.device)
    if not y.is_cuda:
        loss, terms, grad = _msr_numpy(y, table, pos, mean, stddev, levels, lam)
        return loss, terms, (grad if out is None else out.copy_(grad))
    if levels > _lib.SG_MSR_DEVICE_LEVELS:
        raise ValueError(f'multiscale_residual: the device kernel reduces cubes of edge 8 in registers: levels <= {_lib.SG_MSR_DEVICE_LEVELS} '
                         f'on the device, got {levels} (the CPU path takes up to {PROJECT_LEVELS_MAX})')
    import ctypes as C
    lib = _lib.load()
    key = (tuple(float(v) for v in lam), str(y.device))
    lam_dev = _LAMBDA_CACHE.get(key)
    if lam_dev is None:
        lam_dev = _LAMBDA_CACHE[key] = torch.from_numpy(lam.copy()).to(y.device)
    ks = (C.c_double * levels)(*msr_coefficients(lam, (c, d, h, w), levels))
    grad = torch.empty_like(y) if out is None else out      # (empty_like preserves y's memory format)
    terms = torch.empty((n, levels), device=y.device, dtype=torch.float64)
    loss = torch.empty((n,), device=y.device, dtype=torch.float32)
    with torch.cuda.device(y.device):
        nbytes = lib.sg_multiscale_residual_workspace(n, c, d, h, w, levels)
        ws = torch.empty(max(nbytes, 8) // 8, device=y.device, dtype=torch.float64)
        check(lib.sg_multiscale_residual(_ptr(y), STORE_SRC_DT[y.dtype], 1 if channels_last else 0, _ptr(table), SRC_DT[table.dtype],
                                         table.shape[0], _ptr(idx), n, c, d, h, w, float(mean), float(stddev), levels, _ptr(lam_dev), ks,
                                         _ptr(grad), _ptr(terms), _ptr(loss), _ptr(ws), nbytes, _stream()), 'sg_multiscale_residual')
    return loss, terms, grad


class _MultiscaleResidual(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, table, idx, mean, stddev, levels, weights):
        loss, terms, grad = multiscale_residual_raw(y.detach(), table, idx, mean, stddev, levels, weights)
        ctx.save_for_backward(grad)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, g_loss, _g_terms):
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        grad, = ctx.saved_tensors
        return (grad * g_loss.view(-1, 1, 1, 1, 1).to(grad.dtype),) + (None,) * 6


def multiscale_residual(y, table, idx, mean=0.0, stddev=1.0, levels=3, weights=None):
    """(loss f32 [n], terms f64 [n, levels]) of multiscale_residual_raw, with autograd: the gradient is computed in the same pass
    and kept, so loss.sum().backward() delivers it to y (times the incoming gradient of every sample's loss; times 1 is exact)."""
    return _MultiscaleResidual.apply(y, table, idx, mean, stddev, levels, weights)


def _latent_step_numpy(z, m, v, g, loss, best_loss, z_best, best_step, lr, b1, b2, eps, step, sphere):
    """The CPU path: LATENT_STEP_DEFINITION in numpy, operation by operation, in place."""
    import numpy as np
    f = np.float32
    z, m, v, g, loss, best_loss, z_best, best_step = (t.numpy() for t in (z, m, v, g, loss, best_loss, z_best, best_step))
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        take = loss < best_loss
        z_best[take] = z[take]
        best_loss[take] = loss[take]
        best_step[take] = step
        if f(lr) == 0:
            return
        lr, b1, b2, eps = f(lr), f(b1), f(b2), f(eps)
        omb1, omb2 = f(1) - b1, f(1) - b2
        c1, c2 = f(1.0 - float(b1) ** step), f(1.0 - float(b2) ** step)
        m[:] = b1 * m + omb1 * g
        v[:] = b2 * v + (omb2 * g) * g
        z[:] = z - (lr * (m / c1)) / (np.sqrt(v / c2) + eps)
        if not sphere:
            return
        n, L = z.shape
        z64 = z.astype(np.float64)
        sq = np.pad(z64 * z64, [(0, 0), (0, -L % 64)]).reshape(n, -1, 64)
        p = sq[:, 0]
        for k in range(1, sq.shape[1]):
            p = p + sq[:, k]
        for s in (32, 16, 8, 4, 2, 1):
            p = p[:, :s] + p[:, s:2 * s]
        s = p[:, 0]
        ok = (s > 0) & np.isfinite(s)
        scale = np.sqrt(np.float64(L)) / np.sqrt(np.where(ok, s, 1.0))
        z[ok] = (z64 * scale[:, None]).astype(np.float32)[ok]


def latent_step_(z, m, v, grad_z, loss, best_loss, z_best, best_step, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, sphere=False):
    """One iteration of the projection on the latents z [n, L], in place on z, m, v, best_loss [n], z_best [n, L] and best_step (int32
    [n]); grad_z [n, L] and loss [n] are this iteration's (all float32, contiguous, on one device) -- LATENT_STEP_DEFINITION:
    first the best latent so far is kept (a NaN loss never wins, an equal loss does not replace), then Adam moves z, then with
    sphere=True the row is rescaled to norm sqrt(L).  lr and step (>= 1) are host numbers: the caller knows the schedule, nothing is
    read back.  lr = 0 only scores: z, m and v stay.  On the device one launch, one wave per row (sg_latent_step); CPU tensors take
    the same definition in numpy and give the same bits.  Returns z."""
    ts = (z, m, v, grad_z, loss, best_loss, z_best, best_step)
    if not all(torch.is_tensor(t) for t in ts):
        raise TypeError('latent_step_: expected tensors')
    if z.dim() != 2 or z.shape[1] < 1:
        raise ValueError(f'latent_step_: z is [n, L] with L >= 1, got {tuple(z.shape)}')
    n, L = z.shape
    for name, t, shape, dt in (('z', z, (n, L), torch.float32), ('m', m, (n, L), torch.float32), ('v', v, (n, L), torch.float32),
                               ('grad_z', grad_z, (n, L), torch.float32), ('loss', loss, (n,), torch.float32),
                               ('best_loss', best_loss, (n,), torch.float32), ('z_best', z_best, (n, L), torch.float32),
                               ('best_step', best_step, (n,), torch.int32)):
        if tuple(t.shape) != shape or t.dtype != dt or t.device != z.device or not t.is_contiguous() or t.requires_grad:
            raise ValueError(f'latent_step_: {name} must be a contiguous {dt} {shape} tensor on {z.device} that does not require grad')
    step = int(step)
    if step < 1 or step >= 2 ** 31:
        raise ValueError(f'latent_step_: step counts from 1, got {step}')
    lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
    if not (lr >= 0.0 and math.isfinite(lr)) or not 0.0 <= beta1 < 1.0 or not 0.0 <= beta2 < 1.0 or not (eps > 0.0 and math.isfinite(eps)):
        raise ValueError(f'latent_step_: lr >= 0, betas in [0, 1) and eps > 0, got lr={lr!r}, betas=({beta1!r}, {beta2!r}), eps={eps!r}')
    if not z.is_cuda:
        _latent_step_numpy(z, m, v, grad_z, loss, best_loss, z_best, best_step, lr, beta1, beta2, eps, step, bool(sphere))
        return z
    lib = _lib.load()
    with torch.cuda.device(z.device):
        check(lib.sg_latent_step(_ptr(z), _ptr(m), _ptr(v), _ptr(grad_z), _ptr(loss), _ptr(best_loss), _ptr(z_best), _ptr(best_step), n, L,
                                 lr, beta1, beta2, eps, step, 1 if sphere else 0, _stream()), 'sg_latent_step')
    return z


# ---- shell-binned power spectra (metrics/spectrum_metrics.py)
SPECTRUM_WINDOWS = ('none', 'hann')


def trig_tables(n):
    """(c, s): cos and sin of 2 pi m / n for m = 0 .. n - 1 in f64.  The angle is reduced to the first octant with integer
    arithmetic on 8 m / n, so multiples of n / 4 give exactly 0 and +-1, odd multiples of n / 8 one shared sqrt(1/2), and mirrored
    entries are bit-equal: c[n - m] == c[m], s[n - m] == -s[m], c[m + n / 2] == -c[m]."""
    import numpy as np
    n = int(n)
    m = np.arange(n, dtype=np.int64)
    quad = (4 * m) // n                          # the quadrant, 0 .. 3
    p = 8 * m - 2 * quad * n                     # the angle inside the quadrant, in units of pi / (4 n): 0 <= p < 2 n
    low = p <= n
    a = np.where(low, p, 2 * n - p).astype(np.float64) * (np.pi / (4.0 * n))      # in [0, pi / 4]
    ca, sa = np.cos(a), np.sin(a)
    half = p == n
    ca[half] = sa[half] = np.sqrt(0.5)
    cq, sq = np.where(low, ca, sa), np.where(low, sa, ca)
    c = np.choose(quad, [cq, -sq, -cq, sq]) + 0.0      # (+ 0.0: no negative zeros)
    s = np.choose(quad, [sq, cq, -sq, -cq]) + 0.0
    return c, s


def spectrum_window(n, window):
    """The window of one axis: ones, or the periodic Hann window 0.5 - 0.5 cos(2 pi j / n) from the same table.  An axis of
    extent 1 is never windowed (its periodic Hann window would be the single value 0)."""
    import numpy as np
    if window == 'none' or int(n) == 1:
        return np.ones(int(n), dtype=np.float64)
    return 0.5 - 0.5 * trig_tables(n)[0]


def spectrum_matrices(n, window='none', half=False):
    """(Ct, St) of one axis, transposed for the kernel: Mt[j][k] = trig[(k j) mod n] * win[j], k = 0 .. n - 1 (half: 0 .. n // 2)."""
    import numpy as np
    n = int(n)
    c, s = trig_tables(n)
    win = spectrum_window(n, window)
    k = np.arange(n // 2 + 1 if half else n, dtype=np.int64)
    idx = (np.arange(n, dtype=np.int64)[:, None] * k[None, :]) % n
    return np.ascontiguousarray(c[idx] * win[:, None]), np.ascontiguousarray(s[idx] * win[:, None])


class SpectrumPlan:
    """The host tables of power_spectrum for one volume shape (d, h, w) -- or (h, w), read as d = 1 --, voxel spacing in mm, number
    of radial bins (default max(d, h, w) // 2) and window ('none' or 'hann'; with 'hann' the mean is NOT removed: Hann's transform
    has three taps, so DC leaks into |k| <= 1 per axis, equally for both sets of a comparison).  Holds the six transposed matrices,
    the squared frequencies f2 per axis, the squared column edges, the weighted coefficient counts of every column and profile
    bin, and the device copies of the tables, made on first use per device."""

    def __init__(self, shape, spacing=(1.0, 1.0, 1.0), bins=None, window='none'):
        import numpy as np
        shape = tuple(int(v) for v in shape)
        if len(shape) == 2:
            shape = (1,) + shape
        if len(shape) != 3:
            raise ValueError(f'SpectrumPlan: expected a shape (d, h, w) or (h, w), got {shape}')
        if min(shape) < 1 or max(shape) > _lib.POWER_SPECTRUM_MAX_EXTENT:
            raise ValueError(f'SpectrumPlan: extents lie in 1 .. {_lib.POWER_SPECTRUM_MAX_EXTENT}, got {shape}')
        spacing = tuple(float(v) for v in spacing)
        if len(spacing) == 2:
            spacing = (1.0,) + spacing
        if len(spacing) != 3 or not all(math.isfinite(v) and v > 0 for v in spacing):
            raise ValueError(f'SpectrumPlan: the spacing is three positive numbers (mm), got {spacing}')
        if bins is None:
            bins = max(max(shape) // 2, 1)      # (a single voxel still has one column next to DC)
        bins = int(bins)
        if not 1 <= bins <= _lib.POWER_SPECTRUM_MAX_BINS:
            raise ValueError(f'SpectrumPlan: bins lie in 1 .. {_lib.POWER_SPECTRUM_MAX_BINS}, got {bins}')
        if window not in SPECTRUM_WINDOWS:
            raise ValueError(f'SpectrumPlan: the window is one of {SPECTRUM_WINDOWS}, got {window!r}')
        self.shape, self.spacing, self.bins, self.window = shape, spacing, bins, window
        d, h, w = shape
        self.wf = w // 2 + 1
        self.mats = [m for n_, half in ((d, False), (h, False), (w, True)) for m in spectrum_matrices(n_, window, half)]
        self.f2 = [(np.minimum(np.arange(n_), n_ - np.arange(n_)).astype(np.float64) / (n_ * sp)) ** 2
                   for n_, sp in zip(shape, spacing)]
        self.top = float((self.f2[0].max() + self.f2[1].max()) + self.f2[2].max())
        self.edges2 = (np.arange(bins + 1, dtype=np.float64) * np.sqrt(self.top) / bins) ** 2
        self.edges2[bins] = self.top
        self.g = np.full(self.wf, 2.0)
        self.g[0] = 1.0
        if w % 2 == 0:
            self.g[w // 2] = 1.0
        self.q = [np.minimum(np.arange(n_), n_ - np.arange(n_)) for n_ in (d, h)] + [np.arange(self.wf)]
        self.axis_len = (d // 2 + 1, h // 2 + 1, self.wf)
        self.counts = np.zeros(bins + 1, dtype=np.float64)
        for kd in range(d):      # plane by plane: the whole column map is only built where the twin asks for it
            np.add.at(self.counts, self.columns(kd).ravel(), np.broadcast_to(self.g, (h, self.wf)).ravel())
        self.axis_counts = (np.bincount(self.q[0], minlength=d // 2 + 1) * float(h * w),
                            np.bincount(self.q[1], minlength=h // 2 + 1) * float(d * w), self.g * float(d * h))
        self._columns = None
        self._device = {}

    def columns(self, kd=None):
        """The radial column of every coefficient, int64 [d, h, wf] (kd given: of that plane, [h, wf]):
        r2 = (f2_d[kd] + f2_h[kh]) + f2_w[kw]; column 0 where r2 == 0, else min(1 + #{b >= 1: edges2[b] <= r2}, bins)."""
        import numpy as np
        if kd is None:
            if self._columns is None:
                self._columns = np.stack([self.columns(k) for k in range(self.shape[0])])
            return self._columns
        r2 = (self.f2[0][kd] + self.f2[1][:, None]) + self.f2[2][None, :self.wf]
        col = np.minimum(1 + np.searchsorted(self.edges2[1:], r2, 'right'), self.bins)
        return np.where(r2 == 0, 0, col).astype(np.int64)

    def centres(self):
        """The frequency (cycles / mm) at the centre of every radial column; column 0 is DC."""
        import numpy as np
        e = np.sqrt(self.edges2)
        return np.concatenate([[0.0], 0.5 * (e[:-1] + e[1:])])[:self.bins + 1]

    def axis_frequencies(self):
        import numpy as np
        return tuple(np.arange(m) / (n_ * sp) for m, n_, sp in zip(self.axis_len, self.shape, self.spacing))

    def device_tables(self, device):
        import numpy as np
        key = str(device)
        if key not in self._device:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            self._device[key] = (up(np.concatenate([m.ravel() for m in self.mats])), up(np.concatenate(self.f2)), up(self.edges2))
        return self._device[key]


def _spectrum_numpy(x, plan, scale, shift):
    """The numpy twin: the same map, window, columns and weights; np.fft.rfftn in f64, np.add.at into the columns."""
    import numpy as np
    d, h, w = plan.shape
    n = x.shape[0]
    radial = np.zeros((n, plan.bins + 1), dtype=np.float64)
    axes = [np.zeros((n, m), dtype=np.float64) for m in plan.axis_len]
    col = plan.columns().ravel()
    win = [spectrum_window(n_, plan.window) for n_ in plan.shape]
    for i in range(n):
        t = x[i].astype(np.float64) * np.float64(scale) + np.float64(shift)
        if plan.window != 'none':
            t = t * win[0][:, None, None] * win[1][None, :, None] * win[2][None, None, :]
        f = np.fft.rfftn(t, axes=(0, 1, 2))
        p = (f.real ** 2 + f.imag ** 2) * plan.g[None, None, :]
        np.add.at(radial[i], col, p.ravel())
        np.add.at(axes[0][i], plan.q[0], p.sum(axis=(1, 2)))
        np.add.at(axes[1][i], plan.q[1], p.sum(axis=(0, 2)))
        axes[2][i] += p.sum(axis=(0, 1))
    return radial, axes


def power_spectrum(x, plan, scale=1.0, shift=0.0, workspace_mib=512):
    """(radial f64 [n, bins + 1], (axis_d [n, d // 2 + 1], axis_h [n, h // 2 + 1], axis_w [n, w // 2 + 1])): the shell-binned power
    spectrum of every volume of x after t = f64(x) * scale + shift (two roundings), as DESIGN.md 4.14 defines it: sums of g |F|^2
    over the half spectrum, per radial column of the plan and per |k| along each axis.  x: [n, d, h, w] or [n, 1, d, h, w] (one
    channel), or [n, h, w] for a plan with d = 1; u8 / i8 / i16 / u16 / f16 / bf16 / f32.  On the device: sg_power_spectrum, three
    passes of f64 MFMAs per chunk of samples, chunked so that the workspace stays under workspace_mib -- a sample's bits depend on
    neither the chunking nor the batch.  A CPU tensor takes the numpy twin (np.fft.rfftn)."""
    if not isinstance(plan, SpectrumPlan):
        raise TypeError(f'power_spectrum: expected a SpectrumPlan, got {type(plan).__name__}')
    if torch.is_tensor(x) and x.dim() == 3:
        x = x.unsqueeze(1)
    x, (n, d, h, w, c) = view_volumes(x)
    if c != 1:
        raise ValueError(f'power_spectrum: one channel, got {c}')
    if (d, h, w) != plan.shape:
        raise ValueError(f'power_spectrum: the plan is for volumes of {plan.shape}, got {(d, h, w)}')
    scale, shift = float(scale), float(shift)
    if not (math.isfinite(scale) and math.isfinite(shift)):
        raise ValueError(f'power_spectrum: scale {scale} and shift {shift} must be finite')
    if not workspace_mib > 0:
        raise ValueError(f'power_spectrum: workspace_mib {workspace_mib} must be positive')
    nrad, alen = plan.bins + 1, sum(plan.axis_len)
    cut = (plan.axis_len[0], plan.axis_len[0] + plan.axis_len[1])
    if not x.is_cuda:
        xn = x.reshape(n, d, h, w)
        xn = xn.float().numpy() if xn.dtype == torch.bfloat16 else xn.numpy()
        radial, axes = _spectrum_numpy(xn, plan, scale, shift)
        return torch.from_numpy(radial), tuple(torch.from_numpy(a) for a in axes)
    radial = torch.empty((n, nrad), device=x.device, dtype=torch.float64)
    axes = torch.empty((n, alen), device=x.device, dtype=torch.float64)
    if n:
        lib = _lib.load()
        mats, f2, edges2 = plan.device_tables(x.device)
        per = int(lib.sg_power_spectrum_workspace(1, d, h, w))
        chunk = max(1, min(n, int(workspace_mib * 2 ** 20) // per))
        nbytes = int(lib.sg_power_spectrum_workspace(chunk, d, h, w))
        ws = torch.empty(nbytes, device=x.device, dtype=torch.uint8)
        flat = x.reshape(n, d * h * w)
        with torch.cuda.device(x.device):
            for i in range(0, n, chunk):
                m = min(chunk, n - i)
                check(lib.sg_power_spectrum(_ptr(flat[i:i + m]), HIST_DT[x.dtype], m, d, h, w, scale, shift, _ptr(mats), _ptr(f2),
                                            _ptr(edges2), plan.bins, _ptr(radial[i:i + m]), _ptr(axes[i:i + m]), _ptr(ws), nbytes,
                                            _stream()), 'sg_power_spectrum')
    return radial, (axes[:, :cut[0]], axes[:, cut[0]:cut[1]], axes[:, cut[1]:])
