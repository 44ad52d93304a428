"""numpy restatement of sg_render_view (include/saragan_hip.h), of the tile placement and of preview.py's sheet
layout.  Every f32 operation is one numpy operation with np.float32 operands, in the order of the definition:
  v = x[index] | np.fmax.reduce from -inf | np.float32(f64 sum / extent)
  t = v * scale + shift;  u = (t - lo) * inv,  inv = np.float32(255.0 / (f64(hi) - f64(lo)))
  g = u8(floor(fmin(fmax(u, 0), 255) + 0.5)), NaN -> 0
Nothing here imports the package."""
import numpy as np

AXES = {'d': 0, 'h': 1, 'w': 2}


def to_f32(x):
    """The exact f32 value of every source element (bf16 arrives as a torch tensor: widened there)."""
    if hasattr(x, 'detach'):
        x = x.detach().cpu()
        x = (x.float() if x.dtype.is_floating_point else x).numpy()
    return np.asarray(x).astype(np.float32)


def collapse(x, axis, mode, index=None):
    """f32 [n, rows, cols] from x [n, d, h, w] (already f32)."""
    ax = axis + 1
    extent = x.shape[ax]
    if mode == 'slice':
        return np.take(x, extent // 2 if index is None else index, axis=ax)
    if mode == 'max':
        return np.fmax.reduce(x, axis=ax, initial=np.float32(-np.inf))
    assert mode == 'mean'
    with np.errstate(invalid='ignore'):
        s = np.sum(x.astype(np.float64), axis=ax, dtype=np.float64)
    return (s / np.float64(extent)).astype(np.float32)


def grey(v, window, scale=1.0, shift=0.0):
    lo, hi = np.float32(window[0]), np.float32(window[1])
    inv = np.float32(255.0 / (float(hi) - float(lo)))
    with np.errstate(invalid='ignore', over='ignore'):
        t = v.astype(np.float32) * np.float32(scale) + np.float32(shift)
        u = (t - lo) * inv
        nan = np.isnan(u)
        u = np.fmin(np.fmax(u, np.float32(0)), np.float32(255))
        g = np.floor(u + np.float32(0.5))
    assert t.dtype == u.dtype == g.dtype == np.float32
    g[nan] = 0
    return g.astype(np.uint8)


def tiles(x, axis, mode, index=None, window=(-1.0, 2.0), scale=1.0, shift=0.0, zoom=(1, 1), channel=0):
    """u8 [n, rows * zoom_r, cols * zoom_c].  x: [n, d, h, w] or [n, d, h, w, c]."""
    x = to_f32(x)
    if x.ndim == 5:
        x = x[..., channel]
    g = grey(collapse(x, axis, mode, index), window, scale, shift)
    return np.repeat(np.repeat(g, zoom[0], axis=1), zoom[1], axis=2)


def place(canvas, t, origin=(0, 0), grid_cols=None, pitch=None):
    """Writes tile i of t at origin + (i // grid_cols * pitch_r, i % grid_cols * pitch_c) into canvas (in place)."""
    n, th, tw = t.shape
    grid_cols = max(n, 1) if grid_cols is None else grid_cols
    pitch = (th, tw) if pitch is None else pitch
    for i in range(n):
        r, c = origin[0] + (i // grid_cols) * pitch[0], origin[1] + (i % grid_cols) * pitch[1]
        assert r >= 0 and c >= 0 and r + th <= canvas.shape[0] and c + tw <= canvas.shape[1]
        canvas[r:r + th, c:c + tw] = t[i]
    return canvas


def parse_view(name):
    head, _, idx = name.partition(':')
    mode, ax = head.split('_')
    return mode, AXES[ax], (int(idx) if idx else None)


def sheet(x, views, window, scale=1.0, shift=0.0, zoom_d=1):
    """One column per sample, one row band per view; a band as high as its tile, a column as wide as the widest tile, narrower
    tiles left-aligned, background 0.  x: [n, d, h, w] (or [n, 1, d, h, w])."""
    x = to_f32(x)
    if x.ndim == 5:
        x = x[:, 0]
    bands = []
    for name in views:
        mode, axis, index = parse_view(name)
        bands.append(tiles(x, axis, mode, index, window, scale, shift, (1, 1) if axis == 0 else (zoom_d, 1)))
    col_w = max(b.shape[2] for b in bands)
    out = np.zeros((sum(b.shape[1] for b in bands), x.shape[0] * col_w), np.uint8)
    top = 0
    for b in bands:
        place(out, b, origin=(top, 0), pitch=(b.shape[1], col_w))
        top += b.shape[1]
    return out


def slice_grid(x0, window, scale=1.0, shift=0.0):
    """Every D plane of one sample [d, h, w], row-major, 2 ** floor(log2(sqrt(d))) columns."""
    x0 = to_f32(x0)
    d, h, w = x0.shape
    cols = int(2 ** np.floor(np.log2(np.sqrt(d))))
    rows = -(-d // cols)
    t = tiles(x0[:, None], 0, 'slice', 0, window, scale, shift)
    return place(np.zeros((rows * h, min(d, cols) * w), np.uint8), t, grid_cols=cols)


def decode_png(data):
    """(u8 [H, W] array, {keyword: text}) of an 8-bit greyscale, filter-0 PNG; asserts the signature, every chunk CRC and IHDR."""
    import struct
    import zlib
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, kind = struct.unpack('>I4s', data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF
        chunks.append((kind, body))
        pos += 12 + n
    assert chunks[0][0] == b'IHDR' and chunks[-1] == (b'IEND', b'') and pos == len(data)
    w, h, depth, colour, comp, filt, lace = struct.unpack('>IIBBBBB', chunks[0][1])
    assert (depth, colour, comp, filt, lace) == (8, 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(b''.join(b for k, b in chunks if k == b'IDAT')), np.uint8).reshape(h, w + 1)
    assert not raw[:, 0].any()                                      # filter 0 on every row
    text = dict(b.decode('latin-1').split('\0', 1) for k, b in chunks if k == b'tEXt')
    return raw[:, 1:].copy(), text
