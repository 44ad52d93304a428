"""Sample previews (not in the reference's training loop): contact sheets of slices and projections, rendered on
the device by sg_render_view (functional.render_view) and written as plain 8-bit greyscale PNG files by a stdlib encoder.

A VIEW is named `slice_d|h|w[:INDEX]`, `max_d|h|w` or `mean_d|h|w`: the letter is the collapsed axis (a slice without an index
is the middle plane).  A SHEET has one column per sample and one row band per view: a band is as high as its view's tile, a
column as wide as the widest tile, narrower tiles stand left-aligned, the background is 0.  One launch per view draws into one
canvas on the device; one copy brings the canvas to the host.  Voxels are anisotropic in this data (D is size / 4): zoom_d
repeats the D rows of the coronal and sagittal views.

    python -m saragan_amd.preview FILE_OR_DIR --window LO,HI [--views V,...] [--max_samples N] [--scale S --shift T]
                                  [--zoom_d Z] [--out PNG]
renders .npy volumes ([d, h, w], or [n, 1, d, h, w] / [n, d, h, w] batches) in their own dtype."""
import argparse
import glob
import math
import os
import struct
import zlib

import numpy as np

DEFAULT_VIEWS = 'slice_d,slice_h,max_h'
_MODES = ('slice', 'max', 'mean')
_AXES = {'d': 0, 'h': 1, 'w': 2}


# ---- PNG: 8-bit greyscale (colour type 0), filter 0 on every row
def _chunk(kind, body):
    return struct.pack('>I', len(body)) + kind + body + struct.pack('>I', zlib.crc32(kind + body) & 0xFFFFFFFF)


def png_bytes(a, text=None):
    """The PNG file of a numpy uint8 [H, W] array.  text: {keyword: value} for tEXt chunks (Latin-1; keywords of 1-79
    characters), e.g. phase, step, views, window, seed and which weights were rendered."""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError(f'png_bytes: expected a uint8 [H, W] array with H, W >= 1, got {a.dtype} {a.shape}')
    h, w = a.shape
    rows = np.zeros((h, w + 1), dtype=np.uint8)      # a filter byte (0: none) in front of every row
    rows[:, 1:] = a
    out = [b'\x89PNG\r\n\x1a\n', _chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 0, 0, 0, 0))]
    for key, value in (text or {}).items():
        k = str(key).encode('latin-1')
        if not 1 <= len(k) <= 79 or b'\0' in k:
            raise ValueError(f'png_bytes: tEXt keyword {key!r} must have 1 to 79 Latin-1 characters')
        out.append(_chunk(b'tEXt', k + b'\0' + str(value).encode('latin-1')))
    out.append(_chunk(b'IDAT', zlib.compress(rows.tobytes(), 6)))
    out.append(_chunk(b'IEND', b''))
    return b''.join(out)


def write_png(path, a, text=None):
    data = png_bytes(a, text)
    with open(path, 'wb') as f:
        f.write(data)
    return path


# ---- views, windows
def parse_view(name):
    """'slice_d:3' -> ('slice', 0, 3); 'max_h' -> ('max', 1, None).  ValueError for anything else."""
    head, sep, idx = str(name).strip().partition(':')
    mode, _, ax = head.partition('_')
    if mode not in _MODES or ax not in _AXES or (sep and mode != 'slice'):
        raise ValueError(f'unknown view {name!r}: views are slice_d|h|w[:INDEX], max_d|h|w, mean_d|h|w')
    index = None
    if sep:
        if not idx.isdigit():
            raise ValueError(f'view {name!r}: the slice index is a non-negative integer')
        index = int(idx)
    return mode, _AXES[ax], index


def parse_views(text):
    """'slice_d,max_h' (or a sequence of names) -> [(mode, axis, index), ...], at least one."""
    names = [v for v in text.split(',') if v.strip()] if isinstance(text, str) else list(text)
    if not names:
        raise ValueError('no view given: views are slice_d|h|w[:INDEX], max_d|h|w, mean_d|h|w')
    return [v if isinstance(v, tuple) else parse_view(v) for v in names]


def parse_window(text):
    """'LO,HI' -> (lo, hi) floats, lo < hi, both finite."""
    try:
        lo, hi = (float(v) for v in str(text).split(','))
    except ValueError:
        raise ValueError(f'expected a window LO,HI, got {text!r}') from None
    if not (math.isfinite(lo) and math.isfinite(hi)) or hi <= lo:
        raise ValueError(f'the window {lo},{hi} is empty or not finite')
    return lo, hi


def default_window(mean=None, stddev=None):
    """The reference's clip range [-1, 2] of normalised values (generate.py:149), in data units."""
    if mean is None or stddev is None:
        return -1.0, 2.0
    return float(mean) - float(stddev), float(mean) + 2.0 * float(stddev)


def view_zoom(axis, zoom_d):
    """The (row, column) zoom of a view on a sheet: D rows (coronal, sagittal) are repeated zoom_d times."""
    return (1, 1) if axis == 0 else (int(zoom_d), 1)


def sheet_layout(dims, views, zoom_d=1):
    """(band tops, band heights, column width) of a sheet of volumes of dims = (d, h, w)."""
    from .table_ops import view_tile
    tiles = [view_tile(dims, axis, view_zoom(axis, zoom_d)) for _, axis, _ in views]
    heights = [t[0] for t in tiles]
    tops = [sum(heights[:i]) for i in range(len(tiles))]
    return tops, heights, max(t[1] for t in tiles)


def sheet(x, views=DEFAULT_VIEWS, window=(-1.0, 2.0), scale=1.0, shift=0.0, zoom_d=1):
    """numpy uint8 [sum of the band heights, samples * column width]: the contact sheet of x -- a batch render_view takes, or a
    list of such batches (chunks of one set of samples, drawn side by side)."""
    import torch
    from . import table_ops as T
    views = parse_views(views)
    if int(zoom_d) < 1:
        raise ValueError(f'sheet: zoom_d {zoom_d} < 1')
    chunks = [T.view_volumes(c) for c in (x if isinstance(x, (list, tuple)) else [x])]
    if not chunks:
        raise ValueError('sheet: no samples')
    dims = chunks[0][1][1:4]
    if any(s[1:4] != dims for _, s in chunks):
        raise ValueError(f'sheet: the chunks differ in shape: {[s[1:4] for _, s in chunks]}')
    total = sum(s[0] for _, s in chunks)
    if total < 1 or min(dims) < 1:
        raise ValueError(f'sheet: nothing to draw ({total} samples of {tuple(dims)})')
    tops, heights, col_w = sheet_layout(dims, views, zoom_d)
    canvas = torch.zeros((sum(heights), total * col_w), device=chunks[0][0].device, dtype=torch.uint8)
    col = 0
    for c, s in chunks:
        for (mode, axis, index), top, height in zip(views, tops, heights):
            T.render_view(c, axis, mode, index=index, window=window, scale=scale, shift=shift, zoom=view_zoom(axis, zoom_d),
                          canvas=canvas, origin=(top, col * col_w), grid_cols=max(s[0], 1), pitch=(height, col_w))
        col += s[0]
    return canvas.cpu().numpy()


def grid_cols_of(d):
    """The reference's image_grid columns for D planes (generate.py:98): 2 ** floor(log2(sqrt(D)))."""
    return int(2 ** np.floor(np.log(np.sqrt(d)) / np.log(2)))


def slice_grid(x0, window=(-1.0, 2.0), scale=1.0, shift=0.0):
    """numpy uint8: every D plane of ONE sample ([d, h, w], or a one-sample batch), row-major in a grid of grid_cols_of(d) columns
    -- the reference's image_grid (generate.py:96-106), one launch: the planes are a batch [d, 1, h, w] of axial slices."""
    from . import table_ops as T
    if x0.dim() == 3:
        x0 = x0[None]
    x0, (n, d, h, w, c) = T.view_volumes(x0)
    if n != 1 or c != 1 or min(d, h, w) < 1:
        raise ValueError(f'slice_grid: expected one single-channel sample, got {n} of {(d, h, w)} with {c} channels')
    cols = grid_cols_of(d)
    return T.render_view(x0.reshape(d, 1, h, w), 0, 'slice', index=0, window=window, scale=scale, shift=shift,
                         grid_cols=cols).cpu().numpy()


# ---- latents of an interpolation sheet
def slerp(z0, z1, k):
    """[k, L]: k latents on the great arc from z0 to z1 (both [L]), ends included; the norm goes linearly from |z0| to |z1|."""
    import torch
    t = torch.linspace(0.0, 1.0, k, device=z0.device, dtype=torch.float64)[:, None]
    a, b = z0.double(), z1.double()
    na, nb = a.norm(), b.norm()
    ua, ub = a / na, b / nb
    omega = torch.acos(torch.clamp((ua * ub).sum(), -1.0, 1.0))
    if float(omega) < 1e-6:
        u = ua[None] * (1 - t) + ub[None] * t
    else:
        u = (torch.sin((1 - t) * omega) * ua[None] + torch.sin(t * omega) * ub[None]) / torch.sin(omega)
    return (u * (na * (1 - t) + nb * t)).to(z0.dtype)


# ---- the previews of a training run
LATENT_SEED_SALT = 0x70726576      # 'prev': the fixed latents' generator is seeded from --seed and this, apart from every training stream


class LoopPreviews:
    """train.py's previews (rank 0, --preview_every_nsteps > 0): fixed latents drawn ONCE per run from a generator of their own,
    sheets of them under the EMA weights at every preview point and at the end of a phase, the slice grid of fixed sample 0, and
    one sheet of the phase's first training volumes.  Nothing here draws from, or advances, a stream the training reads."""

    def __init__(self, args, logdir, device, label_table=None, tap=None):
        import torch
        self.args, self.device, self.tap = args, device, tap
        self.dir = os.path.join(logdir, 'previews')
        os.makedirs(self.dir, exist_ok=True)
        self.views, self.window, self.zoom_d = args.preview_views, args.preview_window, args.preview_zoom_d
        # samples are in normalised units: data units = v * stddev + mean
        self.scale, self.shift = (1.0, 0.0) if args.data_mean is None else (float(args.data_stddev), float(args.data_mean))
        gen = torch.Generator(device=device).manual_seed((int(args.seed) * 1000003 + LATENT_SEED_SALT) % 2 ** 63)
        k = args.preview_samples
        self.z = torch.randn(k, args.latent_dim, device=device, generator=gen)
        self.labels = self.zi = self.labels_i = None
        if label_table is not None:      # fixed sample i wears label row i mod F
            self.labels = torch.from_numpy(label_table[np.arange(k) % len(label_table)]).to(device)
        if args.preview_interp:
            self.zi = slerp(self.z[0], self.z[1], args.preview_interp)
            if self.labels is not None:      # (the arc keeps the first latent's labels)
                self.labels_i = self.labels[:1].expand(args.preview_interp, -1).contiguous()

    def _text(self, phase, step, weights, **more):
        a = self.args
        text = dict(phase=phase, step=step, views=','.join(_view_name(v) for v in self.views),
                    window=f'{self.window[0]},{self.window[1]}', seed=a.seed, weights=weights)
        text.update(more)
        return text

    def _generate(self, graph, z, labels, batch_size):
        """The samples of z, generated in chunks of the phase's batch size."""
        return [graph.generate(z[i:i + batch_size], None if labels is None else labels[i:i + batch_size])
                for i in range(0, z.shape[0], batch_size)]

    def fakes(self, sess, graph, ema, phase, step, batch_size, tag, grid=False):
        """fakes_{phase}_{tag}.png (and interp_{phase}_{tag}.png; with grid, grid_fake_{phase}.png) under the EMA weights."""
        sess.run(ema.assign_ema_weights())
        try:
            jobs = [('fakes', self.z, self.labels)] + ([('interp', self.zi, self.labels_i)] if self.zi is not None else [])
            for kind, z, labels in jobs:
                chunks = self._generate(graph, z, labels, batch_size)
                name = f'{kind}_{phase}_{tag}.png'
                img = sheet(chunks, self.views, self.window, self.scale, self.shift, self.zoom_d)
                write_png(os.path.join(self.dir, name), img, self._text(phase, step, 'EMA', latents=kind))
                if self.tap is not None:
                    self.tap.append((phase, name, z.cpu(), [c.float().cpu() for c in chunks]))
                if grid and kind == 'fakes':
                    name = f'grid_fake_{phase}.png'
                    write_png(os.path.join(self.dir, name), slice_grid(chunks[0][:1], self.window, self.scale, self.shift),
                              self._text(phase, step, 'EMA', latents='fixed sample 0'))
                    if self.tap is not None:
                        self.tap.append((phase, name, z[:1].cpu(), [chunks[0][:1].float().cpu()]))
        finally:
            sess.run(ema.restore_original_weights())

    def reals(self, files, phase):
        """reals_{phase}.png: the first training volumes as the files hold them (their own dtype, data units: scale 1, shift 0)."""
        import torch
        files = list(files)[:self.args.preview_samples]
        if not files:
            return
        vols = np.ascontiguousarray(np.stack([np.load(f) for f in files]))
        img = sheet(torch.from_numpy(vols).to(self.device), self.views, self.window, 1.0, 0.0, self.zoom_d)
        write_png(os.path.join(self.dir, f'reals_{phase}.png'), img, self._text(phase, 0, 'none', files=len(files)))


def _view_name(v):
    mode, axis, index = v
    return f'{mode}_{"dhw"[axis]}' + ('' if index is None else f':{index}')


# ---- command line
def load_volumes(path, max_samples=None):
    """A contiguous [n, d, h, w] array in the files' own dtype: a .npy file ([d, h, w], [n, d, h, w] or [n, 1, d, h, w]) or the
    sorted *.npy volumes of a directory."""
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, '*.npy')))
        if not files:
            raise ValueError(f'{path}: no .npy files')
        vols = np.stack([np.load(f) for f in files[:max_samples]])
    else:
        vols = np.load(path)
        if vols.ndim == 3:
            vols = vols[None]
    if vols.ndim == 5 and vols.shape[1] == 1:
        vols = vols[:, 0]
    if vols.ndim != 4:
        raise ValueError(f'{path}: expected [d, h, w] volumes or a [n, 1, d, h, w] / [n, d, h, w] batch, got {vols.shape}')
    return np.ascontiguousarray(vols[:max_samples])


def build_parser():
    p = argparse.ArgumentParser(prog='python -m saragan_amd.preview', description=__doc__.split('\n\n')[0])
    p.add_argument('path', help='a .npy file or a directory of .npy volumes')
    p.add_argument('--window', required=True, help='LO,HI in data units: LO is drawn black, HI white (negative LO: --window=LO,HI)')
    p.add_argument('--views', default=DEFAULT_VIEWS)
    p.add_argument('--max_samples', type=int, default=8)
    p.add_argument('--scale', type=float, default=1.0, help='data units = value * scale + shift')
    p.add_argument('--shift', type=float, default=0.0)
    p.add_argument('--zoom_d', type=int, default=1)
    p.add_argument('--out', default=None, help='default: preview.png next to the input')
    return p


def main(argv=None, device='cuda'):
    import torch
    args = build_parser().parse_args(argv)
    try:
        window, views = parse_window(args.window), parse_views(args.views)
        if args.max_samples < 1 or args.zoom_d < 1:
            raise ValueError('--max_samples and --zoom_d are at least 1')
        vols = load_volumes(args.path, args.max_samples)
    except ValueError as e:
        raise SystemExit(f'preview: {e}') from None
    if not torch.cuda.is_available():
        raise RuntimeError('saragan_amd renders on MI355X only: no CPU fallback')
    img = sheet(torch.from_numpy(vols).to(device), views, window, args.scale, args.shift, args.zoom_d)
    base = args.path if os.path.isdir(args.path) else os.path.dirname(os.path.abspath(args.path))
    out = args.out or os.path.join(base, 'preview.png')
    write_png(out, img, dict(views=args.views, window=args.window, scale=args.scale, shift=args.shift, source=args.path))
    print(f'Wrote {out}: {vols.shape[0]} samples of shape {vols.shape[1:]}, {img.shape[1]} x {img.shape[0]} pixels')
    return out


if __name__ == '__main__':
    main()
