"""Spectral normalisation of the discriminator's weights: the device table of a flat buffer's normalised layers, the batched
power-iteration refresh and the gradient's pull-back to the raw weights.  Re-exported by functional."""
import torch

from . import _lib
from ._launch import _ptr, _req_cuda, _stream
from ._lib import check
from ._weight_images import IMAGES

SPECTRAL_MIN_ROWS = 16      # fewest rows of a row block (where the layer has that many): bounds the column workspace at 1/16 of W
SPECTRAL_MAX_BLOCKS = 128   # most row blocks of one layer (while a block stays within `chunk` rows): the layer's ONE normalising
#                             block adds that many partials per column, and the longest such chain bounds the launch


def spectral_rows_per_block(rows, cols, chunk=_lib.SG_SEG_CHUNK):
    """Rows of one row block of an [rows, cols] weight: about `chunk` elements, whole rows only, at least SPECTRAL_MIN_ROWS and
    at least rows / SPECTRAL_MAX_BLOCKS (a large layer's blocks loop), never more than `chunk` rows (the kernel's copy of t)
    or than the layer has."""
    rows, cols = int(rows), int(cols)
    want = max(chunk // cols, SPECTRAL_MIN_ROWS, -(-rows // SPECTRAL_MAX_BLOCKS))
    return max(1, min(rows, chunk, want))


def spectral_table_arrays(segments, total, chunk=_lib.SG_SEG_CHUNK):
    """Host half of SpectralTable: segments [(start, R, C)] of a flat buffer of `total` elements -> (segs [[start, R, C, first
    block, rows per block, u offset, v offset, column offset]], blocks [[segment, row block]], ulen, vlen, collen) as
    include/saragan_hip.h lays them out.  u, v and the column partials of the segments follow each other, each start rounded
    up to a multiple of 4."""
    segs, blocks, end, uoff, voff, coloff = [], [], 0, 0, 0, 0
    pad = lambda n: (n + 3) // 4 * 4
    for s, (start, rows, cols) in enumerate(sorted((int(a), int(b), int(c)) for a, b, c in segments)):
        if start % 4 or rows < 1 or cols < 1 or start < end or start + rows * cols > total:
            raise ValueError(f'segment [{start}, {start + rows * cols}) of a flat buffer of {total}: starts must be multiples '
                             f'of 4 and segments disjoint and inside the buffer')
        end = start + rows * cols
        rpb = spectral_rows_per_block(rows, cols, chunk)
        nb = (rows + rpb - 1) // rpb
        segs.append([start, rows, cols, len(blocks), rpb, uoff, voff, coloff])
        blocks.extend([s, b] for b in range(nb))
        uoff, voff, coloff = uoff + pad(cols), voff + pad(rows), coloff + pad(nb * cols)
    if not segs:
        raise ValueError('a spectral table needs at least one segment')
    return segs, blocks, uoff, voff, coloff


class SpectralTable:
    """Device table of one network's spectrally normalised weights (sg_spectral_*) with their state and workspaces: u (the
    persistent power-iteration vectors, all layers in one buffer), v, sigma, and the partial sums.  Built once per flat
    buffer (it copies to the device); a step only launches with it."""

    def __init__(self, segments, total, device):
        segs, blocks, ulen, vlen, collen = spectral_table_arrays(segments, total)
        self.total, self.nseg, self.nblocks = int(total), len(segs), len(blocks)
        self.ulen, self.vlen, self.collen = ulen, vlen, collen
        self.layout = segs
        self.segs = torch.tensor(segs, dtype=torch.int64).to(device)
        self.blocks = torch.tensor(blocks, dtype=torch.int32).to(device)
        z = lambda n: torch.zeros(n, dtype=torch.float32, device=device)
        self.u, self.v, self.cols = z(ulen), z(vlen), z(collen)
        self.sigma, self.nt, self.partials = z(self.nseg), z(self.nseg), z(self.nblocks)

    def check(self, *bufs):
        _req_cuda(*bufs)
        for b in bufs:
            if b.dtype != torch.float32 or not b.is_contiguous() or b.numel() != self.total:
                raise ValueError(f'the spectral table describes contiguous float32 buffers of {self.total} elements')

    def views(self, s):
        """(u [1, C], v [1, R], sigma [1]) of segment s: views of the table's buffers."""
        _, rows, cols, _, _, uo, vo, _ = self.layout[s]
        return self.u[uo:uo + cols].view(1, cols), self.v[vo:vo + rows].view(1, rows), self.sigma[s:s + 1]


def spectral_refresh_(table, p, eff, iteration=1):
    """One power-iteration refresh of every normalised weight of the flat f32 parameter buffer p: updates table.u, writes
    table.v, table.sigma and W / sigma into the flat effective-weight buffer eff (same offsets) -- 2 * iteration + 1 launches
    whatever the number of layers (sg_spectral_refresh)."""
    lib = _lib.load()
    table.check(p, eff)
    if int(iteration) < 1:
        raise ValueError('spectral_refresh_: iteration >= 1')
    if p.data_ptr() == eff.data_ptr():
        raise ValueError('spectral_refresh_: the effective weights need a buffer of their own')
    IMAGES.params_rewritten()      # the kernel rewrites the effective weights behind torch's version counters
    check(lib.sg_spectral_refresh(_ptr(p), _ptr(eff), table.total, _ptr(table.segs), _ptr(table.blocks), table.nseg,
                                  table.nblocks, _ptr(table.u), table.ulen, _ptr(table.v), table.vlen, _ptr(table.sigma),
                                  _ptr(table.nt), _ptr(table.partials), _ptr(table.cols), table.collen, int(iteration),
                                  _stream()), 'sg_spectral_refresh')


def spectral_pullback_(table, g, eff):
    """In place on the flat gradient buffer: the gradient with respect to the effective weights becomes the one with respect to
    the raw weights, g = (g - <g, W / sigma> v^T u) / sigma per normalised layer with u, v constant -- two launches
    (sg_spectral_pullback).  Elements outside the table's segments keep their bits."""
    lib = _lib.load()
    table.check(g, eff)
    check(lib.sg_spectral_pullback(_ptr(g), _ptr(eff), table.total, _ptr(table.segs), _ptr(table.blocks), table.nseg,
                                   table.nblocks, _ptr(table.u), table.ulen, _ptr(table.v), table.vlen, _ptr(table.sigma),
                                   _ptr(table.partials), _stream()), 'sg_spectral_pullback')
