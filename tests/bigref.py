"""Helpers of tests/test_large_offsets_gpu.py and tests/test_bigref_host.py: where a tensor of several GiB has to be looked at,
and the fp64 reference of a convolution on a box of its output.

A kernel that forms an address in too few bits is wrong only past a boundary: byte offset 2^31 (a signed 32-bit byte offset, the
range of one buffer resource), byte offset 2^32 (an unsigned one) and element offset 2^31 (a signed 32-bit index: byte 2^32 of a
bf16 tensor, byte 2^33 of an f32 one).  A convolution is local, so its exact reference can be evaluated on boxes of the output
from the box of the input it depends on; what matters is WHERE the boxes lie.  required_points() lists, for one tensor, the voxels
a box must contain: the first and the last, the voxel on either side of every boundary the tensor reaches, and for kernels that
rebase a buffer resource per group of samples the first and last voxel of the group the boundary falls into.  choose_boxes() builds
boxes around those voxels, check_cover() verifies a list of boxes against them and rejects a case that reaches no boundary at all
(a case just below a launcher's guard counts when a tensor of it ends within 16 MiB of byte 2^31): the condition is checked, not
sampled.

Tensors are NDHWC in memory.  Boxes are (n, d0, d1, h0, h1) on the BASE grid of a case (the convolution's output grid before any
pooling), all of W; a pooled tensor's voxel t covers the base voxels [t f, (t + 1) f) per dimension.  Nothing here touches the GPU;
box_reference computes on the host from whatever device its arguments live on."""
import torch

from tests import fwdref as R

B31, B32, B33 = 2 ** 31, 2 ** 32, 2 ** 33
NEAR = 2 ** 24      # a case below a launcher's guard counts if a tensor ends this close to byte 2^31 (its last voxel is then required)
SEAM = (4, 16)     # a multiple of 4 planes / 16 rows is a tile seam of every kernel here: kernel_tile() gives TD in 1 2 4 and TH in
                   # 1 2 4 8 16, and tests/test_bigref_host.py checks every case's route against it


class Layout:
    """One tensor of a call: n samples of sp = (D, H, W) voxels with c elements of esize bytes each, NDHWC.  pool: the block of
    base voxels one of its voxels covers; fine: how many of its voxels lie in one base voxel per dimension (the output of an
    up-convolution on the low-resolution base grid).  group: samples per rebased buffer resource (None: one 64-bit address for the
    tensor)."""

    def __init__(self, name, n, sp, c, esize, pool=(1, 1, 1), group=None, fine=(1, 1, 1)):
        self.name, self.n, self.sp, self.c, self.esize, self.pool, self.group = name, n, tuple(sp), c, esize, tuple(pool), group
        self.fine = tuple(fine)

    def base_range(self, t, dim):
        """[lo, hi): the base coordinates that voxel coordinate t of this tensor touches along dimension dim."""
        return t * self.pool[dim] // self.fine[dim], -(-(t + 1) * self.pool[dim] // self.fine[dim])

    def voxel_bytes(self):
        return self.c * self.esize

    def sample_voxels(self):
        return self.sp[0] * self.sp[1] * self.sp[2]

    def nbytes(self):
        return self.n * self.sample_voxels() * self.voxel_bytes()

    def voxel_at_byte(self, b):
        """(n, d, h, w) of the voxel that holds byte offset b."""
        assert 0 <= b < self.nbytes(), (self.name, b)
        v = b // self.voxel_bytes()
        v, w = divmod(v, self.sp[2])
        v, h = divmod(v, self.sp[1])
        n, d = divmod(v, self.sp[0])
        return n, d, h, w

    def boundaries(self):
        """The byte offsets 2^31, 2^32 and (element offset 2^31) 2^31 * esize that the tensor reaches: it ends at or past them."""
        return [b for b in sorted({B31, B32, B31 * self.esize}) if b <= self.nbytes()]


def required_points(t):
    """[(label, (n, d, h, w))] in t's own grid: see the module docstring."""
    last = tuple(v - 1 for v in (t.n, *t.sp))
    pts = [('first', (0, 0, 0, 0)), ('last', last)]
    for b in t.boundaries():
        pts.append((f'below byte 2^{b.bit_length() - 1}', t.voxel_at_byte(b - 1)))
        if b == t.nbytes():
            continue
        at = t.voxel_at_byte(b)
        pts.append((f'at byte 2^{b.bit_length() - 1}', at))
        if t.group:
            g0 = at[0] // t.group * t.group
            g1 = min(g0 + t.group, t.n) - 1
            pts.append((f'first of the group at byte 2^{b.bit_length() - 1}', (g0, 0, 0, 0)))
            pts.append((f'last of the group at byte 2^{b.bit_length() - 1}', (g1, *last[1:])))
    return pts


def _span(x0, x1, extent, seam, align):
    """[lo, hi) around the base coordinates [x0, x1) that also holds the voxels on both sides of the nearest tile seam (where the
    extent has one), widened to whole blocks of `align`."""
    lo, hi = x0, x1
    if extent <= seam:
        lo, hi = 0, extent
    else:
        s = (x0 + seam // 2) // seam * seam
        s = min(max(s, seam), (extent - 1) // seam * seam)
        lo, hi = min(lo, s - 1), max(hi, s + 1)
    lo, hi = lo // align * align, -(-hi // align) * align
    return max(lo, 0), min(hi, extent)


def choose_boxes(layouts, base_sp, seam=SEAM, align=(1, 1)):
    """Boxes (n, d0, d1, h0, h1) on the base grid, one around every required point of every tensor, duplicates merged."""
    boxes = []
    for t in layouts:
        for _, (n, d, h, _w) in required_points(t):
            d0, d1 = _span(*t.base_range(d, 0), base_sp[0], seam[0], align[0])
            h0, h1 = _span(*t.base_range(h, 1), base_sp[1], seam[1], align[1])
            if (n, d0, d1, h0, h1) not in boxes:
                boxes.append((n, d0, d1, h0, h1))
    return sorted(boxes)


def box_holds(box, t, p):
    """Whether the box (base grid) holds all of voxel p of tensor t."""
    n, d0, d1, h0, h1 = box
    (pd0, pd1), (ph0, ph1) = t.base_range(p[1], 0), t.base_range(p[2], 1)
    return p[0] == n and d0 <= pd0 and pd1 <= d1 and h0 <= ph0 and ph1 <= h1


def has_seam(lo, hi, extent, seam):
    """[lo, hi) holds the voxels on both sides of a multiple of `seam`, or the extent has no such seam and is held whole."""
    if extent <= seam:
        return lo == 0 and hi == extent
    return any(lo < s < hi for s in range(seam, extent, seam))


def check_cover(layouts, boxes, base_sp, seam=SEAM):
    """Raises AssertionError unless some tensor reaches a boundary, every required point of every tensor lies in a box and every
    box spans a tile seam in D and in H.  Called on the host before anything is launched."""
    assert any(t.boundaries() or t.nbytes() >= B31 - NEAR for t in layouts), \
        'no tensor of the case comes within 16 MiB of 2^31 bytes: nothing here that the small suites lack'
    for t in layouts:
        assert t.sp[2] * t.pool[2] == base_sp[2] * t.fine[2], (t.name, 'boxes span full rows of W')
        for label, p in required_points(t):
            assert any(box_holds(b, t, p) for b in boxes), f'{t.name}: no box holds the voxel {label} {p}'
    for (n, d0, d1, h0, h1) in boxes:
        assert has_seam(d0, d1, base_sp[0], seam[0]) and has_seam(h0, h1, base_sp[1], seam[1]), ((n, d0, d1, h0, h1), 'spans no tile seam')


def smallest_batch(*sample_bytes, past=B32):
    """The smallest n at which the last sample of every tensor (bytes per sample given) starts at or past byte `past`."""
    return max(-(-past // b) for b in sample_bytes) + 1


def box_reference(x, weff, box, bias=None, slope=None, mask=None, mask_slope=0.25, pool=0):
    """The exact fp64 result of conv3d(x, weff) ('SAME', stride 1, odd filter) + bias + LeakyReLU on the box, from the box of x it
    depends on: (pre, ref) on the host, NCDHW with one sample.  pre is the value before mask and pooling (sign words are taken from
    it), ref the stored value: pre, masked with the box of the sign words `mask` [n D H W][cout / 32] where given, block means
    where pool is set (the box is then whole pooling blocks).  x: NCDHW view of any device; weff: DHWIO, coef folded in."""
    n, d0, d1, h0, h1 = box
    _, _, D, H, Wd = x.shape
    pd, ph = weff.shape[0] // 2, weff.shape[1] // 2
    a0, a1, b0, b1 = max(d0 - pd, 0), min(d1 + pd, D), max(h0 - ph, 0), min(h1 + ph, H)
    xc = x[n:n + 1, :, a0:a1, b0:b1].cpu()      # the planes / rows the tensor does not have stay the zeros conv_ref pads with
    y = R.conv_ref(xc, weff.cpu())[:, :, d0 - a0:d1 - a0, h0 - b0:h1 - b0]
    pre = R.bias_act(y, None if bias is None else bias.cpu(), slope)
    ref = pre
    if mask is not None:
        words = mask.reshape(-1, D, H, Wd, mask.shape[-1])[n, d0:d1, h0:h1].cpu()
        ref = R.apply_mask(ref, words.reshape(-1, words.shape[-1]), mask_slope)
    if pool:
        ref = R.pool_mean(ref, pool)
    return pre, ref


def disjoint(boxes):
    """The boxes with every two of one sample that intersect replaced by their bounding box, until none intersect: the sparse
    right-hand side of a weight gradient is filled, and its reference summed, box by box, so a voxel may lie in one box only."""
    boxes = sorted(set(boxes))
    merged = True
    while merged:
        merged = False
        for i in range(len(boxes)):
            for j in range(i + 1, len(boxes)):
                a, b = boxes[i], boxes[j]
                if a[0] == b[0] and a[1] < b[2] and b[1] < a[2] and a[3] < b[4] and b[3] < a[4]:
                    boxes[i] = (a[0], min(a[1], b[1]), max(a[2], b[2]), min(a[3], b[3]), max(a[4], b[4]))
                    del boxes[j]
                    merged = True
                    break
            if merged:
                break
    return boxes


def box_voxels(boxes, w):
    return sum((d1 - d0) * (h1 - h0) * w for _, d0, d1, h0, h1 in boxes)


def wgrad_box_reference(x, dy, box, k):
    """The exact fp64 contribution (dw [kd][kh][kw][cin][cout], db [cout]) of the voxels of one box to the weight and bias gradient
    of a 'SAME' convolution, for a dy that is zero around the box: wgref.wgrad_ref on the box plus halo of x and the box of dy.
    x, dy: NCDHW views on any device."""
    from tests import wgref
    n, d0, d1, h0, h1 = box
    _, _, D, H, _ = x.shape
    pd, ph = k[0] // 2, k[1] // 2
    a0, a1, b0, b1 = max(d0 - pd, 0), min(d1 + pd, D), max(h0 - ph, 0), min(h1 + ph, H)
    xc = x[n:n + 1, :, a0:a1, b0:b1].cpu()
    dyc = torch.zeros((1, dy.shape[1], a1 - a0, b1 - b0, dy.shape[4]), dtype=dy.dtype)
    dyc[:, :, d0 - a0:d1 - a0, h0 - b0:h1 - b0] = dy[n:n + 1, :, d0:d1, h0:h1].cpu()
    return wgref.wgrad_ref(xc, dyc, k)


def _low_crop(box, D, H):
    n, d0, d1, h0, h1 = box
    return max(d0 - 1, 0), min(d1 + 1, D), max(h0 - 1, 0), min(h1 + 1, H)


def upconv_box_reference(x, weff, box, bias=None, slope=None):
    """conv3d(upscale3d(x), weff) + bias + LeakyReLU on the fine voxels of a LOW-resolution box, from the box of x plus one
    low-resolution voxel around it: fp64, NCDHW, on the host."""
    n, d0, d1, h0, h1 = box
    a0, a1, b0, b1 = _low_crop(box, x.shape[2], x.shape[3])
    y = R.conv_ref(x[n:n + 1, :, a0:a1, b0:b1].cpu(), weff.cpu(), ups=True)
    return R.bias_act(y[:, :, 2 * (d0 - a0):2 * (d1 - a0), 2 * (h0 - b0):2 * (h1 - b0)], None if bias is None else bias.cpu(), slope)


def updgrad_box_reference(gy, weff, box):
    """The gradient of conv3d(upscale3d(x), weff) for the LOW-resolution voxels of a box, from the fine gradient gy of the box plus
    one low-resolution voxel around it."""
    n, d0, d1, h0, h1 = box
    a0, a1, b0, b1 = _low_crop(box, gy.shape[2] // 2, gy.shape[3] // 2)
    g = R.dgrad_ref(gy[n:n + 1, :, 2 * a0:2 * a1, 2 * b0:2 * b1].cpu(), weff.cpu(), ups=True)
    return g[:, :, d0 - a0:d1 - a0, h0 - b0:h1 - b0]


def make_geom(sp, k, bm, prefer_w32=False, force=None):
    """(TD, TH, TW) of sg_make_geom (csrc/common.h): the power-of-two tile of at most bm voxels, TW <= 32, that stages the fewest
    halo voxels; the first of equal scores wins (td runs innermost, so 4 x 2 x 32 comes before 2 x 4 x 32)."""
    d, h, w = sp
    p = [v // 2 for v in k]
    if force:
        return min(force[0], d), min(force[1], h), min(w, 32)
    p2 = lambda v: 1 << max(v - 1, 0).bit_length()
    best, tile = 1e300, (1, 1, 1)
    tw = min(p2(w), 32)
    while tw >= 1:
        th = 1
        while th <= p2(h) and tw * th <= bm:
            td = 1
            while td <= p2(d) and tw * th * td <= bm:
                cw, ch, cd = min(tw, w), min(th, h), min(td, d)
                tiles = float(-(-w // cw) * -(-h // ch) * -(-d // cd))
                score = tiles * ((cw + 2 * p[2]) * (ch + 2 * p[1]) * (cd + 2 * p[0]) + 0.25 * bm) - 1e-3 * cw
                if prefer_w32 and cw != min(w, 32):
                    score *= 4.0
                if score < best:
                    best, tile = score, (cd, ch, cw)
                td <<= 1
            th <<= 1
        tw >>= 1
    return tile


def kernel_tile(kernel, sp, k):
    """(TD, TH) of the output tiles the named kernel cuts a sample of extent sp into: the D and H periods at which two blocks (or two
    steps of one block's walk) meet.  Plane-sliding kernels count the planes they advance by as TD."""
    name = kernel.split('<')[0]
    if name == 'conv_fwd3w':
        return 2, 16                      # columns of 16 x 32.  In D a block walks its column in plane pairs; seams BETWEEN blocks lie at
                                          # multiples of seglen (conv3w.hip:914-924), which is D itself while ncol >= gx, as at every size here
    if name in ('conv_fwd3s', 'conv_fwd3p16', 'conv_fwd3p', 'conv_wgrad3l', 'conv_wgrad3'):
        return 2, 8 if name.startswith('conv_fwd') else 4      # 2 x 4 x 32 tiles; the forward kernels walk H-adjacent pairs
    if name in ('conv_fwd3r', 'conv_fwd4', 'conv_fwd5', 'conv_wgrad2'):
        return make_geom(sp, k, 256, True)[:2]
    if name == 'conv_fwd2':
        return make_geom(sp, k, 256, True)[:2]
    if name in ('conv_fwd', 'conv_wgrad'):
        return make_geom(sp, k, 256)[:2]
    if name in ('upconv_subpixel_fwd', 'upconv_subpixel_dgrad', 'upconv_subpixel_wgrad'):
        w = sp[2]
        return (2, 4) if w % 32 == 0 else ((2, 8) if w % 16 == 0 else (4, 8))      # subpix_tile: 2 x 4 x 32, 2 x 8 x 16, 4 x 8 x 8
    if name == 'conv_small_fwd' or name == 'conv_small_wgrad':
        return 1, 64                      # strips of 64 rows of one image where every wave still gets an item (small.hip:377), as at these sizes
    return 1, 1                           # voxel-wise kernels (pointwise, GEMM over the folded batch, planes): no spatial tile


def upwgrad_box_reference(x, dy, box, k=(3, 3, 3)):
    """The contribution of the fine voxels of a LOW-resolution box to the weight and bias gradient of conv3d(upscale3d(x)), for a fine dy
    that is zero around them: wgref.wgrad_ref(ups=True) on the box of x plus one low-resolution voxel around it."""
    from tests import wgref
    n, d0, d1, h0, h1 = box
    a0, a1, b0, b1 = _low_crop(box, x.shape[2], x.shape[3])
    dyc = torch.zeros((1, dy.shape[1], 2 * (a1 - a0), 2 * (b1 - b0), dy.shape[4]), dtype=dy.dtype)
    dyc[:, :, 2 * (d0 - a0):2 * (d1 - a0), 2 * (h0 - b0):2 * (h1 - b0)] = dy[n:n + 1, :, 2 * d0:2 * d1, 2 * h0:2 * h1].cpu()
    return wgref.wgrad_ref(x[n:n + 1, :, a0:a1, b0:b1].cpu(), dyc, k, ups=True)
