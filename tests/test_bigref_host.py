"""tests/bigref.py on the host: the box reference against the crop of the full reference, the boundary points of every case of
tests/test_large_offsets_gpu.py at its real shape, and that check_cover() can fail."""
import pytest
import torch

from tests import bigref as B
from tests import fwdref as R
from tests import wgref as W
from tests import test_large_offsets_gpu as L


def _full(x, w, bias, slope, mask, pool):
    pre = R.bias_act(R.conv_ref(x, w), bias, slope)
    ref = pre if mask is None else R.apply_mask(pre, mask, 0.25)
    return pre, (R.pool_mean(ref, pool) if pool else ref)


@pytest.mark.parametrize('k,pool,masked', [((3, 3, 3), 0, False), ((3, 3, 3), 0, True), ((3, 3, 3), 1, False), ((3, 3, 3), 3, True),
                                           ((1, 3, 3), 0, False), ((1, 1, 1), 0, True)])
def test_box_reference_is_the_crop_of_the_full_reference(k, pool, masked):
    """Every box the chooser can place in a small tensor, the ones at the tensor's borders included."""
    n, cin, cout, sp = 2, 5, 40, (6, 8, 4)
    x = W.int_data((n, cin, *sp), 1, torch.float32)
    w = W.int_data((*k, cin, cout), 2, torch.float32).contiguous().double() * 0.25
    g = torch.Generator().manual_seed(3)
    bias = torch.randint(-3, 4, (cout,), generator=g).float()
    mask = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * sp[0] * sp[1] * sp[2], 2), generator=g, dtype=torch.int32) if masked else None
    pre, ref = _full(x, w, bias, 0.25, mask, pool)
    f = R.POOL_BLOCK.get(pool, (1, 1, 1))
    seen = 0
    for s in range(n):
        for d0 in range(0, sp[0], 2):
            for d1 in range(d0 + 2, sp[0] + 1, 2):
                for h0 in range(0, sp[1], 2):
                    for h1 in (h0 + 2, sp[1]):
                        bpre, bref = B.box_reference(x, w, (s, d0, d1, h0, h1), bias, 0.25, mask, 0.25, pool)
                        assert torch.equal(bpre, pre[s:s + 1, :, d0:d1, h0:h1])
                        assert torch.equal(bref, ref[s:s + 1, :, d0 // f[0]:d1 // f[0], h0 // f[1]:h1 // f[1]])
                        seen += 1
    assert seen > 50


@pytest.mark.parametrize('b', L.CASES, ids=[b.id for b in L.CASES])
def test_boxes_of_every_case_hold_the_required_points(b):
    """At the case's real shape: first and last voxel, both sides of every boundary, the rebased group at the boundary, for x, y
    and the sign / mask words; every box full rows of W across a tile seam in D and H, and small enough for a host reference."""
    lay, boxes = b.layouts(), b.boxes()
    B.check_cover(lay, boxes, b.c.sp, b.seam)
    for t in lay:
        labels = [lb for lb, _ in B.required_points(t)]
        assert labels[:2] == ['first', 'last']
        for bd in t.boundaries():
            e = bd.bit_length() - 1
            assert f'below byte 2^{e}' in labels and (bd == t.nbytes() or f'at byte 2^{e}' in labels)
            if t.group and bd < t.nbytes():
                assert f'first of the group at byte 2^{e}' in labels and f'last of the group at byte 2^{e}' in labels
    for (_, d0, d1, h0, h1) in boxes:
        assert (d1 - d0) * (h1 - h0) * b.c.sp[2] <= 50000, 'boxes stay small enough for a host reference (5 planes x 17 rows x 512 at most)'
    assert len(boxes) <= 24


@pytest.mark.parametrize('b', L.BATCH, ids=[b.id for b in L.BATCH])
def test_batched_cases_pass_the_boundary_they_name(b):
    """The last sample of x and of y starts at or past byte 2^32 (f32: 2^33, element 2^31), and with one sample fewer one of them
    would not; the gemm pair sits on both sides of n d h w cin = 2^31."""
    c = b.c
    if c.id.startswith('gemm'):
        assert (c.n * 128 * c.cin >= 2 ** 31) == (c.id == 'gemm_declines') and (c.n + (c.id == 'gemm_last')) * 128 * c.cin == 2 ** 31
        return
    past = B.B33 if c.dt == torch.float32 else B.B32
    xs, ys = b.x_layout(1).nbytes(), b.y_layout(1).nbytes()
    assert (c.n - 1) * min(xs, ys) >= past > (c.n - 2) * min(xs, ys)
    assert past // b.es == 2 ** 31               # the byte boundary is element offset 2^31 of this type


def test_check_cover_rejects_what_it_must():
    t = B.Layout('x', 17, (64, 256, 256), 32, 2, group=1)      # 17 samples of 256 MiB: byte 2^32 is the first of sample 16
    boxes = B.choose_boxes([t], t.sp)
    B.check_cover([t], boxes, t.sp)
    pts = dict(B.required_points(t))
    assert pts['below byte 2^32'] == (15, 63, 255, 255) and pts['at byte 2^32'] == (16, 0, 0, 0)
    assert pts['below byte 2^31'] == (7, 63, 255, 255) and pts['at byte 2^31'] == (8, 0, 0, 0)
    for drop in range(len(boxes)):      # every box is there for a point no other box holds
        with pytest.raises(AssertionError, match='no box holds'):
            B.check_cover([t], boxes[:drop] + boxes[drop + 1:], t.sp)
    with pytest.raises(AssertionError, match='tile seam'):      # a box that stops at the seam
        B.check_cover([t], boxes + [(3, 0, 4, 0, 16)], t.sp)
    small = B.Layout('x', 2, (64, 256, 256), 32, 2, group=1)     # 512 MiB: the exact suites' territory
    with pytest.raises(AssertionError, match='2\\^31'):
        B.check_cover([small], B.choose_boxes([small], small.sp), small.sp)
    # a sample that straddles the boundary: its own first and last voxel are required
    u = B.Layout('x', 7, (100, 256, 256), 32, 2, group=1)       # samples of 400 MiB: byte 2^31 lies inside sample 5
    pu = dict(B.required_points(u))
    n_at = pu['at byte 2^31'][0]
    assert n_at == 5 and pu['first of the group at byte 2^31'] == (n_at, 0, 0, 0) and pu['last of the group at byte 2^31'] == (n_at, 99, 255, 255)
    assert 0 < pu['at byte 2^31'][1] < 99


def test_a_narrowed_offset_lands_outside_the_values_a_box_compares():
    """What the GPU cases rely on to be able to fail: the voxel a 32-bit wrap of the byte offset would read instead (2^32 bytes
    earlier) is another voxel of the same allocation, and the boxes hold the first voxel past the boundary, where the wrapped
    offset is 0: the first voxel of the tensor, which holds other random values."""
    b = next(b for b in L.BATCH if b.id == '3w_plain')
    t = b.x_layout()
    at = dict(B.required_points(t))['at byte 2^32']
    assert any(B.box_holds(box, t, at) for box in b.boxes())
    byte = ((((at[0] * t.sp[0] + at[1]) * t.sp[1] + at[2]) * t.sp[2]) + at[3]) * t.voxel_bytes()
    assert byte >= 2 ** 32 and t.voxel_at_byte(byte % 2 ** 32)[0] < at[0]
    # a rebased route (conv3w.hip:217, base + n0 * sample_bytes) with the product narrowed to 32 bits: the last sample, which starts
    # at or past 2^32 by construction, is rebased 2^32 bytes too low, onto other samples' values; its last voxel is in a box
    last = (t.n - 1, *(v - 1 for v in t.sp))
    start = (t.n - 1) * t.sample_voxels() * t.voxel_bytes()
    assert start >= 2 ** 32 and t.voxel_at_byte(start % 2 ** 32)[0] < t.n - 1 and any(B.box_holds(box, t, last) for box in b.boxes())
    # a guard moved up by one plane: the 'above' case of conv3w.hip:902 then runs the guarded kernel with a sample of exactly 2^31
    # bytes, whose last voxels lie at buffer offsets the resource (num_records = (int) 2^31 < 0) does not cover; the last voxel is
    # required of that case's boxes
    g = next(b for b in L.GUARD if b.id == '3w_above')
    ty = g.y_layout()
    assert ty.nbytes() == 2 ** 31 and any(B.box_holds(box, ty, (0, 127, 511, 511)) for box in g.boxes())


@pytest.mark.parametrize('k', [(3, 3, 3), (1, 3, 3), (1, 1, 1)])
def test_weight_gradient_summed_over_boxes_is_the_full_reference(k):
    """dy zero except on disjoint boxes (two of them touching, two at the tensor's borders): the box contributions add up to
    wgref.wgrad_ref of the whole tensors, each is non-zero and no two are equal."""
    n, cin, cout, sp = 2, 5, 7, (6, 8, 4)
    x = W.int_data((n, cin, *sp), 11, torch.float32)
    boxes = B.disjoint([(0, 0, 2, 0, 3), (0, 1, 3, 2, 5), (0, 4, 6, 5, 8), (1, 2, 4, 3, 6), (1, 4, 5, 3, 6), (1, 5, 6, 0, 2)])
    assert (0, 0, 3, 0, 5) in boxes and len(boxes) == 5      # the two that intersect became their bounding box
    full = W.int_data((n, cout, *sp), 12, torch.float32)
    dy = torch.zeros_like(full)
    for (s, d0, d1, h0, h1) in boxes:
        dy[s, :, d0:d1, h0:h1] = full[s, :, d0:d1, h0:h1]
    dw, db = W.wgrad_ref(x, dy, k)
    parts = [B.wgrad_box_reference(x, dy, b, k) for b in boxes]
    assert torch.equal(sum(p[0] for p in parts), dw) and torch.equal(sum(p[1] for p in parts), db)
    for i, p in enumerate(parts):
        assert bool(p[0].abs().sum() > 0) and all(not torch.equal(p[0], q[0]) for q in parts[:i])


@pytest.mark.parametrize('b', L.WGRAD, ids=[b.id for b in L.WGRAD])
def test_weight_gradient_cases_cover_their_points_inside_the_exact_range(b):
    boxes = b.boxes()
    B.check_cover(b.layouts(), boxes, b.c.sp, b.seam)
    for i, p in enumerate(boxes):
        for q in boxes[:i]:
            assert not (p[0] == q[0] and p[1] < q[2] and q[1] < p[2] and p[3] < q[4] and q[3] < p[4]), 'boxes are disjoint'
    L.sparse_rhs_is_exact(b)
    assert 9 * B.box_voxels(boxes, b.c.sp[2]) < 2 ** 24


def test_upconvolution_box_references_are_the_crop_of_the_full_reference():
    n, cin, cout, low = 2, 3, 5, (4, 6, 4)
    x = W.int_data((n, cin, *low), 21, torch.float32)
    gy = W.int_data((n, cout, *(2 * v for v in low)), 22, torch.float32)
    w = W.int_data((3, 3, 3, cin, cout), 23, torch.float32).contiguous().double() * 0.25
    bias = torch.arange(cout).float() - 2
    full = R.bias_act(R.conv_ref(x, w, ups=True), bias, 0.25)
    gfull = R.dgrad_ref(gy, w, ups=True)
    for s in range(n):
        for d0 in range(low[0]):
            for d1 in range(d0 + 1, low[0] + 1):
                for h0, h1 in ((0, 2), (1, 4), (3, 6), (0, 6)):
                    box = (s, d0, d1, h0, h1)
                    assert torch.equal(B.upconv_box_reference(x, w, box, bias, 0.25), full[s:s + 1, :, 2 * d0:2 * d1, 2 * h0:2 * h1])
                    assert torch.equal(B.updgrad_box_reference(gy, w, box), gfull[s:s + 1, :, d0:d1, h0:h1])


@pytest.mark.parametrize('b', L.SUB, ids=[b.id for b in L.SUB])
def test_subpixel_cases_cover_their_points(b):
    lay, boxes = L.sub_layouts(b), L.sub_boxes(b)
    B.check_cover(lay, boxes, b.c.sp, b.seam)
    assert lay[1].sp == tuple(2 * v for v in b.c.sp) and lay[1].nbytes() >= B.B31 - B.NEAR
    assert all((d1 - d0) * (h1 - h0) * b.c.sp[2] <= 50000 for _, d0, d1, h0, h1 in boxes)


@pytest.mark.parametrize('dtype', L.EW_DT, ids=['bf16', 'f32'])
def test_elementwise_cases_cover_their_points(dtype):
    lay, boxes = L._ew_layouts(dtype), L.ew_boxes(dtype)
    B.check_cover(lay, boxes, L.EW_SP, B.SEAM)
    assert lay[0].nbytes() > (B.B32 if dtype == torch.bfloat16 else B.B33)
    W.assert_exact_range(3, 0.25, B.box_voxels(boxes, L.EW_SP[2]))


@pytest.mark.parametrize('up', [True, False], ids=['upscale2x', 'downscale2x'])
def test_scaling_cases_cover_their_points(up):
    base, lay = L.scale_layouts(up)
    B.check_cover(lay, L.scale_boxes(up), base, B.SEAM)
    assert max(t.nbytes() for t in lay) > B.B32


@pytest.mark.parametrize('b', L.CASES + L.WGRAD + L.SUB + L.FALLBACK + [L.SUBW], ids=[b.id for b in L.CASES + L.WGRAD + L.SUB + L.FALLBACK + [L.SUBW]])
def test_the_seam_of_every_case_is_a_seam_of_its_kernels_tile(b):
    """A box spans a multiple of the case's seam in D and H: that is a tile seam only if the seam is a multiple of the kernel's TD
    and TH (bigref.kernel_tile: the launchers' constants, or sg_make_geom restated).  The pieces of the guard cases run other
    kernels; what counts here is the kernel of the large call, the one the case names."""
    td, th = B.kernel_tile(b.c.kernel, b.c.sp, b.c.k)
    for dim, t in ((0, td), (1, th)):      # (an extent within one seam period is held whole by every box: nothing to straddle)
        assert b.c.sp[dim] <= b.seam[dim] or b.seam[dim] % t == 0, (b.c.kernel, (td, th), b.seam)


def test_make_geom_restates_the_launchers_tiles():
    """sg_make_geom (csrc/common.h) restated: 1 x 8 x 32 tiles for 1x3x3 at 128 x 128 (test_conv_fwd_exact_gpu.py's 3r_bf16_133
    comment), the caller-imposed 2 x 4 x 32, the generic kernel's 8 x 4 x 8, and the tie the host condition depends on: 4 x 2 x 32
    comes before 2 x 4 x 32 at equal score, so conv_fwd3r / 4 / 5 and conv_wgrad2 cut D in fours."""
    assert B.make_geom((16, 64, 40), (3, 3, 3), 256, True) == (4, 2, 32)
    assert B.make_geom((127, 512, 512), (3, 3, 3), 256, True) == (4, 2, 32)
    assert B.make_geom((1, 128, 128), (1, 3, 3), 256, True) == (1, 8, 32)
    assert B.make_geom((253, 512, 520), (3, 3, 3), 256) == (8, 4, 8)
    assert B.make_geom((4, 8, 32), (3, 3, 3), 256, True, force=(2, 4)) == (2, 4, 32)


def test_subpixel_weight_gradient_case_covers_its_points_inside_the_exact_range():
    lay, boxes = L.subw_layouts(), L.subw_boxes()
    B.check_cover(lay, boxes, L.SUBW.c.sp, L.SUBW.seam)
    assert min(t.nbytes() - t.nbytes() // t.n for t in lay) >= B.B32      # the last sample of x and of gy starts at or past 2^32
    W.assert_exact_range(9, 1, 8 * B.box_voxels(boxes, L.SUBW.c.sp[2]))


@pytest.mark.parametrize('b', L.FALLBACK, ids=[b.id for b in L.FALLBACK])
def test_refusal_cases_cover_their_points(b):
    """The two refusals at their real shapes: what runs in the entry point's place is checked on boxes that hold the required points
    of every tensor it touches -- for subdg_above also the 2^32-byte full-resolution gradient functional._upconv_dgrad writes and
    reads back, whose byte 2^31 falls at fine plane 64."""
    lay, boxes = L.fallback_layouts(b), L.fallback_boxes(b)
    B.check_cover(lay, boxes, b.c.sp, b.seam)
    assert all((d1 - d0) * (h1 - h0) * b.c.sp[2] <= 50000 for _, d0, d1, h0, h1 in boxes) and len(boxes) <= 24
    if b is L.SUBDG_ABOVE:
        full = lay[-1]
        assert full.nbytes() == 2 ** 32 and dict(B.required_points(full))['at byte 2^31'] == (0, 256, 0, 0)
        assert any(box[1] < 128 < box[2] for box in boxes), 'a box straddles low plane 128, where the gradient crosses byte 2^31'
