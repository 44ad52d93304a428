"""Every weight-gradient route (wgrad_bias_impl in csrc/wgrad.hip, conv_small_wgrad in csrc/small.hip, upconv_subpixel_wgrad
in csrc/subpix.hip) on inputs for which every f32 sum is exact: x and dy are integers in [-3, 3], so each product and each
partial sum is an integer below 9 x (voxels) < 2^24 whatever the tiling, K split, atomic order or slab order, and the fp64
reference of tests/wgref.py is the exact value.  The assertion is torch.equal: one lost halo row, one lost, doubled or
wrong-tap voxel or one skipped slab changes the integer (the N(0, 1) tests allow 2e-3 x max|dw|, 5 to 13 product units
at the benchmarked size, and cannot see any of these).

Each case names the launch constant or dispatch condition it crosses and asserts the kernel that ran by name
(sg_prof_enable / sg_prof_collect): a case that silently lands on another route fails.  coef is 0.25 (exact) in every other
case and 0.37 in the rest: the expected value is then np.float32(0.37) * np.float32(sum), the one rounding the finalize
kernels perform.  Workspaces handed to calls without SG_WGRAD_CLEAN_WORKSPACE are filled with 0xFF bytes (NaNs) and dw / db
with a sentinel, so a word the kernels neither clear nor write shows.

No route was found that rounds before the sum: every case is compared bit for bit."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import wgref as R

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
K333, K133, K111 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
SENTINEL = 7.5


def dev():
    assert torch.cuda.is_available(), 'GPU tests need a GPU'
    return torch.device('cuda:0')


def _libs():
    from saragan_amd import _lib
    return _lib, _lib.load()


def _dt(dtype):
    from saragan_amd import _lib
    return _lib.SG_BF16 if dtype == BF else _lib.SG_F32


def _wgrad_kernels(_lib, lib):
    """Names of the weight-gradient launches (profile kind 1) that succeeded since sg_prof_enable(1)."""
    ents = (_lib.ProfEntry * 16)()
    cnt = C.c_int32(0)
    lib.sg_prof_collect(ents, 16, C.byref(cnt))
    return sorted({ents[i].kernel.decode() for i in range(cnt.value) if ents[i].kind == 1})


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _garbage(nbytes):
    return torch.full((max(int(nbytes), 16),), 255, dtype=torch.uint8, device=dev())


class Case:
    def __init__(self, cid, kernel, n, cin, cout, sp, k=K333, ups=False, dt=BF, env=None, det=False, gain=None, db=True):
        self.id, self.kernel, self.n, self.cin, self.cout, self.sp, self.k = cid, kernel, n, cin, cout, tuple(sp), tuple(k)
        self.ups, self.dt, self.env, self.det, self.gain, self.db = ups, dt, env or {}, det, gain, db


@functools.lru_cache(maxsize=64)
def _data(n, cin, cout, sp, k, ups, dt, gain):
    """Inputs (on the device, NDHWC) and the exact fp64 dw / db of one case: computed once, shared by every mode of the case and
    never modified.  gain (masked gather cases): dy is the half-resolution gradient, the reference uses the effective dy."""
    seed = 1000 + 7 * cin + 3 * cout + sp[0] + 5 * sp[1] + 11 * sp[2] + n
    half = tuple(v // 2 for v in sp)
    x = R.int_data((n, cin, *(half if ups else sp)), seed, dt)
    dy = R.int_data((n, cout, *(half if gain is not None else sp)), seed + 1, dt)
    bits = None
    if gain is None:
        R.assert_exact_range(9, 1, n * sp[0] * sp[1] * sp[2])
        dw, db = R.wgrad_ref(x, dy, k, ups=ups)
    else:
        # slope 0.25 and a power-of-two gain: the staged bf16(dy * gain * slope) is exact; unit = gain * slope, 36 units per term
        R.assert_exact_range(9 * gain, gain * 0.25, n * sp[0] * sp[1] * sp[2])
        g = torch.Generator().manual_seed(seed + 2)
        bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (n * sp[0] * sp[1] * sp[2], cout // 32), generator=g, dtype=torch.int32)
        dw, db = R.wgrad_ref(x, R.masked_dy(dy, bits, 0.25, gain, (n, cout, *sp)), k)
        bits = bits.to(dev())
    return x.to(dev()), dy.to(dev()), bits, dw, db


@pytest.fixture(scope='module', autouse=True)
def _release_case_data():
    """The cached inputs live on the device (the pointwise second-trip cases are tens of MB): released when the module is done."""
    yield
    _data.cache_clear()


def _case_data(c):
    return _data(c.n, c.cin, c.cout, c.sp, c.k, c.ups, c.dt, c.gain)


def _shape(c):
    _lib, _ = _libs()
    return _lib.ConvShape(c.n, *c.sp, c.cin, c.cout, *c.k, 1 if c.ups else 0)


def _launch(c, x, dy, bits, dw, db, coef, flags=0, ws=None):
    """One call of the C ABI for case c; returns (code, names of the weight-gradient kernels that ran)."""
    _lib, lib = _libs()
    shp = _shape(c)
    dt = _dt(c.dt)
    if ws is None:
        ws = _garbage(lib.sg_conv3d_wgrad_workspace(C.byref(shp), dt))
    dbp = db.data_ptr() if db is not None else None
    lib.sg_prof_enable(1)
    try:
        if flags:
            rc = lib.sg_conv3d_wgrad_bias_ex(x.data_ptr(), dy.data_ptr(), bits.data_ptr() if bits is not None else None, 0.25,
                                             c.gain if c.gain is not None else 1.0, dw.data_ptr(), dbp, coef, flags, ws.data_ptr(),
                                             ws.numel(), C.byref(shp), dt, _stream())
        elif bits is not None:
            rc = lib.sg_conv3d_wgrad_bias_up_masked(x.data_ptr(), dy.data_ptr(), bits.data_ptr(), 0.25, c.gain, dw.data_ptr(), dbp, coef,
                                                    ws.data_ptr(), ws.numel(), C.byref(shp), dt, _stream())
        else:
            rc = lib.sg_conv3d_wgrad_bias(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), dbp, coef, ws.data_ptr(), ws.numel(), C.byref(shp),
                                          dt, _stream())
        torch.cuda.synchronize()
        names = _wgrad_kernels(_lib, lib)
    finally:
        lib.sg_prof_enable(0)
    return rc, names


def _outputs(c):
    dw = torch.full((*c.k, c.cin, c.cout), SENTINEL, device=dev())
    db = torch.full((c.cout,), SENTINEL, device=dev()) if c.db else None
    return dw, db


def _check(c, dw, db, coef, dw64, db64, what=''):
    want = R.scaled(dw64, coef)
    got = dw.cpu()
    if not torch.equal(got, want):
        bad = (got != want)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError(f'{c.id} {what}: dw differs in {int(bad.sum())} of {bad.numel()} entries, first at {idx}: '
                             f'{float(got[tuple(idx)])!r} != {float(want[tuple(idx)])!r}')
    if db is not None:
        assert torch.equal(db.cpu(), db64.float()), f'{c.id} {what}: db'


def _run_exact(c, coef, slabs, sg_env):
    import saragan_amd
    _lib, lib = _libs()
    x, dy, bits, dw64, db64 = _case_data(c)
    if c.env:
        sg_env(**c.env)
    if slabs:
        saragan_amd.set_deterministic(True)
    try:
        dw, db = _outputs(c)
        rc, names = _launch(c, x, dy, bits, dw, db, coef)
        _lib.check(rc, c.id)
    finally:
        if slabs:
            saragan_amd.set_deterministic(False)
    assert names == [c.kernel], (c.id, names)
    _check(c, dw, db, coef, dw64, db64, 'slabs' if slabs else 'atomics')


# ----------------------------------------------------------------------------------------------------------------------
# Sliding-halo family (launch_wgrad3): bf16, 3x3x3, tiles 2 x 4 x 32 (w16: 2 x 8 x 16).  gx = (256 / pairs) / 8 * 8, lowered by 8
# while ncol < 2 gx and (gx - 8) * pairs >= 64 (w16: 128); ncol = n * nTh * nTw columns, nTd = cdiv(D, 2) tiles per column.
# A block's XCD group owns cpx = cdiv(ncol, 8) columns, block slot b of per_x = gx / 8 takes cdiv(cpx - b, per_x) of them, its two
# wave groups alternate.  Reproducible mode: the lean kernels write gx slabs, conv_wgrad3 2 gx (one per wave group).
# ----------------------------------------------------------------------------------------------------------------------
HALO = [
    # pairs = 1: gx = 256 -> 64; ncol = 2 (nTh = 2), nTd = 2: cpx = 1, only slots 0 of XCD groups 0 and 1 hold a column, every second
    # wave group and 62 whole blocks have none and must send nothing.  slabs: 64, 62 of them all zero.
    Case('3l_two_columns', 'conv_wgrad3l', 1, 32, 32, (4, 8, 32), det=True),
    Case('3l_D5', 'conv_wgrad3l', 1, 32, 32, (5, 8, 32)),                  # nTd = 3, the last D tile half filled
    Case('3l_H6', 'conv_wgrad3l', 1, 32, 32, (4, 6, 32)),                  # nTh = 2, the last H tile has 2 of 4 rows
    Case('3l_H10', 'conv_wgrad3l', 1, 32, 32, (4, 10, 32)),                # nTh = 3, ncol = 3
    # ciT x coT = 2 x 3 partial channel tiles (8 of 32 rows in the last): pairs = 6, gx = 40 -> 16 ((16 - 8) * 6 < 64).  slabs: 16
    Case('3l_40to72', 'conv_wgrad3l', 1, 40, 72, (4, 8, 32), det=True),
    # a wave group that walks three columns: pairs = 3 * 4 = 12, gx = 16 (ncol = 65 >= 2 gx), per_x = 2, cpx = cdiv(65, 8) = 9;
    # slot 0 takes cdiv(9, 2) = 5 columns, its group 0 three of them and group 1 two; D = 3: nTd = 2, half-filled last tile
    Case('3l_three_columns_per_group', 'conv_wgrad3l', 1, 72, 104, (3, 260, 32)),
    Case('3l_W64', 'conv_wgrad3l', 1, 32, 32, (4, 4, 64)),                 # nTw = 2: one seam in W
    Case('3l_W96', 'conv_wgrad3l', 1, 32, 32, (4, 4, 96)),                 # nTw = 3: a tile with a neighbour on both sides
    # x at half resolution, gathered nearest-x2 while staged
    Case('3l_ups_two_columns', 'conv_wgrad3l<ups>', 1, 32, 32, (4, 8, 32), ups=True, det=True),
    Case('3l_ups_D6_H6_W64_40to72', 'conv_wgrad3l<ups>', 1, 40, 72, (6, 6, 64), ups=True, det=True),   # nTd = 3, partial H tile, W seam
    Case('3l_ups_H10', 'conv_wgrad3l<ups>', 1, 32, 32, (4, 10, 32), ups=True),
    Case('3l_ups_W96', 'conv_wgrad3l<ups>', 1, 32, 32, (4, 4, 96), ups=True),     # nTw = 3 over low W = 48: neighbours on both sides
    # the three-column walk of 3l_three_columns_per_group on the gathered x (low 2 x 130 x 16): gx = 16, ncol = 65, cpx = 9
    Case('3l_ups_three_columns_per_group', 'conv_wgrad3l<ups>', 1, 72, 104, (4, 260, 32), ups=True),
    # half-resolution dy, masked and scaled while staged (sg_conv3d_wgrad_bias_up_masked): slope 0.25, gains 1/8 and 1
    Case('3l_gather_32', 'conv_wgrad3l<dy gather>', 1, 32, 32, (4, 8, 32), gain=0.125, det=True),
    Case('3l_gather_96_ragged', 'conv_wgrad3l<dy gather>', 1, 40, 96, (6, 6, 64), gain=1.0, det=True),  # coT = 3 mask words per voxel
    # 16-wide levels: ncol = n * H / 8.  pairs = 1: gx = 256 -> 128 ((gx - 8) >= 128 stops at 128)
    Case('w16_minimum', 'conv_wgrad3l<w16>', 2, 32, 32, (4, 8, 16), det=True),      # ncol = 2, nTd = 2; slabs: 128
    Case('w16_H24', 'conv_wgrad3l<w16>', 1, 32, 32, (4, 24, 16)),                   # three H tiles
    Case('w16_D6', 'conv_wgrad3l<w16>', 2, 32, 32, (6, 8, 16)),                     # nTd = 3
    Case('w16_batch1_128to512', 'conv_wgrad3l<w16>', 1, 128, 512, (4, 16, 16)),     # pairs = 64, gx = 8 blocks, ncol = 2 columns
    Case('w16_ragged', 'conv_wgrad3l<w16>', 2, 40, 72, (6, 24, 16), det=True),      # pairs = 6, gx = 40 -> 24, ncol = 6; slabs: 24
    Case('w16_ups_minimum', 'conv_wgrad3l<ups,w16>', 2, 32, 32, (4, 8, 16), ups=True, det=True),
    Case('w16_ups_H24_D6_ragged', 'conv_wgrad3l<ups,w16>', 1, 40, 72, (6, 24, 16), ups=True, det=True),
    Case('w16_ups_batch1_128to512', 'conv_wgrad3l<ups,w16>', 1, 128, 512, (4, 16, 16), ups=True),
    # the K loop on the 16x16x32 MFMA (SG_WGRAD3L_16=1): every variant at a regular and a ragged shape
    Case('m16_3l', 'conv_wgrad3l', 1, 32, 32, (4, 8, 32), env={'SG_WGRAD3L_16': 1}),
    Case('m16_3l_ragged', 'conv_wgrad3l', 1, 40, 72, (5, 6, 64), env={'SG_WGRAD3L_16': 1}),
    Case('m16_ups', 'conv_wgrad3l<ups>', 1, 32, 32, (4, 8, 32), ups=True, env={'SG_WGRAD3L_16': 1}),
    Case('m16_ups_ragged', 'conv_wgrad3l<ups>', 1, 40, 72, (6, 6, 64), ups=True, env={'SG_WGRAD3L_16': 1}),
    Case('m16_gather', 'conv_wgrad3l<dy gather>', 1, 32, 32, (4, 8, 32), gain=0.125, env={'SG_WGRAD3L_16': 1}),
    Case('m16_gather_ragged', 'conv_wgrad3l<dy gather>', 1, 40, 96, (6, 6, 64), gain=1.0, env={'SG_WGRAD3L_16': 1}),
    Case('m16_w16', 'conv_wgrad3l<w16>', 2, 32, 32, (4, 8, 16), env={'SG_WGRAD3L_16': 1}),
    Case('m16_w16_ragged', 'conv_wgrad3l<w16>', 2, 40, 72, (6, 24, 16), env={'SG_WGRAD3L_16': 1}),
    Case('m16_w16_ups', 'conv_wgrad3l<ups,w16>', 2, 32, 32, (4, 8, 16), ups=True, env={'SG_WGRAD3L_16': 1}),
    Case('m16_w16_ups_ragged', 'conv_wgrad3l<ups,w16>', 1, 40, 72, (6, 24, 16), ups=True, env={'SG_WGRAD3L_16': 1}),
    # W = 40 >= 32 and no multiple of 32: 32-wide tiles, the second 8 wide, so not lean.  slabs: 2 gx = 128
    Case('wgrad3_W40', 'conv_wgrad3<3,3,3>', 1, 32, 32, (4, 8, 40), det=True),
    Case('wgrad3_W40_ragged', 'conv_wgrad3<3,3,3>', 1, 40, 72, (5, 6, 40), det=True),
    Case('wgrad3_no_lean', 'conv_wgrad3<3,3,3>', 1, 32, 32, (4, 8, 32), env={'SG_WGRAD_NO_LEAN': 1}),
]

# ----------------------------------------------------------------------------------------------------------------------
# The other MFMA routes, bf16.
# conv_wgrad_planes<HW>: 1x3x3, H = W = 4 | 8, channels multiples of 32, tiles of P = 128 / (H W) whole (n, d) planes through a ring
#   of three LDS buffers; gx = min(16, cdiv(512, pairs), ntiles) blocks per pair, one slab each.
# conv_wgrad2: 256-voxel tiles 32 or 16 wide, gx = max(8, (256 / pairs) / 8 * 8), engaged from ntiles >= 2 gx; slabs: 2 gx.
# conv_wgrad<T,BM> (generic): P = min(cdiv(512, pairs), ntiles) blocks per pair, 28 taps per launch; slabs: P.
# ----------------------------------------------------------------------------------------------------------------------
MFMA = [
    Case('planes8_one_tile', 'conv_wgrad_planes<8>', 1, 32, 32, (2, 8, 8), K133, det=True),          # n d = 2 = P: ntiles = 1, gx = 1
    Case('planes4_one_tile', 'conv_wgrad_planes<4>', 2, 32, 32, (4, 4, 4), K133, det=True),          # n d = 8 = P
    Case('planes8_two_tiles', 'conv_wgrad_planes<8>', 2, 32, 32, (2, 8, 8), K133),                   # fewer tiles than the 3 ring slots
    # ntiles = 17 > gx = 16: block 0 takes a second tile; cin != cout, pairs = 2.  slabs: 16
    Case('planes8_more_tiles_than_blocks', 'conv_wgrad_planes<8>', 17, 32, 64, (2, 8, 8), K133, det=True),
    # ntiles = 5: one and two thirds ring turns; pairs = 2, gx = 5.  slabs: 5
    Case('planes4_five_tiles_64to32', 'conv_wgrad_planes<4>', 5, 64, 32, (8, 4, 4), K133, det=True),
    # (n d) % P != 0: the first shape the planes kernel refuses; 8-wide tiles are not conv_wgrad2's either
    Case('planes8_refused_odd_planes', 'conv_wgrad<bf16,256>', 3, 32, 32, (1, 8, 8), K133),
    Case('planes4_refused_odd_planes', 'conv_wgrad<bf16,256>', 3, 32, 32, (3, 4, 4), K133),
    # D = 2: a single D tile per column, nothing to slide over; pairs = 16, gx = 16; 1 x 32 x 1 tiles of 2 x 4 x 32 = 32 = 2 gx,
    # the engaging edge.  slabs: 32
    Case('wgrad2_333_engaging_edge', 'conv_wgrad2<3,3,3>', 1, 128, 128, (2, 128, 32), det=True),
    # pairs = 5 x 4 = 20 partial channel tiles, gx = 8; H = 130: 33 tiles of 2 x 4 x 32, the last with 2 of 4 rows.  slabs: 16
    Case('wgrad2_333_ragged', 'conv_wgrad2<3,3,3>', 1, 136, 120, (2, 130, 32), det=True),
    Case('wgrad2_333_one_tile_fewer', 'conv_wgrad<bf16,256>', 1, 128, 128, (2, 124, 32)),            # 31 tiles < 2 gx: generic kernel
    Case('wgrad2_133_16_wide', 'conv_wgrad2<1,3,3>', 32, 128, 128, (1, 16, 16), K133, det=True),     # tiles 1 x 16 x 16, 32 of them
    Case('wgrad2_133_32_wide', 'conv_wgrad2<1,3,3>', 32, 128, 128, (1, 8, 32), K133),                # tiles 1 x 8 x 32
    Case('wgrad2_133_ragged', 'conv_wgrad2<1,3,3>', 11, 136, 120, (1, 22, 32), K133, det=True),      # pairs = 20, gx = 8; 11 x 3 tiles, last of 6 rows
]
for _dt_, _nm in ((BF, 'conv_wgrad<bf16,256>'), (F32, 'conv_wgrad<f32,128>')):
    _t = 'bf16' if _dt_ == BF else 'f32'
    MFMA += [
        # channels no multiple of 8 (4 in f32): vec_x = vec_y = 0, the element-wise staging; one tile of 2 x 3 x 5 x 7 (TN = 2)
        Case(f'generic_{_t}_6to10', _nm, 2, 6, 10, (3, 5, 7), dt=_dt_, det=True),
        Case(f'generic_{_t}_24to40', _nm, 2, 24, 40, (3, 5, 7), dt=_dt_),           # vec on, partial 32 x 32 tiles on both sides
        Case(f'generic_{_t}_batch_folded', _nm, 4, 16, 16, (2, 4, 4), dt=_dt_),     # 32 voxels per sample: TN = 4 (f32: 4)
        Case(f'generic_{_t}_111_16to16', _nm, 2, 16, 16, (3, 5, 6), K111, dt=_dt_),  # 16 > 4 channels: not the pointwise reduction
        Case(f'generic_{_t}_555', _nm, 2, 8, 8, (3, 5, 6), (5, 5, 5), dt=_dt_, det=True),   # 125 taps: five launches of 28 into one tile
        Case(f'generic_{_t}_311', _nm, 2, 8, 8, (3, 5, 6), (3, 1, 1), dt=_dt_),
        Case(f'generic_{_t}_113', _nm, 2, 8, 8, (3, 5, 6), (1, 1, 3), dt=_dt_),
        Case(f'generic_{_t}_777', _nm, 1, 8, 8, (2, 3, 4), (7, 7, 7), dt=_dt_),     # the largest kernel the ABI accepts: 343 taps, 13 launches
        # 7x7x7 where a full 256 (128) voxel tile's halo, 8 x 10 x 38 rows, does not fit 160 KiB of LDS: the launcher comes down to
        # a smaller tile, as it does for generic_f32_555's two-sample tile (2 x 7 x 9 x 8 rows of 144 bytes)
        Case(f'generic_{_t}_777_halo_over_lds', _nm, 1, 8, 8, (4, 8, 32), (7, 7, 7), dt=_dt_),
        Case(f'generic_{_t}_many_tiles', _nm, 2, 12, 20, (6, 20, 24), dt=_dt_, det=True),   # ragged tiles in D, H and W; slabs: P = ntiles
    ]

ROUTES = HALO + MFMA
RUNS = [(c, False) for c in ROUTES] + [(c, True) for c in ROUTES if c.det]


@pytest.mark.parametrize('run', RUNS, ids=[f'{c.id}{"-slabs" if s else ""}' for c, s in RUNS])
def test_route_is_exact(run, sg_env):
    """Atomics, and for one regular and one ragged case per route the reproducible slab mode: the same exact reference."""
    c, slabs = run
    coef = 0.25 if ROUTES.index(c) % 2 == 0 else 0.37
    _run_exact(c, coef, slabs, sg_env)


def test_generic_kernel_slab_cap_holds_under_a_raised_block_target(sg_env):
    """SG_WGRAD_V1_BLOCKS=4096 in reproducible mode: 2 x 1 x 504 x 130 voxels in tiles of 1 x 32 x 8 are 544 tiles, pairs = 1, so the
    block target is min(4096, 544) = 544 where the workspace holds wgrad_slab_count = max(16, cdiv(512, 1)) = 512 slabs: the cap in
    launch_wgrad is what keeps the launch inside it (6 input channels: neither the small-channel nor a vector-staged kernel)."""
    c = Case('generic_slab_cap', 'conv_wgrad<bf16,256>', 2, 6, 10, (1, 504, 130), K133, env={'SG_WGRAD_V1_BLOCKS': 4096})
    _run_exact(c, 0.37, True, sg_env)


def test_upsampled_layer_the_subpixel_route_declines(monkeypatch):
    """Through functional.raw_wgrad with the sub-pixel route allowed: low W = 16 is no multiple of 32, so
    sg_upconv3d_subpixel_wgrad_supported declines and the layer must reach conv_wgrad3l<ups> (with the kept workspace)."""
    from saragan_amd import functional as F
    _lib, lib = _libs()
    c = Case('3l_ups_two_columns', 'conv_wgrad3l<ups>', 1, 32, 32, (4, 8, 32), ups=True)
    x, dy, _, dw64, db64 = _case_data(c)
    monkeypatch.setattr(F, '_NO_SUBPIXEL', False)
    low = _lib.ConvShape(1, 2, 4, 16, 32, 32, 3, 3, 3, 0)
    assert not lib.sg_upconv3d_subpixel_wgrad_supported(C.byref(low), _lib.SG_BF16)
    lib.sg_prof_enable(1)
    try:
        dw, db = F.raw_wgrad(x, dy, K333, 0.37, ups=True, want_db=True)
        torch.cuda.synchronize()
        names = _wgrad_kernels(_lib, lib)
    finally:
        lib.sg_prof_enable(0)
    assert names == [c.kernel], names
    _check(c, dw, db, 0.37, dw64, db64)


# ----------------------------------------------------------------------------------------------------------------------
# SG_WGRAD_ACCUMULATE / SG_WGRAD_CLEAN_WORKSPACE: every route that ends in wgrad_finalize_kernel
# ----------------------------------------------------------------------------------------------------------------------
FINALIZE = ['generic_bf16_24to40', 'generic_f32_6to10', 'wgrad2_333_engaging_edge', 'wgrad2_133_ragged', 'wgrad3_W40_ragged', '3l_40to72',
            '3l_ups_D6_H6_W64_40to72', '3l_gather_96_ragged', 'w16_ragged', 'w16_ups_minimum', 'planes8_more_tiles_than_blocks',
            'planes4_one_tile']
BY_ID = {c.id: c for c in ROUTES}


@pytest.mark.parametrize('cid', FINALIZE)
def test_accumulate_and_clean_workspace_are_exact(cid):
    """Accumulate: dw = prefill + np.float32(0.37) * sum, the __fmul_rn / __fadd_rn pair, onto an integer-valued prefill; db is written.
    Clean workspace: two calls in a row on a kept, zeroed buffer are both exact and leave sg_conv3d_wgrad_clean_bytes bytes zero."""
    _lib, lib = _libs()
    c = BY_ID[cid]
    x, dy, bits, dw64, db64 = _case_data(c)
    g = torch.Generator().manual_seed(5)
    pre = torch.randint(-50, 51, (*c.k, c.cin, c.cout), generator=g).float()
    dw, db = pre.to(dev()), torch.full((c.cout,), SENTINEL, device=dev())
    rc, names = _launch(c, x, dy, bits, dw, db, 0.37, flags=_lib.SG_WGRAD_ACCUMULATE)
    _lib.check(rc, cid)
    assert names == [c.kernel], names
    assert torch.equal(dw.cpu(), R.scaled(dw64, 0.37, prefill=pre)), 'accumulate'
    assert torch.equal(db.cpu(), db64.float())
    shp = _shape(c)
    ws_bytes = lib.sg_conv3d_wgrad_workspace(C.byref(shp), _dt(c.dt))
    clean = lib.sg_conv3d_wgrad_clean_bytes(C.byref(shp), _dt(c.dt))
    assert 0 < clean <= ws_bytes
    kept = _garbage(ws_bytes)
    kept[:clean] = 0
    for i in range(2):
        dw, db = _outputs(c)
        rc, names = _launch(c, x, dy, bits, dw, db, 0.25, flags=_lib.SG_WGRAD_CLEAN_WORKSPACE, ws=kept)
        _lib.check(rc, cid)
        assert names == [c.kernel], names
        _check(c, dw, db, 0.25, dw64, db64, f'kept workspace, call {i}')
        assert int(kept[:clean].count_nonzero()) == 0, f'call {i} left the workspace dirty'


def test_kept_workspace_between_a_ragged_layer_and_a_wider_one():
    """40 -> 72 channels (partial 32 x 32 tiles: the kernels add what their staging left in the padding rows) and then 64 -> 96 on the
    same kept buffer, whose tile region covers those padding rows with real channels: both exact, twice over."""
    _lib, lib = _libs()
    first, second = BY_ID['3l_40to72'], Case('3l_64to96', 'conv_wgrad3l', 1, 64, 96, (4, 8, 32))
    sizes = [lib.sg_conv3d_wgrad_workspace(C.byref(_shape(c)), _lib.SG_BF16) for c in (first, second)]
    kept = torch.zeros(max(sizes), dtype=torch.uint8, device=dev())
    for i in range(2):
        for c in (first, second):
            x, dy, bits, dw64, db64 = _case_data(c)
            dw, db = _outputs(c)
            rc, names = _launch(c, x, dy, bits, dw, db, 0.37, flags=_lib.SG_WGRAD_CLEAN_WORKSPACE, ws=kept)
            _lib.check(rc, c.id)
            assert names == [c.kernel], names
            _check(c, dw, db, 0.37, dw64, db64, f'round {i}')
            clean = lib.sg_conv3d_wgrad_clean_bytes(C.byref(_shape(c)), _lib.SG_BF16)
            assert int(kept[:clean].count_nonzero()) == 0


# ----------------------------------------------------------------------------------------------------------------------
# Pointwise column reduction (pw_wgrad_partial + pw_wgrad_final): 1x1x1, cs <= 4 channels on the small side, cb on the big one.
# E = 8 (bf16) | 4 (f32) elements per 16-byte piece, P = cb / E lanes per voxel, rows = 256 / P voxels per block and row group,
# U = 4 row groups per trip; nb = min(1024, cdiv(nvox, rows)) blocks, the final kernel adds nb rows 4 x 8 at a time.
# ----------------------------------------------------------------------------------------------------------------------
PW = [
    # id, dtype, cin, cout, nvox -- the arithmetic of each case
    ('bf16_cs1_P2_nb8', BF, 1, 16, 1000),         # rows = 128, nb = cdiv(1000, 128) = 8; U rows = 512: a live tail of 488 voxels
    ('bf16_cs3_P4_nb25', BF, 3, 32, 1600),        # rows = 64, nb = 25 (24 in the 4-way loop + 1); 1600 = 6 x 256 + 64
    ('bf16_cs4_P64_nb33_to_rgb', BF, 512, 4, 132),  # cout small: bias by the fallback pass; rows = 4, nb = 33 (32 + 1)
    ('bf16_cs2_P256_nb1', BF, 2, 2048, 1),        # rows = 1, a single voxel, nb = 1
    ('bf16_cs2_P256_nb3_to_rgb', BF, 2048, 2, 3),
    ('bf16_cs1_P256_second_trip', BF, 1, 2048, 4101),   # nb = 1024, 1024 x U x rows = 4096 < 4101: five blocks take a second trip
    ('bf16_cs2_P2_second_trip_to_rgb', BF, 16, 2, 1024 * 4 * 128 + 77),   # the same cap at P = 2: 524 365 voxels
    ('f32_cs1_P2_nb8', F32, 1, 8, 1000),
    ('f32_cs3_P4_nb25', F32, 3, 16, 1600),
    ('f32_cs4_P64_nb33_to_rgb', F32, 256, 4, 132),
    ('f32_cs2_P256_second_trip', F32, 2, 1024, 4101),
    ('f32_cs4_P4_nb1024', F32, 4, 16, 64 * 1024 + 5),   # rows = 64: nb = cdiv(65541, 64) = 1025 -> 1024
]


@pytest.mark.parametrize('case', PW, ids=[c[0] for c in PW])
@pytest.mark.parametrize('want_db', [True, False], ids=['db', 'nodb'])
def test_pointwise_column_reduction_is_exact(case, want_db):
    _lib, lib = _libs()
    cid, dt, cin, cout, nvox = case
    c = Case(cid, 'pw_wgrad_partial', 1, cin, cout, (1, 1, nvox), K111, dt=dt, db=want_db)
    x, dy, _, dw64, db64 = _case_data(c)
    coef = 0.25 if PW.index(case) % 2 == 0 else 0.37
    dw, db = _outputs(c)
    rc, names = _launch(c, x, dy, None, dw, db, coef)
    _lib.check(rc, cid)
    assert names == [c.kernel], names
    _check(c, dw, db, coef, dw64, db64)
    # both finalize options are refused on this route with nothing touched
    for flag in (_lib.SG_WGRAD_ACCUMULATE, _lib.SG_WGRAD_CLEAN_WORKSPACE):
        dw, db = _outputs(c)
        rc, names = _launch(c, x, dy, None, dw, db, coef, flags=flag)
        assert rc == _lib.SG_EUNSUPPORTED and names == []
        assert bool((dw == SENTINEL).all()) and (db is None or bool((db == SENTINEL).all()))


PW_BWD = [
    # id, dtype, cin, cout, nvox: the P lanes of a voxel add their parts of dx -- P = 4 by two DPP exchanges, else by wave shuffles,
    # so P <= 64 (more lanes per voxel are refused: test_pointwise_backward_refusals_touch_nothing)
    ('bf16_P4_dpp', BF, 3, 32, 1600), ('bf16_P2', BF, 1, 16, 1000), ('bf16_P16', BF, 2, 128, 333),
    ('bf16_P64_second_trip', BF, 4, 512, 1024 * 4 * 4 + 5),      # rows = 4: 16 384 voxels per round of 1 024 blocks, five more
    ('f32_P4_dpp', F32, 3, 16, 1600), ('f32_P2', F32, 1, 8, 1000), ('f32_P32', F32, 2, 128, 37), ('f32_P64', F32, 4, 256, 132),
]


@pytest.mark.parametrize('case', PW_BWD, ids=[c[0] for c in PW_BWD])
def test_pointwise_backward_dx_dw_db_are_exact(case):
    """sg_conv3d_pw_bwd: dw / db as above and dx[v][j] = sum_c dy[v][c] * w_mat[j][c] from the same read of dy.  w_mat in
    {-1, 0, 1}: the f32 sum is an integer of at most 3 cb, exact; dx is that sum converted once to the tensor's type."""
    _lib, lib = _libs()
    cid, dt, cin, cout, nvox = case
    c = Case(cid, 'pw_wgrad_partial', 1, cin, cout, (1, 1, nvox), K111, dt=dt)
    x, dy, _, dw64, db64 = _case_data(c)
    R.assert_exact_range(3, 1, cout)
    wm = R.int_data((cin, cout), 77, F32, -1, 1)
    exact = dy.cpu().double().permute(0, 2, 3, 4, 1).reshape(nvox, cout) @ wm.double().t()
    shp = _shape(c)
    ws = _garbage(lib.sg_conv3d_wgrad_workspace(C.byref(shp), _dt(dt)))
    dw, db = _outputs(c)
    dx = torch.full((nvox, cin), SENTINEL, dtype=dt, device=dev())
    wmd = wm.to(dev())
    lib.sg_prof_enable(1)
    try:
        rc = lib.sg_conv3d_pw_bwd(x.data_ptr(), dy.data_ptr(), wmd.data_ptr(), dw.data_ptr(), db.data_ptr(), dx.data_ptr(), 0.37,
                                  ws.data_ptr(), ws.numel(), C.byref(shp), _dt(dt), _stream())
        torch.cuda.synchronize()
        names = _wgrad_kernels(_lib, lib)
    finally:
        lib.sg_prof_enable(0)
    _lib.check(rc, cid)
    assert names == [c.kernel], names
    _check(c, dw, db, 0.37, dw64, db64)
    assert torch.equal(dx.cpu(), exact.to(dt)), 'dx'


@pytest.mark.parametrize('case', [('cin_above_4', 8, 16, K111, False), ('cin_above_cout', 4, 2, K111, False), ('taps', 2, 16, K133, False),
                                  ('upsampled', 2, 16, K111, True), ('pieces_do_not_divide_256', 2, 24, K111, False),
                                  ('128_lanes_per_voxel', 2, 1024, K111, False), ('256_lanes_per_voxel', 2, 2048, K111, False)],
                         ids=lambda c: c[0])
def test_pointwise_backward_refusals_touch_nothing(case):
    """The last two: a voxel's 128 / 256 lanes span two / four waves, where the shuffle sum of dx cannot reach."""
    _lib, lib = _libs()
    _, cin, cout, k, ups = case
    sp = (2, 4, 8)
    shp = _lib.ConvShape(1, *sp, cin, cout, *k, 1 if ups else 0)
    x = R.int_data((1, cin, *(tuple(v // 2 for v in sp) if ups else sp)), 1, BF).to(dev())
    dy = R.int_data((1, cout, *sp), 2, BF).to(dev())
    wm = torch.ones((cin, cout), device=dev())
    ws = _garbage(max(lib.sg_conv3d_wgrad_workspace(C.byref(shp), _lib.SG_BF16), 1 << 16))
    dw = torch.full((*k, cin, cout), SENTINEL, device=dev())
    db = torch.full((cout,), SENTINEL, device=dev())
    dx = torch.full((64, cin), SENTINEL, dtype=BF, device=dev())
    rc = lib.sg_conv3d_pw_bwd(x.data_ptr(), dy.data_ptr(), wm.data_ptr(), dw.data_ptr(), db.data_ptr(), dx.data_ptr(), 0.5, ws.data_ptr(),
                              ws.numel(), C.byref(shp), _lib.SG_BF16, _stream())
    torch.cuda.synchronize()
    assert rc == _lib.SG_EUNSUPPORTED
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all()) and bool((dx == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------------------------
# Small-channel VALU kernel (conv_small_wgrad): 1x3x3 at D = 1, channels in {4, 8, 16}, from n h w >= 65 536 voxels.
# 505 x 130 = 65 650: W = 130 is three 64-wide segments, the last 2 wide; H = 505 is odd, no multiple of any strip height.
# ----------------------------------------------------------------------------------------------------------------------
SMALL = [(ci, co) for ci, co in ((4, 4), (4, 8), (4, 16), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16))]


@pytest.mark.parametrize('dtype', [BF, F32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('chan', SMALL, ids=[f'{a}to{b}' for a, b in SMALL])
def test_small_channel_kernel_is_exact(chan, dtype):
    _lib, lib = _libs()
    cin, cout = chan
    want_db = SMALL.index(chan) % 2 == 0
    t = 'bf16' if dtype == BF else 'f32'
    c = Case(f'small_{cin}to{cout}', f'conv_small_wgrad<{t}>', 1, cin, cout, (1, 505, 130), K133, dt=dtype, db=want_db)
    x, dy, _, dw64, db64 = _case_data(c)
    coef = 0.37 if want_db else 0.25
    dw, db = _outputs(c)
    rc, names = _launch(c, x, dy, None, dw, db, coef)
    _lib.check(rc, c.id)
    assert names == [c.kernel], names
    _check(c, dw, db, coef, dw64, db64)
    if chan in ((4, 8), (16, 16)):      # the finalize options are refused here too, nothing touched
        for flag in (_lib.SG_WGRAD_ACCUMULATE, _lib.SG_WGRAD_CLEAN_WORKSPACE):
            dw, db = _outputs(c)
            rc, names = _launch(c, x, dy, None, dw, db, coef, flags=flag)
            assert rc == _lib.SG_EUNSUPPORTED and names == []
            assert bool((dw == SENTINEL).all()) and (db is None or bool((db == SENTINEL).all()))


@pytest.mark.parametrize('dtype', [BF, F32], ids=['bf16', 'f32'])
@pytest.mark.parametrize('chan', [(4, 8), (16, 16)], ids=['4to8', '16to16'])
def test_one_row_below_the_small_channel_threshold_takes_an_mfma_route(chan, dtype):
    """504 x 130 = 65 520 < 65 536: the same layer one voxel row shorter is the generic MFMA kernel's (272 tiles of 32 x 8)."""
    _lib, lib = _libs()
    cin, cout = chan
    c = Case(f'below_small_{cin}to{cout}', 'conv_wgrad<bf16,256>' if dtype == BF else 'conv_wgrad<f32,128>', 1, cin, cout, (1, 504, 130),
             K133, dt=dtype)
    x, dy, _, dw64, db64 = _case_data(c)
    dw, db = _outputs(c)
    rc, names = _launch(c, x, dy, None, dw, db, 0.37)
    _lib.check(rc, c.id)
    assert names == [c.kernel], names
    _check(c, dw, db, 0.37, dw64, db64)


# ----------------------------------------------------------------------------------------------------------------------
# Sub-pixel weight gradient (upconv_subpixel_wgrad, through sg_upconv3d_subpixel_wgrad): tiles of 2 x 32 low-resolution voxels,
# ntiles = n d (h / 2) (w / 32), gx = max(8, 256 / pairs) blocks per pair; reproducible mode: gx slabs
# ----------------------------------------------------------------------------------------------------------------------
SUBPIX = [
    # id, n, cin, cout, low (d, h, w), bias
    ('one_tile_per_sample', 3, 32, 32, (1, 2, 32), True),           # 3 tiles on gx = 256 blocks: 253 blocks send nothing
    ('several_tiles_per_block_odd_D', 1, 64, 32, (3, 86, 32), False),   # pairs = 2, gx = 128; 3 x 43 = 129 tiles: block 0 takes two
    ('128to64', 1, 128, 64, (1, 4, 32), True),                      # pairs = 8, gx = 32, 2 tiles
    ('two_W_tiles_odd_D', 2, 32, 64, (3, 2, 64), True),             # w / 32 = 2
]


@pytest.mark.parametrize('slabs', [False, True], ids=['atomics', 'slabs'])
@pytest.mark.parametrize('case', SUBPIX, ids=[c[0] for c in SUBPIX])
def test_subpixel_weight_gradient_is_exact(case, slabs):
    import saragan_amd
    _lib, lib = _libs()
    cid, n, cin, cout, low, want_db = case
    fine = tuple(2 * v for v in low)
    c = Case(cid, 'upconv_subpixel_wgrad', n, cin, cout, fine, ups=True, db=want_db)
    x, dy, _, dw64, db64 = _case_data(c)
    coef = 0.25 if SUBPIX.index(case) % 2 == 0 else 0.37
    shp = _lib.ConvShape(n, *low, cin, cout, 3, 3, 3, 0)
    assert lib.sg_upconv3d_subpixel_wgrad_supported(C.byref(shp), _lib.SG_BF16)
    if slabs:
        saragan_amd.set_deterministic(True)
    try:
        ws = _garbage(lib.sg_upconv3d_subpixel_wgrad_workspace(C.byref(shp), _lib.SG_BF16))
        dw, db = _outputs(c)
        lib.sg_prof_enable(1)
        try:
            rc = lib.sg_upconv3d_subpixel_wgrad(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr() if want_db else None, coef,
                                                ws.data_ptr(), ws.numel(), C.byref(shp), _lib.SG_BF16, _stream())
            torch.cuda.synchronize()
            names = _wgrad_kernels(_lib, lib)
        finally:
            lib.sg_prof_enable(0)
    finally:
        if slabs:
            saragan_amd.set_deterministic(False)
    _lib.check(rc, cid)
    assert names == [c.kernel], names
    _check(c, dw, db, coef, dw64, db64)


# ----------------------------------------------------------------------------------------------------------------------
# Refusals: dw and db keep their sentinel
# ----------------------------------------------------------------------------------------------------------------------
def _offset(t, nbytes):
    """The same values in a buffer whose base address is `nbytes` past a 16-byte boundary."""
    raw = torch.zeros(t.numel() * t.element_size() + 32, dtype=torch.uint8, device=t.device)
    view = raw[nbytes:nbytes + t.numel() * t.element_size()].view(t.dtype)
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == nbytes % 16
    return view


@pytest.mark.parametrize('what', ['x', 'dy', 'workspace', 'mask', 'short_workspace', 'mask_on_16_wide', 'mask_on_odd_cout', 'mask_gain_not_pow2',
                                  'mask_on_f32', 'mask_on_single_D_tile'])
def test_refusals_touch_nothing(what):
    _lib, lib = _libs()
    SG_EWORKSPACE, SG_EALIGN = -2, -3
    n, cin, cout, sp, dt, gain = 1, 32, 32, (4, 8, 32), BF, 0.125
    masked = what.startswith('mask')
    if what == 'mask_on_16_wide':
        sp = (4, 8, 16)
    elif what == 'mask_on_odd_cout':
        cout = 40
    elif what == 'mask_gain_not_pow2':
        gain = 0.3
    elif what == 'mask_on_f32':
        dt = F32
    elif what == 'mask_on_single_D_tile':
        sp = (2, 8, 32)
    half = tuple(v // 2 for v in sp)
    x = R.int_data((n, cin, *sp), 1, dt).to(dev())
    dy = R.int_data((n, cout, *(half if masked else sp)), 2, dt).to(dev())
    bits = torch.zeros((n * sp[0] * sp[1] * sp[2], (cout + 31) // 32), dtype=torch.int32, device=dev()) if masked else None
    shp = _lib.ConvShape(n, *sp, cin, cout, 3, 3, 3, 0)
    ws_bytes = lib.sg_conv3d_wgrad_workspace(C.byref(shp), _dt(dt))
    ws = _garbage(ws_bytes + 32)
    wsp, wsn = ws.data_ptr(), ws_bytes
    want = _lib.SG_EUNSUPPORTED
    if what == 'x':
        x, want = _offset(x, 2), SG_EALIGN
    elif what == 'dy':
        dy, want = _offset(dy, 8), SG_EALIGN
    elif what == 'workspace':
        wsp, want = wsp + 4, SG_EALIGN
    elif what == 'mask':
        bits, want = _offset(bits, 4), SG_EALIGN
    elif what == 'short_workspace':
        wsn, want = ws_bytes - 1, SG_EWORKSPACE
    dw = torch.full((3, 3, 3, cin, cout), SENTINEL, device=dev())
    db = torch.full((cout,), SENTINEL, device=dev())
    before = ws.clone()
    if masked:
        rc = lib.sg_conv3d_wgrad_bias_up_masked(x.data_ptr(), dy.data_ptr(), bits.data_ptr(), 0.25, gain, dw.data_ptr(), db.data_ptr(), 0.25,
                                                wsp, wsn, C.byref(shp), _dt(dt), _stream())
    else:
        rc = lib.sg_conv3d_wgrad_bias(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), db.data_ptr(), 0.25, wsp, wsn, C.byref(shp), _dt(dt),
                                      _stream())
    torch.cuda.synchronize()
    assert rc == want, (what, rc)
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())
    if what not in ('mask_on_single_D_tile', 'mask_on_16_wide'):   # (those two are refused once the sliding-halo launcher has declined
        assert torch.equal(ws, before)                             #  the tile: the workspace, scratch, was cleared by then)
