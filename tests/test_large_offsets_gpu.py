"""The forward / data-gradient routes of sg_conv3d_fwd on tensors past 2 GiB and 4 GiB: the dispatch dimension the exact suites do
not reach, how far an address lies from the tensor's base.

Inputs are those of tests/test_conv_fwd_exact_gpu.py (integers in [-3, 3], power-of-two coef, integer bias, slope 0.25: every f32
sum is exact and the comparison is torch.equal), generated on the device.  Random content makes an aliased read visible: a read
displaced by 2^31 or 2^32 bytes sees other values; a buffer offset at or past 2^31 reads zeros and drops the store, which leaves the
sentinel y is pre-filled with.  Each case is checked twice:
  * on the boxes of tests/bigref.py (first and last voxel, both sides of every boundary every tensor reaches, first and last voxel of
    the rebased sample group at each boundary; check_cover() verifies that on the host BEFORE the launch) against the fp64
    reference computed on the host from the box plus halo of x;
  * as a whole, on the device, against the same entry point called on pieces below 2^30 bytes (sub-batches; D slabs with a halo
    for the single-sample cases, the halo planes of the output dropped), which run at offsets the exact suites pin.
Every case asserts the kernel that ran by name.  Each test computes the device memory it needs, skips only if the device has
less, and frees everything before it returns.

BATCH: samples small, the batch past 2^32 bytes (f32: 2^33, element offset 2^31): n is the smallest value at which the last
sample of x and the last sample of y both start at or past that byte (bigref.smallest_batch).
GUARD: one sample on both sides of a launcher's host guard: the largest D below it (the guarded kernel must still run, its offsets
within 16 MiB of 2^31) and the smallest above (it must not; the route that takes over is named and must be exact).

case                 kernel                         address expression whose width matters           guard                 shape (n computed), boundary       fallback
3w_plain             conv_fwd3w<bf16,32->32>        conv3w.hip:217 base + n0 * sample_bytes (64 bit) rebased per sample    32->64 (5,20,64), batch past 2^32
3w_bias_act_sign     conv_fwd3w<bf16,32->32>        same; sign words: wsb = svox ntile 4 (:220)      rebased per sample    32->64 (5,20,64), batch past 2^32
3w_pool1             conv_fwd3w<bf16,32->32>        same; pooled y rebased by its own sample bytes   rebased per sample    32->64 (6,20,64), pooled y past 2^32
3w_dgrad_mask        conv_fwd3w<bf16,32->32>        same; mask words rebased by wsb                  rebased per sample    32->64 (5,20,64), batch past 2^32
3s2                  conv_fwd3s<bf16,2>             conv3d.hip:1221 base + n0 * sample_bytes         rebased per sample    24->32 (4,32,256), batch past 2^32
3p16                 conv_fwd3p16<bf16,64->32>      conv3p.hip:519 base + n0 * sample_bytes          rebased per sample    64->32 (4,32,64), y past 2^32
3p                   conv_fwd3p<bf16,64->32>        conv3p.hip:183 base + n0 * sample_bytes          rebased per sample    64->32 (4,32,64), y past 2^32
x2                   conv_fwd3s<bf16,2> x2 (K split) conv3d.hip:1221; f32 partials ysb = svox cout 4  rebased per sample    64->32 (4,32,256), y past 2^32
3r_lean              conv_fwd3r<bf16,2,2,3,3,3>     conv3d.hip:866 base + (int64) n0 * sample_bytes, rebased per TN        32->32 (16,64,40), batch past 2^32
                                                    :879 32-bit lane offset it_rel * es + tile_off   samples (TN = 1)
5                    conv_fwd5<bf16,2,2,3,3,3>      conv3d.hip:2317 base + n0 * sample_bytes         rebased per sample    48->64 (16,64,64), batch past 2^32
4                    conv_fwd4<bf16,2,1,3,3,3>      conv3d.hip:1927 base + (int64) n0 * sample_bytes rebased per TN        48->32 (5,30,64), batch past 2^32
2                    conv_fwd2<bf16,2,1,2>          conv3d.hip:453 (int64) voxel index * cin          one 64-bit address    24->32 (4,32,32), batch past 2^32
1                    conv_fwd<bf16,2,1>             common.h:375 (int64) voxel index * cin            one 64-bit address    6->10 (3,5,7), batch past 2^32
small                conv_small_fwd<bf16>           small.hip:78 base + off, rebased per sample       rebased per sample    16->8 (1,256,256) 1x3x3, y past 2^32
pw_cin               pw_fwd_small_cin<bf16>         conv3d.hip:2668 int64 voxel index v               one 64-bit address    4->8 (4,40,64) 1x1x1, batch past 2^32
pw_cout              pw_fwd_small_cout<bf16>        conv3d.hip:2734 int64 voxel index vb              one 64-bit address    8->4 (4,40,64) 1x1x1, y past 2^32
3r_f32               conv_fwd3r<f32,2,2,3,3,3>      as 3r_lean                                       rebased per TN        16->32 (16,64,64) f32, x past 2^33
2_f32                conv_fwd2<f32,2,1,2>           as 2                                             one 64-bit address    32->32 (4,32,32) f32, x past 2^33
pw_cin_f32           pw_fwd_small_cin<f32>          as pw_cin                                        one 64-bit address    4->4 (4,40,64) f32, x past 2^33
gemm_last            conv_gemm                      gemm.hip:105 int xoff = voxel * cin               gemm.hip:279          128->128 (2,8,8) 1x3x3, n = 131071: x ends 16384 elements below element 2^31
gemm_declines        (declined)                     n d h w cin = 2^31 exactly                        gemm.hip:279          n = 131072                        conv_fwd4<bf16,2,1,1,3,3>
3w_below / _above    conv_fwd3w<bf16,32->32>        conv3w.hip:220 (int) xsb, ysb as resource size    conv3w.hip:902: x and y bytes trip together at cout 32       32->32 (127 | 128,512,512)   conv_fwd3r<bf16,2,2,3,3,3>
                     (non-lean staging; conv_fwd3s declines at conv3d.hip:1714 too)
x2_below / _above    conv_fwd3s<bf16,2> x2 (K split) conv3d.hip:1224 xsb = svox 64 2, ysb = svox 32 4  conv3d.hip:1714: the xcs term and the f32-partials term     64->32 (127 | 128,512,256)   conv_fwd2<bf16,2,1,2>
                     trip together in the K split (in a plain conv_fwd3s call xcs <= 32 and the partials term counts cout 4 where y holds cout 2 bytes: the guard
                     declines before any tensor of the call comes near 2^31, so that pair would cross no boundary; the K split's workspace really holds cout 4);
                     conv_fwd4 declines at conv3d.hip:2160 too
3p_below / _above    conv_fwd3p16<bf16,64->32>      conv3p.hip:522 xsb = svox 64 2                   conv3p.hip:898: the x term                                   64->32 (127 | 128,512,256)   conv_fwd2<bf16,2,1,2>
                     (the K split declines at conv3d.hip:1714, conv_fwd4 at :2160)
5_below / _above     conv_fwd5<bf16,2,2,3,3,3>      conv3d.hip:2315 ysb = svox cout 2                conv3d.hip:2586: the y term                                  48->64 (127 | 128,512,256)   conv_fwd4<bf16,2,2,3,3,3>
4_below / _above     conv_fwd4<bf16,2,1,3,3,3>      conv3d.hip:1931 (int) tile_off                   conv3d.hip:2160                                              48->32 (170 | 171,512,256)   conv_fwd2<bf16,2,1,2>
3r_below / _above    conv_fwd3r<bf16,2,2,3,3,3>     conv3d.hip:879 (lean) | :897 int64 (non-lean)    conv3d.hip:1052                                              32->32 (126 | 127,512,520)   the same kernel, its second staging path
3r_f32_below/_above  conv_fwd3r<f32,2,2,3,3,3>      as above                                         conv3d.hip:1052                                              16->32 (127 | 128,512,512)   the same kernel, its second staging path
small_below/_above   conv_small_fwd<f32>            small.hip:107 (int) simg CIN ES as resource size  small.hip:352 (h w 16 4 < 2^31)                              16->8 f32 (1,65535 | 65536,512) 1x3x3  conv_fwd3r<f32,2,2,1,3,3> (non-lean)
                     (f32: in bf16 the guard trips at a sample of 1 GiB and the pair would cross no boundary.  small.hip:437, the weight gradient's
                     guard, trips at 1 GiB too: its pair is a batch of five images, w_small_below / w_small_above in the weight-gradient table.)
(conv_fwd3r's two staging paths share a kernel name: the route is asserted, the path follows from a.lean at conv3d.hip:1052.)

Weight gradients (sg_conv3d_wgrad_bias; test_weight_gradient_is_exact_past_the_boundary): x dense, dy zero except on the boxes.
case               kernel                 address expression whose width matters                   guard                      shape, boundary                        fallback
w_generic          conv_wgrad<bf16,256>   common.h:375 (int64) voxel index * c                      one 64-bit address         6->10 (3,5,7), batch past 2^32
w_2                conv_wgrad2<3,3,3>     wgrad.hip:531-533 int64 tile base + int relx / rely       rebased per TN (= 1)       128->128 (2,128,32), batch past 2^32
w_3                conv_wgrad3<3,3,3>     wgrad.hip:911, :939 int64 tile bases                      rebased per TN (= 1)       32->32 (4,8,40), batch past 2^32
w_3l               conv_wgrad3l           wgrad.hip:1494 base + n0 * xsb, (int) xsb as the size    rebased per sample         32->32 (4,8,32), batch past 2^32
w_pw               pw_wgrad_partial       wgrad.hip:264 big + v * cb, int64 v                       one 64-bit address         4->8 (4,40,64) 1x1x1, batch past 2^32
w_small            conv_small_wgrad<bf16> small.hip:235 base + n simg c es, rebased per sample      rebased per sample         16->8 (1,256,256) 1x3x3, dy past 2^32
w_planes_below     conv_wgrad_planes<8>   wgrad.hip:1859 (int) ntiles 128 c 2: ONE resource         wgrad.hip:1963             32->32 (2,8,8) 1x3x3, n = 262143: 8 KiB below 2^31
w_planes_above     (declined)             the same                                                  wgrad.hip:1963             n = 262144: exactly 2^31 bytes         conv_wgrad<bf16,256>
w_2_below          conv_wgrad2<1,3,3>     wgrad.hip:511 int relx (elements)                         wgrad.hip:699 (elements)   128->128 (127,512,256) 1x3x3, 2^24 elements below 2^31
w_2_above          (declined)             the same                                                  wgrad.hip:699              (128,512,256): 2^31 elements           conv_wgrad<bf16,256>
w_3_below          conv_wgrad3<3,3,3>     wgrad.hip:911 int64 base + int element offsets            wgrad.hip:1741 (elements)  32->32 (252,512,520), 2^19 elements below 2^31
w_3_above          (declined)             the same                                                  wgrad.hip:1741             (253,512,520)                          conv_wgrad<bf16,256>
w_3l_below         conv_wgrad3l           wgrad.hip:1494 (int) xsb, DEAD = 2^31                     wgrad.hip:1769 `fits`      32->32 (127,512,512): 16 MiB below 2^31 bytes
w_3l_above         (declined)             the same                                                  wgrad.hip:1769 (BYTES)     (128,512,512): exactly 2^31 bytes      conv_wgrad3<3,3,3>
w_small_below      conv_small_wgrad<bf16> small.hip:235 (int) simg CINT ES as the resource size     small.hip:437 (h w 32 4)   16->8 five images (1,32767,512) 1x3x3: x past 2^31
w_small_above      (declined)             the same                                                  small.hip:437              five images (1,32768,512)              conv_wgrad2<1,3,3>
w_sub              upconv_subpixel_wgrad  subpix.hip:1062 / :1071 int64 off for x and gy            subpix.hip:1200 is 2^40    128->64 low (1,4,32), x and gy past 2^32
                   (test_subpixel_weight_gradient_is_exact_past_the_boundary)                       elements: unreachable

Sub-pixel up-convolution (subpix.hip; s the LOW-resolution shape, boxes on the low-resolution grid, y / gy on the fine one).
case               kernel                                  address expression whose width matters                 guard               shape, boundary                          fallback
sub_fwd            upconv_subpixel_fwd                     subpix.hip:265 a.x + n0 * xsb, :362 int64 ov           rebased per sample  64->32 low (4,16,16), x and y past 2^32
sub_dgrad          upconv_subpixel_dgrad                   subpix.hip:748 a.gy + n0 * ysb, :880 int64 ov          rebased per sample  64->32 low (4,16,16), gy and gx past 2^32
sub_below          upconv_subpixel_fwd                     subpix.hip:247 (int) xsb as the resource size          subpix.hip:661      64->32 low (128,508,256): x 16 MiB below 2^31
sub_above          upconv_subpixel_fwd<one tile per block> subpix.hip:107 int xoff on a 64-bit sample base        subpix.hip:661      low (128,512,256): x exactly 2^31 bytes; reached by size, no debug flag
sub_638_below      upconv_subpixel_fwd<one tile per block> subpix.hip:107 int xoff within one plane of 2^31       subpix.hip:638      low (254,512,256): x 2^24 elements below 2^31 elements
sub_refused        (SG_EUNSUPPORTED)                       the same                                               subpix.hip:638      low (128,512,512): 2^31 elements         conv_fwd2<bf16,2,1,2> through functional.raw_conv
                   (test_subpixel_refusal_and_what_functional_runs_in_its_place)
subdg_below        upconv_subpixel_dgrad                   subpix.hip:734 (int) ysb as the resource size          subpix.hip:936      64->32 low (254,256,64): gy 16 MiB below 2^31
subdg_above        (SG_EUNSUPPORTED)                       the same                                               subpix.hip:936      low (256,256,64): gy exactly 2^31 bytes  conv_fwd3r<bf16,2,2,3,3,3> + sg_downscale_sum
                   its fallback writes and reads back the full-resolution gradient, 64 channels on the fine grid, exactly 2^32 bytes (conv3d.hip:1002 int64 yrow;
                   elementwise.hip:594 int64 vox): a Layout of its own, boxes on both sides of its byte 2^31 (low plane 128); whole gx against D slabs
                   (test_subpixel_dgrad_refusal_and_what_functional_runs_in_its_place)                                                                                         through functional._upconv_dgrad

Elementwise and reduction kernels of the step through saragan_amd.functional (elementwise.hip): 1025 samples of 16 x 64 x 64 x 32
channels, bf16 just past 2^32 bytes (element 2^31 inside the last sample), f32 just past 2^33.  All index with int64; none has a guard.
case (test[id])                                     kernel                         address expression                              tensor past the boundary
bias_act_forward[bf16] / [f32]                      bias_act_fwd_kernel<VEC>       :74 int64 total = nvox P, x + i E                x and y, bf16 2^32 / f32 2^33
bias_act_backward[bf16-y] / [bf16-bits] / [f32-y]   bias_act_bwd_vec_kernel        :114 int64 off = v c + p E, :123 words by v      dy, y | sign words, dx; dbias from a sparse dy
pixel_norm_forward[bf16] / [f32]                    pixel_norm_kernel              :313 a + v c + p E, int64 v                      x and y
pixel_norm_backward                                 pixel_norm_kernel<BWD>         :313-315 a + v c, yv + v c; scale_in[v]          gy, y, dx; 2^26 + scales
sign_words_and_cast                                 sign_words_kernel, cast_kernel :213 int64 v = i / nw; int64 numel               x bf16; the f32 copy past 2^33
nearest_scaling[upscale2x-plain] / [-masked]        upscale2x_rows_kernel          :526-528 int64 row bases, mrow = mask + row OW nw y (and its sign words)
nearest_scaling[downscale2x-plain] / [-masked]      downscale2x_kernel             :594-597 int64 vox, bits[vox nw]                 x (and its sign words)
trilinear[up] / [adjoint]                           trilinear_up2x(_adj)_kernel    :656 / :712 int64 src, y + i E                   y | g
lerp                                                axpby_kernel                   :747 a + i E, int64 i                            a, b, out
interpolate_rows                                    lerp_rows_kernel               :774 gamma[i / pv], a + i E                      a, b, out
sumsq_keep_w[atomic] / [ordered]                    sumsq_keep_w(_ordered)_kernel  :829 / :852 ((int64) nn dh + rr) w + ww) c       g
add_noise_windows                                   add_noise_kernel               :797 ctr = gi + offset, :813 int64 i             2^32 + 2^20 elements; the counter's low word
                                                                                                                                    carries at element 2^32"""
import ctypes as C

import pytest
import torch

from tests import bigref as B
from tests import fwdref as R
from tests import wgref as W
from tests.test_conv_fwd_exact_gpu import BF, F32, K111, K133, K333, NOP, SENTINEL, Case, _assert_equal, _launch, _libs, dev

pytestmark = pytest.mark.gpu

PIECE = 2 ** 30      # the pieces of the whole-tensor comparison stay below this many bytes per tensor


def route_seam(c):
    """The D and H periods a box of case c must straddle: bigref.SEAM, widened where the tile of the kernel the case names is larger
    (the generic weight-gradient kernel's 8 x 4 x 8 tiles, the small-channel kernels' 64-row strips)."""
    td, th = B.kernel_tile(c.kernel, c.sp, c.k)
    return max(B.SEAM[0], td), max(B.SEAM[1], th)


class Big:
    """A Case of the exact suite at a size past a boundary.  n = None: the smallest batch whose last samples of x and y start at
    or past byte `past`.  group: samples per rebased buffer resource (None: plain 64-bit addresses).  slabs: compare against D slabs
    (single-sample cases) instead of sub-batches."""

    def __init__(self, case, past=B.B32, group=1, slabs=False, seam=None):
        self.c, self.group, self.slabs, self.seam = case, group, slabs, seam or route_seam(case)
        c = case
        self.es = 2 if c.dt == BF else 4
        if c.n is None:
            c.n = B.smallest_batch(self.x_layout(1).nbytes(), self.y_layout(1).nbytes(), past=past)
        self.id = c.id

    def x_layout(self, n=None):
        c = self.c
        return B.Layout('x', n or c.n, c.sp, c.cin, self.es, group=self.group)

    def y_layout(self, n=None):
        c = self.c
        f = R.POOL_BLOCK.get(c.pool, (1, 1, 1))
        return B.Layout('y', n or c.n, c.out_sp(), c.cout, self.es, pool=f, group=self.group)

    def layouts(self):
        c = self.c
        out = [self.x_layout(), self.y_layout()]
        nw = (c.cout + 31) // 32
        if c.sign:
            out.append(B.Layout('sign words', c.n, c.sp, nw, 4, group=self.group))
        if c.mask:
            out.append(B.Layout('mask words', c.n, c.sp, nw, 4, group=self.group))
        return out

    def align(self):
        f = R.POOL_BLOCK.get(self.c.pool, (1, 1, 1))
        return f[0], f[1]

    def boxes(self):
        return B.choose_boxes(self.layouts(), self.c.sp, seam=self.seam, align=self.align())

    def device_bytes(self):
        """x, y and the piecewise y, sign and mask words twice, one piece of everything; the test adds what the library reports for
        the call's workspace and packed weights (_fwd_extra), for the large call and for one piece."""
        c = self.c
        nvox = c.n * c.sp[0] * c.sp[1] * c.sp[2]
        words = nvox * ((c.cout + 31) // 32) * 4
        return self.x_layout().nbytes() + 2 * self.y_layout().nbytes() + 3 * words + 5 * PIECE + 2 ** 28


def _b(cid, kernel, cin, cout, sp, n=None, past=B.B32, group=1, slabs=False, seam=None, **kw):
    return Big(Case(cid, kernel, n, cin, cout, sp, **kw), past=past, group=group, slabs=slabs, seam=seam)


NO3P = {'SG_FWD_NO_3P': 1}
BATCH = [
    _b('3w_plain', 'conv_fwd3w<bf16,32->32>', 32, 64, (5, 20, 64)),
    _b('3w_bias_act_sign', 'conv_fwd3w<bf16,32->32>', 32, 64, (5, 20, 64), bias=True, act=True, sign=True),
    _b('3w_pool1', 'conv_fwd3w<bf16,32->32>', 32, 64, (6, 20, 64), bias=True, act=True, pool=1),
    _b('3w_dgrad_mask', 'conv_fwd3w<bf16,32->32>', 32, 64, (5, 20, 64), flip=True, mask=True),
    _b('3s2', 'conv_fwd3s<bf16,2>', 24, 32, (4, 32, 256)),
    _b('3p16', 'conv_fwd3p16<bf16,64->32>', 64, 32, (4, 32, 64)),
    _b('3p', 'conv_fwd3p<bf16,64->32>', 64, 32, (4, 32, 64), env={'SG_FWD3P_16': 0}),
    _b('x2', 'conv_fwd3s<bf16,2> x2 (K split)', 64, 32, (4, 32, 256), env=NO3P),
    _b('3r_lean', 'conv_fwd3r<bf16,2,2,3,3,3>', 32, 32, (16, 64, 40)),
    _b('5', 'conv_fwd5<bf16,2,2,3,3,3>', 48, 64, (16, 64, 64)),
    _b('4', 'conv_fwd4<bf16,2,1,3,3,3>', 48, 32, (5, 30, 64), bias=True, act=True, sign=True),
    _b('2', 'conv_fwd2<bf16,2,1,2>', 24, 32, (4, 32, 32), env=NOP, group=None),
    _b('1', 'conv_fwd<bf16,2,1>', 6, 10, (3, 5, 7), bias=True, act=True, sign=True, group=None),
    _b('small', 'conv_small_fwd<bf16>', 16, 8, (1, 256, 256), k=K133, bias=True, act=True, sign=True),
    _b('pw_cin', 'pw_fwd_small_cin<bf16>', 4, 8, (4, 40, 64), k=K111, bias=True, act=True, sign=True, group=None),
    _b('pw_cout', 'pw_fwd_small_cout<bf16>', 8, 4, (4, 40, 64), k=K111, bias=True, group=None),
    # f32: x past 2^33 bytes, which is element offset 2^31
    _b('3r_f32', 'conv_fwd3r<f32,2,2,3,3,3>', 16, 32, (16, 64, 64), dt=F32, past=B.B33),
    _b('2_f32', 'conv_fwd2<f32,2,1,2>', 32, 32, (4, 32, 32), dt=F32, env=NOP, past=B.B33, group=None),
    _b('pw_cin_f32', 'pw_fwd_small_cin<f32>', 4, 4, (4, 40, 64), k=K111, dt=F32, bias=True, past=B.B33, group=None),
    # gemm.hip:279 declines from n d h w cin = 2^31: 131072 samples of 2 x 8 x 8 x 128; one fewer still runs it
    _b('gemm_last', 'conv_gemm', 128, 128, (2, 8, 8), n=131071, k=K133, group=None),
    _b('gemm_declines', 'conv_fwd4<bf16,2,1,1,3,3>', 128, 128, (2, 8, 8), n=131072, k=K133, group=None),
]

GUARD = [
    _b('3w_below', 'conv_fwd3w<bf16,32->32>', 32, 32, (127, 512, 512), n=1, slabs=True),
    _b('3w_above', 'conv_fwd3r<bf16,2,2,3,3,3>', 32, 32, (128, 512, 512), n=1, slabs=True),
    _b('x2_below', 'conv_fwd3s<bf16,2> x2 (K split)', 64, 32, (127, 512, 256), n=1, slabs=True, env=NO3P),
    _b('x2_above', 'conv_fwd2<bf16,2,1,2>', 64, 32, (128, 512, 256), n=1, slabs=True, env=NO3P),
    _b('3p_below', 'conv_fwd3p16<bf16,64->32>', 64, 32, (127, 512, 256), n=1, slabs=True),
    _b('3p_above', 'conv_fwd2<bf16,2,1,2>', 64, 32, (128, 512, 256), n=1, slabs=True),
    _b('5_below', 'conv_fwd5<bf16,2,2,3,3,3>', 48, 64, (127, 512, 256), n=1, slabs=True),
    _b('5_above', 'conv_fwd4<bf16,2,2,3,3,3>', 48, 64, (128, 512, 256), n=1, slabs=True),
    _b('4_below', 'conv_fwd4<bf16,2,1,3,3,3>', 48, 32, (170, 512, 256), n=1, slabs=True),
    _b('4_above', 'conv_fwd2<bf16,2,1,2>', 48, 32, (171, 512, 256), n=1, slabs=True),
    _b('3r_below', 'conv_fwd3r<bf16,2,2,3,3,3>', 32, 32, (126, 512, 520), n=1, slabs=True),
    _b('3r_above', 'conv_fwd3r<bf16,2,2,3,3,3>', 32, 32, (127, 512, 520), n=1, slabs=True),
    _b('3r_f32_below', 'conv_fwd3r<f32,2,2,3,3,3>', 16, 32, (127, 512, 512), n=1, dt=F32, slabs=True),
    _b('3r_f32_above', 'conv_fwd3r<f32,2,2,3,3,3>', 16, 32, (128, 512, 512), n=1, dt=F32, slabs=True),
    # small.hip:352: a 2-D image of 16 channels with h w just below and at 2^25: h w 16 4 bytes against 2^31, so in f32 (in bf16 the
    # same guard trips at 1 GiB and no tensor comes near a boundary)
    _b('small_below', 'conv_small_fwd<f32>', 16, 8, (1, 65535, 512), n=1, k=K133, dt=F32, slabs='h', bias=True, act=True, sign=True),
    _b('small_above', 'conv_fwd3r<f32,2,2,1,3,3>', 16, 8, (1, 65536, 512), n=1, k=K133, dt=F32, slabs='h', bias=True, act=True, sign=True),
]

CASES = BATCH + GUARD
assert len({b.id for b in CASES}) == len(CASES)


def _fwd_extra(c):
    """Bytes of the workspace _launch hands the call and of its packed weights, as the library reports them."""
    from tests.test_conv_fwd_exact_gpu import _dt, _shape
    _, lib = _libs()
    shp = _shape(c)
    return lib.sg_conv3d_fwd_workspace(C.byref(shp), _dt(c.dt)) + lib.sg_conv3d_packed_bytes(C.byref(shp), _dt(c.dt))


def _fill_ints(t, seed):
    """Integers in [-3, 3] into the contiguous tensor t, drawn on the device as int8 in slices of 2^28 elements."""
    g = torch.Generator(device=t.device).manual_seed(seed)
    flat = t.view(-1)
    step = 2 ** 28
    for i in range(0, flat.numel(), step):
        m = min(step, flat.numel() - i)
        flat[i:i + m] = torch.randint(-3, 4, (m,), generator=g, dtype=torch.int8, device=t.device)


def _ncdhw(n, c, sp, dtype, fill=None):
    """An NDHWC-contiguous tensor as its NCDHW view."""
    t = torch.empty((n, *sp, c), dtype=dtype, device=dev())
    if fill is not None:
        t.fill_(fill)
    return t.permute(0, 4, 1, 2, 3)


def _inputs(b):
    c = b.c
    seed = 9000 + 7 * c.cin + 3 * c.cout + c.sp[0] + 5 * c.sp[1] + 11 * c.sp[2]
    x = _ncdhw(c.n, c.cin, c.sp, c.dt)
    _fill_ints(x.permute(0, 2, 3, 4, 1), seed)
    wshape = (*c.k, c.cout, c.cin) if c.flip else (*c.k, c.cin, c.cout)
    w = W.int_data(wshape, seed + 1, F32).contiguous().to(dev())
    g = torch.Generator().manual_seed(seed + 2)
    d = {'x': x, 'w': w, 'bias': None, 'mask': None, 'in_mask': None}
    if c.bias:
        d['bias'] = torch.randint(-3, 4, (c.cout,), generator=g).float().to(dev())
    if c.mask:
        gd = torch.Generator(device=dev()).manual_seed(seed + 3)
        nvox = c.n * c.sp[0] * c.sp[1] * c.sp[2]
        d['mask'] = torch.randint(-2 ** 31, 2 ** 31 - 1, (nvox, (c.cout + 31) // 32), generator=gd, dtype=torch.int32, device=dev())
    terms = c.k[0] * c.k[1] * c.k[2] * c.cin + (1 if c.bias else 0)
    f = R.POOL_BLOCK.get(c.pool, (1, 1, 1))
    unit = c.coef * (0.25 if c.act else 1.0) * (0.25 if c.mask else 1.0) / (f[0] * f[1] * f[2])
    W.assert_exact_range(9 * c.coef, unit, terms * f[0] * f[1] * f[2])
    return d


def _sub(c, n, sp):
    """Case c with another batch and extent."""
    return Case(c.id, c.kernel, n, c.cin, c.cout, sp, k=c.k, dt=c.dt, flip=c.flip, env=c.env, coef=c.coef, bias=c.bias, act=c.act,
                mask=c.mask, sign=c.sign, pool=c.pool)


def _words(t, n, sp):
    return t.reshape(n, *sp, t.shape[-1])


def _pieces_batch(b, d, y2, s2):
    """The call on sub-batches below PIECE bytes per tensor, written into y2 / s2."""
    c = b.c
    _lib, _ = _libs()
    per = max(b.x_layout(1).nbytes(), b.y_layout(1).nbytes(), c.sp[0] * c.sp[1] * c.sp[2] * c.cout * 4)
    m = max(1, (PIECE - 1) // per)
    svox = c.sp[0] * c.sp[1] * c.sp[2]
    for i in range(0, c.n, m):
        j = min(i + m, c.n)
        dd = dict(d, x=d['x'][i:j], mask=None if d['mask'] is None else d['mask'][i * svox:j * svox])
        rc, _, _, signs, _ = _launch(_sub(c, j - i, c.sp), dd, y=y2[i:j])
        _lib.check(rc, f'{c.id} samples {i}:{j}')
        if signs is not None:
            s2[i * svox:j * svox] = signs


def _pieces_slabs(b, d, y2, s2):
    """The single-sample call on slabs with a two-voxel halo, the halo of the output dropped: D slabs, or (b.slabs == 'h', the 2-D
    images with D = 1) H slabs.  Either is a contiguous stretch of the one NDHWC sample."""
    c = b.c
    _lib, _ = _libs()
    D, H, Wd = c.sp
    ax = 3 if b.slabs == 'h' else 2                    # the NCDHW dimension that is cut
    ext, row = (H, Wd) if ax == 3 else (D, H * Wd)     # its extent, and the voxels of one of its slices
    assert ax == 2 or D == 1
    step = (PIECE - 1) // (row * max(c.cin, c.cout) * b.es) - 4
    step -= step & 1                                   # even: pooling pairs stay inside a slab
    assert step >= 4, (c.id, step)
    fd = R.POOL_BLOCK.get(c.pool, (1, 1, 1))[0] if ax == 2 else 1
    for s0 in range(0, ext, step):
        s1 = min(s0 + step, ext)
        a0, a1 = max(s0 - 2, 0), min(s1 + 2, ext)      # (two: the slab stays whole pooling pairs)
        dd = dict(d, x=d['x'].narrow(ax, a0, a1 - a0), mask=None if d['mask'] is None else d['mask'][a0 * row:a1 * row])
        sub = _sub(c, 1, (a1 - a0, H, Wd) if ax == 2 else (1, a1 - a0, Wd))
        yp = _ncdhw(1, c.cout, sub.out_sp(), c.dt, SENTINEL)
        rc, _, _, signs, _ = _launch(sub, dd, y=yp)
        _lib.check(rc, f'{c.id} slab {s0}:{s1}')
        y2.narrow(ax, s0 // fd, (s1 - s0) // fd).copy_(yp.narrow(ax, (s0 - a0) // fd, (s1 - s0) // fd))
        if signs is not None:
            s2[s0 * row:s1 * row] = signs[(s0 - a0) * row:(s1 - a0) * row]
        del yp, signs


def _same(a, b):
    """torch.equal of two contiguous tensors in slices of 2^30 elements (no temporary of the tensors' size)."""
    a, b = a.reshape(-1), b.reshape(-1)
    return a.numel() == b.numel() and all(torch.equal(a[i:i + 2 ** 30], b[i:i + 2 ** 30]) for i in range(0, a.numel(), 2 ** 30))


@pytest.mark.parametrize('b', CASES, ids=[b.id for b in CASES])
def test_route_is_exact_past_the_boundary(b, sg_env):
    c = b.c
    _lib, _ = _libs()
    boxes = b.boxes()
    B.check_cover(b.layouts(), boxes, c.sp, b.seam)          # on the host, before anything is launched
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = b.device_bytes() + 2 * _fwd_extra(c)       # (a piece's workspace is no larger than the large call's)
    if free < need:
        pytest.skip(f'{c.id} needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    d = y = y2 = signs = s2 = None
    try:
        d = _inputs(b)
        if c.env:
            sg_env(**c.env)
        y = _ncdhw(c.n, c.cout, c.out_sp(), c.dt, SENTINEL)
        rc, names, _, signs, _ = _launch(c, d, y=y)
        _lib.check(rc, c.id)
        assert names == [c.kernel], (c.id, names)
        weff = (R.flip_transpose(d['w']) if c.flip else d['w']).double() * c.coef
        f = R.POOL_BLOCK.get(c.pool, (1, 1, 1))
        for box in boxes:
            n, d0, d1, h0, h1 = box
            pre, ref = B.box_reference(d['x'], weff, box, d['bias'], 0.25 if c.act else None, d['mask'], 0.25, c.pool)
            got = y[n:n + 1, :, d0 // f[0]:d1 // f[0], h0 // f[1]:h1 // f[1]].cpu()
            _assert_equal(f'{c.id} box {box}', got, R.expected(ref, c.dt))
            if c.sign:
                sw = _words(signs, c.n, c.sp)[n, d0:d1, h0:h1].reshape(-1, signs.shape[-1]).cpu()
                _assert_equal(f'{c.id} box {box}', sw, R.sign_words(pre), 'sign words')
        y2 = _ncdhw(c.n, c.cout, c.out_sp(), c.dt, SENTINEL)
        s2 = torch.zeros_like(signs) if signs is not None else None
        (_pieces_slabs if b.slabs else _pieces_batch)(b, d, y2, s2)
        assert _same(y.permute(0, 2, 3, 4, 1), y2.permute(0, 2, 3, 4, 1)), f'{c.id}: the large call and the call on pieces differ'
        if signs is not None:
            assert _same(signs, s2), f'{c.id}: the sign words of the large call and of the call on pieces differ'
    finally:
        del d, y, y2, signs, s2
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------------
# Weight gradients (sg_conv3d_wgrad_bias).  A weight gradient sums over every voxel, so exactness needs a sparse right-hand side: x
# is dense random integers, dy is zero except on the (disjoint) boxes, where it is random integers in [-3, 3]; with V non-zero
# voxels every partial sum is an integer below 9 V < 2^24 (asserted).  The reference is wgref.wgrad_ref summed over the boxes, from
# the box plus halo of x; each box contributes a non-zero amount and no two the same (asserted on the host), so a box read as
# zeros, or read twice in another's place, changes the sum.  dw and db are compared with torch.equal.
#
# ----------------------------------------------------------------------------------------------------------------------
from tests import test_wgrad_exact_gpu as WG      # noqa: E402


class BigW:
    def __init__(self, case, group=1, seam=None):
        self.c, self.group, self.seam, self.id = case, group, seam or route_seam(case), case.id
        c = case
        if c.n is None:
            c.n = B.smallest_batch(self.layout('x', c.cin, 1).nbytes(), self.layout('dy', c.cout, 1).nbytes())

    def layout(self, name, ch, n=None):
        return B.Layout(name, n or self.c.n, self.c.sp, ch, 2, group=self.group)

    def layouts(self):
        return [self.layout('x', self.c.cin), self.layout('dy', self.c.cout)]

    def boxes(self):
        return B.disjoint(B.choose_boxes(self.layouts(), self.c.sp, seam=self.seam))

    def device_bytes(self):
        return sum(t.nbytes() for t in self.layouts()) + 2 ** 30


def _w(cid, kernel, cin, cout, sp, n=None, k=K333, group=1, seam=None, **kw):
    return BigW(WG.Case(cid, kernel, n, cin, cout, sp, k, **kw), group=group, seam=seam)


WGRAD = [
    _w('w_generic', 'conv_wgrad<bf16,256>', 6, 10, (3, 5, 7), group=None),
    _w('w_2', 'conv_wgrad2<3,3,3>', 128, 128, (2, 128, 32)),
    _w('w_3', 'conv_wgrad3<3,3,3>', 32, 32, (4, 8, 40)),
    _w('w_3l', 'conv_wgrad3l', 32, 32, (4, 8, 32)),
    _w('w_pw', 'pw_wgrad_partial', 4, 8, (4, 40, 64), k=K111, group=None),
    _w('w_small', 'conv_small_wgrad<bf16>', 16, 8, (1, 256, 256), k=K133),
    _w('w_planes_below', 'conv_wgrad_planes<8>', 32, 32, (2, 8, 8), n=262143, k=K133, group=None),
    _w('w_planes_above', 'conv_wgrad<bf16,256>', 32, 32, (2, 8, 8), n=262144, k=K133, group=None),
    _w('w_2_below', 'conv_wgrad2<1,3,3>', 128, 128, (127, 512, 256), n=1, k=K133),
    _w('w_2_above', 'conv_wgrad<bf16,256>', 128, 128, (128, 512, 256), n=1, k=K133),
    _w('w_3_below', 'conv_wgrad3<3,3,3>', 32, 32, (252, 512, 520), n=1),
    _w('w_3_above', 'conv_wgrad<bf16,256>', 32, 32, (253, 512, 520), n=1),
    _w('w_3l_below', 'conv_wgrad3l', 32, 32, (127, 512, 512), n=1),
    _w('w_3l_above', 'conv_wgrad3<3,3,3>', 32, 32, (128, 512, 512), n=1),
    # small.hip:437 (see the table below the sub-pixel weight gradient): five images of h w = 2^24 - 512 | 2^24
    _w('w_small_below', 'conv_small_wgrad<bf16>', 16, 8, (1, 32767, 512), n=5, k=K133),
    _w('w_small_above', 'conv_wgrad2<1,3,3>', 16, 8, (1, 32768, 512), n=5, k=K133),
]


def sparse_rhs_is_exact(b):
    """The host condition of a weight-gradient case: V non-zero voxels of dy, every partial sum below 9 V < 2^24."""
    W.assert_exact_range(9, 1, B.box_voxels(b.boxes(), b.c.sp[2]))


@pytest.mark.parametrize('b', WGRAD, ids=[b.id for b in WGRAD])
def test_weight_gradient_is_exact_past_the_boundary(b, sg_env):
    c = b.c
    _lib, _ = _libs()
    boxes = b.boxes()
    B.check_cover(b.layouts(), boxes, c.sp, b.seam)
    sparse_rhs_is_exact(b)
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    need = b.device_bytes() + _lib.load().sg_conv3d_wgrad_workspace(C.byref(WG._shape(c)), WG._dt(c.dt)) + 8 * c.k[0] * c.k[1] * c.k[2] * c.cin * c.cout
    if free < need:
        pytest.skip(f'{c.id} needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    x = dy = dw = db = None
    try:
        seed = 9500 + 7 * c.cin + 3 * c.cout + c.sp[0] + 5 * c.sp[1] + 11 * c.sp[2]
        x = _ncdhw(c.n, c.cin, c.sp, BF)
        _fill_ints(x.permute(0, 2, 3, 4, 1), seed)
        dy = _ncdhw(c.n, c.cout, c.sp, BF, 0.0)
        g = torch.Generator(device=dev()).manual_seed(seed + 1)
        dw64 = torch.zeros((*c.k, c.cin, c.cout), dtype=torch.float64)
        db64 = torch.zeros((c.cout,), dtype=torch.float64)
        parts = []
        for (n, d0, d1, h0, h1) in boxes:
            v = torch.randint(-3, 4, (d1 - d0, h1 - h0, c.sp[2], c.cout), generator=g, dtype=torch.int8, device=dev())
            dy[n, :, d0:d1, h0:h1] = v.permute(3, 0, 1, 2).to(BF)
            pw_, pb_ = B.wgrad_box_reference(x, dy, (n, d0, d1, h0, h1), c.k)
            assert bool(pw_.abs().sum() > 0) and bool(pb_.abs().sum() > 0), f'{c.id}: box {(n, d0, d1, h0, h1)} contributes nothing'
            assert all(not torch.equal(pw_, q) for q in parts), f'{c.id}: two boxes contribute the same amount'
            parts.append(pw_)
            dw64 += pw_
            db64 += pb_
        if c.env:
            sg_env(**c.env)
        dw, db = WG._outputs(c)
        rc, names = WG._launch(c, x, dy, None, dw, db, 0.25)
        _lib.check(rc, c.id)
        assert names == [c.kernel], (c.id, names)
        WG._check(c, dw, db, 0.25, dw64, db64)
    finally:
        del x, dy, dw, db
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------------
# Elementwise kernels of the step through saragan_amd.functional: 1025 samples of 16 x 64 x 64 x 32 channels -- bf16 just past 2^32
# bytes (the last voxel's channels past element 2^31), f32 just past 2^33.  Integer inputs, integer bias and slope 0.25 make bias_act
# exact in both types, so its boxes are compared with torch.equal; pixel_norm keeps the tolerances of tests/test_elementwise_gpu.py
# for the same kernel and dtype.  The whole tensor is compared with the same call on sub-batches below 2^30 bytes.  The bias
# gradient sums over the tensor: dy is zero except on the boxes (integers there), every term a multiple of 0.25 up to 3, V < 2^24 / 12.
#
# ----------------------------------------------------------------------------------------------------------------------
EW_N, EW_C, EW_SP = 1025, 32, (16, 64, 64)
EW_DT = [BF, F32]


def _ew_layouts(dtype):
    es = 2 if dtype == BF else 4
    out = [B.Layout('x', EW_N, EW_SP, EW_C, es)]
    if dtype == BF:
        out.append(B.Layout('sign words', EW_N, EW_SP, 1, 4))
    return out


def ew_boxes(dtype):
    return B.disjoint(B.choose_boxes(_ew_layouts(dtype), EW_SP, seam=B.SEAM))


def _ew_guard(dtype, tensors):
    lay = _ew_layouts(dtype)
    boxes = ew_boxes(dtype)
    B.check_cover(lay, boxes, EW_SP, B.SEAM)
    assert lay[0].nbytes() > (B.B32 if dtype == BF else B.B33) and EW_N * EW_SP[0] * EW_SP[1] * EW_SP[2] * EW_C > 2 ** 31
    need = tensors * lay[0].nbytes() + 2 ** 30
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    return boxes


def _ew_pieces(dtype):
    m = (PIECE - 1) // (EW_SP[0] * EW_SP[1] * EW_SP[2] * EW_C * (2 if dtype == BF else 4))
    return [(i, min(i + m, EW_N)) for i in range(0, EW_N, m)]


def _crop(t, box):
    n, d0, d1, h0, h1 = box
    return t[n:n + 1, :, d0:d1, h0:h1].cpu()


@pytest.mark.parametrize('dtype', EW_DT, ids=['bf16', 'f32'])
def test_bias_act_forward_past_the_boundary(dtype):
    from saragan_amd import functional as F
    boxes = _ew_guard(dtype, 3)
    x = y = y2 = None
    try:
        x = _ncdhw(EW_N, EW_C, EW_SP, dtype)
        _fill_ints(x.permute(0, 2, 3, 4, 1), 71)
        bias = torch.randint(-3, 4, (EW_C,), generator=torch.Generator().manual_seed(72)).float().to(dev())
        y = F.bias_act(x, bias, True, 0.25)
        for box in boxes:
            want = R.expected(R.bias_act(_crop(x, box).double(), bias.cpu(), 0.25), dtype)
            _assert_equal(f'bias_act box {box}', _crop(y, box), want)
        y2 = torch.empty_like(y)
        for i, j in _ew_pieces(dtype):
            y2[i:j] = F.bias_act(x[i:j], bias, True, 0.25)
        assert _same(y.permute(0, 2, 3, 4, 1), y2.permute(0, 2, 3, 4, 1))
    finally:
        del x, y, y2
        torch.cuda.empty_cache()


@pytest.mark.parametrize('form', ['bf16-y', 'bf16-bits', 'f32-y'])
def test_bias_act_backward_past_the_boundary(form):
    from saragan_amd import functional as F
    dtype = BF if form.startswith('bf16') else F32
    boxes = _ew_guard(dtype, 4)
    W.assert_exact_range(3, 0.25, B.box_voxels(boxes, EW_SP[2]))
    y = dy = dx = mask = None
    try:
        y = _ncdhw(EW_N, EW_C, EW_SP, dtype)
        _fill_ints(y.permute(0, 2, 3, 4, 1), 73)
        dy = _ncdhw(EW_N, EW_C, EW_SP, dtype, 0.0)
        g = torch.Generator(device=dev()).manual_seed(74)
        db64 = torch.zeros(EW_C, dtype=torch.float64)
        want = {}
        for box in boxes:
            n, d0, d1, h0, h1 = box
            v = torch.randint(-3, 4, (d1 - d0, h1 - h0, EW_SP[2], EW_C), generator=g, dtype=torch.int8, device=dev())
            dy[n, :, d0:d1, h0:h1] = v.permute(3, 0, 1, 2).to(dtype)
            yb, gb = _crop(y, box).double(), _crop(dy, box).double()
            want[box] = torch.where(yb >= 0, gb, gb * 0.25)
            part = want[box].sum((0, 2, 3, 4))
            assert bool(part.abs().sum() > 0)
            db64 += part
        mask = F.sign_words(y) if form.endswith('bits') else y
        dx, db = F.raw_bias_act_bwd(dy, mask, 0.25, True, True)
        for box in boxes:
            _assert_equal(f'bias_act bwd box {box}', _crop(dx, box), R.expected(want[box], dtype), 'dx')
        assert torch.equal(db.cpu().double(), db64), 'dbias'
        # everywhere else dy is zero: dx is zero (+0 or -0) outside the boxes, so the sum of |dx| is the boxes' own
        total = sum(float(dx[i:j].abs().double().sum()) for i, j in _ew_pieces(dtype))
        assert total == float(sum(w.abs().sum() for w in want.values()))
    finally:
        del y, dy, dx, mask
        torch.cuda.empty_cache()


@pytest.mark.parametrize('dtype', EW_DT, ids=['bf16', 'f32'])
def test_pixel_norm_forward_past_the_boundary(dtype):
    from saragan_amd import functional as F
    from tests import ewref as E
    boxes = _ew_guard(dtype, 3)
    x = y = y2 = None
    try:
        x = _ncdhw(EW_N, EW_C, EW_SP, dtype)
        _fill_ints(x.permute(0, 2, 3, 4, 1), 75)
        y = F.pixel_norm(x)
        for box in boxes:
            xb = _crop(x, box).double()
            E.close(_crop(y, box), xb * E.pn_scale(xb), dtype, f'pixel_norm box {box}')
        y2 = torch.empty_like(y)
        for i, j in _ew_pieces(dtype):
            y2[i:j] = F.pixel_norm(x[i:j])
        assert _same(y.permute(0, 2, 3, 4, 1), y2.permute(0, 2, 3, 4, 1))
    finally:
        del x, y, y2
        torch.cuda.empty_cache()


def test_sign_words_and_cast_past_the_boundary():
    """sg_sign_words on the bf16 tensor (boxes against fwdref.sign_words, the whole against sub-batches), and sg_cast bf16 -> f32
    (an f32 tensor past 2^33 bytes) -> bf16: both conversions are exact for these integers, the whole tensors are compared."""
    from saragan_amd import functional as F
    boxes = _ew_guard(BF, 5)
    _lib, lib = _libs()
    x = words = w2 = f = back = None
    try:
        x = _ncdhw(EW_N, EW_C, EW_SP, BF)
        _fill_ints(x.permute(0, 2, 3, 4, 1), 76)
        words = F.sign_words(x)
        assert tuple(words.shape) == (EW_N, *EW_SP, 1)
        for box in boxes:
            n, d0, d1, h0, h1 = box
            _assert_equal(f'sign words box {box}', words[n, d0:d1, h0:h1].reshape(-1, 1).cpu(), R.sign_words(_crop(x, box)), 'sign words')
        w2 = torch.empty_like(words)
        for i, j in _ew_pieces(BF):
            w2[i:j] = F.sign_words(x[i:j])
        assert _same(words, w2)
        xs = x.permute(0, 2, 3, 4, 1)
        f = torch.full(xs.shape, SENTINEL, dtype=F32, device=dev())
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.sg_cast(xs.data_ptr(), _lib.SG_BF16, f.data_ptr(), _lib.SG_F32, xs.numel(), stream), 'cast to f32')
        fl, xl = f.reshape(-1), xs.reshape(-1)
        assert all(torch.equal(fl[i:i + 2 ** 30], xl[i:i + 2 ** 30].float()) for i in range(0, xl.numel(), 2 ** 30))
        back = torch.full(xs.shape, SENTINEL, dtype=BF, device=dev())
        _lib.check(lib.sg_cast(f.data_ptr(), _lib.SG_F32, back.data_ptr(), _lib.SG_BF16, xs.numel(), stream), 'cast to bf16')
        torch.cuda.synchronize()
        assert _same(back, xs)
    finally:
        del x, words, w2, f, back
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------------
# Sub-pixel up-convolution (subpix.hip), s the LOW-resolution shape; boxes live on the low-resolution grid, y on the fine one.
#
# ----------------------------------------------------------------------------------------------------------------------
SUB = [
    Big(Case('sub_fwd', 'upconv_subpixel_fwd', None, 64, 32, (4, 16, 16), bias=True, act=True, sign=True, par=(0, 0, 0))),
    Big(Case('sub_dgrad', 'upconv_subpixel_dgrad', None, 64, 32, (4, 16, 16), flip=True, par=(0, 0, 0))),
    Big(Case('sub_below', 'upconv_subpixel_fwd', 1, 64, 32, (128, 508, 256), bias=True, act=True, sign=True, par=(0, 0, 0)), slabs=True),
    Big(Case('sub_above', 'upconv_subpixel_fwd<one tile per block>', 1, 64, 32, (128, 512, 256), bias=True, act=True, sign=True,
             par=(0, 0, 0)), slabs=True),
    # subpix.hip:638 from below: the one-tile-per-block kernel at the largest sample the guard admits, int xoff (:107) within one plane of
    # 2^31 elements (254: D in whole 2-plane tiles)
    Big(Case('sub_638_below', 'upconv_subpixel_fwd<one tile per block>', 1, 64, 32, (254, 512, 256), bias=True, act=True, sign=True,
             par=(0, 0, 0)), slabs=True),
    # subpix.hip:936 from below: one sample of the fine gy 16 MiB below 2^31 bytes (the other side: test_subpixel_dgrad_refusal...)
    Big(Case('subdg_below', 'upconv_subpixel_dgrad', 1, 64, 32, (127 * 2, 256, 64), flip=True, par=(0, 0, 0)), slabs=True),
]


def sub_layouts(b):
    """(par marks the case as sub-pixel: Case.out_sp() is then the fine extent.)  flip: the data gradient, whose input is the
    fine gy [cout] and whose output the low-resolution gx [cin]."""
    c = b.c
    low = B.Layout('x' if not c.flip else 'gx', c.n, c.sp, c.cin, 2, group=b.group)
    fine = B.Layout('y' if not c.flip else 'gy', c.n, c.out_sp(), c.cout, 2, group=b.group, fine=(2, 2, 2))
    out = [low, fine]
    if c.sign:
        out.append(B.Layout('sign words', c.n, c.out_sp(), 1, 4, group=b.group, fine=(2, 2, 2)))
    return out


def sub_boxes(b):
    return B.choose_boxes(sub_layouts(b), b.c.sp, seam=b.seam)


def _sub_call(c, n, sp, src, w, bias, dst, signs):
    """One sg_upconv3d_subpixel_fwd / _dgrad call on n samples of low-resolution extent sp; returns the kernel names."""
    from tests.test_conv_fwd_exact_gpu import _fwd_kernels, _garbage, _stream
    _lib, lib = _libs()
    shp = _lib.ConvShape(n, *sp, c.cin, c.cout, 3, 3, 3, 0)
    lib.sg_prof_enable(1)
    try:
        if c.flip:
            assert lib.sg_upconv3d_subpixel_dgrad_supported(C.byref(shp), _lib.SG_BF16)
            wp = _garbage(lib.sg_upconv3d_subpixel_dgrad_packed_bytes(C.byref(shp), _lib.SG_BF16))
            _lib.check(lib.sg_upconv3d_subpixel_dgrad_pack(w.data_ptr(), c.coef, wp.data_ptr(), C.byref(shp), _lib.SG_BF16, _stream()), 'pack')
            rc = lib.sg_upconv3d_subpixel_dgrad(src.data_ptr(), wp.data_ptr(), dst.data_ptr(), C.byref(shp), _lib.SG_BF16, _stream())
        else:
            assert lib.sg_upconv3d_subpixel_supported(C.byref(shp), _lib.SG_BF16)
            wp = _garbage(lib.sg_upconv3d_subpixel_packed_bytes(C.byref(shp), _lib.SG_BF16))
            _lib.check(lib.sg_upconv3d_subpixel_pack(w.data_ptr(), c.coef, wp.data_ptr(), C.byref(shp), _lib.SG_BF16, _stream()), 'pack')
            ep = _lib.ConvEpilogue()
            ep.bias, ep.act, ep.slope, ep.sign_out = bias.data_ptr(), 1, 0.25, signs.data_ptr()
            rc = lib.sg_upconv3d_subpixel_fwd(src.data_ptr(), wp.data_ptr(), dst.data_ptr(), C.byref(shp), C.byref(ep), _lib.SG_BF16, _stream())
        torch.cuda.synchronize()
        names = _fwd_kernels(_lib, lib)
    finally:
        lib.sg_prof_enable(0)
    _lib.check(rc, c.id)
    return names


@pytest.mark.parametrize('b', SUB, ids=[b.id for b in SUB])
def test_subpixel_route_is_exact_past_the_boundary(b):
    c = b.c
    boxes = sub_boxes(b)
    B.check_cover(sub_layouts(b), boxes, c.sp, b.seam)
    W.assert_exact_range(9 * c.coef, c.coef * 0.25, 27 * 8 * max(c.cin, c.cout) + 1)
    need = 2 * sum(t.nbytes() for t in sub_layouts(b)) + 3 * PIECE
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'{c.id} needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    fine = c.out_sp()
    src = dst = dst2 = signs = s2 = None
    try:
        seed = 9700 + c.sp[0] + (1 if c.flip else 0)
        w = W.int_data((3, 3, 3, c.cin, c.cout), seed + 1, F32).contiguous().to(dev())
        bias = torch.randint(-3, 4, (c.cout,), generator=torch.Generator().manual_seed(seed + 2)).float().to(dev())
        weff = w.double() * c.coef
        if c.flip:
            src, dst = _ncdhw(c.n, c.cout, fine, BF), _ncdhw(c.n, c.cin, c.sp, BF, SENTINEL)
        else:
            src, dst = _ncdhw(c.n, c.cin, c.sp, BF), _ncdhw(c.n, c.cout, fine, BF, SENTINEL)
            signs = torch.full((c.n, *fine, 1), 0x5A5A5A5A, dtype=torch.int32, device=dev())
        _fill_ints(src.permute(0, 2, 3, 4, 1), seed)
        names = _sub_call(c, c.n, c.sp, src, w, bias, dst, signs)
        assert names == [c.kernel], (c.id, names)
        for box in boxes:
            n, d0, d1, h0, h1 = box
            if c.flip:
                ref = B.updgrad_box_reference(src, weff, box)
                _assert_equal(f'{c.id} box {box}', dst[n:n + 1, :, d0:d1, h0:h1].cpu(), R.expected(ref, BF), 'gx')
            else:
                ref = B.upconv_box_reference(src, weff, box, bias, 0.25)
                _assert_equal(f'{c.id} box {box}', dst[n:n + 1, :, 2 * d0:2 * d1, 2 * h0:2 * h1].cpu(), R.expected(ref, BF))
                sw = signs[n, 2 * d0:2 * d1, 2 * h0:2 * h1].reshape(-1, 1).cpu()
                _assert_equal(f'{c.id} box {box}', sw, R.sign_words(ref), 'sign words')
        dst2 = torch.full_like(dst, SENTINEL)
        s2 = torch.zeros_like(signs) if signs is not None else None
        if b.slabs:      # D slabs of the low-resolution grid with two planes of halo, the halo's planes of the output dropped
            D = c.sp[0]
            step = (PIECE - 1) // (8 * c.sp[1] * c.sp[2] * c.cout * 2) - 4
            step -= step & 1
            assert step >= 2
            for s0 in range(0, D, step):
                s1 = min(s0 + step, D)
                a0, a1 = max(s0 - 2, 0), min(s1 + 2, D)      # (two planes: every slab keeps an even number of planes)
                sub_sp = (a1 - a0, c.sp[1], c.sp[2])
                if c.flip:
                    yp = _ncdhw(1, c.cin, sub_sp, BF, SENTINEL)
                    _sub_call(c, 1, sub_sp, src[:, :, 2 * a0:2 * a1], w, bias, yp, None)
                    dst2[:, :, s0:s1] = yp[:, :, s0 - a0:s1 - a0]
                    del yp
                    continue
                yp = _ncdhw(1, c.cout, (2 * (a1 - a0), fine[1], fine[2]), BF, SENTINEL)
                sp_ = torch.zeros((1, 2 * (a1 - a0), fine[1], fine[2], 1), dtype=torch.int32, device=dev())
                _sub_call(c, 1, sub_sp, src[:, :, a0:a1], w, bias, yp, sp_)
                dst2[:, :, 2 * s0:2 * s1] = yp[:, :, 2 * (s0 - a0):2 * (s1 - a0)]
                s2[:, 2 * s0:2 * s1] = sp_[:, 2 * (s0 - a0):2 * (s1 - a0)]
                del yp, sp_
        else:
            per = max(t.nbytes() for t in sub_layouts(b)) // c.n
            m = max(1, (PIECE - 1) // per)
            for i in range(0, c.n, m):
                j = min(i + m, c.n)
                _sub_call(c, j - i, c.sp, src[i:j], w, bias, dst2[i:j], None if s2 is None else s2[i:j])
        assert _same(dst.permute(0, 2, 3, 4, 1), dst2.permute(0, 2, 3, 4, 1)), f'{c.id}: the large call and the call on pieces differ'
        if signs is not None:
            assert _same(signs, s2), f'{c.id}: the sign words of the large call and of the call on pieces differ'
    finally:
        del src, dst, dst2, signs, s2
        torch.cuda.empty_cache()


REFUSED = Big(Case('sub_refused', 'conv_fwd2<bf16,2,1,2>', 1, 64, 32, (128, 512, 512), bias=True, act=True, sign=True, par=(0, 0, 0)), slabs=True)
SUBDG_ABOVE = Big(Case('subdg_above', 'conv_fwd3r<bf16,2,2,3,3,3>', 1, 64, 32, (256, 256, 64), flip=True, par=(0, 0, 0)), slabs=True)
FALLBACK = [REFUSED, SUBDG_ABOVE]      # the refusals: what runs in the entry point's place (tests/test_bigref_host.py checks their boxes too)


def fallback_layouts(b):
    """The tensors of a refusal case's fallback.  subdg_above: functional._upconv_dgrad writes the full-resolution gradient (cin
    channels on the fine grid: 2^32 bytes) before sg_downscale_sum reads it back; that tensor is required of the boxes like gy and gx."""
    lay = sub_layouts(b)
    if b is SUBDG_ABOVE:
        lay.append(B.Layout('full-resolution gradient', b.c.n, b.c.out_sp(), b.c.cin, 2, fine=(2, 2, 2)))
    return lay


def fallback_boxes(b):
    return B.choose_boxes(fallback_layouts(b), b.c.sp, seam=b.seam)


def test_subpixel_refusal_and_what_functional_runs_in_its_place(monkeypatch):
    """subpix.hip:638: one sample of x of 2^31 ELEMENTS (64 channels at low 128 x 512 x 512: x is 4 GiB, y 16 GiB).  The entry point
    returns SG_EUNSUPPORTED, launches nothing and leaves y alone; functional.raw_conv, with the sub-pixel route allowed, then runs the
    layer as conv3d(upscale3d(x)) through sg_conv3d_fwd.  There conv_fwd3p16 (conv3p.hip:898), the K split (conv3d.hip:1714) and
    conv_fwd4 (conv3d.hip:2160) decline a fine sample of 32 GiB in turn and conv_fwd2's fused gather (conv3d.hip:453, int64) takes
    it.  Its result is exact on the boxes and equals the same call on D slabs of x."""
    from saragan_amd import functional as F
    from tests.test_conv_fwd_exact_gpu import _fwd_kernels, _garbage, _stream
    _lib, lib = _libs()
    b, c = REFUSED, REFUSED.c
    boxes = fallback_boxes(b)
    B.check_cover(fallback_layouts(b), boxes, c.sp, b.seam)
    W.assert_exact_range(9 * c.coef, c.coef * 0.25, 27 * 8 * c.cin + 1)      # (the slabs run the sub-pixel form: 8 summed weights a tap)
    need = 4 * sum(t.nbytes() for t in sub_layouts(b)) + 3 * PIECE
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'{c.id} needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    monkeypatch.setattr(F, '_NO_SUBPIXEL', False)
    x = y = y2 = signs = s2 = None
    try:
        x = _ncdhw(1, c.cin, c.sp, BF)
        _fill_ints(x.permute(0, 2, 3, 4, 1), 9800)
        w = W.int_data((3, 3, 3, c.cin, c.cout), 9801, F32).contiguous().to(dev())
        bias = torch.randint(-3, 4, (c.cout,), generator=torch.Generator().manual_seed(9802)).float().to(dev())
        shp = _lib.ConvShape(1, *c.sp, c.cin, c.cout, 3, 3, 3, 0)
        assert not lib.sg_upconv3d_subpixel_supported(C.byref(shp), _lib.SG_BF16)
        y = _ncdhw(1, c.cout, c.out_sp(), BF, SENTINEL)
        wp = _garbage(lib.sg_upconv3d_subpixel_packed_bytes(C.byref(shp), _lib.SG_BF16))
        ep = _lib.ConvEpilogue()
        lib.sg_prof_enable(1)
        try:
            rc = lib.sg_upconv3d_subpixel_fwd(x.data_ptr(), wp.data_ptr(), y.data_ptr(), C.byref(shp), C.byref(ep), _lib.SG_BF16, _stream())
            torch.cuda.synchronize()
            assert rc == _lib.SG_EUNSUPPORTED and _fwd_kernels(_lib, lib) == []
        finally:
            lib.sg_prof_enable(0)
        assert all(bool((y[:, :, i:i + 16] == SENTINEL).all()) for i in range(0, c.out_sp()[0], 16)), 'a refused call wrote to y'
        del y
        lib.sg_prof_enable(1)
        try:
            y, _, signs = F.raw_conv(x, w, c.coef, False, ups=True, bias=bias, act=True, slope=0.25, want_signs=True)
            torch.cuda.synchronize()
            names = _fwd_kernels(_lib, lib)
        finally:
            lib.sg_prof_enable(0)
        assert names == [c.kernel], names
        weff = w.double() * c.coef
        for box in boxes:
            n, d0, d1, h0, h1 = box
            ref = B.upconv_box_reference(x, weff, box, bias, 0.25)
            _assert_equal(f'{c.id} box {box}', y[n:n + 1, :, 2 * d0:2 * d1, 2 * h0:2 * h1].cpu(), R.expected(ref, BF))
            _assert_equal(f'{c.id} box {box}', signs[n, 2 * d0:2 * d1, 2 * h0:2 * h1].reshape(-1, 1).cpu(), R.sign_words(ref), 'sign words')
        y2, s2 = torch.full_like(y, SENTINEL), torch.zeros_like(signs)
        D, step = c.sp[0], 2
        for s0 in range(0, D, step):
            s1 = min(s0 + step, D)
            a0, a1 = max(s0 - 2, 0), min(s1 + 2, D)
            yp, _, sp_ = F.raw_conv(x[:, :, a0:a1], w, c.coef, False, ups=True, bias=bias, act=True, slope=0.25, want_signs=True)
            assert yp.numel() * 2 < PIECE
            y2[:, :, 2 * s0:2 * s1] = yp[:, :, 2 * (s0 - a0):2 * (s1 - a0)]
            s2[:, 2 * s0:2 * s1] = sp_[:, 2 * (s0 - a0):2 * (s1 - a0)]
            del yp, sp_
        assert _same(y.permute(0, 2, 3, 4, 1), y2.permute(0, 2, 3, 4, 1)), 'the large call and the call on slabs differ'
        assert _same(signs, s2), 'the sign words of the large call and of the call on slabs differ'
    finally:
        del x, y, y2, signs, s2
        F.mark_packs_stale()
        torch.cuda.empty_cache()


def scale_layouts(up):
    """upscale2x: x on the low-resolution base grid, y = the elementwise tensor on the fine one; downscale2x: x the elementwise
    tensor on the base grid, y its 2 x 2 x 2 block means."""
    low = tuple(v // 2 for v in EW_SP)
    if up:
        return low, [B.Layout('x', EW_N, low, EW_C, 2), B.Layout('y', EW_N, EW_SP, EW_C, 2, fine=(2, 2, 2))]
    return EW_SP, [B.Layout('x', EW_N, EW_SP, EW_C, 2), B.Layout('y', EW_N, low, EW_C, 2, pool=(2, 2, 2))]


def scale_boxes(up):
    base, lay = scale_layouts(up)
    return B.choose_boxes(lay, base, seam=B.SEAM, align=(1, 1) if up else (2, 2))


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('up', [True, False], ids=['upscale2x', 'downscale2x'])
def test_nearest_scaling_past_the_boundary(up, masked):
    """upscale2x_rows_kernel (elementwise.hip:526-528, int64 row bases) writing a bf16 y past 2^32 bytes, and downscale2x_kernel
    (:594 int64 vox) reading such an x: integer inputs, gains 0.5 and 1/8, exact, so the boxes are compared with torch.equal.
    masked: the sign words of the LARGE tensor (y of the up-scale, :528 mrow = mask_bits + row OW nw; x of the block sum, :597
    bits[vox nw]) select a factor 0.25 per element: multiples of 1/32 no larger than 3, still exact in bf16."""
    from saragan_amd import functional as F
    base, lay = scale_layouts(up)
    boxes = scale_boxes(up)
    B.check_cover(lay, boxes, base, B.SEAM)
    need = 2 * sum(t.nbytes() for t in lay) + 2 ** 30 + EW_N * EW_SP[0] * EW_SP[1] * EW_SP[2] * 4
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    x = y = y2 = words = None
    try:
        x = _ncdhw(EW_N, EW_C, lay[0].sp, BF)
        _fill_ints(x.permute(0, 2, 3, 4, 1), 77)
        words = None
        if masked:
            words = torch.randint(-2 ** 31, 2 ** 31 - 1, (EW_N, *EW_SP, 1), dtype=torch.int32, device=dev(),
                                  generator=torch.Generator(device=dev()).manual_seed(80))

        def call(xs, ws):
            if not masked:
                return F.upscale2x(xs, 0.5) if up else F.downscale2x(xs, 0.125)
            return F._Up.apply(xs, 0.5, ws, 0.25, (2, 2, 2)) if up else F._Down.apply(xs, 0.125, None, (2, 2, 2), ws, 0.25)

        y = call(x, words)
        assert tuple(y.shape) == (EW_N, EW_C, *lay[1].sp)
        for (n, d0, d1, h0, h1) in boxes:
            xb = x[n:n + 1, :, d0:d1, h0:h1].cpu().double()
            f = 2 if up else 1      # the box on the grid of the large tensor, which is the one the sign words belong to
            wb = None if not masked else words[n, f * d0:f * d1, f * h0:f * h1].reshape(-1, 1).cpu()
            if up:
                want, got = W.up2(xb) * 0.5, y[n:n + 1, :, 2 * d0:2 * d1, 2 * h0:2 * h1].cpu()
                want = want if wb is None else R.apply_mask(want, wb, 0.25)
            else:
                want = R.block_sum(xb if wb is None else R.apply_mask(xb, wb, 0.25), (2, 2, 2)) * 0.125
                got = y[n:n + 1, :, d0 // 2:d1 // 2, h0 // 2:h1 // 2].cpu()
            _assert_equal(f'box {(n, d0, d1, h0, h1)}', got, R.expected(want, BF))
        y2 = torch.empty_like(y)
        m = (PIECE - 1) // (max(t.nbytes() for t in lay) // EW_N)
        for i in range(0, EW_N, m):
            y2[i:i + m] = call(x[i:i + m], None if words is None else words[i:i + m])
        assert _same(y.permute(0, 2, 3, 4, 1), y2.permute(0, 2, 3, 4, 1))
    finally:
        del x, y, y2, words
        torch.cuda.empty_cache()


def test_lerp_past_the_boundary():
    """axpby_kernel (sg_axpby, int64 numel) through F.lerp on two bf16 tensors past 2^32 bytes: 0.5 a + 0.25 b of integers, exact."""
    from saragan_amd import functional as F
    boxes = _ew_guard(BF, 4)
    a = b_ = y = None
    try:
        a, b_ = _ncdhw(EW_N, EW_C, EW_SP, BF), _ncdhw(EW_N, EW_C, EW_SP, BF)
        _fill_ints(a.permute(0, 2, 3, 4, 1), 78)
        _fill_ints(b_.permute(0, 2, 3, 4, 1), 79)
        y = F.lerp(a, b_, 0.5, 0.25)
        for box in boxes:
            _assert_equal(f'lerp box {box}', _crop(y, box), R.expected(0.5 * _crop(a, box).double() + 0.25 * _crop(b_, box).double(), BF))
        for i, j in _ew_pieces(BF):
            assert torch.equal(y[i:j], F.lerp(a[i:j], b_[i:j], 0.5, 0.25)), f'samples {i}:{j}'
    finally:
        del a, b_, y
        torch.cuda.empty_cache()


def test_pixel_norm_backward_past_the_boundary():
    """F._PixelNormBwd (pixel_norm_kernel<BWD>, elementwise.hip:313-315 a + v c, yv + v c with int64 v) on bf16 gy and y past 2^32
    bytes with a saved scale of 2^26 + voxels: dx = scale (gy - y mean_c(gy y)) with integer gy, y and power-of-two scales is exact in
    f32; the boxes keep the bf16 tolerance tests/test_elementwise_gpu.py uses for this kernel (it reads the rounded y)."""
    from saragan_amd import functional as F
    from tests import ewref as E
    boxes = _ew_guard(BF, 4)
    gy = y = sc = dx = None
    try:
        gy, y = _ncdhw(EW_N, EW_C, EW_SP, BF), _ncdhw(EW_N, EW_C, EW_SP, BF)
        _fill_ints(gy.permute(0, 2, 3, 4, 1), 81)
        _fill_ints(y.permute(0, 2, 3, 4, 1), 82)
        nv = EW_N * EW_SP[0] * EW_SP[1] * EW_SP[2]
        sc = torch.randint(-2, 1, (nv,), device=dev(), generator=torch.Generator(device=dev()).manual_seed(83)).float().exp2()
        dx = F._PixelNormBwd.apply(gy, y, sc)
        sv = sc.reshape(EW_N, 1, *EW_SP)
        for box in boxes:
            E.close(_crop(dx, box), E.pn_bwd(_crop(gy, box).double(), _crop(y, box).double(), _crop(sv, box).double()), BF,
                    f'pixel_norm bwd box {box}', (3e-2, 3e-2))
        sv1 = EW_SP[0] * EW_SP[1] * EW_SP[2]
        for i, j in _ew_pieces(BF):
            assert torch.equal(dx[i:j], F._PixelNormBwd.apply(gy[i:j], y[i:j], sc[i * sv1:j * sv1])), f'samples {i}:{j}'
    finally:
        del gy, y, sc, dx
        torch.cuda.empty_cache()


def _low_halo(box, sp):
    n, d0, d1, h0, h1 = box
    return max(d0 - 1, 0), min(d1 + 1, sp[0]), max(h0 - 1, 0), min(h1 + 1, sp[1])


@pytest.mark.parametrize('adjoint', [False, True], ids=['up', 'adjoint'])
def test_trilinear_past_the_boundary(adjoint):
    """trilinear_up2x_kernel writing, and its adjoint reading, the bf16 tensor past 2^32 bytes (elementwise.hip:656 / :712, int64 src;
    y + i E with int64 i).  Weights are products of 1/4 and 3/4: every f32 sum of integer inputs is exact and the one bf16 rounding is
    inside the tolerance of tests/test_elementwise_gpu.py.  The box reference is torch's CPU interpolate (ewref.tri_up / tri_up_adj) on
    the box plus one low-resolution voxel around it, that ring dropped: its border rules apply at the tensor's own borders only."""
    from saragan_amd import functional as F
    from tests import ewref as E
    base, lay = scale_layouts(True)
    boxes = scale_boxes(True)
    B.check_cover(lay, boxes, base, B.SEAM)
    need = 2 * sum(t.nbytes() for t in lay) + 2 ** 30
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    src = out = None
    try:
        src = _ncdhw(EW_N, EW_C, EW_SP if adjoint else base, BF)
        _fill_ints(src.permute(0, 2, 3, 4, 1), 84)
        out = F._TriUp.apply(src, adjoint)
        assert tuple(out.shape) == (EW_N, EW_C, *(base if adjoint else EW_SP))
        for box in boxes:
            n, d0, d1, h0, h1 = box
            a0, a1, b0, b1 = _low_halo(box, base)
            if adjoint:
                ref = E.tri_up_adj(src[n:n + 1, :, 2 * a0:2 * a1, 2 * b0:2 * b1].cpu().double())[:, :, d0 - a0:d1 - a0, h0 - b0:h1 - b0]
                got = out[n:n + 1, :, d0:d1, h0:h1]
            else:
                ref = E.tri_up(src[n:n + 1, :, a0:a1, b0:b1].cpu().double())[:, :, 2 * (d0 - a0):2 * (d1 - a0), 2 * (h0 - b0):2 * (h1 - b0)]
                got = out[n:n + 1, :, 2 * d0:2 * d1, 2 * h0:2 * h1]
            E.close(got, ref, BF, f'trilinear box {box}')
        m = (PIECE - 1) // (lay[1].nbytes() // EW_N)
        for i in range(0, EW_N, m):
            assert torch.equal(out[i:i + m], F._TriUp.apply(src[i:i + m], adjoint)), f'samples {i}:{i + m}'
    finally:
        del src, out
        torch.cuda.empty_cache()


def test_interpolate_rows_past_the_boundary():
    """lerp_rows_kernel (elementwise.hip:774 gamma[i / pv], a + i E with int64 i) on bf16 operands past 2^32 bytes: one weight per
    sample out of 0, 1, 1/2, 1/4, integers: exact.  gamma = 0 and 1 reproduce an operand bit for bit, also in the last sample."""
    from saragan_amd import functional as F
    boxes = _ew_guard(BF, 4)
    a = b_ = y = None
    try:
        a, b_ = _ncdhw(EW_N, EW_C, EW_SP, BF), _ncdhw(EW_N, EW_C, EW_SP, BF)
        _fill_ints(a.permute(0, 2, 3, 4, 1), 85)
        _fill_ints(b_.permute(0, 2, 3, 4, 1), 86)
        gam = torch.tensor([0.0, 1.0, 0.5, 0.25]).repeat(EW_N // 4 + 1)[:EW_N].contiguous()
        y = F.interpolate_rows(gam.to(dev()), a, b_)
        for box in boxes:
            g = float(gam[box[0]])
            _assert_equal(f'interpolate_rows box {box}', _crop(y, box), R.expected(g * _crop(a, box).double() + (1 - g) * _crop(b_, box).double(), BF))
        assert float(gam[EW_N - 1]) == 0.0 and torch.equal(y[EW_N - 1], b_[EW_N - 1]) and float(gam[EW_N - 4]) == 1.0 and torch.equal(y[EW_N - 4], a[EW_N - 4])
        for i, j in _ew_pieces(BF):
            assert torch.equal(y[i:j], F.interpolate_rows(gam[i:j].to(dev()), a[i:j], b_[i:j])), f'samples {i}:{j}'
    finally:
        del a, b_, y
        torch.cuda.empty_cache()


@pytest.mark.parametrize('ordered', [False, True], ids=['atomic', 'ordered'])
def test_sumsq_keep_w_past_the_boundary(ordered, sg_env):
    """sumsq_keep_w_kernel / _ordered_kernel (elementwise.hip:829 / :852, g + ((int64) nn dh + rr) w + ww) c) on the bf16 tensor past
    2^32 bytes.  out[n, w] sums 32 x 16 x 64 squares of integers in [-3, 3]: at most 9 x 32768 < 2^24, exact in any order, so the
    dense tensor needs no sparse construction and the comparison is == (a departure from the sparse right-hand side asked for this
    kernel: every element of the tensor then takes part in the sum, which a sparse tensor would not test).  The reference is the fp64 sum over the whole sample for
    every sample a required point lies in; the whole result equals the call on sub-batches."""
    from saragan_amd import functional as F
    boxes = _ew_guard(BF, 2)
    W.assert_exact_range(9, 1, EW_C * EW_SP[0] * EW_SP[1])
    x = out = None
    try:
        sg_env(SG_DETERMINISTIC=1 if ordered else 0)
        x = _ncdhw(EW_N, EW_C, EW_SP, BF)
        _fill_ints(x.permute(0, 2, 3, 4, 1), 87)
        out = F.sumsq_keep_w(x)
        assert tuple(out.shape) == (EW_N, EW_SP[2])
        for n in sorted({box[0] for box in boxes}):
            xs = x[n].cpu().double()
            assert torch.equal(out[n].cpu().double(), (xs * xs).sum((0, 1, 2))), f'sample {n}'
        for i, j in _ew_pieces(BF):
            assert torch.equal(out[i:j], F.sumsq_keep_w(x[i:j])), f'samples {i}:{j}'
    finally:
        del x, out
        torch.cuda.empty_cache()


def test_add_noise_windows_on_both_sides_of_element_2_32():
    """add_noise_kernel (elementwise.hip:797 ctr = gi + offset, :813 int64 i = 4 gi + k) on 2^32 + 2^20 bf16 zeros (8 GiB) with the
    Philox offset 3 x 2^30: group gi = 2^30 holds element 2^32, and there the counter's low word carries into the high one.  The
    property of test_add_noise_exact_properties: elements [k, k + m) of the large call equal a small call with the offset advanced by
    k / 4 groups -- for the first window, the window that ends at element 2^32, the one that starts there and the last one."""
    from saragan_amd import functional as F
    N, m, off, sd, seed = 2 ** 32 + 2 ** 20, 2 ** 16, 3 * 2 ** 30, 0.5, 11
    need = 2 * 2 * N + 2 ** 28
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    x = big = None
    try:
        x = torch.zeros((1, N), dtype=BF, device=dev())
        big = F.add_noise(x, sd, seed, off)
        small = torch.zeros((1, m), dtype=BF, device=dev())
        for k in (0, 2 ** 32 - m, 2 ** 32, N - m):
            assert (off + k // 4 < 2 ** 32) == (k < 2 ** 32)
            win = F.add_noise(small, sd, seed, off + k // 4)
            assert int((win != 0).sum()) > 0.9 * m
            assert torch.equal(big[:, k:k + m], win), f'window at element {k}'
        assert not torch.equal(big[:, 2 ** 32:2 ** 32 + m], big[:, :m]), 'the noise past element 2^32 repeats the first elements'
    finally:
        del x, big
        torch.cuda.empty_cache()


def test_subpixel_dgrad_refusal_and_what_functional_runs_in_its_place(monkeypatch):
    """subpix.hip:936 from above: one sample of the fine gy of exactly 2^31 bytes (32 channels at low 256 x 256 x 64).
    sg_upconv3d_subpixel_dgrad_supported says no, the entry point returns SG_EUNSUPPORTED, launches nothing and leaves gx alone;
    functional._upconv_dgrad, with the sub-pixel route allowed, then forms the gradient as the 2 x 2 x 2 block sum of the data
    gradient of the plain convolution.  There conv_fwd3w (conv3w.hip:902) and conv_fwd3s (conv3d.hip:1714) decline the pooled
    epilogue on a 2 GiB sample, so the full-resolution gradient is written by conv_fwd3r on its non-lean staging and summed by
    sg_downscale_sum: each of the two stores rounds once, and the boxes are compared with exactly that value."""
    from saragan_amd import functional as F
    from tests.test_conv_fwd_exact_gpu import _fwd_kernels, _garbage, _stream
    _lib, lib = _libs()
    b, c = SUBDG_ABOVE, SUBDG_ABOVE.c
    boxes = fallback_boxes(b)
    B.check_cover(fallback_layouts(b), boxes, c.sp, b.seam)
    W.assert_exact_range(9 * c.coef, c.coef, 27 * 8 * c.cout + 1)
    need = 2 ** 31 + 2 ** 32 + 2 * 2 ** 29 + 3 * PIECE      # gy, the full-resolution gradient, gx twice, one slab of each
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'{c.id} needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    monkeypatch.setattr(F, '_NO_SUBPIXEL', False)
    gy = gx = gx2 = None
    try:
        gy = _ncdhw(1, c.cout, c.out_sp(), BF)
        assert gy.numel() * 2 == 2 ** 31
        _fill_ints(gy.permute(0, 2, 3, 4, 1), 9900)
        w = W.int_data((3, 3, 3, c.cin, c.cout), 9901, F32).contiguous().to(dev())
        shp = _lib.ConvShape(1, *c.sp, c.cin, c.cout, 3, 3, 3, 0)
        assert not lib.sg_upconv3d_subpixel_dgrad_supported(C.byref(shp), _lib.SG_BF16)
        gx = _ncdhw(1, c.cin, c.sp, BF, SENTINEL)
        wp = _garbage(lib.sg_upconv3d_subpixel_dgrad_packed_bytes(C.byref(shp), _lib.SG_BF16))
        lib.sg_prof_enable(1)
        try:
            rc = lib.sg_upconv3d_subpixel_dgrad(gy.data_ptr(), wp.data_ptr(), gx.data_ptr(), C.byref(shp), _lib.SG_BF16, _stream())
            torch.cuda.synchronize()
            assert rc == _lib.SG_EUNSUPPORTED and _fwd_kernels(_lib, lib) == []
            assert bool((gx == SENTINEL).all()), 'a refused call wrote to gx'
            with torch.no_grad():
                gx = F._upconv_dgrad(gy, w, c.coef, True)
            torch.cuda.synchronize()
            names = _fwd_kernels(_lib, lib)
        finally:
            lib.sg_prof_enable(0)
        assert names == [c.kernel], names
        weff = w.double() * c.coef
        for box in boxes:
            n, d0, d1, h0, h1 = box
            # two kernels, two stores: the full-resolution gradient rounded once to bf16 by the convolution, then the block sum of those
            # eight stored values (exact in f32) rounded once by sg_downscale_sum
            a0, a1, b0, b1 = _low_halo(box, c.sp)
            full = R.conv_ref(gy[n:n + 1, :, 2 * a0:2 * a1, 2 * b0:2 * b1].cpu(), R.flip_transpose(weff.cpu()))
            ref = R.block_sum(R.expected(full, BF).double(), (2, 2, 2))[:, :, d0 - a0:d1 - a0, h0 - b0:h1 - b0]
            _assert_equal(f'{c.id} box {box}', gx[n:n + 1, :, d0:d1, h0:h1].cpu(), R.expected(ref, BF), 'gx')
        # the whole gx against the same two entry points (sg_conv3d_fwd with the flipped filter, then sg_downscale_sum: the last line
        # of _upconv_dgrad) on D slabs of gy with one low-resolution plane of halo, the halo planes dropped.  (_upconv_dgrad itself
        # would hand a slab to the sub-pixel kernel, which rounds once and so stores another value by design.)
        gx2 = _ncdhw(1, c.cin, c.sp, BF, SENTINEL)
        D, step = c.sp[0], 32
        with torch.no_grad():
            for s0 in range(0, D, step):
                s1 = min(s0 + step, D)
                a0, a1 = max(s0 - 1, 0), min(s1 + 1, D)
                part = F._Conv.apply(gy[:, :, 2 * a0:2 * a1], w, c.coef, True, False)
                assert part.numel() * 2 < PIECE
                gx2[:, :, s0:s1] = F._Down.apply(part, 1.0)[:, :, s0 - a0:s1 - a0]
                del part
        assert _same(gx.permute(0, 2, 3, 4, 1), gx2.permute(0, 2, 3, 4, 1)), f'{c.id}: the large call and the call on slabs differ'
    finally:
        del gy, gx, gx2
        F.mark_packs_stale()
        torch.cuda.empty_cache()


# ----------------------------------------------------------------------------------------------------------------------
# upconv_subpixel_wgrad (sg_upconv3d_subpixel_wgrad; subpix.hip:1062 / :1071, int64 off for x and gy) with the batch past 2^32
# bytes: 128 -> 64 at low (1, 4, 32), x dense, the fine gy zero except on the boxes.  Its own guard (subpix.hip:1200) is
# n d h w 8 cout < 2^40 elements, two terabytes of gy: no case can stand on either side of it.
# conv_small_wgrad under small.hip:437 (h w 32 4 < 2^31): a single image at the guard is 1 GiB, so the pair below / above the guard
# is run as a batch of five such images, which takes x past 2^31 bytes on the guarded kernel; above the guard the same batch
# falls to conv_wgrad2<1,3,3>.
# ----------------------------------------------------------------------------------------------------------------------
SUBW = _w('w_sub', 'upconv_subpixel_wgrad', 128, 64, (1, 4, 32), k=K333)


def subw_layouts():
    c = SUBW.c
    return [B.Layout('x', c.n, c.sp, c.cin, 2), B.Layout('gy', c.n, tuple(2 * v for v in c.sp), c.cout, 2, fine=(2, 2, 2))]


def _subw_n():
    c = SUBW.c
    c.n = B.smallest_batch(4 * 32 * c.cin * 2, 8 * 4 * 32 * c.cout * 2)
    return c.n


_subw_n()


def subw_boxes():
    return B.disjoint(B.choose_boxes(subw_layouts(), SUBW.c.sp, seam=SUBW.seam))


def test_subpixel_weight_gradient_is_exact_past_the_boundary():
    c = SUBW.c
    _lib, lib = _libs()
    lay, boxes = subw_layouts(), subw_boxes()
    B.check_cover(lay, boxes, c.sp, SUBW.seam)
    W.assert_exact_range(9, 1, 8 * B.box_voxels(boxes, c.sp[2]))
    need = sum(t.nbytes() for t in lay) + 2 ** 30
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f'{c.id} needs {need >> 20} MiB of device memory, {free >> 20} MiB are free')
    x = gy = None
    try:
        fine = lay[1].sp
        x = _ncdhw(c.n, c.cin, c.sp, BF)
        _fill_ints(x.permute(0, 2, 3, 4, 1), 9950)
        gy = _ncdhw(c.n, c.cout, fine, BF, 0.0)
        g = torch.Generator(device=dev()).manual_seed(9951)
        dw64, db64, parts = torch.zeros((3, 3, 3, c.cin, c.cout), dtype=torch.float64), torch.zeros(c.cout, dtype=torch.float64), []
        for box in boxes:
            n, d0, d1, h0, h1 = box
            v = torch.randint(-3, 4, (2 * (d1 - d0), 2 * (h1 - h0), fine[2], c.cout), generator=g, dtype=torch.int8, device=dev())
            gy[n, :, 2 * d0:2 * d1, 2 * h0:2 * h1] = v.permute(3, 0, 1, 2).to(BF)
            pw_, pb_ = B.upwgrad_box_reference(x, gy, box)
            assert bool(pw_.abs().sum() > 0) and all(not torch.equal(pw_, q) for q in parts), f'box {box}'
            parts.append(pw_)
            dw64 += pw_
            db64 += pb_
        shp = _lib.ConvShape(c.n, *c.sp, c.cin, c.cout, 3, 3, 3, 0)
        assert lib.sg_upconv3d_subpixel_wgrad_supported(C.byref(shp), _lib.SG_BF16)
        ws = WG._garbage(lib.sg_upconv3d_subpixel_wgrad_workspace(C.byref(shp), _lib.SG_BF16))
        dw, db = WG._outputs(c)
        lib.sg_prof_enable(1)
        try:
            rc = lib.sg_upconv3d_subpixel_wgrad(x.data_ptr(), gy.data_ptr(), dw.data_ptr(), db.data_ptr(), 0.25, ws.data_ptr(), ws.numel(),
                                                C.byref(shp), _lib.SG_BF16, WG._stream())
            torch.cuda.synchronize()
            names = WG._wgrad_kernels(_lib, lib)
        finally:
            lib.sg_prof_enable(0)
        _lib.check(rc, c.id)
        assert names == [c.kernel], names
        WG._check(c, dw, db, 0.25, dw64, db64)
    finally:
        del x, gy
        torch.cuda.empty_cache()
