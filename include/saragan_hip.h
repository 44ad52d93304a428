/*
 * saragan_hip.h -- C ABI of libsaragan_hip.so: the MI355X (gfx950) kernels behind the SURFGAN_3D
 * `pgan` generator + discriminator training step.
 *
 * The reference (sara-nl/saraGAN) has no FFI on this path: its boundary is Python calling TensorFlow-1
 * ops (SURFGAN_3D/networks/ops.py).  Each entry point below replaces the TF op(s) named in its
 * comment; INTEGRATION.md shows the ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C: pointers, sizes and small POD structs only; no torch / HIP types in signatures
 *    (`sg_stream_t` is a hipStream_t passed as void*; NULL = the default stream);
 *  - every buffer is caller-owned DEVICE memory; no entry point allocates, frees or synchronises;
 *    kernels are enqueued on the stream given; entry points are re-entrant.  Process-wide state is limited to the
 *    opt-in profiler (sg_prof_*), an immutable snapshot of the SG_* diagnostic environment switches taken at
 *    the first launch (sg_config_reload) and the one-time registration of each kernel's LDS size;
 *  - activations are NDHWC (channels-last 3-D): element (n,d,h,w,c) at (((n*D+d)*H+h)*W+w)*C+c.
 *    A 2-D image batch is D == 1.  dtype SG_F32 or SG_BF16 (storage AND MFMA input type; accumulation
 *    is always f32);
 *  - weights stay in the reference's layouts: conv DHWIO [kD][kH][kW][Cin][Cout] f32
 *    (networks/ops.py:148), dense [in][out] f32 (networks/ops.py:142); the equalised-LR runtime
 *    coefficient (networks/ops.py:111-122) is an argument, applied when packing;
 *  - return value: 0 on success, a negative SG_E* code for bad arguments, or a positive hipError_t.
 */
#ifndef SARAGAN_HIP_H
#define SARAGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* sg_stream_t;

typedef enum { SG_F32 = 0, SG_BF16 = 1 } sg_dtype;

enum {
  SG_OK = 0,
  SG_EINVAL = -1,      /* bad shape / null pointer / unsupported combination */
  SG_EWORKSPACE = -2,  /* workspace too small */
  SG_EALIGN = -3,      /* pointer not 16-byte aligned */
  SG_EUNSUPPORTED = -4 /* valid request that no kernel of this build covers (sub-pixel epilogue on a small layer): the
                          caller falls back to the plain formulation */
};

/* Geometry of one stride-1 'SAME' convolution (tf.nn.conv3d at networks/ops.py:150).
 * (d,h,w) is the OUTPUT extent.  If `upsample_in` != 0 the input tensor is half resolution
 * ((d/2,h/2,w/2), all even) and is read through a nearest-neighbour x2 gather, i.e. the kernel
 * computes conv3d(upscale3d(x)) (networks/ops.py:276-289 + :147-150) without materialising it. */
typedef struct {
  int32_t n, d, h, w;
  int32_t cin, cout;
  int32_t kd, kh, kw; /* odd */
  int32_t upsample_in;
} sg_conv_shape;

/* Epilogue fused into sg_conv3d_fwd (apply_bias + act + pixel_norm: networks/ops.py:130-136,167-192,308-310).
 * struct_size MUST be sizeof(sg_conv_epilogue) of the header the caller was built against: the library rejects any
 * other value with SG_EINVAL instead of reading past a shorter (older) struct. */
typedef struct {
  uint32_t struct_size;
  const float* bias;   /* [cout] or NULL */
  int32_t act;         /* 0 = linear, 1 = leaky_relu */
  float slope;         /* leaky_relu negative slope */
  int32_t pixel_norm;  /* 1: y *= rsqrt(mean_c(y^2)+eps); requires cout <= 128 */
  float eps;
  float* pn_scale;     /* optional [n*d*h*w] f32: the per-voxel rsqrt factor (saved for backward) */
  const void* mask_bits; /* optional sign words (layout below) of a tensor shaped like y: y *= (bit ? mask_slope : 1),
                            applied last.  Fuses the LeakyReLU backward of the layer whose output gradient this
                            data-gradient convolution produces (networks/ops.py:175-178: dx = where(y >= 0, dy,
                            dy*alpha)) into the convolution. */
  float mask_slope;
  void* sign_out;        /* optional: receives the sign words of y (after bias + act) for a later mask_bits */
  /* Sub-pixel form of conv3d(upscale3d(x)) (networks/ops.py:276-289 + :147-150): the output voxels of one parity class
   * (2i+a, 2j+b, 2k+c) are a 2x2x2-tap convolution of the LOW-resolution input with summed weights (27 -> 8 taps,
   * 3.4x fewer FLOPs).  A launch with kd = kh = kw = 2 computes one class: out_scale = 2 makes y the full-resolution
   * tensor [n,2d,2h,2w,cout] (pn_scale / sign words likewise) written at the voxels of class out_off; tap t of a
   * dimension reads input offset t - 1 + tap_off (tap_off = parity: taps {-1,0} for even, {0,+1} for odd outputs).
   * All zero: the ordinary convolution. */
  int32_t out_scale;
  int32_t out_off[3];
  int32_t tap_off[3];
  /* pool = 1: y is NOT the full-resolution output but its mean over 2 (D) x 1 (H) x 2 (W) blocks, [n, d/2, h, w/2, cout]
   * -- the first stage of downscale3d(act(conv3d(x) + b)) (pgan/discriminator.py:39-44), finished by
   * sg_downscale_sum(1,2,1, gain 1/2).  sign_out still receives the FULL-resolution sign words (all the backward
   * needs).  Only the sliding-halo kernel implements it (bf16, 3x3x3, cin <= 32, w % 32 == 0, cout % 32 == 0, even
   * d and h, no pixel-norm; mask_bits only without bias / activation / sign_out and with 32 input channels: the block means
   * of M * conv(x), the double backward of such a layer): anything else returns SG_EUNSUPPORTED and the caller runs conv +
   * downscale.
   * pool = 2: the mean over 1 (D) x 2 (H) x 2 (W) blocks instead, [n, d, h/2, w/2, cout], finished by
   * sg_downscale_sum(2,1,1, gain 1/2): the streamed ping-pong kernel's tile (bf16, 3x3x3, cin % 16 == 0, cout % 64 == 0,
   * even h and w, no pixel-norm / mask), for the layers with more than 32 input channels.  With act = 0 and no bias
   * either mode is the block mean of a plain convolution (the gradient of conv3d(upscale3d(x)), 8 x the mean).
   * pool = 3: the mean over whole 2 x 2 x 2 blocks, [n, d/2, h/2, w/2, cout] -- downscale3d finished inside the epilogue, no
   * second pass (32 input channels, even d / h / w, otherwise as pool = 1; SG_EUNSUPPORTED elsewhere: use pool = 1). */
  int32_t pool;
  /* Optional scratch for layers the library computes in two passes over halves of the input channels (64 -> 32 at
   * 3x3x3, bf16: f32 partial sums of the first half, n*d*h*w*cout*4 bytes, 16-byte aligned, contents irrelevant on
   * entry).  NULL: such layers run as one pass of the streamed kernel.  sg_conv3d_fwd_workspace() gives the size. */
  void* workspace;
  size_t workspace_bytes;
  /* 0: x is one NDHWC tensor of cin channels.  32: x is cin / 32 separate NDHWC tensors of 32 channels each, one after
   * the other (what sg_upscale_nn_planes writes).  The two passes of a 64 -> 32 layer (see workspace) then read whole
   * 64-byte rows instead of one half of every 128-byte row -- a half row costs the whole line from HBM.  Only that
   * path reads the layout: anything else returns SG_EUNSUPPORTED. */
  int32_t x_plane_channels;
  /* Pixel-norm backward in the epilogue of a DATA-GRADIENT convolution: the convolution's result is the gradient g for the
   * output y = pixel_norm(leaky_relu(z + b)) of a generator stage (pgan/generator.py:33-45); with pn_bwd_y = y [n,d,h,w,cout]
   * and pn_bwd_scale = the stage's rsqrt factor [n*d*h*w] the epilogue turns it into the gradient for z,
   * mask_bits(y's sign words) * pn_bwd_scale * (g - y * mean_c(g * y)), before it is written (what sg_pixel_norm_act_bwd
   * computes in a pass of its own).  Needs mask_bits, cout == 32, the sliding-halo kernel's shapes (bf16, 3x3x3,
   * cin <= 32, w % 32 == 0), no bias / activation / pooling; otherwise SG_EUNSUPPORTED.  Both NULL: off. */
  const void* pn_bwd_y;
  const float* pn_bwd_scale;
  /* Masked nearest up-scale of the INPUT in the gather (with s->upsample_in = 1): the convolution reads
   * in_gain * where(bit, in_mask_slope, 1) * upscale3d(x) instead of upscale3d(x); in_mask_bits are the sign words of a
   * tensor of the FINE shape [n,d,h,w,cin] (ceil(cin/32) words per voxel).  This is the gradient of
   * downscale3d(leaky_relu(.)) (pgan/discriminator.py:39-44 backward: networks/ops.py:265-273 then :175-178, gain 1/8)
   * formed while the halo is staged, so the full-resolution gradient -- 8 x the bytes of x -- is never written.  Values are
   * rounded to the storage type exactly as sg_upscale2x_masked rounds them; in_gain must be a power of two (1/8 for downscale3d).  Implemented by the two-pass 64 -> 32 path
   * (see workspace; bf16, 3x3x3, even d/h/w, w % 32 == 0): anything else returns SG_EUNSUPPORTED.  NULL: off. */
  const void* in_mask_bits;
  float in_mask_slope;
  float in_gain;
  /* to_rgb (networks/ops.py:239-240, pgan/generator.py:96-97: a 1x1x1 convolution to ONE image channel) of this convolution's
   * output inside its epilogue: rgb_out[n,d,h,w,1] = sum_c y[..,c] * rgb_w[c] + rgb_bias[0] with y as it is stored (rounded to dt)
   * and rgb_w the [cout] f32 values to_rgb's forward multiplies with -- the full-resolution stage output is not read again for the
   * image.  With pixel_norm + act + sign_out, cout == 32, the 32-input-channel 3x3x3 kernel's shapes (bf16, w % 32 == 0);
   * otherwise SG_EUNSUPPORTED (run sg_conv3d_fwd on y).  rgb_out NULL: off. */
  const float* rgb_w;
  const float* rgb_bias;
  void* rgb_out;
  /* from_rgb's WHOLE backward (networks/ops.py:243-247, pgan/discriminator.py:9-12: 1x1x1 from ONE image channel, bias, LeakyReLU)
   * in the epilogue of the data-gradient convolution that produces the gradient g of its output (mask_bits = from_rgb's sign
   * words): pw_dx[n,d,h,w,1] = sum_c g_c * pw_wmat[c] (optional), pw_dw[c] = pw_coef * sum_v pw_x[v] * g[v][c], pw_dbias[c] =
   * sum_v g[v][c] (each optional), g as it would have been stored (rounded to dt) -- and y is NOT written (y may be NULL): the
   * 32-channel gradient, the largest tensor of the discriminator's backward, is needed by nobody else.  workspace must hold
   * sg_conv3d_pw_epilogue_workspace() bytes (per-wave partial sums, added in a fixed order).  Same kernel and shapes as rgb_*
   * (cout == 32, no bias / activation / pooling); otherwise SG_EUNSUPPORTED (run the convolution, then sg_conv3d_pw_bwd).
   * pw_x NULL: off. */
  const void* pw_x;
  const float* pw_wmat;
  void* pw_dx;
  float* pw_dw;
  float* pw_dbias;
  float pw_coef;
} sg_conv_epilogue;

/* Sign words of an NDHWC tensor t[nvox][c]: uint32 words[nvox][ceil(c/32)], bit j of word (v, k) = (t[v][32k+j] < 0),
 * bits of channels >= c are 0.  One bit per element instead of re-reading the bf16/f32 activation in backward. */
size_t sg_sign_words_bytes(int64_t nvox, int32_t c);
int sg_sign_words(const void* t, void* words, int64_t nvox, int32_t c, sg_dtype dt, sg_stream_t st);

const char* sg_version(void);
const char* sg_error_string(int code);

/* ---- conv3d / dense (networks/ops.py:139-150) -------------------------------------------------- */
/* Bytes of the MFMA-fragment-ordered weight image sg_conv3d_pack_weights writes. */
size_t sg_conv3d_packed_bytes(const sg_conv_shape* s, sg_dtype dt);
/* wp <- coef * w, cast to dt, in fragment order.  transpose_flip != 0 packs the weights of the
 * data-gradient convolution instead: w is then [kD][kH][kW][s->cout][s->cin] and is mirrored in
 * (kD,kH,kW) and transposed in (I,O) (what tf's Conv3DBackpropInputV2 computes for stride 1). */
int sg_conv3d_pack_weights(const float* w_dhwio, float coef, int transpose_flip, void* wp,
                           const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
/* The images of n layers at once -- what n calls of sg_conv3d_pack_weights write, the fragment images in one launch per 56
 * layers.  After an optimiser step (optimization.py:16-73: every variable of the network moves) all of a network's images are
 * stale together; w / coef / transpose_flip / wp / shapes are host arrays of n entries. */
int sg_conv3d_pack_weights_batch(int n, const float* const* w_dhwio, const float* coef, const int* transpose_flip,
                                 void* const* wp, const sg_conv_shape* shapes, sg_dtype dt, sg_stream_t st);
/* Bytes of sg_conv_epilogue.workspace that let this shape take its fastest path (0: none needed). */
size_t sg_conv3d_fwd_workspace(const sg_conv_shape* s, sg_dtype dt);
size_t sg_conv3d_pw_epilogue_workspace(void);     /* bytes of sg_conv_epilogue.workspace for the pw_* epilogue */
/* y = epilogue(conv3d(x, wp)).  x: [n,d,h,w,cin] (or half-res if upsample_in), y: [n,d,h,w,cout]. */
int sg_conv3d_fwd(const void* x, const void* wp, void* y, const sg_conv_shape* s,
                  const sg_conv_epilogue* ep, sg_dtype dt, sg_stream_t st);
/* conv3d(upscale3d(x)) (networks/ops.py:276-289 followed by :147-150; pgan/generator.py:49-57) in sub-pixel form, ONE
 * launch for all eight parity classes: 64 instead of 216 tap products per low-resolution voxel.  `s` is the LOW-resolution
 * shape (n, d, h, w, cin, cout; kd = kh = kw = 3 of the original convolution, upsample_in ignored); x: [n,d,h,w,cin],
 * y: [n,2d,2h,2w,cout].  wp comes from sg_upconv3d_subpixel_pack (the summed weights of the 8 classes, coef applied, in
 * fragment order; sg_upconv3d_subpixel_packed_bytes bytes).  Epilogue: bias, act / slope, pixel_norm (cout 32 or 64) with
 * pn_scale, sign_out; anything else, f32, or a shape that does not tile (256 low-resolution voxels per tile; cin % 16,
 * cout % 32): SG_EUNSUPPORTED -- run sg_conv3d_fwd with upsample_in = 1. */
int sg_upconv3d_subpixel_supported(const sg_conv_shape* s, sg_dtype dt);   /* 1 if the shape tiles (no launch, no GPU needed) */
size_t sg_upconv3d_subpixel_packed_bytes(const sg_conv_shape* s, sg_dtype dt);
int sg_upconv3d_subpixel_pack(const float* w_dhwio, float coef, void* wp, const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
int sg_upconv3d_subpixel_fwd(const void* x, const void* wp, void* y, const sg_conv_shape* s, const sg_conv_epilogue* ep,
                             sg_dtype dt, sg_stream_t st);
/* Weight (and bias) gradient of conv3d(upscale3d(x)) in the same sub-pixel form: 64 accumulator tiles per (cin, cout) tile
 * pair instead of 8 x 27 tap products per low-resolution voxel, folded to the 27-tap gradient at the end.  `s`: the
 * LOW-resolution shape; x: [n,d,h,w,cin], gy: [n,2d,2h,2w,cout]; dw: [3][3][3][cin][cout] f32 = coef * gradient, dbias: [cout]
 * or NULL.  bf16, w % 32 == 0, even h, cin and cout multiples of 32; otherwise SG_EUNSUPPORTED (run sg_conv3d_wgrad_bias
 * with upsample_in = 1). */
int sg_upconv3d_subpixel_wgrad_supported(const sg_conv_shape* s, sg_dtype dt);
size_t sg_upconv3d_subpixel_wgrad_workspace(const sg_conv_shape* s, sg_dtype dt);
int sg_upconv3d_subpixel_wgrad(const void* x, const void* gy, float* dw_dhwio, float* dbias, float coef, void* workspace,
                               size_t workspace_bytes, const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
/* Data gradient of conv3d(upscale3d(x)) (what tf.gradients delivers for x at pgan/generator.py:33-34) in the same form: a
 * stride-2 convolution of the fine gradient with 4 x 4 x 4 taps whose weights are the forward's summed sets transposed, 64 tap
 * products per low-resolution voxel instead of the 216 of the 27-tap data gradient followed by the 2x2x2 block sum, rounded
 * once.  `s`: the LOW-resolution shape (cin = channels of x and gx, cout = channels of gy); gy: [n,2d,2h,2w,cout],
 * gx: [n,d,h,w,cin]; w_dhwio is the FORWARD weight [3][3][3][cin][cout].  bf16, cin % 64 == 0, cout % 16 == 0, the tiles of the
 * forward kernel with 32- or 16-wide rows; otherwise SG_EUNSUPPORTED (run sg_conv3d_fwd with transposed weights and
 * sg_conv_epilogue.pool, then sg_downscale_sum). */
int sg_upconv3d_subpixel_dgrad_supported(const sg_conv_shape* s, sg_dtype dt);
size_t sg_upconv3d_subpixel_dgrad_packed_bytes(const sg_conv_shape* s, sg_dtype dt);
int sg_upconv3d_subpixel_dgrad_pack(const float* w_dhwio, float coef, void* wp, const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
int sg_upconv3d_subpixel_dgrad(const void* gy, const void* wp, void* gx, const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
/* dw[kD][kH][kW][cin][cout] (f32) = coef * sum_v x[v+tap] (x) dy[v]   (tf Conv3DBackpropFilterV2).
 * workspace: sg_conv3d_wgrad_workspace() bytes, contents irrelevant on entry. */
size_t sg_conv3d_wgrad_workspace(const sg_conv_shape* s, sg_dtype dt);
int sg_conv3d_wgrad(const void* x, const void* dy, float* dw_dhwio, float coef, void* workspace,
                    size_t workspace_bytes, const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
/* Same, and dbias[cout] (f32, overwritten) = sum_v dy[v]: the gradient of apply_bias (networks/ops.py:130-136)
 * from the pass that reads dy anyway. */
int sg_conv3d_wgrad_bias(const void* x, const void* dy, float* dw_dhwio, float* dbias, float coef, void* workspace,
                         size_t workspace_bytes, const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
/* The same for one discriminator block's pooled tail, downscale3d(leaky_relu(conv3d(x) + b)) (pgan/discriminator.py:39-44):
 * dy_half [n, d/2, h/2, w/2, cout] is the gradient of the POOLED output; the gradients are taken against
 * dy_gain * where(bit, mask_slope, 1) * upscale3d(dy_half) -- networks/ops.py:265-273 backward (dy_gain = 1/8) followed by
 * :175-178 with the layer's sign words mask_bits [n*d*h*w][cout/32] -- formed while each tile is staged, with the rounding
 * of sg_upscale2x_masked (dy_gain: a power of two), so the full-resolution gradient is never written.  s is the FINE shape.  bf16, 3x3x3,
 * cout % 32 == 0, even d/h/w, w % 32 == 0 and the sliding-halo kernel's tile: otherwise SG_EUNSUPPORTED.  Same workspace
 * as sg_conv3d_wgrad_bias. */
int sg_conv3d_wgrad_bias_up_masked(const void* x, const void* dy_half, const void* mask_bits, float mask_slope, float dy_gain,
                                   float* dw, float* dbias, float coef, void* workspace, size_t workspace_bytes,
                                   const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
/* sg_conv3d_wgrad_bias (mask_bits == NULL) / sg_conv3d_wgrad_bias_up_masked (mask_bits != NULL) with options:
 * SG_WGRAD_ACCUMULATE: dw_dhwio += coef * sum -- the weights are used more than once in the graph a training step
 *   differentiates (the discriminator under WGAN-GP: networks/loss.py:136-140 differentiates D a second time,
 *   optimization.py:128-163 asks for one gradient per variable) and the parameter's gradient buffer already holds the other
 *   contribution.  The sum is rounded to f32 before it is added: the value tf.gradients' add_n of the two finished gradients
 *   has.  dbias (optional) is WRITTEN, not added to.
 * SG_WGRAD_CLEAN_WORKSPACE: the caller keeps the workspace between calls; its first sg_conv3d_wgrad_clean_bytes(s, dt) bytes are
 *   zero on entry and are left zero (the finalize pass clears what it reads), and the call launches no memset.  (A failed
 *   call leaves the workspace undefined: clear it before the next use.)
 * SG_EUNSUPPORTED, with nothing touched, where the layer runs on the pointwise (<= 4 channels on one side) or the small-channel
 * (<= 16, 2-D top levels) kernels. */
#define SG_WGRAD_ACCUMULATE 1u
#define SG_WGRAD_CLEAN_WORKSPACE 2u
int sg_conv3d_wgrad_bias_ex(const void* x, const void* dy, const void* mask_bits, float mask_slope, float dy_gain,
                            float* dw_dhwio, float* dbias, float coef, unsigned flags, void* workspace, size_t workspace_bytes,
                            const sg_conv_shape* s, sg_dtype dt, sg_stream_t st);
size_t sg_conv3d_wgrad_clean_bytes(const sg_conv_shape* s, sg_dtype dt);

/* Whole backward of a pointwise convolution FROM cin <= 4 channels (from_rgb, pgan/discriminator.py:9-12) in one pass over
 * dy: dw, dbias as sg_conv3d_wgrad_bias, and dx[n,d,h,w,cin] = sum_c dy[..,c] * w_mat[j][c] (w_mat: [cin][cout] f32, the
 * values the forward multiplied with).  cout at most 64 sixteen-byte pieces (512 channels in bf16, 256 in f32: a voxel's
 * lanes add their parts of dx within one wave).  Other shapes: SG_EUNSUPPORTED, nothing touched (run sg_conv3d_fwd +
 * sg_conv3d_wgrad_bias). */
int sg_conv3d_pw_bwd(const void* x, const void* dy, const float* w_mat, float* dw_dhwio, float* dbias, void* dx,
                     float coef, void* workspace, size_t workspace_bytes, const sg_conv_shape* s, sg_dtype dt,
                     sg_stream_t st);

/* ---- elementwise / reductions over NDHWC -------------------------------------------------------- */
/* y = act(x + bias[c])                       (apply_bias + act, networks/ops.py:130-136,185-192) */
int sg_bias_act_fwd(const void* x, const float* bias, void* y, int64_t nvox, int32_t c, int32_t act,
                    float slope, sg_dtype dt, sg_stream_t st);
/* dx = (y >= 0 ? dy : slope*dy) (mask from the OUTPUT, networks/ops.py:177); y == NULL: dx = dy.
 * dbias (optional, [c] f32, overwritten) = sum_v dx.  workspace >= sg_bias_act_bwd_workspace(c). */
size_t sg_bias_act_bwd_workspace(int32_t c);
int sg_bias_act_bwd(const void* dy, const void* y, void* dx, float* dbias, void* workspace, int64_t nvox,
                    int32_t c, float slope, sg_dtype dt, sg_stream_t st);
/* Same with the mask taken from the sign words of y (sg_sign_words / sg_conv_epilogue.sign_out). */
int sg_bias_act_bwd_bits(const void* dy, const void* y_sign_words, void* dx, float* dbias, void* workspace,
                         int64_t nvox, int32_t c, float slope, sg_dtype dt, sg_stream_t st);
/* y = x * rsqrt(mean_c(x^2) + eps); scale (optional, [nvox] f32) receives the rsqrt factor.
 * (pixel_norm, networks/ops.py:308-310) */
int sg_pixel_norm_fwd(const void* x, void* y, float* scale, int64_t nvox, int32_t c, float eps,
                      sg_dtype dt, sg_stream_t st);
/* dx = scale * (dy - y * mean_c(dy*y)),  y = forward OUTPUT, scale = forward rsqrt factor. */
int sg_pixel_norm_bwd(const void* dy, const void* y, const float* scale, void* dx, int64_t nvox,
                      int32_t c, sg_dtype dt, sg_stream_t st);
/* Gradient of y = pixel_norm(leaky_relu(z + b)) (one generator stage, pgan/generator.py:49-71) in one pass:
 * dz = mask(sign words of y) * pixel_norm_bwd(dy), dbias (optional, [c] f32) = sum_v dz.
 * workspace >= sg_bias_act_bwd_workspace(c) when dbias is given. */
int sg_pixel_norm_act_bwd(const void* dy, const void* y, const float* scale, const void* y_sign_words, float slope,
                          void* dz, float* dbias, void* workspace, int64_t nvox, int32_t c, sg_dtype dt,
                          sg_stream_t st);
/* The same when dy is the data gradient of a pointwise convolution to cs <= 4 channels (to_rgb of the stage's output,
 * pgan/generator.py:13-16,96-97): dy[v][c] = sum_j g_small[v][j] * w_small[j][c] is formed in registers from
 * g_small [nvox][cs] and w_small [cs][c] (f32, the values the forward multiplied with) instead of being written and read
 * back.  c a multiple of the 16-byte piece, c <= 512 (bf16) / 256 (f32); otherwise SG_EUNSUPPORTED. */
int sg_pixel_norm_act_bwd_pw(const void* g_small, int32_t cs, const float* w_small, const void* y, const float* scale,
                             const void* y_sign_words, float slope, void* dz, float* dbias, void* workspace,
                             int64_t nvox, int32_t c, sg_dtype dt, sg_stream_t st);
/* The same pass also returning the pointwise convolution's OWN gradients (to_rgb's filter and bias, pgan/generator.py:13-16), which
 * need exactly the two tensors it reads: dw_small [c][cs] (a [1,1,1,c,cs] filter) = coef_small * sum_v y[v][ch] * g_small[v][j],
 * db_small [cs] = sum_v g_small[v][j] -- instead of another pass over y (sg_conv3d_wgrad_bias: 1.07 GB at the benchmarked size).
 * dbias, dw_small, db_small: each optional.  cs == 1; otherwise SG_EUNSUPPORTED.  workspace >= sg_pixel_norm_act_bwd_pw_wg_workspace(c, cs). */
size_t sg_pixel_norm_act_bwd_pw_wg_workspace(int32_t c, int32_t cs);
int sg_pixel_norm_act_bwd_pw_wg(const void* g_small, int32_t cs, const float* w_small, const void* y, const float* scale,
                                const void* y_sign_words, float slope, void* dz, float* dbias, float* dw_small, float* db_small,
                                float coef_small, void* workspace, size_t workspace_bytes, int64_t nvox, int32_t c, sg_dtype dt,
                                sg_stream_t st);
/* y[n,2d,2h,2w,c] = gain * x[n,d,h,w,c] nearest-neighbour    (upscale3d / avg_unpool3d, ops.py:250-262) */
int sg_upscale2x(const void* x, void* y, int32_t n, int32_t d, int32_t h, int32_t w, int32_t c,
                 float gain, sg_dtype dt, sg_stream_t st);
/* Same with a fused LeakyReLU backward: y *= (bit ? mask_slope : 1), mask_bits = sign words of a tensor shaped like
 * y.  This is the gradient of `downscale3d(leaky_relu(.))` (pgan/discriminator.py:39-44) in one pass. */
int sg_upscale2x_masked(const void* x, void* y, const void* mask_bits, float mask_slope, int32_t n, int32_t d,
                        int32_t h, int32_t w, int32_t c, float gain, sg_dtype dt, sg_stream_t st);
/* y[n,d/2,h/2,w/2,c] = gain * sum of the 2x2x2 block; gain = 1/8 is downscale3d (ops.py:265-273),
 * gain = 1 is the gradient of upscale3d (ops.py:284).  (d,h,w) = INPUT extent, all even. */
int sg_downscale2x(const void* x, void* y, int32_t n, int32_t d, int32_t h, int32_t w, int32_t c,
                   float gain, sg_dtype dt, sg_stream_t st);
/* The same two operations with a factor of 1 or 2 PER DIMENSION (fd, fh, fw): (1,2,2) are upscale2d / downscale2d of the
 * 2-D tree on D == 1 tensors (SURFGAN_2D/networks/ops.py:176-231); (1,2,1) finishes a D x W-pooled convolution output.
 * sg_upscale_nn: x [n,d,h,w,c] -> y [n,d*fd,h*fh,w*fw,c], optional sign-word mask of a tensor shaped like y.
 * sg_upscale_nn_planes: the same values, y written as c / plane_channels separate NDHWC tensors of plane_channels
 * channels each, back to back (sg_conv_epilogue.x_plane_channels; 16-byte channel pieces, rows of >= 128 pieces).
 * sg_downscale_sum: x [n,d,h,w,c] (INPUT extent, divisible by the factors) -> y [n,d/fd,h/fh,w/fw,c] = gain * block sum. */
int sg_upscale_nn(const void* x, void* y, const void* mask_bits, float mask_slope, int32_t n, int32_t d, int32_t h,
                  int32_t w, int32_t c, int32_t fd, int32_t fh, int32_t fw, float gain, sg_dtype dt, sg_stream_t st);
int sg_upscale_nn_planes(const void* x, void* y, const void* mask_bits, float mask_slope, int32_t n, int32_t d, int32_t h,
                         int32_t w, int32_t c, int32_t fd, int32_t fh, int32_t fw, float gain, int32_t plane_channels,
                         sg_dtype dt, sg_stream_t st);
int sg_downscale_sum(const void* x, void* y, int32_t n, int32_t d, int32_t h, int32_t w, int32_t c, int32_t fd,
                     int32_t fh, int32_t fw, float gain, sg_dtype dt, sg_stream_t st);
/* The same over M * x, M = where(sign bit, mask_slope, 1) from sign words shaped like x [n*d*h*w][ceil(c/32)]: the
 * gradient of sg_upscale_nn with a mask (networks/ops.py:175-178 composed with :265-273) in one pass. */
int sg_downscale_sum_masked(const void* x, const void* mask_bits, float mask_slope, void* y, int32_t n, int32_t d, int32_t h,
                            int32_t w, int32_t c, int32_t fd, int32_t fh, int32_t fw, float gain, sg_dtype dt, sg_stream_t st);
/* Trilinear x2 up-sampling with half-pixel centres (`align_corners=False`; BASELINE north_star names a trilinear
 * resampler, the reference itself only has the nearest one): adjoint == 0: x [n,d,h,w,c] -> y [n,2d,2h,2w,c];
 * adjoint != 0: the gradient, x = dy [n,2d,2h,2w,c] -> y = dx [n,d,h,w,c] ((d,h,w) is always the LOW-resolution
 * extent).  Trilinear x2 down-sampling with half-pixel centres is the 2x2x2 mean: sg_downscale2x(gain 1/8). */
int sg_trilinear_up2x(const void* x, void* y, int32_t n, int32_t d, int32_t h, int32_t w, int32_t c, int32_t adjoint,
                      sg_dtype dt, sg_stream_t st);
/* out = wa*a + wb*b     (fade-in lerp pgan/generator.py:100-101, pgan/discriminator.py:105; b may be NULL) */
int sg_axpby(const void* a, const void* b, void* out, float wa, float wb, int64_t numel, sg_dtype dt,
             sg_stream_t st);
/* The same with the coefficients read from DEVICE memory, out = w[0]*a + w[1]*b (b NULL: w[0]*a, w[1] is not read): the
 * fade-in of a step captured as a hipGraph, whose alpha moves every step (networks/ops.py:4-23, optuna_objective.py:446-467:
 * the reference feeds alpha as a graph variable too).  Same f32 arithmetic as sg_axpby. */
int sg_axpby_dev(const void* a, const void* b, void* out, const float* w, int64_t numel, sg_dtype dt, sg_stream_t st);
/* out[s][i] = gamma[s]*a[s][i] + (1-gamma[s])*b[s][i], one f32 DEVICE weight per batch sample, f32 arithmetic, one rounding:
 * the gradient penalty's interpolates `gamma*real + (1-gamma)*fake` (networks/loss.py:70-71, :133-134). */
int sg_lerp_rows(const void* a, const void* b, const float* gamma, void* out, int32_t n, int64_t per_sample, sg_dtype dt,
                 sg_stream_t st);
/* out = x + stddev * N(0,1), counter-based Philox4x32-10 keyed by (seed, element index)
 * (instance noise, networks/loss.py:122-123). */
int sg_add_noise(const void* x, void* out, float stddev, uint64_t seed, uint64_t offset, int64_t numel,
                 sg_dtype dt, sg_stream_t st);
/* The same with the Philox offset read from DEVICE memory (one uint64) and, after the launch, advanced by `bump` on the
 * device: a captured hipGraph of the training step (SARAGAN_HIPGRAPH=1) draws fresh instance noise at every replay. */
int sg_add_noise_dev(const void* x, void* out, float stddev, uint64_t seed, uint64_t* offset_dev, uint64_t bump,
                     int64_t numel, sg_dtype dt, sg_stream_t st);
/* out[n*w_extent + w] = sum_{d,h,c} g[n,d,h,w,c]^2   (the reduce_sum of networks/loss.py:140, quirk Q1:
 * axes (1,2,3) of NCDHW = c,d,h).  out f32 [n*w], overwritten. */
int sg_sumsq_ndhwc_keep_w(const void* g, float* out, int32_t n, int32_t d, int32_t h, int32_t w, int32_t c,
                          sg_dtype dt, sg_stream_t st);
/* minibatch_stddev_layer (networks/ops.py:313-325): y[n,d,h,w,c+1] = concat(x, stat[n % (n/group)]) with
 * stat[m] = mean_{c,d,h,w} sqrt(var_group(x) + 1e-8), group = min(group_size, n), n % group == 0.
 * workspace: (n/group) floats. */
int sg_minibatch_stddev_fwd(const void* x, void* y, float* workspace, int32_t n, int64_t vox_per_sample,
                            int32_t c, int32_t group_size, sg_dtype dt, sg_stream_t st);
/* Its gradient: dx[n,d,h,w,c] from dy[n,d,h,w,c+1] and the forward input x (same workspace size). */
int sg_minibatch_stddev_bwd(const void* dy, const void* x, void* dx, float* workspace, int32_t n,
                            int64_t vox_per_sample, int32_t c, int32_t group_size, sg_dtype dt, sg_stream_t st);
/* Minibatch standard deviation as a per-sample statistic, twice differentiable (csrc/mbstd.hip).  The batch is
 * `nseg` consecutive sub-batches of n / nseg samples; inside each, G = min(group_size, n / nseg), M = (n / nseg) / G and group m
 * holds the samples g * M + m (the reshape of networks/ops.py:317).  P = c * vox_per_sample; per position i of a group:
 * mu_i the group mean, d_gi = x_gi - mu_i, sigma_i = sqrt(mean_g d_gi^2 + 1e-8).  x is NDHWC (any c, any alignment), all
 * arithmetic f32, every sum in a fixed order (no float atomics).  SG_EINVAL before any launch: a NULL pointer, n % nseg != 0,
 * (n / nseg) % G != 0, a workspace smaller than sg_mbstd_stat_workspace().
 *   fwd  (2 launches): stat[n] (f32, every sample of a group holds the same value) = (1/P) sum_i sigma_i
 *   bwd  (1 launch):   dx_gi = S / (P G) * d_gi / sigma_i,  S = sum of gstat over the group's samples
 *   bwd2 (<= 2 launches): h the cotangent of dx (shaped and typed like x);
 *        ggstat[n] (f32, per sample of the group) = (1 / (P G)) sum_{g,i} h_gi d_gi / sigma_i
 *        gx_gi = S / (P G) * [(h_gi - hbar_i) / sigma_i - d_gi (sum_g' h_g'i d_g'i) / (G sigma_i^3)],  hbar_i = mean_g h_gi
 *        gx or ggstat may be NULL (not both): that output is not computed. */
size_t sg_mbstd_stat_workspace(int32_t n, int64_t vox_per_sample, int32_t c, int32_t group_size, int32_t nseg);
int sg_mbstd_stat_fwd(const void* x, float* stat, float* workspace, size_t workspace_bytes, int32_t n, int64_t vox_per_sample,
                      int32_t c, int32_t group_size, int32_t nseg, sg_dtype dt, sg_stream_t st);
int sg_mbstd_stat_bwd(const float* gstat, const void* x, void* dx, int32_t n, int64_t vox_per_sample, int32_t c,
                      int32_t group_size, int32_t nseg, sg_dtype dt, sg_stream_t st);
int sg_mbstd_stat_bwd2(const void* h, const void* x, const float* gstat, void* gx, float* ggstat, float* workspace,
                       size_t workspace_bytes, int32_t n, int64_t vox_per_sample, int32_t c, int32_t group_size, int32_t nseg,
                       sg_dtype dt, sg_stream_t st);
/* The rank-1 term a per-sample constant channel adds to the SAME-padded convolution after it: with B f32 [plane]
 * (plane = voxels * cout of the convolution's output, NDHWC order) and s f32 [n], one launch each:
 *   term_fwd:   out[n][j] = y[n][j] + s[n] * B[j]   (f32 add, one rounding to dt; y NULL: the outer product alone)
 *   term_dot:   r[n] = sum_j g[n][j] * B[j]          (f32)
 *   term_outer: Bg[j] = sum_n s[n] * g[n][j]         (f32, n ascending)
 * Each one's derivatives are the other two. */
int sg_mbstd_term_fwd(const void* y, const float* s, const float* B, void* out, int32_t n, int64_t plane, sg_dtype dt,
                      sg_stream_t st);
int sg_mbstd_term_dot(const void* g, const float* B, float* r, int32_t n, int64_t plane, sg_dtype dt, sg_stream_t st);
int sg_mbstd_term_outer(const float* s, const void* g, float* Bg, int32_t n, int64_t plane, sg_dtype dt, sg_stream_t st);
/* Label conditioning of the 3-D pgan (csrc/cond.hip).  c f32 [n, l]: one label row per sample; W f32 [l, zdim]:
 * the generator's embedding; z [n, zdim], out [n, 2 * zdim], o [n, l] of type dt, row-major.  One launch per call, f32 sums in
 * ascending index order, no atomics.  SG_EINVAL before any launch: a NULL pointer (but see adjoint), a size < 1.
 *   sg_cond_embed, adjoint 0:  out[i, :zdim] = z[i],  out[i, zdim + j] = sum_k c[i, k] * W[k, j]
 *                  adjoint 1:  out holds the gradient g of the forward's output (read); W[k, j] = sum_i c[i, k] * g[i, zdim + j]
 *                              (f32, i ascending) and z[i, j] = g[i, j] are WRITTEN; W or z may be NULL (not both): not computed.
 *   sg_cond_project, adjoint 0: out[i] = sum_k o[i, k] * c[i, k]          (out [n] of type dt)
 *                    adjoint 1: o holds the gradient g [n] of the forward's output; out[i, k] = g[i] * c[i, k]  (out [n, l]).
 * Each op is linear in z, W / o: the adjoint is its gradient, and the forward is the adjoint's. */
int sg_cond_embed(void* z, const float* c, float* W, void* out, int32_t n, int32_t zdim, int32_t l, int32_t adjoint, sg_dtype dt,
                  sg_stream_t st);
int sg_cond_project(const void* o, const float* c, void* out, int32_t n, int32_t l, int32_t adjoint, sg_dtype dt, sg_stream_t st);
/* dtype conversion between f32 and bf16 buffers (dst dtype = dt_dst). */
int sg_cast(const void* src, sg_dtype dt_src, void* dst, sg_dtype dt_dst, int64_t numel, sg_stream_t st);

/* ---- optimiser (optimization.py:16,28 tf.train.AdamOptimizer; ExtendedEMA.py:56-59) ------------ */
/* Fused TF-formulation Adam + EMA over one contiguous f32 range:
 *   m = b1*m + (1-b1)*g*gscale; v = b2*v + (1-b2)*(g*gscale)^2; p -= lr_t * m / (sqrt(v) + eps);
 *   if (ema) ema -= (1-ema_decay)*(ema - p)
 * lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is computed by the caller.  g NULL => EMA only. */
int sg_adam_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, float lr_t,
                float b1, float b2, float eps, float gscale, float ema_decay, sg_stream_t st);
/* The other optimisers optimization.py:17-22,29-35 can create, fused with the EMA update in the same way
 * (TF training_ops rules; g is scaled by gscale first; ema may be NULL):
 *   SG_OPT_SGD       tf.train.GradientDescentOptimizer      p -= lr*g
 *   SG_OPT_MOMENTUM  tf.train.MomentumOptimizer(momentum=h) s1 = h*s1 + g; p -= nesterov ? lr*g + lr*h*s1 : lr*s1
 *   SG_OPT_ADADELTA  tf.train.AdadeltaOptimizer(rho=h, eps) s1 = h*s1 + (1-h)*g^2; u = sqrt(s2+eps)*rsqrt(s1+eps)*g;
 *                                                          p -= lr*u; s2 = h*s2 + (1-h)*u^2
 * s1 / s2: f32 state ranges like p (unused ones may be NULL). */
enum { SG_OPT_SGD = 0, SG_OPT_MOMENTUM = 1, SG_OPT_ADADELTA = 2 };
int sg_optim_step(int kind, float* p, const float* g, float* s1, float* s2, float* ema, int64_t numel, float lr,
                  float h, float eps, int nesterov, float gscale, float ema_decay, sg_stream_t st);
/* sg_adam_ema / sg_optim_step with the step size read from DEVICE memory (one float: lr_t resp. lr): the optimiser launches
 * of a captured step, whose learning-rate schedule (optimization.py:227-296) and Adam bias correction stay host arithmetic
 * -- the host writes the value before each replay. */
int sg_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, const float* lr_t,
                    float b1, float b2, float eps, float gscale, float ema_decay, sg_stream_t st);
int sg_optim_step_dev(int kind, float* p, const float* g, float* s1, float* s2, float* ema, int64_t numel, const float* lr,
                      float h, float eps, int nesterov, float gscale, float ema_decay, sg_stream_t st);
/* out[i] = sum of squares of segment i (offsets[i]..offsets[i+1]) of a flat f32 buffer
 * (tf.norm per gradient + tf.clip_by_global_norm, optimization.py:66-71).  offsets: DEVICE int64[nseg+1]. */
int sg_segment_sumsq(const float* flat, const int64_t* offsets, float* out, int32_t nseg, sg_stream_t st);
/* Non-finite step guard (not in the reference; optimization.StepGraph with the guard on).  A train op whose gradient holds a
 * NaN or +-Inf after the data-parallel reduction does nothing this step: parameters, optimiser state and step count stay
 * as they were, the EMA update still runs.  All flags are DEVICE int32 (0 = all finite), all counters DEVICE int64.
 * sg_nonfinite_flag: *flag = 1 if any x[i] is non-finite (isfinite, not an overflow test: 3e38 is finite); accumulate = 0
 * clears *flag first (a memset on `st`), 1 ORs into it (several ranges of one network).  x 16-byte aligned.
 * sg_segment_sumsq_flag: sg_segment_sumsq that also sets *flag from the values it reads (the clipping path: no second pass).
 * sg_guard_step (one thread): flag clear -> ++*t, counters[1] = 0, *lr_t = adam ? (float)(lr*sqrt(1-b2^t)/(1-b1^t)) in
 * double : (float)lr; flag set -> ++counters[0], ++counters[1], counters[2] = max(counters[2], counters[1]).
 * counters: [skipped, consecutive skips, longest run].  lr_dev (may be NULL): a DEVICE double read instead of lr (captured
 * step: the host writes the base learning rate before each replay).
 * sg_adam_ema_guarded / sg_optim_step_guarded: sg_adam_ema_dev / sg_optim_step_dev with a skip flag: clear -> exactly their
 * result with the step size *lr_t / *lr; set -> the EMA-only update (sg_adam_ema with g NULL), or nothing if ema is NULL. */
int sg_nonfinite_flag(const float* x, int64_t numel, int32_t* flag, int32_t accumulate, sg_stream_t st);
int sg_segment_sumsq_flag(const float* flat, const int64_t* offsets, float* out, int32_t nseg, int32_t* flag,
                          int32_t accumulate, sg_stream_t st);
int sg_guard_step(const int32_t* flag, int64_t* t, int64_t* counters, double lr, const double* lr_dev, float* lr_t,
                  int32_t adam, double b1, double b2, sg_stream_t st);
int sg_adam_ema_guarded(float* p, const float* g, float* m, float* v, float* ema, int64_t numel, const float* lr_t,
                        const int32_t* skip, float b1, float b2, float eps, float gscale, float ema_decay, sg_stream_t st);
int sg_optim_step_guarded(int kind, float* p, const float* g, float* s1, float* s2, float* ema, int64_t numel,
                          const float* lr, const int32_t* skip, float h, float eps, int nesterov, float gscale,
                          float ema_decay, sg_stream_t st);
/* Layer-wise adaptive optimisers (SURFGAN_2D/optim.py:60-80: LAMBOptimizer, AdamWeightDecayOptimizer; rules optim.py:246-267,
 * 354-398), fused with the EMA update, over ALL variables of a train op per launch.  g is scaled by gscale first:
 *   m = b1*m + (1-b1)*g;  v = b2*v + (1-b2)*g^2
 *   AdamW  u = m / (sqrt(v) + eps) + lam*w;                        w -= lr*u              (no bias correction)
 *   LAMB   u = (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) + lam*w;    w -= lr*r*u,  r = |w|/|u| if |w| > 0 and |u| > 0 else 1
 *   (norms over the whole variable, of w before the update);  if (ema) ema -= (1-ema_decay)*(ema - w)
 * Segment table (DEVICE, built once per train op): p, g, m, v, ema are the bases of flat f32 buffers of `total` elements;
 *   segs   int64[nseg][4]    {start (a multiple of 4), count, decay flag (lam = flag ? decay : 0), first block}
 *   blocks int32[nblocks][2] {segment, chunk}: block b covers elements [chunk*SG_SEG_CHUNK, (chunk+1)*SG_SEG_CHUNK) of its
 *          segment; a segment's ceil(count / SG_SEG_CHUNK) blocks are consecutive, starting at its `first block`.
 * Elements outside the segments (alignment padding) are neither read nor written.
 * lr_dev (may be NULL): a DEVICE float read instead of lr.  skip (may be NULL; needs lr_dev): the non-finite guard's flag --
 * set: parameters, moments and step count stay, only the EMA update runs; clear: exactly the unguarded result.
 * LAMB is three launches: sg_lamb_moments (updates m, v; block b leaves its sums of w^2 and u^2 in partials[2b], [2b+1]:
 * f32[2*nblocks]), sg_lamb_ratios (sums each segment's partials in double in a fixed order, writes ratios f32[nseg]) and
 * sg_lamb_update (recomputes u, updates w and ema).  No atomics: equal inputs give equal bits.  t: the DEVICE int64 count of
 * applied updates; 1 - b^t is computed from it in double.  advance = 1 (unguarded): sg_lamb_moments uses *t + 1 and
 * sg_lamb_ratios stores it; advance = 0: *t was advanced by sg_guard_step. */
#define SG_SEG_CHUNK 4096
int sg_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t total, const int64_t* segs,
                 const int32_t* blocks, int32_t nseg, int32_t nblocks, float lr, const float* lr_dev, const int32_t* skip,
                 float b1, float b2, float eps, float decay, float gscale, float ema_decay, sg_stream_t st);
int sg_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t total, const int64_t* segs,
                    const int32_t* blocks, int32_t nseg, int32_t nblocks, float* partials, const int64_t* t, int32_t advance,
                    const int32_t* skip, double b1, double b2, float eps, float decay, float gscale, sg_stream_t st);
int sg_lamb_ratios(const int64_t* segs, int32_t nseg, int32_t nblocks, const float* partials, float* ratios, int64_t* t,
                   int32_t advance, const int32_t* skip, sg_stream_t st);
int sg_lamb_update(float* p, const float* m, const float* v, float* ema, int64_t total, const int64_t* segs,
                   const int32_t* blocks, int32_t nseg, int32_t nblocks, const float* ratios, const int64_t* t, float lr,
                   const float* lr_dev, const int32_t* skip, double b1, double b2, float eps, float decay, float ema_decay,
                   sg_stream_t st);

/* ---- spectral normalisation (SURFGAN_3D/networks/ops.py:80-127), batched over the normalised weights of one network -----
 * A weight is W = reshape(w, [R, C]), C = cout, a segment of the flat f32 parameter buffer p; u [C] is its persistent state.
 * One refresh with `iteration` = k: k times { v = normalise(u W^T); u = normalise(v W) }, normalise(x) = x / sqrt(max(|x|^2,
 * 1e-12)); then sigma = v W u^T and eff = W / sigma at the same offsets of the effective-weight buffer (eff != p).  sigma = 0
 * is not protected against (as the reference).  The pull-back maps G = dL/d(eff) to dL/dW with u, v held constant, in place:
 *   g = (g - <g, eff> v_r u_c) / sigma
 * Table (DEVICE, built once per network):
 *   segs   int64[nseg][SG_SPECTRAL_SEG_FIELDS] {start (a multiple of 4), R, C, first block, rows per block (1..SG_SEG_CHUNK),
 *          offset of u in `u`, offset of v in `v`, offset of the column partials in `cols`}
 *   blocks int32[nblocks][2] {segment, row block}: block b covers rows [rb*rpb, min(R, (rb+1)*rpb)) of its segment; a segment's
 *          ceil(R / rpb) blocks are consecutive, starting at its `first block`.
 * Workspaces (f32): sigma[nseg], nt[nseg], partials[nblocks], cols[collen] with ceil(R / rpb) * C elements per segment; v[vlen]
 * holds R elements per segment, u[ulen] C.  Padding between segments is neither read nor written.  A segment that does not
 * fit its buffers is left alone as a whole.  sg_spectral_refresh is 2*iteration + 1 launches and sg_spectral_pullback two,
 * whatever nseg; partial sums are combined in an order fixed by the table (no atomics): equal inputs give equal bits. */
#define SG_SPECTRAL_SEG_FIELDS 8
int sg_spectral_refresh(const float* p, float* eff, int64_t total, const int64_t* segs, const int32_t* blocks, int32_t nseg,
                        int32_t nblocks, float* u, int64_t ulen, float* v, int64_t vlen, float* sigma, float* nt,
                        float* partials, float* cols, int64_t collen, int32_t iteration, sg_stream_t st);
int sg_spectral_pullback(float* g, const float* eff, int64_t total, const int64_t* segs, const int32_t* blocks, int32_t nseg,
                         int32_t nblocks, const float* u, int64_t ulen, const float* v, int64_t vlen, const float* sigma,
                         float* partials, sg_stream_t st);

/* ---- discriminator augmentation with adaptive probability (Karras et al. 2020; not in the reference) ------------------
 * Pixel-blitting transforms only -- axis flips, 90-degree rotations in the (h, w) plane, integer translations with a constant
 * fill: index gathers, so values are copied bit for bit and the adjoint is another gather.  Per-sample parameters live in
 * DEVICE memory as int32 params[n][8] = {flip_d, flip_h, flip_w, rot_k, t_d, t_h, t_w, 0}.  `ops` is a mask of SG_AUG_* bits.
 *
 * sg_augment_draw: one thread per sample i.  ctr = offset + i, key = seed ^ 0x4155474D454E5431 (the instance noise's key is
 * `seed` itself: its streams are untouched).  Three Philox4x32-10 blocks, counter {lo32 ctr, hi32 ctr, j, 0}, j = 0, 1, 2:
 *     block 0: gate flip_w, gate flip_h, gate flip_d, gate rot90
 *     block 1: gate translate, value flip_w, value flip_h, value flip_d
 *     block 2: value rot_k, value t_d, value t_h, value t_w
 *   gate r       : (uint64)r < (uint64)((double)p * 4294967296.0)     (p <= 0 or NaN: never; p >= 1: always)
 *   value r, cnt : (int)(((uint64)r * cnt) >> 32), uniform in [0, cnt)
 *   flip_a = gate ? value(2) : 0;  rot_k = gate ? value(4) : 0;  t_a = gate ? value(2 m_a + 1) - m_a : 0  (one gate for all t)
 * Integer arithmetic only after the conversion of p; a transform whose bit is clear in `ops` yields 0.  p_dev (may be NULL):
 * a DEVICE float read instead of p.  offset_dev (may be NULL): a DEVICE counter read instead of `offset` and then advanced
 * by `bump` in stream order (the contract of sg_add_noise_dev: the form a captured step uses).
 *
 * sg_augment_apply on NDHWC x, y [n, d, h, w, c] (x != y), params as above:
 *   forward  y[i] = shift(rot90(flip(x[i], axes), k, plane (h, w)), t, fill)   -- numpy's flip / rot90 conventions on the
 *            sample's [d, h, w, c] array; shift(a, t, fill)[v] = a[v - t] where v - t is in range, else fill
 *   adjoint  y[i] = flip(rot90(shift(x[i], -t, 0), -k), axes)                  -- the transpose of the forward's linear part
 * Only the transforms whose bit is set in `ops` are read from params (rot_k mod 4; every source voxel is range-checked);
 * SG_AUG_ROT90 with h != w is SG_EINVAL.
 *
 * sg_ada_update: the controller of the adaptive probability, one thread.  logits: D's outputs on the real batch (f32 [n]);
 * state: DEVICE int64[4] = {sum_sign, count, steps, adjustments}; p: DEVICE float.
 *     sum_sign += sum_i sign(logits[i])  (+1 / -1; 0 for zeros and NaN);  count += n;  steps += 1
 *     if steps % interval == 0:  up = sum_sign * target_den > target_num * count          (int64)
 *                                p = min(max(p + (up ? delta : -delta), 0), p_max)        (f32)
 *                                adjustments += 1;  sum_sign = count = 0 */
enum { SG_AUG_FLIP_W = 1, SG_AUG_FLIP_H = 2, SG_AUG_FLIP_D = 4, SG_AUG_ROT90 = 8, SG_AUG_TRANSLATE = 16, SG_AUG_ALL = 31 };
int sg_augment_draw(int32_t* params, int32_t n, uint32_t ops, int32_t m_d, int32_t m_h, int32_t m_w, float p,
                    const float* p_dev, uint64_t seed, uint64_t offset, uint64_t* offset_dev, uint64_t bump, sg_stream_t st);
int sg_augment_apply(const void* x, void* y, const int32_t* params, int32_t n, int32_t d, int32_t h, int32_t w, int32_t c,
                     uint32_t ops, float fill, int32_t adjoint, sg_dtype dt, sg_stream_t st);
int sg_ada_update(const float* logits, int32_t n, int64_t* state, float* p, int32_t interval, int64_t target_num,
                  int64_t target_den, float delta, float p_max, sg_stream_t st);

/* ---- intensity and fractional-geometry augmentation (Karras et al. 2020: "geom" and "color"; not in the reference) --------
 * Isotropic scaling, rotation in the (h, w) plane, sub-voxel translation, brightness, contrast: one trilinear resampling pass
 * with an exact, deterministic adjoint (a gather: no atomics).  `ops` is a mask of SG_AUGF_* bits, a mask of its own next to
 * SG_AUG_*.  Per-sample parameters live in DEVICE memory as float params[n][16]:
 *     [0..11] row-major 3 x 4 matrix A: the SOURCE coordinate of output voxel v = (vd, vh, vw) is u = A[:, :3] v + A[:, 3],
 *             in voxel units;  [12] gain a;  [13] bias b;  [14..15] 0.
 *
 * sg_augment_affine_draw: one thread per sample i.  p / p_dev / offset / offset_dev / bump as sg_augment_draw; key =
 * seed ^ 0x4155474D454E5432; three Philox4x32-10 blocks, counter {lo32 ctr, hi32 ctr, j, 0}, j = 0, 1, 2:
 *     block 0: gate scale, gate rotate, gate shift, gate brightness
 *     block 1: gate contrast, value scale, value angle, value brightness
 *     block 2: value contrast, value t_d, value t_h, value t_w
 *   gate(r) as sg_augment_draw;  a value word r becomes sym = 2 (r 2^-32) - 1; everything below in double:
 *   s = exp2(sym log2 max_scale);  theta = sym max_angle (radians);  t_a = sym_a max_shift_a (voxels);
 *   b = sym max_brightness;  a = exp2(sym log2 max_contrast);  disabled or gated off: s = 1, theta = 0, t = 0, b = 0, a = 1.
 *   With c_a = (extent_a - 1) / 2:  u = c + (1/s) R(-theta) (v - c - t),  R(-theta) = [[cos, sin], [-sin, cos]] on (h, w):
 *     A = [[1/s, 0, 0, o_d], [0, cos/s, sin/s, o_h], [0, -sin/s, cos/s, o_w]],  o = c - A[:, :3] (c + t)
 *   rounded to f32 once.  With every gate off the row is EXACTLY the identity matrix, a = 1, b = 0.
 *   SG_EINVAL: unknown bits in ops, max_scale outside [1, 2], max_angle outside [0, pi], a negative maximum, max_contrast
 *   outside [1, 4] (NaN is outside).
 *
 * sg_augment_affine_apply on NDHWC x, y [n, d, h, w, c], f32 or bf16, x != y.  flags bit 0: adjoint; bit 1: linear part only
 * (fill and b read as 0).  Every product and sum below rounds to f32 on its own (no FMA):
 *   1. u_a = ((A[a][0] vd + A[a][1] vh) + A[a][2] vw) + A[a][3]
 *   2. support: -1 < u_a < extent_a on every axis, tested in float (NaN fails).  Outside: forward y = a fill (then step 5's
 *      bias); the adjoint gets nothing from this voxel.
 *   3. f_a = floor(u_a), r_a = u_a - f_a, w0_a = 1 + (-r_a), w1_a = r_a
 *   4. corner k = 4 bd + 2 bh + bw: W_k = ((wd wh) ww) a, value x[f + bits]; outside the volume: `fill` forward, absent adjoint
 *   5. forward: corners in ascending k, W_k == 0 skipped and never read; acc = the first W_k x_k, the later ones added;
 *      y = b != 0 ? acc + b : acc, rounded to the output type once.  An identity row reproduces every finite input's bits.
 *   6. adjoint: gx[u] = sum of W_k(v) gy[v] over the output voxels v that have u among their in-range corners with W_k != 0,
 *      in ascending linear order of v, starting from the first term, rounded once; 0 where no v reaches u.  The kernel
 *      gathers over a window of candidate v around A^-1 (u - A[:, 3]) whose half-width per axis is the absolute row sum of
 *      A^-1 plus a slack; absolute row sums above 3 are outside the adjoint's contract.  For ANY bit pattern in params both
 *      directions stay inside their buffers and the window loops stay within 8 candidates per axis. */
enum { SG_AUGF_SCALE = 32, SG_AUGF_ROTATE = 64, SG_AUGF_SHIFT = 128, SG_AUGF_BRIGHTNESS = 256, SG_AUGF_CONTRAST = 512,
       SG_AUGF_ALL = 992 };
int sg_augment_affine_draw(float* params, int32_t n, uint32_t ops, int32_t d, int32_t h, int32_t w, double max_scale,
                           double max_angle, double max_shift_d, double max_shift_h, double max_shift_w, double max_brightness,
                           double max_contrast, float p, const float* p_dev, uint64_t seed, uint64_t offset, uint64_t* offset_dev,
                           uint64_t bump, sg_stream_t st);
int sg_augment_affine_apply(const void* x, void* y, const float* params, int32_t n, int32_t d, int32_t h, int32_t w, int32_t c,
                            float fill, uint32_t flags, sg_dtype dt, sg_stream_t st);

/* ---- validation metrics on device tensors (metrics/swd.py:13-123, metrics/skim_metrics.py:8-45) ---------------- */
/* One axis of a separable FIR filter over x viewed as [outer, n, inner], accumulated in f64: y = alpha * value + add (add
 * may be NULL; it is shaped and typed like y; alpha * value is rounded to y's type before the addition, as a caller that
 * stores the filtered value and then adds would have it).  `f64` names the types of x and y: 0 f32 -> f32, 1 f64 -> f64,
 * 2 f32 -> f64, 3 f64 -> f32 (any other value: SG_EINVAL).  The pyramid runs its three passes as 2, 1, 3: the f64
 * intermediates are exact for f32 volumes of moderate range, so a step rounds once, like the reference's one 5x5x5
 * convolution (which scipy accumulates in f64).
 *   mode 0: value[o] = sum_t taps[t] x[B(o + t - r)]                    extent n      (scipy.ndimage.gaussian_filter1d)
 *   mode 1: value[o] = sum_t taps[t] x[B(2o + t - r)]                   extent (n+1)/2  (pyr_down, swd.py:63-66:
 *           the 5x5x5 binomial filter is separable, then [::2])
 *   mode 2: value[o] = sum_t taps[t] z[B(o + t - r)], z[2k] = x[k], z[odd] = 0, extent 2n  (pyr_up, swd.py:69-74)
 * r = ntaps / 2, ntaps odd <= 15, taps on the HOST.  border B: 0 scipy 'mirror', 1 scipy 'reflect'.  x != y. */
int sg_filter_axis(const void* x, void* y, const void* add, int64_t outer, int32_t n, int64_t inner, const double* taps,
                   int32_t ntaps, int32_t mode, int32_t border, double alpha, int32_t f64, sg_stream_t st);
/* get_descriptors_for_minibatch (swd.py:13-26): x f32 [n_img, c, d, h, w] (NCDHW, as the metrics receive it);
 * out[nh, c, i, j, k] = x[nh / per_image, c, d0[nh] + i - rd, h0[nh] + k - rw, w0[nh] + j - rh], out shaped
 * [n_img * per_image, c, 2rd+1, 2rh+1, 2rw+1] -- the reference adds its fourth-axis offsets to the W centre and its
 * fifth-axis offsets to the H centre, and so does this.  d0 / h0 / w0: DEVICE int32[n_img * per_image].
 * PRECONDITION on the centres, with the offsets each one really carries: d0 in [rd, d - rd), h0 in [rw, h - rw), w0 in
 * [rh, w - rh).  The library cannot see device-side centres: it only refuses (SG_EINVAL, before any launch) a NULL pointer,
 * n_img, c or per_image < 1, a negative radius, and extents with no legal centre at all (d < 2rd+1, h < 2rw+1, w < 2rh+1);
 * a centre outside its range reads outside x.  The reference draws the W centre from [rw, w - rw) and the H centre from
 * [rh, h - rh): with rh != rw the caller has to check its draws on the host (saragan_amd/metrics/swd.py raises ValueError). */
int sg_swd_gather(const float* x, float* out, const int32_t* d0, const int32_t* h0, const int32_t* w0, int32_t n_img,
                  int32_t c, int32_t d, int32_t h, int32_t w, int32_t per_image, int32_t rd, int32_t rh, int32_t rw,
                  sg_stream_t st);
/* finalize_descriptors (swd.py:31-39), in place: desc [n, c, inner] -> (desc - mean_c) / std_c over (n, inner). */
size_t sg_desc_normalize_workspace(int32_t c);
int sg_desc_normalize(float* desc, int64_t n, int32_t c, int64_t inner, void* workspace, size_t workspace_bytes,
                      sg_stream_t st);
/* sliced_wasserstein (swd.py:44-58) in three steps.  sg_swd_project: pt[dir][row] = sum_f a[row][f] * dirs[f][dir],
 * a [n, f], dirs [f, ndirs], pt [ndirs, npad] with npad = sg_swd_padded_rows(n) (a power of two >= 64; rows n.. are
 * +inf).  sg_sort_rows: every row of [rows, npad] ascending, in place (np.sort(axis=0) of the reference's layout).
 * sg_swd_distance: out[0] = mean_{row, i < n} |pa - pb|; out: 1 + rows doubles (out[1..] the row sums). */
int32_t sg_swd_padded_rows(int32_t n);
int sg_swd_project(const float* a, const float* dirs, float* pt, int32_t n, int32_t f, int32_t ndirs, int32_t npad,
                   sg_stream_t st);
int sg_sort_rows(float* data, int32_t rows, int32_t npad, sg_stream_t st);
int sg_swd_distance(const float* pa, const float* pb, double* out, int32_t rows, int32_t n, int32_t npad, sg_stream_t st);
/* skimage.metrics restated on f64 device buffers (skim_metrics.py:8-45); workspace: sg_metric_workspace() bytes.
 * sg_sqdiff_mean: out[0] = mean((a - b)^2).  sg_minmax: out[0] = min, out[1] = max.
 * sg_ssim_products: xx = x*x, yy = y*y, xy = x*y.  sg_ssim_mean: out[0] = mean over the channels-last map
 * [s0, s1, s2, c], cropped by crop0 on the first and crop on the other two spatial extents, of
 * (2 ux uy + c1)(2 vxy + c2) / ((ux^2 + uy^2 + c1)(vx + vy + c2)), v* = cov_norm * (u** - u* u*). */
size_t sg_metric_workspace(void);
int sg_sqdiff_mean(const double* a, const double* b, double* out, int64_t numel, void* workspace, size_t workspace_bytes,
                   sg_stream_t st);
int sg_minmax(const double* a, double* out, int64_t numel, void* workspace, size_t workspace_bytes, sg_stream_t st);
int sg_ssim_products(const double* x, const double* y, double* xx, double* yy, double* xy, int64_t numel, sg_stream_t st);
int sg_ssim_mean(const double* ux, const double* uy, const double* uxx, const double* uyy, const double* uxy, double* out,
                 int32_t s0, int32_t s1, int32_t s2, int32_t c, int32_t crop0, int32_t crop, double cov_norm, double c1,
                 double c2, void* workspace, size_t workspace_bytes, sg_stream_t st);

/* ---- squared distances between every pair of volumes (metrics/sample_metrics.py: MMD, 1-NN accuracy, precision/recall) ----
 * a [ma, v] and b [mb, v]: f32, row-major, contiguous, on the device; out: f64 [ma, mb],
 *   out[i][j] = max(0, |a_i|^2 + |b_j|^2 - 2 a_i.b_j).
 * The dot products are f32-input MFMAs (exact f32 products, f32 fmaf chain) over at most sg_pairwise_sqdist_chunk()
 * consecutive voxels; each chunk's accumulators are added into f64.  The row norms are summed in f64 throughout and the
 * combination is f64.  The grid comes from splitting v: partial tiles go to the workspace and are added in ascending
 * split order -- no floating-point atomics, two calls on the same input give the same bits whatever SG_DETERMINISTIC says.
 * b == a (same pointer, mb == ma) is the symmetric case: only tiles on and above the diagonal are computed, out[j][i] is
 * out[i][j] bit for bit and the diagonal is exactly 0.  Every offset is 64-bit (ma * v may exceed 2^32); ma, mb need not
 * be multiples of the tile nor v of the K step or the chunk, and nothing is padded or copied.
 * workspace: sg_pairwise_sqdist_workspace(ma, mb, v) bytes (covers the symmetric call of the same sizes), 8-byte aligned.
 * SG_EINVAL before any launch: a NULL pointer, ma < 1, mb < 1, v < 1.  SG_EWORKSPACE: the workspace is too small.
 * SG_EALIGN: a, b not 4-byte or out, workspace not 8-byte aligned.  16-byte aligned inputs with v % 4 == 0 are read by
 * 16-byte loads. */
int32_t sg_pairwise_sqdist_chunk(void);      /* the longest f32 accumulation chain, in elements of v */
size_t sg_pairwise_sqdist_workspace(int32_t ma, int32_t mb, int64_t v);
int sg_pairwise_sqdist(const float* a, const float* b, double* out, int32_t ma, int32_t mb, int64_t v, void* workspace,
                       size_t workspace_bytes, sg_stream_t st);

/* ---- batches from a device-resident table (csrc/deck.hip; dataset.ResidentLoader) ----------------------------
 * table [rows, row_elems] of the source type sdt, row-major, contiguous, on the device (a phase's `.npy` volumes in the files'
 * own dtype, or the f32 label table); idx: DEVICE int32[n]; out: DEVICE f32 [n, row_elems]:
 *   out[i][e] = f32(table[idx[i]][e])                         (every source type converts exactly)
 *   normalise != 0: (f32(table[idx[i]][e]) - mean) / stddev   two correctly rounded f32 operations, no reciprocal, no fused
 *                                                            form: the bits of np.subtract / np.divide with np.float32 scalars
 * One launch.  Row offsets are 64-bit (rows * row_elems * element size may pass 4 GiB).  16-byte loads and stores when table,
 * out and the row length in bytes are multiples of 16, an element path otherwise -- chosen per launch.  An index outside
 * [0, rows) fills its output row with quiet NaN and the table is not read for it: nothing out of bounds can be read.
 * SG_EINVAL before any launch: a NULL pointer, rows < 0, row_elems < 1, n < 0, an unknown sdt.  SG_EALIGN: table not aligned to
 * its element size, idx or out not 4-byte aligned.  n == 0: SG_OK, nothing launched.
 * SG_SRC_BF16 is read by sg_intensity_hist only: sg_gather_rows answers it with SG_EINVAL, as it does every unknown sdt. */
typedef enum { SG_SRC_U8 = 0, SG_SRC_I8 = 1, SG_SRC_I16 = 2, SG_SRC_U16 = 3, SG_SRC_F16 = 4, SG_SRC_F32 = 5, SG_SRC_BF16 = 6 } sg_src_dtype;
int sg_gather_rows(const void* table, sg_src_dtype sdt, int64_t rows, int64_t row_elems, const int32_t* idx, int32_t n, float* out,
                   int32_t normalise, float mean, float stddev, sg_stream_t st);

/* ---- voxel-intensity histograms (csrc/hist.hip; metrics/intensity_metrics.py) --------------------------------
 * x [rows, row_elems] of the source type dt (any sg_src_dtype, SG_SRC_BF16 included), row-major, contiguous, on the device;
 * out: DEVICE int64 [rows][bins + 1].  Per element, in f32 and exactly:
 *   t = x * scale + shift          two correctly rounded operations, never fused: numpy's x * np.float32(scale) + np.float32(shift)
 *   column = bins                  where t is NaN (the extra column)
 *            bins - 1              where t >= lo + bins (saturated: +inf too)
 *            0                     where t <  lo        (saturated: -inf too)
 *            min(floor(t) - lo, bins - 1) otherwise
 * Both saturation tests are float comparisons made before any conversion.  The top edge is closed: the last bin holds hi - 1
 * and hi = lo + bins, as np.histogram(bins = hi - lo, range = (lo, hi)) does.  Every row of `out` grows by row_elems.
 * accumulate == 0: out is zeroed on the stream first; != 0: the counts are added to what is there.  rows = 1 with
 * row_elems = n * v is the pooled histogram of a batch.  Counts are integers added with atomics: the result does not depend
 * on the order, two calls give the same tensor.  Every offset is 64-bit.  x need only be aligned to its element size
 * (16-byte loads from the first 16-byte boundary of every chunk, an element path in front of it and behind the last whole
 * load).
 * SG_EINVAL before any launch: bins < 1, bins > sg_intensity_hist_max_bins(), rows < 0, row_elems < 0, scale not finite,
 * an unknown dt, lo + bins > 2147483520 (the largest int32 an f32 holds), a NULL pointer with work to do.  SG_EALIGN: x not aligned to its element size, out
 * not 8-byte aligned.  rows == 0: SG_OK, nothing launched; row_elems == 0: only the zeroing. */
int32_t sg_intensity_hist_max_bins(void);      /* the LDS image of a block: 8191 */
int sg_intensity_hist(const void* x, sg_src_dtype dt, int64_t rows, int64_t row_elems, float scale, float shift, int32_t lo,
                      int32_t bins, int64_t* out, int accumulate, sg_stream_t st);

/* ---- sample previews (csrc/render.hip; preview.py) ----------------------------------------------------------------
 * One launch renders one VIEW of every sample of x [n, d, h, w, c] (the source type dt: any sg_src_dtype, SG_SRC_BF16 included;
 * contiguous, on the device; channel `channel` of c) into the DEVICE u8 canvas [canvas_h, canvas_w].  With c == 1 NDHWC is the
 * memory of NCDHW: a batch of the networks, a volume file and a row of a resident table pass as they are.
 * axis: the collapsed axis, 0 = D, 1 = H, 2 = W; the image's rows and columns are the remaining two in their original order:
 *   axis 0 -> H x W (axial), axis 1 -> D x W (coronal), axis 2 -> D x H (sagittal).
 * Per image pixel, in f32 unless said otherwise, exactly and in this order:
 *   v = x[index along the axis]                          SG_VIEW_SLICE
 *       the maximum over the axis, from -inf              SG_VIEW_MAX   NaN voxels are ignored; an all-NaN column gives -inf
 *       f32(sum over the axis / extent)                   SG_VIEW_MEAN  the sum in f64 (any order), one f64 division, one rounding
 *   t = v * scale + shift                                two correctly rounded operations, never fused, as in sg_intensity_hist
 *   u = (t - lo) * inv                                   inv: the caller's f32(255.0 / (f64(hi) - f64(lo)))
 *   g = u8(floorf(fminf(fmaxf(u, 0), 255) + 0.5f))       a NaN u gives 0
 * g is written zoom_r x zoom_c times (nearest repeat): sample i's tile of (rows * zoom_r) x (columns * zoom_c) pixels starts at
 * (r0 + (i / grid_cols) * pitch_r, c0 + (i % grid_cols) * pitch_c).  Pixels outside the tiles are not touched: the caller zeroes
 * the canvas.  No atomics: every pixel has one writer.  Every offset is 64-bit.  x need only be aligned to its element size
 * (16-byte loads where c == 1, from the first 16-byte boundary; an element path in front of it and behind the last whole load).
 * SG_EINVAL before any launch: a NULL pointer with work to do; n, d, h, w < 0 or c < 1; channel outside [0, c); an unknown dt,
 * axis or mode; a slice index outside the axis; a zoom < 1 or grid_cols < 1; hi <= lo or a non-finite lo, hi or scale; a negative
 * canvas size, origin or pitch; a pitch smaller than the tile where a second tile follows along it; ANY TILE THAT DOES NOT LIE
 * WHOLLY INSIDE THE CANVAS (computed on the host from n, the tile size and the pitches: nothing out of bounds can be written).
 * SG_EALIGN: x not aligned to its element size.  n == 0 or an empty extent: SG_OK, nothing launched. */
enum { SG_VIEW_SLICE = 0, SG_VIEW_MAX = 1, SG_VIEW_MEAN = 2 };
int sg_render_view(const void* x, sg_src_dtype dt, int64_t n, int64_t d, int64_t h, int64_t w, int32_t c, int32_t channel,
                   int32_t axis, int32_t mode, int64_t index, int32_t zoom_r, int32_t zoom_c, float scale, float shift, float lo,
                   float hi, float inv, uint8_t* canvas, int64_t canvas_h, int64_t canvas_w, int64_t r0, int64_t c0,
                   int32_t grid_cols, int64_t pitch_r, int64_t pitch_c, sg_stream_t st);

/* ---- the per-phase dataset pyramid (csrc/pyramid.hip; prepare_data.py) ---------------------------------------------
 * One launch reads a batch of source volumes x [n, sd, sh, sw] (the source type dt: any sg_src_dtype except SG_SRC_BF16;
 * contiguous, on the device, aligned to its element size) ONCE and writes `levels` (1 .. SG_PYRAMID_LEVELS_PER_LAUNCH) levels of
 * its block-reduction pyramid: out[i], i < levels, is [n, D >> i, H >> i, W >> i] of the output type out_dt (SG_SRC_U16,
 * SG_SRC_I16 or SG_SRC_F32; integer sources take any of the three, f16 / f32 sources SG_SRC_F32 only).  `out` is a HOST array
 * of `levels` device pointers.
 * The window: target voxel (td, th, tw) of the target shape (D, H, W) is source voxel (td + off_d, th + off_h, tw + off_w); the
 * offsets may be negative or run past the source, and a target voxel whose source index lies outside [0, extent) on any axis
 * reads pad_value.  Nothing outside the source is read.
 * Integer sources (u8, i8, i16, u16) use the *_i scalars, and exactly, per output voxel o of level i (its cube: the 2^i x 2^i
 * x 2^i target voxels from 2^i * o):
 *   v = int32(x or pad_value) - intercept                 (|intercept|, |pad_value| <= 2^30: v is a 32-bit integer)
 *   s = the sum of v over the cube, a 64-bit integer      SG_PYR_MEAN
 *       the maximum of v over the cube                    SG_PYR_MAX
 *   q = s / 8^i truncated toward zero                     SG_PYR_MEAN (integers; -1.5 gives -1);   q = s for SG_PYR_MAX
 *   stored: clamp(q, clip_lo, clip_hi) as out_dt          u16 / i16
 *           clamp(f32(f64(s) / 8^i), f32(clip_lo), f32(clip_hi))     SG_SRC_F32 (one rounding; MAX: f32(s))
 * which for MEAN is bit for bit np.clip(block_reduce(v, 2^i, np.average), lo, hi).astype(T): an f64 sum of integers under 2^53 is
 * exact in any order, the division by a power of two is exact, and clipping then truncating equals truncating then clamping
 * for integer bounds.
 * Float sources (f16, f32) use the *_f scalars:
 *   v = f32(x or pad_value) - intercept                   one f32 rounding
 *   s = the f64 sum of v over the cube, in any order      SG_PYR_MEAN: a NaN voxel makes its cubes NaN
 *       the maximum over the cube from -inf               SG_PYR_MAX: NaN voxels are ignored, an all-NaN cube gives -inf
 *   stored: clamp(f32(s / 8^i), clip_lo, clip_hi)         one f64 division, one rounding, as SG_VIEW_MEAN; a NaN stays NaN
 * Level i is built from level i - 1's unclamped, untruncated partials s (int64, f64, or the running maxima), never from stored
 * values.  No output voxel has two writers; no atomics touch the outputs.  Every offset is 64-bit.  Source rows are read with
 * 16-byte loads from each row's first 16-byte boundary, the elements in front of it and behind the last whole load one by one.
 * A pyramid is at most SG_PYRAMID_LEVELS_PER_LAUNCH levels deep (a 128 x 512 x 512 volume down to 4 x 16 x 16): there is no entry
 * that continues from the partials of a launch's deepest level.
 * stats (may be NULL; integer out_dt only, ignored for SG_SRC_F32): DEVICE int64 [n][levels][4] = the sum, the sum of squares,
 * the minimum and the maximum of the STORED values of every level of every sample.  Set to (0, 0, INT64_MAX, INT64_MIN) on the
 * stream first, then accumulated with integer atomics, one per block after a block-level reduction: exact, independent of order.
 * SG_EINVAL before any launch: a NULL pointer with work to do; a negative extent; levels outside [1, 6]; a target extent not
 * divisible by 2^(levels-1); an unknown dt, mode or out_dt, SG_SRC_BF16; a float
 * source with an integer out_dt; clip_lo > clip_hi (a NaN bound), integer bounds outside an integer out_dt; |intercept_i| or
 * |pad_i| > 2^30; an extent or |offset| > 2^29.  SG_EALIGN: x, an output or stats not aligned to its element size.  n == 0 or an empty
 * target: SG_OK, nothing launched. */
#define SG_PYRAMID_LEVELS_PER_LAUNCH 6
enum { SG_PYR_MEAN = 0, SG_PYR_MAX = 1 };
int sg_block_pyramid(const void* x, sg_src_dtype dt, int64_t n, int64_t sd, int64_t sh, int64_t sw, int64_t D, int64_t H, int64_t W,
                     int64_t off_d, int64_t off_h, int64_t off_w, int32_t levels, int32_t mode, int32_t intercept_i, int32_t pad_i,
                     int32_t clip_lo_i, int32_t clip_hi_i, float intercept_f, float pad_f, float clip_lo_f, float clip_hi_f,
                     sg_src_dtype out_dt, void* const* out, int64_t* stats, sg_stream_t st);

/* ---- resampling to a common voxel spacing (csrc/resample.hip; prepare_data.py --spacing) --------------------------
 * One launch resamples a batch of source volumes x [n, sd, sh, sw] (the source type dt: any sg_src_dtype except SG_SRC_BF16;
 * contiguous, on the device, aligned to its element size) to y [n, od, oh, ow] of the output type out_dt (SG_SRC_U16, SG_SRC_I16
 * or SG_SRC_F32 -- the types sg_block_pyramid takes as sources; integer sources take any of the three, f16 / f32 sources
 * SG_SRC_F32 only), separably, through one TAP TABLE per axis that the caller built (table_ops.resample_taps: nearest,
 * linear, a triangle antialiasing filter; a negative step flips the axis).
 * The table of an axis with O outputs and T taps (taps_d, taps_h, taps_w: 1 .. SG_RESAMPLE_MAX_TAPS, one count per axis per
 * launch) is a DEVICE int32 [1 + 2 T][O], tap-major: row 0 holds the `inside` flag of every output index (0: outside), rows
 * 1 .. T the source index of tap k, rows T + 1 .. 2 T the bits of its f32 weight.
 * Exactly, per output voxel (o_d, o_h, o_w), with (id, wd), (ih, wh), (iw, ww) the taps of its three output indices:
 *   outside on any axis (or an empty source):  y = the fill value, stored as a value is
 *   inner(d, h) = sum_k f64(ww[k]) * f64(x[d, h, iw[k]])      taps in table order, sequential adds from 0.0
 *   mid(d)      = sum_j f64(wh[j]) * inner(d, ih[j])
 *   acc         = sum_i f64(wd[i]) * mid(id[i])
 *   a tap whose weight is exactly 0 is skipped: its voxel (row, plane) is not read and nothing is added, so a NaN behind a
 *   zero weight does not leak
 *   stored: SG_SRC_F32: f32(acc), one rounding;  SG_SRC_I16 / SG_SRC_U16: clamp(rint(acc), the type's range), ties to even
 * Every product and every sum rounds on its own (no fused multiply-add).  The fill value is f64(fill_i) for integer sources and
 * f64(fill_f) for float sources.  Weights are finite; a source index outside [0, extent) is clamped to it in the kernel, so
 * nothing outside x is read whatever the tables hold (the Python wrapper builds and checks its tables on the host).
 * Every output voxel has one writer; there are no atomics; every offset is 64-bit; source rows need only element alignment.
 * SG_EINVAL before any launch: a NULL pointer with work to do; a negative extent; a tap count outside [1, 32]; an unknown dt
 * or out_dt, SG_SRC_BF16; a float source with an integer out_dt; an extent > 2^29.  SG_EALIGN: x or y not aligned to its
 * element size, a table not 4-byte aligned.  n == 0 or an empty output: SG_OK, nothing launched. */
#define SG_RESAMPLE_MAX_TAPS 32
int sg_resample_axes(const void* x, sg_src_dtype dt, int64_t n, int64_t sd, int64_t sh, int64_t sw, int64_t od, int64_t oh, int64_t ow,
                     const int32_t* tab_d, int32_t taps_d, const int32_t* tab_h, int32_t taps_h, const int32_t* tab_w,
                     int32_t taps_w, int32_t fill_i, float fill_f, sg_src_dtype out_dt, void* y, sg_stream_t st);

/* ---- typed volumes from the generator's output (csrc/export.hip; generate.py) ------------------------------------
 * The mirror image of sg_gather_rows: one pass reads a batch x [n, c, d, h, w] (the source type dt: SG_SRC_F32, SG_SRC_BF16 or
 * SG_SRC_F16; on the device, aligned to its element size; channels_last == 0: NCDHW-contiguous, != 0: the memory of NDHWC -- with
 * c == 1 the two are the same memory) once and writes out [n, c, d, h, w], NCDHW-contiguous, of the output type out_dt (SG_SRC_I16,
 * SG_SRC_U16, SG_SRC_U8 or SG_SRC_F32); a channels-last source with c > 1 is transposed on the way.  Per element, in f32 and exactly:
 *   t      = x * scale + shift                 two correctly rounded operations, never fused: numpy's x * np.float32(scale) +
 *                                              np.float32(shift) (scale = stddev, shift = mean undoes the training normalisation)
 *   nan    = t is NaN;  below = t < lo;  above = t > hi        float comparisons, made before any conversion; +-inf saturate
 *   u      = nan or below ? lo : above ? hi : t                 (min(max(t, lo), hi), a zero keeping its own sign)
 *   stored = T(trunc(u))                       integer T, SG_ROUND_TRUNC: numpy's .astype, what (np.clip(x, a, b) * s).astype(T) stores
 *            T(rint(u))                        integer T, SG_ROUND_RINT: ties to even, as sg_resample_axes stores
 *            nan ? the quiet NaN 0x7FC00000 : u                 SG_SRC_F32 (rounding is checked and not used)
 * For an integer T lo and hi are integers inside T's range, so no conversion can overflow; for SG_SRC_F32 they may be infinite.
 * stats (may be NULL): DEVICE int64 [n][7] = the sum, the sum of squares, the minimum and the maximum of sample i's STORED values
 * (integer T; four zeros for SG_SRC_F32), then the numbers of its below, above and nan elements.  Set to their identities on the
 * stream first, then accumulated with integer atomics, one per block, row and statistic after a reduction per wave and per block:
 * exact, independent of the order, two calls give the same bits.  No output element has two writers.  Every offset is 64-bit:
 * n * c * d * h * w may pass 2^31.  Whole 16-byte loads and stores when the source is one contiguous row per sample (NCDHW, or
 * c == 1), c * d * h * w is a multiple of the 16, 8 or 4 elements that make 16 bytes of the narrower type, and x and out reach
 * a 16-byte boundary after the same number of elements (those, and as many at each row's end, go one by one); an element path
 * otherwise -- chosen per launch.
 * SG_EINVAL before any launch: a NULL pointer with work to do; n, d, h, w < 0 or c < 1; an unknown dt, out_dt or rounding, or a dt
 * / out_dt outside the lists above; scale not finite; lo > hi or a NaN bound; for an integer T a bound that is not an integer or
 * lies outside T.  SG_EALIGN: x or out not aligned to its element size, stats not 8-byte aligned.  n == 0 or an empty volume:
 * SG_OK, nothing launched. */
enum { SG_ROUND_TRUNC = 0, SG_ROUND_RINT = 1 };
int sg_store_volumes(const void* x, sg_src_dtype dt, int32_t channels_last, int64_t n, int64_t c, int64_t d, int64_t h, int64_t w,
                     float scale, float shift, float lo, float hi, int32_t rounding, sg_src_dtype out_dt, void* out, int64_t* stats,
                     sg_stream_t st);

/* ---- exact squared distances between typed integer rows, and the running k nearest (csrc/sqdist_exact.hip; DESIGN.md 4.12;
 * metrics/memorisation.py) -------------------------------------------------------------------------------------------------------
 * q [mq, v] and r [mr, v] of the source type dt (SG_SRC_U8, SG_SRC_I8, SG_SRC_I16 or SG_SRC_U16), row-major, contiguous, on the
 * device, aligned to their element size; out: DEVICE int64 [mq, mr]:
 *   out[i][j] = sum over e of (q[i][e] - r[j][e])^2,  exactly (v < 2^31 keeps it inside int64).
 * A 16-bit voxel s (u16: minus 32768, a common shift) splits into the signed bytes h = s >> 8 and l = (s & 255) - 128;
 * t = 256 h + l = s - 128, and out = |tq|^2 + |tr|^2 - 2 tq.tr with tq.tr = 65536 h.h + 256 (h.l + l.h) + l.l: four dot products
 * on v_mfma_i32_16x16x64_i8 (8-bit types: one, u8 minus 128), accumulated in i32 over at most sg_sqdist_exact_chunk() voxels
 * (|product| <= 2^14, two products per voxel in the cross sum: 2^29 at most) and then in i64; the row norms and the combination
 * are i64.  K is split over the grid; the splits' integer partial tiles meet in the workspace and are added by a last kernel: no
 * atomics, exact, independent of the split -- two calls give the same bits.  r == q with mr == mq is the symmetric case: only
 * tiles on and above the diagonal are computed, out[j][i] == out[i][j] and the diagonal is 0.  mq, mr need not be multiples of
 * the 64-row tile nor v of anything; rows past the end and voxels past a split's end are staged as zeros, never read.  16-byte
 * loads where a row's bytes are 16-byte aligned, element loads elsewhere (chosen per 16 bytes, so a row of an odd v or a view
 * that starts mid-buffer only needs element alignment).  Every offset is 64-bit: mr * v may pass 2^32 bytes.
 * workspace: sg_sqdist_exact_workspace(mq, mr, v) bytes (covers the symmetric call of the same sizes), 8-byte aligned.
 * SG_EINVAL before any launch: a NULL pointer, mq < 1, mr < 1, v < 1, v >= 2^31, any other dt.  SG_EWORKSPACE: the workspace is
 * too small.  SG_EALIGN: q, r not aligned to their element size, or out, workspace not 8-byte aligned. */
int32_t sg_sqdist_exact_chunk(void);      /* the longest i32 accumulation, in elements of v */
size_t sg_sqdist_exact_workspace(int32_t mq, int32_t mr, int64_t v);
int sg_sqdist_exact(const void* q, const void* r, sg_src_dtype dt, int32_t mq, int32_t mr, int64_t v, int64_t* out, void* workspace,
                    size_t workspace_bytes, sg_stream_t st);
/* best_d, best_id: DEVICE int64 [mq, k], every row sorted ascending by (distance, id); the caller starts them at INT64_MAX / -1
 * (an entry with id -1 is empty).  The call merges into them the mr candidates of every row of d [mq, mr] (DEVICE int64), whose
 * ids are r_base + j.  q_ids (may be NULL): DEVICE int64 [mq]; the candidate whose id equals q_ids[i] is skipped in row i
 * (leave-one-out for a set against itself).  Equal distances go to the lower id, so the result does not depend on how the
 * reference set was cut into calls.  One wave per row and one writer per row: no atomics.
 * SG_EINVAL before any launch: a NULL d, best_d or best_id; mq < 1, mr < 1, r_base < 0; k outside 1 .. 16.  SG_EALIGN: a pointer
 * not 8-byte aligned. */
int sg_topk_merge(const int64_t* d, int32_t mq, int32_t mr, int64_t r_base, const int64_t* q_ids, int32_t k, int64_t* best_d,
                  int64_t* best_id, sg_stream_t st);

/* ---- projection of volumes onto the generator (csrc/project.hip; project.py) -----------------------------------------
 * sg_multiscale_residual: the multi-scale residual loss between y [n, c, d, h, w] (ydt: SG_SRC_F32, SG_SRC_BF16 or SG_SRC_F16;
 * channels_last as in sg_store_volumes) and the rows idx[i] (DEVICE int32 [n]; repeats allowed) of table [rows, c, d, h, w]
 * (tdt: one of sg_gather_rows' six types, NCDHW), with its gradient grad (y's type and memory format).  Per sample, exactly:
 *   t = (f32(x) - mean) / stddev, two roundings as sg_gather_rows;  r = f32(y) - t, one rounding;
 *   S_0 = f64(r), S_l(B) = the sum of the eight children of the cube B of edge 2^l: the w pairs, then the h pairs, then the d pair;
 *   m_l = S_l * 8^-l;  Q_l = m_l^2 carried up the same tree to the edge-8 cubes that tile the volume from its origin (children
 *   outside count as +0); the cubes are added along w, those sums along h, those over (channel, d) in index order, each sum
 *   sequential from its first element;  terms[i][l] = total / N_l, N_l = c d h w / 8^l (DEVICE f64 [n][levels]);
 *   loss[i] = f32(lambda[0] terms[0] + lambda[1] terms[1] + ...) in f64 and this order (lambda: DEVICE f32 [levels]);
 *   grad[v] = k[0] r + (k[1] m_1 + (k[2] m_2 + k[3] m_3)) in f64 (k: HOST f64 [levels], read before the call returns; the caller
 *   gives k[l] = lambda[l] * (2 / N_l) / 8^l), rounded once to y's type.
 * Two calls give the same bits.  d, h and w are multiples of 2^(levels - 1).  A position outside [0, rows) is not addressed: that
 * sample's loss, terms and gradients are NaN.  workspace: DEVICE, sg_multiscale_residual_workspace bytes, 8-byte aligned; its
 * contents are scratch.  Two launches (the pass, and one block per sample that adds the cubes); 64-bit offsets throughout.
 * SG_EUNSUPPORTED: levels above sg_multiscale_residual_max_levels() (4: the cube a wave reduces in registers).  SG_EINVAL: a
 * NULL pointer with work to do, bad extents or types, levels < 1, extents that are no multiple of 2^(levels - 1), a workspace that
 * is too small.  SG_EALIGN: a pointer not aligned to its element size.  n == 0: SG_OK, nothing launched. */
int32_t sg_multiscale_residual_max_levels(void);
size_t sg_multiscale_residual_workspace(int64_t n, int64_t c, int64_t d, int64_t h, int64_t w, int32_t levels);
int sg_multiscale_residual(const void* y, sg_src_dtype ydt, int32_t channels_last, const void* table, sg_src_dtype tdt, int64_t rows,
                           const int32_t* idx, int64_t n, int64_t c, int64_t d, int64_t h, int64_t w, float mean, float stddev,
                           int32_t levels, const float* lambda, const double* k, void* grad, double* terms, float* loss,
                           void* workspace, size_t workspace_bytes, sg_stream_t st);
/* sg_latent_step: one wave per row i of z [n, L] (all DEVICE f32 but best_step, int32 [n]), in place, in this order:
 *   if loss[i] < best_loss[i] (never for a NaN; an equal loss keeps the earlier one): best_loss[i] = loss[i], z_best[i] = z[i],
 *   best_step[i] = step;  then, unless lr == 0 (the scoring launch: nothing else moves), Adam in f32, every operation rounded on
 *   its own:  m = b1 m + (1 - b1) g;  v = b2 v + ((1 - b2) g) g;  z = z - (lr (m / c1)) / (sqrt(v / c2) + eps), c_j = f32(1 -
 *   pow(f64(b_j), step)) computed on the host;  then, with sphere != 0, z *= sqrt(L) / sqrt(s) in f64, rounded to f32, where s is
 *   the f64 sum of z_k^2: 64 partial sums over k = j, j + 64, ... in increasing k, then added pairwise 32, 16, ..., 1 apart
 *   (a row whose s is 0, NaN or infinite is left alone).  step >= 1.  SG_EINVAL: NULL pointers with work to do, L < 1, step < 1,
 *   betas outside [0, 1), eps <= 0, lr < 0 or NaN.  SG_EALIGN: a pointer not 4-byte aligned. */
int sg_latent_step(float* z, float* m, float* v, const float* grad_z, const float* loss, float* best_loss, float* z_best,
                   int32_t* best_step, int64_t n, int64_t L, float lr, float beta1, float beta2, float eps, int32_t step,
                   int32_t sphere, sg_stream_t st);

/* ---- shell-binned power spectra (csrc/spectrum.hip; table_ops.power_spectrum) --------------------------------------
 * x [n, d, h, w] of the source type dt (any sg_src_dtype, SG_SRC_BF16 included), contiguous, on the device.  Per sample:
 *   t = (double)x * scale + shift, two roundings in f64;  F = the half spectrum (kw = 0 .. w / 2) of t as three one-axis passes
 *   (W, H, D) of f64 matrix products on v_mfma_f64_16x16x4_f64;  P = Fr^2 + Fi^2;  g = 1 at kw = 0 and kw = w / 2 (w even), else 2;
 *   radial[i][c] = sum g P over the coefficients whose r2 = (f2_d[kd] + f2_h[kh]) + f2_w[kw] falls into column c: 0 where
 *   r2 == 0, otherwise min(1 + #{b >= 1 : edges2[b] <= r2}, bins);
 *   axes[i] = axis_d (d / 2 + 1 sums over min(kd, d - kd) = q), then axis_h (h / 2 + 1), then axis_w (w / 2 + 1 sums at kw = q).
 * All DEVICE f64: mats = Cd^T [d][d], Sd^T [d][d], Ch^T [h][h], Sh^T [h][h], Cw^T [w][w / 2 + 1], Sw^T [w][w / 2 + 1], each
 * stored as Mt[j][k] = trig[(k j) mod n] * window[j];  f2 = f2_d [d], f2_h [h], f2_w [w];  edges2 [bins + 1], non-decreasing;
 * radial [n][bins + 1];  axes [n][(d / 2 + 1) + (h / 2 + 1) + (w / 2 + 1)];  workspace: sg_power_spectrum_workspace(n, d, h, w)
 * bytes, 8-byte aligned, scratch (the planar complex intermediates and one partial row per block of the last pass).
 * Every sum has a fixed order that depends on (d, h, w, bins) only: no floating-point atomics; two calls, another batch size or
 * another position in the batch give the same bits per sample.  Extents need not be multiples of anything; 64-bit offsets.
 * SG_EINVAL before any launch: an extent below 1 or above sg_power_spectrum_max_extent(), bins outside 1 .. 4096, an unknown dt,
 * a scale or shift that is not finite, n < 0, a NULL pointer with work to do.  SG_EWORKSPACE: the workspace is too small.
 * SG_EALIGN: x not aligned to its element size, another pointer not 8-byte aligned.  n == 0: SG_OK, nothing launched. */
int32_t sg_power_spectrum_max_extent(void);      /* 1024 */
size_t sg_power_spectrum_workspace(int64_t n, int64_t d, int64_t h, int64_t w);
int sg_power_spectrum(const void* x, sg_src_dtype dt, int64_t n, int64_t d, int64_t h, int64_t w, double scale, double shift,
                      const double* mats, const double* f2, const double* edges2, int32_t bins, double* radial, double* axes,
                      void* workspace, size_t workspace_bytes, sg_stream_t st);

/* ---- opt-in kernel timing (used by bench.py's roofline leg) ------------------------------------- */
/* When enabled, every sg_conv3d_fwd / sg_conv3d_wgrad launch is bracketed by hipEvents on its stream.
 * sg_prof_collect synchronises those events and returns, per kind (0 = conv fwd, 1 = wgrad) and per
 * distinct shape, the launch count, total milliseconds and algorithmic FLOPs. */
typedef struct {
  int32_t kind;
  sg_conv_shape shape;
  int32_t dtype;
  int64_t launches;
  double total_ms;
  double flops_per_launch;
  char kernel[64];     /* kernel family + template arguments the dispatcher chose for this shape, e.g. "conv_fwd4<bf16,2,1,3,3,3>" */
} sg_prof_entry;
int sg_prof_enable(int on);
/* 1 while the timing is enabled.  A caller that captures launches into a hipGraph (optimization.StepGraph) must not capture
 * the profiler's event records: it checks this and runs that step eagerly. */
int sg_prof_enabled(void);
/* Restrict the timing to ONE (kind, shape) (NULL: every launch again): two event records per launch are not free, and a
 * throughput measurement that wants the dominant kernel's duration from inside its own timed region brackets only
 * that kernel's launches. */
int sg_prof_set_filter(int kind, const sg_conv_shape* shape);
int sg_prof_collect(sg_prof_entry* out, int32_t max_entries, int32_t* n_entries);

/* The SG_* environment switches (kernel-selection overrides for diagnosis, e.g. SG_FWD_NO_V4=1) are read once, at the
 * first launch.  Tools that change one between launches call this to take a new snapshot. */
int sg_config_reload(void);

#ifdef __cplusplus
}
#endif
#endif /* SARAGAN_HIP_H */
