"""The images the kernels read a weight through, cached while the parameter is unchanged (same storage, same version counter):
the four discriminator passes and their gradients all read one image per orientation.  One type, one instance (IMAGES), four
kinds of image; what differs between the kinds is written down once, in the Kind records."""
import collections
import ctypes as C

import torch

from ._launch import _ptr
from ._lib import ConvShape, check

# nbytes / pack: the library's entry points that size and write the image (None: a small matrix made with torch operations).
# in_place: the image stays where it is when the parameters are rewritten and is rewritten with all the others by ONE
#   sg_conv3d_pack_weights_batch launch (only f32 contiguous weights: the launch reads the parameter itself); the other kinds are
#   few, are dropped then and rebuilt on use.
# takes_flip: the pack call has an orientation argument.  counted: a pack is a 'single' of the statistics.
# listed: a captured step carries the image's address (live()).
# keeps: the kind's long-lived rule -- which weights' images are worth an entry.
class Kind:      # (a plain object: it sits in every key, and hashes by identity)
    def __init__(self, name, nbytes, pack, takes_flip, counted, in_place, listed, keeps):
        self.name, self.nbytes, self.pack, self.takes_flip, self.counted = name, nbytes, pack, takes_flip, counted
        self.in_place, self.listed, self.keeps = in_place, listed, keeps

    def __repr__(self):
        return self.name


def _parameter(w):
    """Parameters (and constants), not transient gradients."""
    return w.is_leaf or not w.requires_grad


def _parameter_or_view(w):
    """A VIEW of a parameter -- the 2-D networks hand [kh, kw, ci, co] filters over as [1, kh, kw, ci, co] -- lives as long as the
    parameter and shares its version counter: configs[4] packed its 42 filters 126 times per step before this was recognised."""
    return w.is_leaf or not w.requires_grad or (w._is_view() and w._base.is_leaf)


def _any_weight(w):
    """(The few matrices of a step are kept whatever their weight is; they go when the parameters are rewritten.)"""
    return True


FRAGMENT = Kind('fragment', 'sg_conv3d_packed_bytes', 'sg_conv3d_pack_weights', takes_flip=True, counted=True, in_place=True,
                listed=True, keeps=_parameter_or_view)
SUBPIXEL_FWD = Kind('subpixel_fwd', 'sg_upconv3d_subpixel_packed_bytes', 'sg_upconv3d_subpixel_pack', takes_flip=False,
                    counted=False, in_place=False, listed=False, keeps=_parameter)
SUBPIXEL_DGRAD = Kind('subpixel_dgrad', 'sg_upconv3d_subpixel_dgrad_packed_bytes', 'sg_upconv3d_subpixel_dgrad_pack',
                      takes_flip=False, counted=False, in_place=False, listed=False, keeps=_parameter)
RGB_MATRIX = Kind('rgb_matrix', None, None, takes_flip=False, counted=False, in_place=False, listed=True, keeps=_any_weight)

# ptr / version: data_ptr and version counter of the weight when the image was made; flip: the data-gradient orientation (a
# matrix: small_is_cin); dt: the compute type, the library's code (a matrix: the torch dtype it is rounded to); the rest: the filter
ImageKey = collections.namedtuple('ImageKey', 'kind ptr version coef flip dt cin cout kd kh kw')
# weight: the tensor whose storage the key names, held so that the address is not recycled; shape: what the batch launch needs
ImageEntry = collections.namedtuple('ImageEntry', 'image weight shape')
_new_key = tuple.__new__


class WeightImages:
    def __init__(self):
        self._entries = {}       # ImageKey -> ImageEntry (only ever mutated in place: _get stays its lookup)
        self._get = self._entries.get
        self.stale = False       # the parameters were rewritten since the in-place images were
        self.stats = {'single': 0, 'batches': 0, 'batched': 0}      # counters for the tests (host side only)
        # What a launch that rewrites parameters behind torch's version counters calls (the optimiser kernels, the spectral
        # refresh).  functional points it at its mark_packs_stale, which reads the NO_PACK_BATCH switch; until functional is
        # imported there is no switch to read (the diagnostic switches live there), and it is the plain mark_stale.
        self.params_rewritten = self.mark_stale

    def clear(self):
        self._entries.clear()
        self.stale = False

    def mark_stale(self, drop_all=False):
        """The parameters were rewritten behind torch's version counters (the optimiser kernels; a graph capture, which records
        launches without running them).  The fragment images stay where they are and are rewritten together, one launch for all
        layers (sg_conv3d_pack_weights_batch), when the next convolution asks for one -- 44 pack launches per step at the
        benchmarked configuration otherwise.  The few images of other kinds (sub-pixel forms, to_rgb matrices) are dropped and
        rebuilt on use.  drop_all (the NO_PACK_BATCH diagnostic): every image is dropped, one pack launch per layer and use."""
        if drop_all:
            return self.clear()
        for key in [k for k in self._entries if not k.kind.in_place]:
            del self._entries[key]
        self.stale = bool(self._entries)

    def live(self):
        """The cached images (tensors) whose addresses the launches of a captured graph carry."""
        return [e.image for k, e in self._entries.items() if k.kind.listed]

    def _refresh(self, lib, st):
        self.stale = False
        by_dt = {}
        for key, ent in list(self._entries.items()):
            if not key.kind.in_place:
                continue
            if ent.weight._version != key.version or ent.weight.data_ptr() != key.ptr:
                del self._entries[key]      # modified through torch since: a new key is in use, this one is dead
                continue
            by_dt.setdefault(key.dt, []).append((key, ent))
        for dt, items in by_dt.items():
            n = len(items)
            ws = (C.c_void_p * n)(*[k.ptr for k, e in items])       # (the weight itself: in-place images are of f32 contiguous ones)
            coefs = (C.c_float * n)(*[k.coef for k, e in items])
            flips = (C.c_int * n)(*[1 if k.flip else 0 for k, e in items])
            wps = (C.c_void_p * n)(*[e.image.data_ptr() for k, e in items])
            shapes = (ConvShape * n)(*[e.shape for k, e in items])
            check(lib.sg_conv3d_pack_weights_batch(n, ws, coefs, flips, wps, shapes, dt, st), 'sg_conv3d_pack_weights_batch')
            self.stats['batches'] += 1
            self.stats['batched'] += n

    def fragment(self, w, coef, flip, shp, dt, lib, st):
        """The MFMA fragment image of conv3d's weights (sg_conv3d_pack_weights); `flip`: the data-gradient orientation."""
        if self.stale:
            self._refresh(lib, st)
        # (hundreds of lookups per eager step: the key is made by tuple.__new__, a third of the generated constructor's cost, and
        # coef / flip go in as they come: host numbers -- float or a subclass (DevCoef), int, bool, numpy scalar -- which hash and
        # compare like the float / bool that _build stores; _build refuses anything that does not)
        key = _new_key(ImageKey, (FRAGMENT, w.data_ptr(), w._version, coef, flip, dt, shp.cin, shp.cout, shp.kd, shp.kh, shp.kw))
        hit = self._get(key)
        return hit.image if hit is not None else self._build(key, w, shp, lib, st)

    def subpixel(self, w, coef, shp, dt, lib, st, dgrad=False):
        """The summed weights of the eight parity classes of conv3d(upscale3d(x)) (sg_upconv3d_subpixel_pack), or with dgrad their
        transposes for the data gradient (sg_upconv3d_subpixel_dgrad_pack).  shp: the low-resolution convolution."""
        key = ImageKey(SUBPIXEL_DGRAD if dgrad else SUBPIXEL_FWD, w.data_ptr(), w._version, float(coef), False, dt,
                       shp.cin, shp.cout, shp.kd, shp.kh, shp.kw)
        hit = self._entries.get(key)
        return hit.image if hit is not None else self._build(key, w, shp, lib, st)

    def rgb_matrix(self, w_rgb, coef, dtype, small_is_cin=False):
        """[cs][c] f32 of a pointwise convolution between cs <= 4 and c channels: the values its forward multiplied with
        (coef * w rounded to the compute dtype, as the packed weight image holds them), for sg_pixel_norm_act_bwd_pw (to_rgb:
        cs = cout) and sg_conv3d_pw_bwd (from_rgb: cs = cin)."""
        key = ImageKey(RGB_MATRIX, w_rgb.data_ptr(), w_rgb._version, float(coef), bool(small_is_cin), dtype,
                       w_rgb.shape[-2], w_rgb.shape[-1], 1, 1, 1)
        hit = self._entries.get(key)
        return hit.image if hit is not None else self._build(key, w_rgb, None, None, None)

    def _build(self, key, w, shp, lib, st):
        """The one way an image is made and kept: the weight as f32 contiguous, the kind's pack, an entry if the weight will be
        there next time."""
        asked, key = key, key._replace(coef=float(key.coef), flip=bool(key.flip))
        if hash(asked) != hash(key) or asked != key:      # (a 0-d tensor, say: its lookups would miss every time, a pack per call)
            raise TypeError(f'the weight coefficient and flip are host numbers (float, int, bool, numpy scalar), got {asked.coef!r}, '
                            f'{asked.flip!r}')
        kind = key.kind
        w32 = w.detach()
        if w32.dtype != torch.float32 or not w32.is_contiguous():
            w32 = w32.contiguous().float()
        if kind.pack is None:
            image = (w32.reshape(key.cin, key.cout) * key.coef).to(key.dt).float()
            image = (image if key.flip else image.t()).contiguous()
        else:
            image = torch.empty(getattr(lib, kind.nbytes)(C.byref(shp), key.dt), device=w.device, dtype=torch.uint8)
            flip = (1 if key.flip else 0,) if kind.takes_flip else ()
            check(getattr(lib, kind.pack)(_ptr(w32), key.coef, *flip, _ptr(image), C.byref(shp), key.dt, st), kind.pack)
            if kind.counted:
                self.stats['single'] += 1
        # an in-place image needs the batch launch to find the values of the day where the key points: w32 must BE the weight
        if kind.keeps(w) and (not kind.in_place or w32.data_ptr() == w.data_ptr()):
            # holding the tensor keeps its storage (and so the key) from being recycled; for a view its DETACHED alias is held (same
            # storage, same version counter, no autograd node of the step that made the view)
            keep = ConvShape(shp.n, shp.d, shp.h, shp.w, shp.cin, shp.cout, shp.kd, shp.kh, shp.kw, shp.upsample_in) if kind.in_place else None
            self._entries[key] = ImageEntry(image, w if (w.is_leaf or not w.requires_grad) else w.detach(), keep)
        return image


IMAGES = WeightImages()
