"""numpy restatement of the dataset pyramid (include/saragan_hip.h, sg_block_pyramid), written the way the
original's conversion script works and not the way the kernel does: pad every volume with np.pad(constant_values=pad_value),
crop it as crop_to does, subtract the intercept (int64, or float32 for float sources), reshape to [D/b, b, H/b, b, W/b, b] and
take .mean(axis=(1, 3, 5), dtype=np.float64) or the maximum, np.clip, .astype.  (Reshape-mean is skimage's block_reduce with
np.average for divisible shapes.)  Nothing here imports the package."""
import numpy as np

RANGE = {np.dtype(np.uint16): (0, 65535), np.dtype(np.int16): (-32768, 32767)}


def pad_to(data, target, anchor):
    """The original's pad_to: a centred axis gets floor(p / 2) in front and ceil(p / 2) behind; 'start' pads at the end of the axis
    (its center=False), 'end' in front."""
    pads = []
    for s, t, a in zip(data.shape, target, anchor):
        p = t - s
        if p <= 0:
            pads.append((0, 0))
        elif a == 'center':
            pads.append((int(np.floor(p / 2)), int(np.ceil(p / 2))))
        elif a == 'start':
            pads.append((0, p))
        else:
            pads.append((p, 0))
    return pads


def crop_to(shape, target, anchor):
    """The original's crop_to: a centred axis starts at S // 2 - T // 2; 'start' keeps the front, 'end' the back."""
    starts = []
    for s, t, a in zip(shape, target, anchor):
        starts.append(s // 2 - t // 2 if a == 'center' else 0 if a == 'start' else s - t)
    return starts


def window(vol, target, pad_value, anchor=('center',) * 3):
    """One volume [d, h, w] padded, then cropped, to the target."""
    vol = np.pad(vol, pad_to(vol, target, anchor), mode='constant', constant_values=pad_value)
    st = crop_to(vol.shape, target, anchor)
    out = vol[st[0]:st[0] + target[0], st[1]:st[1] + target[1], st[2]:st[2] + target[2]]
    assert out.shape == tuple(target)
    return out


def pyramid(x, target, levels, reduce='mean', intercept=0, pad_value=None, clip=None, out_dtype=np.uint16, anchor=('center',) * 3):
    """A list of `levels` arrays [n, D >> i, H >> i, W >> i] of out_dtype from x [n, sd, sh, sw] (a numpy array)."""
    x = np.asarray(x)
    out_dtype = np.dtype(out_dtype)
    pad_value = intercept if pad_value is None else pad_value
    is_int = x.dtype.kind in 'iu'
    if is_int:
        wide = x.astype(np.int64)
        v = np.stack([window(vol, target, int(pad_value), anchor) for vol in wide]) - np.int64(intercept) if len(x) else \
            np.zeros((0,) + tuple(target), np.int64)
    else:
        wide = x.astype(np.float32)
        v = np.stack([window(vol, target, np.float32(pad_value), anchor) for vol in wide]) - np.float32(intercept)
        assert v.dtype == np.float32
    if clip is None:
        clip = RANGE.get(out_dtype, (-np.inf, np.inf))
    n, (D, H, W) = v.shape[0], target
    outs = []
    for i in range(levels):
        b = 1 << i
        cubes = v.reshape(n, D // b, b, H // b, b, W // b, b)
        with np.errstate(invalid='ignore'):
            if reduce == 'mean':
                m = cubes.mean(axis=(2, 4, 6), dtype=np.float64)
            elif is_int:
                m = cubes.max(axis=(2, 4, 6))
            else:      # NaN voxels are ignored; a cube of nothing else gives -inf
                m = cubes
                for ax in (6, 4, 2):
                    m = np.fmax.reduce(m, axis=ax, initial=np.float32(-np.inf))
            if not is_int:
                m = m.astype(np.float32)      # (the one rounding; the clip below is in float32)
                lo, hi = np.float32(clip[0]), np.float32(clip[1])
            else:
                lo, hi = clip
            outs.append(np.clip(m, lo, hi).astype(out_dtype))
    return outs


def stats(levels_of_arrays):
    """int64 [n, levels, 4]: sum, sum of squares, minimum, maximum of every level's stored values, per sample."""
    n = levels_of_arrays[0].shape[0]
    out = np.zeros((n, len(levels_of_arrays), 4), np.int64)
    for i, a in enumerate(levels_of_arrays):
        s = a.reshape(n, -1).astype(np.int64)
        out[:, i] = np.stack([s.sum(1), (s * s).sum(1), s.min(1), s.max(1)], axis=1)
    return out
