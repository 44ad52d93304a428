"""numpy restatement of the discriminator augmentation (include/saragan_hip.h: sg_augment_draw, sg_augment_apply,
sg_ada_update): the transforms through np.flip / np.rot90 / slicing, the draw through a numpy Philox4x32-10 and the
header's word assignment, the controller in np.float32.  Everything here is exact: the device results are compared
bit for bit."""
import numpy as np

FLIP_W, FLIP_H, FLIP_D, ROT90, TRANSLATE, ALL = 1, 2, 4, 8, 16, 31
OPS = {'flip_w': FLIP_W, 'flip_h': FLIP_H, 'flip_d': FLIP_D, 'rot90': ROT90, 'translate': TRANSLATE}
KEY = 0x4155474D454E5431
IDENTITY = (0, 0, 0, 0, 0, 0, 0, 0)


def params_of(flip_d=0, flip_h=0, flip_w=0, k=0, t=(0, 0, 0)):
    return (int(flip_d), int(flip_h), int(flip_w), int(k), int(t[0]), int(t[1]), int(t[2]), 0)


def shift(a, t, fill):
    """out[v] = a[v - t] where v - t is in range, else fill; a: [d, h, w, c], t: three ints."""
    out = np.full_like(a, fill)
    dst, src = [], []
    for ax in range(3):
        e, s = a.shape[ax], int(t[ax])
        if abs(s) >= e:
            return out
        dst.append(slice(max(s, 0), e + min(s, 0)))
        src.append(slice(max(-s, 0), e + min(-s, 0)))
    out[tuple(dst)] = a[tuple(src)]
    return out


def apply_one(a, prm, fill=0.0, adjoint=False):
    """a: one sample [d, h, w, c]; prm: its 8 parameters."""
    fd, fh, fw, k, td, th, tw = (int(v) for v in prm[:7])
    axes = tuple(ax for ax, f in ((0, fd), (1, fh), (2, fw)) if f)
    k &= 3
    if k and a.shape[1] != a.shape[2]:
        raise ValueError('rot90 needs h == w')
    if not adjoint:
        y = np.flip(a, axes) if axes else a
        y = np.rot90(y, k, axes=(1, 2))
        return shift(y, (td, th, tw), fill)
    y = shift(a, (-td, -th, -tw), 0)
    y = np.rot90(y, -k, axes=(1, 2))
    return np.ascontiguousarray(np.flip(y, axes) if axes else y)


def apply(x, params, fill=0.0, adjoint=False):
    """x: [n, d, h, w, c] (NDHWC); params: [n, 8] ints."""
    params = np.asarray(params).reshape(x.shape[0], 8)
    return np.stack([apply_one(x[i], params[i], fill, adjoint) for i in range(x.shape[0])])


def philox4x32_10(ctr, key):
    """ctr: uint32 [..., 4]; key: uint32 [..., 2] (broadcast) -> uint32 [..., 4]."""
    c = [np.asarray(ctr[..., j], dtype=np.uint64) for j in range(4)]
    key = np.asarray(key, dtype=np.uint64)
    k0, k1 = key[..., 0] + np.zeros_like(c[0]), key[..., 1] + np.zeros_like(c[0])
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & m32
        k1 = (k1 + np.uint64(0xBB67AE85)) & m32
    return np.stack(c, axis=-1).astype(np.uint32)


def threshold(p):
    p = float(np.float32(p))
    if not p > 0.0:
        return 0
    return 1 << 32 if p >= 1.0 else int(p * 4294967296.0)


def draw(n, ops, max_shift, p, seed, offset, return_gates=False):
    """-> int32 [n, 8] (and bool [n, 5] gates flip_w, flip_h, flip_d, rot90, translate of the enabled transforms)."""
    ctr = (np.uint64(int(offset) & (2 ** 64 - 1)) + np.arange(n, dtype=np.uint64))
    key = (int(seed) ^ KEY) & (2 ** 64 - 1)
    kk = np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint32)
    blocks = []
    for j in range(3):
        c4 = np.stack([ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), np.full(n, j, np.uint64), np.zeros(n, np.uint64)], -1)
        blocks.append(philox4x32_10(c4.astype(np.uint32), kk).astype(np.uint64))
    a, b, c = blocks
    thr = np.uint64(threshold(p))

    def gate(r, bit):
        return (r < thr) if ops & bit else np.zeros(n, bool)

    def value(r, cnt):
        return ((r * np.uint64(cnt)) >> np.uint64(32)).astype(np.int64)

    g_fw, g_fh, g_fd, g_rot = gate(a[:, 0], FLIP_W), gate(a[:, 1], FLIP_H), gate(a[:, 2], FLIP_D), gate(a[:, 3], ROT90)
    g_tr = gate(b[:, 0], TRANSLATE)
    m_d, m_h, m_w = (int(m) for m in max_shift)
    out = np.zeros((n, 8), np.int64)
    out[:, 0] = np.where(g_fd, value(b[:, 3], 2), 0)
    out[:, 1] = np.where(g_fh, value(b[:, 2], 2), 0)
    out[:, 2] = np.where(g_fw, value(b[:, 1], 2), 0)
    out[:, 3] = np.where(g_rot, value(c[:, 0], 4), 0)
    out[:, 4] = np.where(g_tr, value(c[:, 1], 2 * m_d + 1) - m_d, 0)
    out[:, 5] = np.where(g_tr, value(c[:, 2], 2 * m_h + 1) - m_h, 0)
    out[:, 6] = np.where(g_tr, value(c[:, 3], 2 * m_w + 1) - m_w, 0)
    out = out.astype(np.int32)
    if return_gates:
        return out, np.stack([g_fw, g_fh, g_fd, g_rot, g_tr], -1)
    return out


def ada_update(state, p, logits, interval, target_num, target_den, delta, p_max):
    """state: four Python ints (sum_sign, count, steps, adjustments); p: np.float32 -> (state, p) after one call."""
    logits = np.asarray(logits, np.float32).reshape(-1)
    s = int((logits > 0).sum()) - int((logits < 0).sum())
    sum_sign, count, steps, adj = state[0] + s, state[1] + logits.size, state[2] + 1, state[3]
    p = np.float32(p)
    if steps % interval == 0:
        up = sum_sign * int(target_den) > int(target_num) * count
        q = np.float32(p + (np.float32(delta) if up else -np.float32(delta)))
        p = np.float32(min(max(q, np.float32(0.0)), np.float32(p_max)))
        adj += 1
        sum_sign = count = 0
    return (sum_sign, count, steps, adj), p
