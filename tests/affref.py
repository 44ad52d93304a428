"""numpy restatement of the affine discriminator augmentation (include/saragan_hip.h: sg_augment_affine_draw,
sg_augment_affine_apply).  The draw follows the header's word table in float64; the forward and the adjoint follow its steps
1-6 in np.float32 with one operation per statement, so the device results are compared bit for bit.  The adjoint is an ordered
scatter (np.add.at over (v ascending, k ascending)); it equals the kernel's gather order because one output voxel reaches a
given input voxel through at most one corner.  `dense` is an independent float64 matrix form for cross-checks."""
import numpy as np

from tests import augref

SCALE, ROTATE, SHIFT, BRIGHTNESS, CONTRAST, ALL = 32, 64, 128, 256, 512, 992
OPS = {'scale': SCALE, 'rotate': ROTATE, 'shift': SHIFT, 'brightness': BRIGHTNESS, 'contrast': CONTRAST}
KEY = 0x4155474D454E5432
F = np.float32


def row_of(lin=None, off=(0, 0, 0), a=1.0, b=0.0):
    """lin: 3 x 3 (default identity), off: the matrix's last column -> one float32 [16] parameter row."""
    r = np.zeros(16, F)
    m = np.eye(3) if lin is None else np.asarray(lin, np.float64)
    r[:12] = np.concatenate([m, np.asarray(off, np.float64).reshape(3, 1)], 1).reshape(12)
    r[12], r[13] = a, b
    return r


IDENTITY = row_of()


def shift_row(t, **kw):
    """out[v] = in[v - t] (augref.shift's convention), t in voxels, fractions allowed."""
    return row_of(off=[-float(s) for s in t], **kw)


def scale_row(s, shape, **kw):
    """u = c + (v - c) / s about the centre of a [d, h, w] volume."""
    c = (np.asarray(shape[:3], np.float64) - 1) / 2
    return row_of(np.eye(3) / s, c - c / s, **kw)


def quarter_turn_row(k, e):
    """np.rot90(sample, k, axes=(h, w)) on an e x e plane as a matrix row with entries 0 / +-1 and integer offsets."""
    lin, off = {1: ([[1, 0, 0], [0, 0, 1], [0, -1, 0]], (0, 0, e - 1)),
                2: ([[1, 0, 0], [0, -1, 0], [0, 0, -1]], (0, e - 1, e - 1)),
                3: ([[1, 0, 0], [0, 0, -1], [0, 1, 0]], (0, e - 1, 0))}[k & 3]
    return row_of(lin, off)


def shear_row(g):
    return row_of([[1, 0, 0], [0, 1, g], [0, 0, 1]])


def bf16_round(x):
    """float32 -> the nearest bfloat16 (ties to even), returned as float32.  Finite values only."""
    u = np.ascontiguousarray(x, F).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(F).reshape(np.shape(x))


# ---- the draw ----------------------------------------------------------------------------------------------------------------
def draw(n, ops, extent, p, seed, offset, max_scale=1.25, max_angle=np.pi, max_shift=(0.0, 0.0, 0.0), max_brightness=0.2,
         max_contrast=1.5, return_gates=False):
    """-> float32 [n, 16] (and bool [n, 5] gates scale, rotate, shift, brightness, contrast of the enabled transforms)."""
    ctr = (np.uint64(int(offset) & (2 ** 64 - 1)) + np.arange(n, dtype=np.uint64))
    key = (int(seed) ^ KEY) & (2 ** 64 - 1)
    kk = np.array([key & 0xFFFFFFFF, key >> 32], dtype=np.uint32)
    blocks = []
    for j in range(3):
        c4 = np.stack([ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), np.full(n, j, np.uint64), np.zeros(n, np.uint64)], -1)
        blocks.append(augref.philox4x32_10(c4.astype(np.uint32), kk).astype(np.uint64))
    a, b, c = blocks
    thr = np.uint64(augref.threshold(p))

    def gate(r, bit):
        return (r < thr) if ops & bit else np.zeros(n, bool)

    def sym(r):
        return 2.0 * (r.astype(np.float64) * (1.0 / 4294967296.0)) - 1.0

    g_sc, g_rot, g_sh, g_br = gate(a[:, 0], SCALE), gate(a[:, 1], ROTATE), gate(a[:, 2], SHIFT), gate(a[:, 3], BRIGHTNESS)
    g_ct = gate(b[:, 0], CONTRAST)
    inv = np.where(g_sc, 1.0 / np.exp2(sym(b[:, 1]) * np.log2(max_scale)), 1.0)
    theta = sym(b[:, 2]) * float(max_angle)
    sn, cs = np.sin(theta), np.cos(theta)
    bias = np.where(g_br, sym(b[:, 3]) * float(max_brightness), 0.0)
    gain = np.where(g_ct, np.exp2(sym(c[:, 0]) * np.log2(max_contrast)), 1.0)
    t = [np.where(g_sh, sym(c[:, 1 + ax]) * float(max_shift[ax]), 0.0) for ax in range(3)]
    a_dd = inv
    a_hh = np.where(g_rot, cs * inv, inv)
    a_hw = np.where(g_rot, sn * inv, 0.0)
    a_wh = np.where(g_rot, -(sn * inv), 0.0)
    cen = [(int(e) - 1) * 0.5 for e in extent]
    q = [cen[ax] + t[ax] for ax in range(3)]
    out = np.zeros((n, 16), np.float64)
    out[:, 0], out[:, 3] = a_dd, cen[0] - a_dd * q[0]
    out[:, 5], out[:, 6], out[:, 7] = a_hh, a_hw, cen[1] - (a_hh * q[1] + a_hw * q[2])
    out[:, 9], out[:, 10], out[:, 11] = a_wh, a_hh, cen[2] - (a_wh * q[1] + a_hh * q[2])
    out[:, 12], out[:, 13] = gain, bias
    out = out.astype(F)
    if return_gates:
        return out, np.stack([g_sc, g_rot, g_sh, g_br, g_ct], -1)
    return out


# ---- steps 1-4: what one output voxel reads -----------------------------------------------------------------------------------
def geometry(row, d, h, w):
    """For every output voxel v in linear order (V = d h w): sup [V] (step 2), W [V, 8] float32 (step 4), tgt [V, 8] the linear
    index of corner k's voxel (clipped where out of range), inr [V, 8] whether it lies in the volume."""
    row = np.asarray(row, F)
    vd, vh, vw = (g.reshape(-1).astype(F) for g in np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing='ij'))
    ext = (d, h, w)
    sup = np.ones(d * h * w, bool)
    f, w0, w1 = [], [], []
    with np.errstate(all='ignore'):
        for ax in range(3):
            p0 = row[4 * ax] * vd
            p1 = row[4 * ax + 1] * vh
            p2 = row[4 * ax + 2] * vw
            s = p0 + p1
            s = s + p2
            u = s + row[4 * ax + 3]
            ok = (u > F(-1)) & (u < F(ext[ax]))
            sup &= ok
            u = np.where(ok, u, F(0))
            fl = np.floor(u)
            r = u - fl
            f.append(fl.astype(np.int64))
            w0.append(F(1) + (-r))
            w1.append(r)
        W = np.zeros((d * h * w, 8), F)
        tgt = np.zeros((d * h * w, 8), np.int64)
        inr = np.zeros((d * h * w, 8), bool)
        for k in range(8):
            bd, bh, bw = k >> 2, (k >> 1) & 1, k & 1
            t = (w1[0] if bd else w0[0]) * (w1[1] if bh else w0[1])
            t = t * (w1[2] if bw else w0[2])
            W[:, k] = t * row[12]
            i_d, i_h, i_w = f[0] + bd, f[1] + bh, f[2] + bw
            inr[:, k] = (i_d >= 0) & (i_d < d) & (i_h >= 0) & (i_h < h) & (i_w >= 0) & (i_w < w)
            tgt[:, k] = (np.clip(i_d, 0, d - 1) * h + np.clip(i_h, 0, h - 1)) * w + np.clip(i_w, 0, w - 1)
    return sup, W, tgt, inr


def forward_one(x, row, fill=0.0, linear=False):
    """x: one sample [d, h, w, c] float32 -> float32 (step 5; round to the output type afterwards)."""
    x = np.asarray(x, F)
    d, h, w, c = x.shape
    row = np.asarray(row, F)
    fill = F(0) if linear else F(fill)
    a, b = row[12], (F(0) if linear else row[13])
    sup, W, tgt, inr = geometry(row, d, h, w)
    xf = x.reshape(-1, c)
    acc = np.zeros((d * h * w, c), F)
    started = np.zeros(d * h * w, bool)
    with np.errstate(all='ignore'):
        for k in range(8):
            use = sup & (W[:, k] != 0)
            xk = np.where(inr[:, k, None], xf[tgt[:, k]], fill)
            term = W[:, k, None] * xk
            acc = np.where((use & started)[:, None], acc + term, np.where(use[:, None], term, acc))
            started |= use
        acc = np.where(sup[:, None], acc, a * fill)
        if b != 0:
            acc = acc + b
    return acc.astype(F).reshape(x.shape)


def adjoint_one(gy, row):
    """gy: one sample [d, h, w, c] float32 -> float32 (step 6)."""
    gy = np.asarray(gy, F)
    d, h, w, c = gy.shape
    sup, W, tgt, inr = geometry(row, d, h, w)
    use = (sup[:, None] & inr & (W != 0)).reshape(-1)            # (v ascending, k ascending)
    src = np.repeat(np.arange(d * h * w), 8)[use]
    dst = tgt.reshape(-1)[use]
    with np.errstate(all='ignore'):
        terms = W.reshape(-1)[use][:, None] * gy.reshape(-1, c)[src]
        gx = np.full((d * h * w, c), -0.0, F)                    # -0.0 + t == t for every t: the first term starts the sum
        np.add.at(gx, dst, terms.astype(F))
    touched = np.zeros(d * h * w, bool)
    touched[dst] = True
    gx[~touched] = 0.0
    return gx.reshape(gy.shape)


def forward(x, rows, fill=0.0, linear=False):
    """x: [n, d, h, w, c] (NDHWC); rows: [n, 16]."""
    rows = np.asarray(rows, F).reshape(x.shape[0], 16)
    return np.stack([forward_one(x[i], rows[i], fill, linear) for i in range(x.shape[0])])


def adjoint(gy, rows):
    rows = np.asarray(rows, F).reshape(gy.shape[0], 16)
    return np.stack([adjoint_one(gy[i], rows[i]) for i in range(gy.shape[0])])


def summands(rows, shape):
    """The largest number of summands of any output of either pass over these rows ([d, h, w] volumes): per output voxel of the
    forward its nonzero-weight corners (+1 for a bias), per input voxel of the adjoint the output voxels that reach it."""
    d, h, w = shape
    most = 1
    for row in np.asarray(rows, F).reshape(-1, 16):
        sup, W, tgt, inr = geometry(row, d, h, w)
        fwd = (sup[:, None] & (W != 0)).sum(1).max() + (1 if row[13] != 0 else 0)
        use = (sup[:, None] & inr & (W != 0)).reshape(-1)
        adj = np.bincount(tgt.reshape(-1)[use], minlength=1).max() if use.any() else 0
        most = max(most, int(fwd), int(adj))
    return most


# ---- an independent float64 form ---------------------------------------------------------------------------------------------
def dense(row, d, h, w):
    """-> (M [V, V] float64, f [V] float64): forward(x) = M x + f * fill + b per channel, adjoint(g) = M^T g.  Coordinates,
    weights and products in float64 by plain loops."""
    row = np.asarray(row, np.float64)
    A, a = row[:12].reshape(3, 4), row[12]
    ext = (d, h, w)
    V = d * h * w
    M, f = np.zeros((V, V)), np.zeros(V)
    for v in range(V):
        vv = (v // (h * w), (v // w) % h, v % w)
        u = [A[ax, 0] * vv[0] + A[ax, 1] * vv[1] + A[ax, 2] * vv[2] + A[ax, 3] for ax in range(3)]
        if not all(-1 < u[ax] < ext[ax] for ax in range(3)):
            f[v] = a
            continue
        fl = [int(np.floor(t)) for t in u]
        r = [u[ax] - fl[ax] for ax in range(3)]
        for k in range(8):
            bits = (k >> 2, (k >> 1) & 1, k & 1)
            wk = a
            for ax in range(3):
                wk = wk * (r[ax] if bits[ax] else 1.0 - r[ax])
            if wk == 0:
                continue
            i = [fl[ax] + bits[ax] for ax in range(3)]
            if all(0 <= i[ax] < ext[ax] for ax in range(3)):
                M[v, (i[0] * h + i[1]) * w + i[2]] += wk
            else:
                f[v] += wk
    return M, f
