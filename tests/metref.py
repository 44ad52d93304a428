"""Plain references for the validation-metric kernels (csrc/metrics.hip), written from the definitions in the header
comment of that file, include/saragan_hip.h, the reference's metrics/swd.py and scikit-image's published SSIM, and not from
the kernels: numpy float64, Python integers / fractions.Fraction and math.fsum, loops where loops are clearest.
tests/test_metref_host.py checks them on the CPU against scipy and oracle/metrics_oracle.py, and checks that deliberately
wrong variants give other answers on the very inputs of tests/test_metrics_exact_gpu.py (the input sets at the end of
this file).

Exactness recipe of the GPU tests: small integers (|x| <= 8) and dyadic taps (integers / 64).  Every product and every
partial sum is then a small multiple of a power of two that float32 (24 bits) and float64 (53 bits) hold exactly, so a sum
is the same in every order and in both precisions, and the comparison is `==`."""
import math
from fractions import Fraction

import numpy as np

MIRROR, REFLECT = 0, 1
U32, U64 = 2.0 ** -24, 2.0 ** -53          # unit roundoffs of float32 and float64


# ---- sg_filter_axis ------------------------------------------------------------------------------------------------
def border_index(i, n, border):
    """Index into a line of n samples for ANY integer i, by scipy.ndimage's rules.  The line is continued periodically:
    'mirror' (0) repeats  a b c d | c b  (the edge samples are not doubled: d c b | a b c d | c b a), 'reflect' (1) repeats
    a b c d | d c b a  (they are: d c b a | a b c d | d c b a)."""
    fwd = list(range(n))
    if border == MIRROR:
        seq = fwd + fwd[-2:0:-1]
    elif border == REFLECT:
        seq = fwd + fwd[::-1]
    else:
        raise ValueError(border)
    return seq[i % len(seq)]            # Python's % is non-negative


def filter_axis(x, taps, mode, border, alpha=1.0, add=None):
    """x [outer, n, inner] -> float64 [outer, n_out, inner]:  alpha * value + add  with r = len(taps) // 2 and
      mode 0  value[o] = sum_t taps[t] x[B(o + t - r)]                                   n_out = n
      mode 1  the same at the kept samples 2 o                                           n_out = ceil(n / 2)
      mode 2  value[o] = sum_t taps[t] z[B(o + t - r)], z[2k] = x[k], z[odd] = 0,         n_out = 2 n,
              the border rule B applied on z's extent 2 n.
    A correlation (taps[t] meets the sample t - r to the right), vectorised over outer and inner only."""
    x = np.asarray(x, dtype=np.float64)
    assert x.ndim == 3 and len(taps) % 2 == 1
    outer, n, inner = x.shape
    r = len(taps) // 2
    if mode == 2:
        src = np.zeros((outer, 2 * n, inner))
        src[:, 0::2, :] = x
        centres = range(2 * n)
    elif mode == 1:
        src, centres = x, range(0, n, 2)
    elif mode == 0:
        src, centres = x, range(n)
    else:
        raise ValueError(mode)
    ext = src.shape[1]
    out = np.zeros((outer, len(centres), inner))
    for o, c in enumerate(centres):
        for t, tap in enumerate(taps):
            out[:, o, :] += float(tap) * src[:, border_index(c + t - r, ext, border), :]
    out *= float(alpha)
    if add is not None:
        out += np.asarray(add, dtype=np.float64)
    return out


# ---- sg_swd_gather -------------------------------------------------------------------------------------------------
def gather(x, d0, h0, w0, per_image, rd, rh, rw):
    """x [n_img, c, d, h, w]; centres d0, h0, w0 [n_img * per_image] -> [N, c, 2rd+1, 2rh+1, 2rw+1].  The reference's quirk
    (metrics/swd.py:20-25), index by index: the FOURTH output axis has 2rh+1 entries, and its offset j - rh moves the W
    coordinate; the FIFTH has 2rw+1, and its offset k - rw moves the H coordinate:
        out[nh, ch, i, j, k] = x[nh // per_image, ch, d0[nh] + i - rd, h0[nh] + (k - rw), w0[nh] + (j - rh)].
    A coordinate outside the volume is an error here (numpy would wrap a negative one silently)."""
    x = np.asarray(x)
    n_img, c, d, h, w = x.shape
    d0, h0, w0 = (np.asarray(v, dtype=np.int64).reshape(-1) for v in (d0, h0, w0))
    N = n_img * per_image
    assert d0.shape == h0.shape == w0.shape == (N,)
    img = np.arange(N) // per_image
    out = np.empty((N, c, 2 * rd + 1, 2 * rh + 1, 2 * rw + 1), dtype=x.dtype)
    for i in range(2 * rd + 1):
        for j in range(2 * rh + 1):
            for k in range(2 * rw + 1):
                dd, hh, ww = d0 + (i - rd), h0 + (k - rw), w0 + (j - rh)
                for v, ext, name in ((dd, d, 'D'), (hh, h, 'H'), (ww, w, 'W')):
                    if v.min() < 0 or v.max() >= ext:
                        raise IndexError(f'{name} coordinate outside [0, {ext}) at offset ({i}, {j}, {k})')
                out[:, :, i, j, k] = x[img, :, dd, hh, ww]       # [N, c]: one voxel per neighbourhood and channel
    return out


def gather_centres_in_bounds(shape, d0, h0, w0, rd, rh, rw):
    """The precondition of sg_swd_gather on its centres, with the quirk's real offsets: D centre in [rd, d - rd), H centre
    in [rw, h - rw), W centre in [rh, w - rh)."""
    _, _, d, h, w = shape
    ok = lambda v, r, ext: bool((np.asarray(v) >= r).all() and (np.asarray(v) < ext - r).all())
    return ok(d0, rd, d) and ok(h0, rw, h) and ok(w0, rh, w)


# ---- sg_desc_normalize ---------------------------------------------------------------------------------------------
def _channel_stats(desc):
    """(mean, population variance, mean of squares) per channel of desc [n, c, ...]: fsum, variance by the two-pass form."""
    desc = np.asarray(desc, dtype=np.float64)
    c = desc.shape[1]
    mean, var, msq = np.empty(c), np.empty(c), np.empty(c)
    for ch in range(c):
        v = desc[:, ch].reshape(-1)
        mean[ch] = math.fsum(v) / v.size
        var[ch] = math.fsum((v - mean[ch]) ** 2) / v.size
        msq[ch] = math.fsum(v * v) / v.size
    return mean, var, msq


def normalize(desc):
    """finalize_descriptors (swd.py:31-39): (desc - mean_c) / std_c, population mean and std of channel c over every other
    axis of desc [n, c, ...], in float64."""
    desc = np.asarray(desc, dtype=np.float64)
    mean, var, _ = _channel_stats(desc)
    shape = (1, -1) + (1,) * (desc.ndim - 2)
    return (desc - mean.reshape(shape)) / np.sqrt(var).reshape(shape)


def normalize_bound(desc, want):
    """|float32 result - want| for a kernel that accumulates s = sum v and ss = sum v^2 of a channel's N values in float64 in
    any order and forms  mean = s / N,  var = ss / N - mean^2,  out = float32((v - mean) * (1 / sqrt(var))).
    With u = 2^-53, A = mean |v| and Q = mean v^2 of the channel (first order in u, the slack absorbs the second):
      |s^ - s| <= (N - 1) u sum |v|, and the division rounds once:             |mean^ - mean| <= em = (N + 1) u A
      ss^: N squares rounded, then summed: (N + 1) u ss; / N rounds once:     |ss^/N - Q| <= (N + 2) u Q
      mean^^2: 2 |mean| em + u mean^2 <= (2 N + 3) u Q  (|mean| A <= Q and mean^2 <= Q); the subtraction rounds once: u var <= u Q
      =>  |var^ - var| <= ev = (3 N + 8) u Q,    rho = ev / var  (the cancellation of ss / N - mean^2 shows here: Q / var)
      1 / sqrt(var^) is off by rho / 2 relatively, sqrt and the division round once each: below rho + 2 u  (rho < 0.1)
      (v - mean^) rounds once, the product once:   t64 = em / std + |want| (rho + 4 u)
      the float32 store rounds what was computed:  2^-24 (|want| + t64)
    The reference (`normalize`, fsum and a two-pass variance) is off by a few u |want|, inside the slack of rho."""
    desc = np.asarray(desc, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    mean, var, msq = _channel_stats(desc)
    N = desc.size // desc.shape[1]
    shape = (1, -1) + (1,) * (desc.ndim - 2)
    a = np.array([math.fsum(np.abs(desc[:, ch]).reshape(-1)) / N for ch in range(desc.shape[1])])
    em = (N + 1) * U64 * a
    rho = (3 * N + 8) * U64 * msq / var
    assert (rho < 0.1).all(), rho
    t64 = (em / np.sqrt(var)).reshape(shape) + np.abs(want) * (rho.reshape(shape) + 4 * U64)
    return U32 * (np.abs(want) + t64) + t64


# ---- sg_swd_project / sg_sort_rows / sg_swd_distance ---------------------------------------------------------------
def project(a, dirs, npad):
    """pt [ndirs, npad] float64: pt[dir][row] = sum_k a[row][k] * dirs[k][dir] in float64 for row < n, +inf in rows n..npad."""
    a, dirs = np.asarray(a, dtype=np.float64), np.asarray(dirs, dtype=np.float64)
    n, f = a.shape
    assert dirs.shape[0] == f and npad >= n
    pt = np.full((dirs.shape[1], npad), np.inf)
    for dr in range(dirs.shape[1]):
        pt[dr, :n] = (a * dirs[:, dr][None, :]).sum(axis=1)
    return pt


def gamma(n, u=U32):
    """Higham's gamma_n = n u / (1 - n u): n successive roundings of relative size u compound to at most this."""
    assert n * u < 1
    return n * u / (1 - n * u)


def project_bound(a, dirs):
    """[ndirs, n]: a chain of f fused multiply-adds in float32 rounds f times, so (Higham, Accuracy and Stability, 3.1)
    |computed - exact| <= gamma_f sum_k |a_k| |d_k| in ANY order of the k.  The float64 reference of `project` is itself
    within gamma_f(2^-53) of that sum; that term is added."""
    a, dirs = np.abs(np.asarray(a, dtype=np.float64)), np.abs(np.asarray(dirs, dtype=np.float64))
    f = a.shape[1]
    return (gamma(f, U32) + gamma(f + 1, U64)) * (1 + 2 * f * U64) * (a @ dirs).T


def sort_rows(p):
    return np.sort(np.asarray(p), axis=1)


def distance_rows(pa, pb, n):
    """out[1 + row] of sg_swd_distance: sum_{i < n} |pa[row][i] - pb[row][i]|, the difference and abs in float32 (as
    np.abs(pa - pb) of the reference's float32 projections), the sum exact (fsum)."""
    pa, pb = np.asarray(pa, dtype=np.float32), np.asarray(pb, dtype=np.float32)
    diff = np.abs(pa[:, :n] - pb[:, :n])
    assert diff.dtype == np.float32
    return np.array([math.fsum(row.astype(np.float64)) for row in diff])


def distance(pa, pb, n):
    """np.mean(np.abs(pa - pb)) over the rows * n compared entries (the +inf padding past n is never compared)."""
    rows = distance_rows(pa, pb, n)
    return math.fsum(rows) / (len(rows) * n)


# ---- sg_sqdiff_mean / sg_minmax ------------------------------------------------------------------------------------
def sqdiff_mean(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    return math.fsum((a - b) ** 2) / a.size


def minmax(a):
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    lo = hi = float(a[0])
    for v in a.tolist():
        lo, hi = (v if v < lo else lo), (v if v > hi else hi)
    return lo, hi


# ---- sg_ssim_mean --------------------------------------------------------------------------------------------------
_FRAC_BITS = 256


def _common_ints(arrays, scalars):
    """Every float64 is an integer times a power of two: returns K, the arrays as lists of Python integers and the scalars as
    integers, all in units of 2^-K."""
    arrays = [np.asarray(a, dtype=np.float64).reshape(-1) for a in arrays]
    every = np.concatenate(arrays + [np.asarray(scalars, dtype=np.float64)])
    assert np.isfinite(every).all()
    m, e = np.frexp(every[every != 0])                      # v = m 2^e, m 2^53 an integer
    M = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = np.log2((M & -M).astype(np.float64)).astype(np.int64)         # trailing zero bits of the mantissa
    K = int(max(0, (53 - low - e).max())) if M.size else 0
    ints = lambda a: [int(v) for v in np.ldexp(a, K).tolist()]          # exact: ldexp only moves the exponent
    return K, [ints(a) for a in arrays], ints(np.asarray(scalars, dtype=np.float64))


def ssim_box_sums(ux, uy, uxx, uyy, uxy, shape, c, lo, hi, cov_norm, C1, C2):
    """(sum S, sum |S|, count) over the voxels lo[a] <= i_a < hi[a] of the channels-last map [s0, s1, s2, c] of
        S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),   v** = cov_norm (u** - u* u*)
    (Wang et al. 2004 as scikit-image's structural_similarity evaluates it).  Every S is an exact rational of Python
    integers; the two sums carry 256 fractional bits (each quotient floored to 2^-256, so they are exact to count * 2^-256)."""
    s0, s1, s2 = shape
    K, (UX, UY, UXX, UYY, UXY), (CN, c1, c2) = _common_ints([ux, uy, uxx, uyy, uxy], [cov_norm, C1, C2])
    c1 <<= K                  # units of 2^-2K, as ux * uy
    c2 <<= 2 * K              # units of 2^-3K, as cov_norm * (uxy - ux uy)
    total = total_abs = count = 0
    for i0 in range(max(lo[0], 0), min(hi[0], s0)):
        for i1 in range(max(lo[1], 0), min(hi[1], s1)):
            for i2 in range(max(lo[2], 0), min(hi[2], s2)):
                for ch in range(c):
                    e = ((i0 * s1 + i1) * s2 + i2) * c + ch
                    mx, my = UX[e], UY[e]
                    vx, vy, vxy = CN * ((UXX[e] << K) - mx * mx), CN * ((UYY[e] << K) - my * my), CN * ((UXY[e] << K) - mx * my)
                    num = (2 * mx * my + c1) * (2 * vxy + c2)
                    den = (mx * mx + my * my + c1) * (vx + vy + c2)
                    q = (num << _FRAC_BITS) // den
                    total += q
                    total_abs += abs(q)
                    count += 1
    one = 1 << _FRAC_BITS
    return Fraction(total, one), Fraction(total_abs, one), count


def ssim_mean(ux, uy, uxx, uyy, uxy, shape, c, crop0, crop, cov_norm, C1, C2):
    """Mean of S over the map cropped by crop0 on BOTH sides of the first spatial axis and by crop on both sides of the
    other two, every channel: a Fraction."""
    s0, s1, s2 = shape
    total, _, count = ssim_box_sums(ux, uy, uxx, uyy, uxy, shape, c, (crop0, crop, crop), (s0 - crop0, s1 - crop, s2 - crop),
                                    cov_norm, C1, C2)
    assert count == (s0 - 2 * crop0) * (s1 - 2 * crop) * (s2 - 2 * crop) * c and count > 0
    return total / count


def ssim_mean_bound(sum_abs, count):
    """|kernel - ssim_mean| when numerator and denominator of every S_i are exact in float64 (dyadic moments of few bits):
    the quotient rounds once (u |S_i|), N = count terms summed in any order add at most gamma_(N-1) sum |S_i|, the division
    by N rounds once:  (1 + u)^(N + 1) - 1 <= (N + 2) u  for N u < 0.01.  So  (N + 2) 2^-53 sum |S_i| / N  (a Fraction)."""
    assert count * U64 < 0.01
    return (count + 2) * Fraction(1, 2 ** 53) * sum_abs / count


# ======== the input sets of tests/test_metrics_exact_gpu.py (tests/test_metref_host.py runs its mutants on them) ========
def _ints(rng, shape, lo=-8, hi=8, nonzero=False):
    v = rng.integers(lo, hi + 1, size=shape)
    if nonzero:
        v = np.where(v == 0, hi, v)
    return v.astype(np.float64)


FILTER_N, FILTER_NTAPS, FILTER_OUTER, FILTER_INNER = (1, 2, 3, 7, 16, 33), (1, 3, 5, 11, 15), (1, 3), (1, 5)
FILTER_ALPHA = (1.0, 2.0, -2.0, 0.5)
FILTER_WRAP = (1, 2100, 2048, 5, 0, MIRROR)         # outer, n, inner, ntaps, mode, border: 4 300 800 outputs > 16384 * 256


def filter_taps(ntaps):
    """Non-zero integers in [-8, 8] over 64, no two mirror-image taps equal (a convolution differs from the correlation)."""
    t = _ints(np.random.default_rng(1000 + ntaps), ntaps, nonzero=True)
    for k in range(ntaps // 2):
        if t[k] == t[ntaps - 1 - k]:
            t[k] = -t[k]
    return t / 64.0


def filter_input(outer, n, inner):
    """Non-zero integers in [-8, 8], float64.  |value| <= 15 * 8 * 8 / 64, times |alpha| <= 2 plus |add| <= 8: below 2^6 in units of
    2^-7, exact in float32."""
    x = _ints(np.random.default_rng(7 * outer + 131 * n + 17 * inner), (outer, n, inner), nonzero=True)
    for k in range(n // 2):             # no line is its own mirror image in any pair of samples (a short one easily is)
        x[:, k, :] = np.where(x[:, k, :] == x[:, n - 1 - k, :], -x[:, k, :], x[:, k, :])
    return x


def filter_add(shape):
    return _ints(np.random.default_rng(int(np.prod(shape)) + 5), shape)


def filter_n_out(n, mode):
    return (n, (n + 1) // 2, 2 * n)[mode]


GATHER_SHAPE = (3, 2, 7, 11, 13)                    # n_img, c, d, h (odd, != w), w: every extent different
GATHER_RADII = ((1, 2, 3), (0, 4, 1), (2, 0, 0))    # rd, rh, rw
GATHER_PER_IMAGE = (1, 5)
GATHER_WRAP = dict(shape=(4, 4, 6, 20, 24), per_image=1200, radii=(1, 4, 4))     # 4800 * 4 * 3 * 9 * 9 outputs > 16384 * 256


def gather_volume(shape=GATHER_SHAPE):
    """arange: every element names its own address (below 2^24, exact in float32)."""
    assert int(np.prod(shape)) < 2 ** 24
    return np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)


def gather_centres(shape, rd, rh, rw):
    """(d0, h0, w0) lists: all eight combinations of a centre at its lowest / highest legal position on each axis (the
    neighbourhood touches that border of the volume), then four interior ones.  Legal with the quirk's true bounds: W centre
    in [rh, w - rh), H centre in [rw, h - rw)."""
    _, _, d, h, w = shape
    cd, chh, cw = [], [], []
    for dd in (rd, d - 1 - rd):
        for hh in (rw, h - 1 - rw):
            for ww in (rh, w - 1 - rh):
                cd.append(dd), chh.append(hh), cw.append(ww)
    rng = np.random.default_rng(d * h * w + rd + 3 * rh + 7 * rw)
    for _ in range(4):
        cd.append(int(rng.integers(rd, d - rd))), chh.append(int(rng.integers(rw, h - rw))), cw.append(int(rng.integers(rh, w - rh)))
    return np.array(cd), np.array(chh), np.array(cw)


def gather_calls(n_img, per_image, centres):
    """The centre list cut into calls of n_img * per_image neighbourhoods (cycling), so that every centre is used."""
    d0, h0, w0 = centres
    N = n_img * per_image
    for s in range(0, len(d0), N):
        idx = np.arange(s, s + N) % len(d0)
        yield d0[idx], h0[idx], w0[idx]


def gather_wrap_centres():
    n_img, _, d, h, w = GATHER_WRAP['shape']
    rd, rh, rw = GATHER_WRAP['radii']
    N = n_img * GATHER_WRAP['per_image']
    rng = np.random.default_rng(77)
    return rng.integers(rd, d - rd, N), rng.integers(rw, h - rw, N), rng.integers(rh, w - rh, N)


NORMALIZE_SHAPES = ((300, 3, 45), (2, 1, 1), (1536, 2, 243))     # n, c, inner; the last: 373 248 > 256 * 256 per channel
NORMALIZE_WRAP = (8700, 2, 243)          # 4 228 200 elements > 16384 * 256: the second trip of desc_normalize_kernel's loop
NORMALIZE_M, NORMALIZE_S = (3.0, -16.0, 0.5), (2.0, 0.25, 8.0)


def normalize_exact_input(n, c, inner):
    """Channel ch holds m[ch] + s[ch] and m[ch] - s[ch] in equal numbers at random places: mean m, variance s^2, all sums
    exact; the normalised value is exactly +1 / -1.  Returns (desc float32, signs)."""
    rng = np.random.default_rng(n + c + inner)
    count = n * inner
    assert count % 2 == 0
    desc = np.empty((n, c, inner), dtype=np.float32)
    sign = np.empty((n, c, inner))
    for ch in range(c):
        s = np.repeat([1.0, -1.0], count // 2)
        rng.shuffle(s)
        sign[:, ch, :] = s.reshape(n, inner)
        desc[:, ch, :] = NORMALIZE_M[ch] + NORMALIZE_S[ch] * sign[:, ch, :]
    return desc, sign


def normalize_float_input(n, c, inner):
    rng = np.random.default_rng(3 * n + c)
    off = np.array([1000.0, -37.5, 0.0, 250.0])[:c]
    return (rng.standard_normal((n, c, inner)) + off[None, :, None]).astype(np.float32)


DISTANCE_CASES = ((1, 1, 64), (5, 255, 256), (5, 257, 512), (300, 300, 512), (512, 1000, 1024))      # rows, n, npad


def distance_input(rows, n, npad):
    """Two buffers [rows, npad] of sorted multiples of 1/8 in [-64, 64], +inf past n (as the sort leaves them)."""
    rng = np.random.default_rng(rows + n)
    out = []
    for _ in range(2):
        p = np.full((rows, npad), np.inf, dtype=np.float32)
        p[:, :n] = np.sort(rng.integers(-512, 513, size=(rows, n)) / 8.0, axis=1)
        out.append(p)
    return out


SSIM_CASES = ((1, 12, 13, 1, 0, 5), (11, 11, 11, 2, 5, 5), (7, 13, 12, 3, 2, 5), (40, 90, 90, 1, 5, 5))   # s0 s1 s2 c crop0 crop
SSIM_CONST = (1.125, 0.25, 0.5625)                 # cov_norm, C1, C2: dyadic


def ssim_moments(s0, s1, s2, c):
    """ux, uy, uxx, uyy, uxy [s0, s1, s2, c]: multiples of 1/8; ux, uy in [-4, 4], uxx >= ux^2 and uyy >= uy^2 (variances
    >= 0, so every denominator is >= C1 C2 > 0); at most 7 bits each, so every product in S stays far below 53 bits."""
    rng = np.random.default_rng(s0 * s1 + s2 + c)
    shape = (s0, s1, s2, c)
    ux, uy = rng.integers(-32, 33, shape) / 8.0, rng.integers(-32, 33, shape) / 8.0
    uxx = np.ceil(ux * ux * 8) / 8 + rng.integers(0, 17, shape) / 8.0
    uyy = np.ceil(uy * uy * 8) / 8 + rng.integers(0, 17, shape) / 8.0
    uxy = ux * uy + rng.integers(-16, 17, shape) / 8.0
    uxy = np.round(uxy * 8) / 8
    return ux, uy, uxx, uyy, uxy
