"""References for the power-spectrum tests: the derived bound between two summation orders, an independent
statement of the statistic (a full complex np.fft.fftn folded with explicit loops over k), and the twin with the matrix
transform swapped in (the arithmetic the kernel performs, in numpy), whose tables can be tampered with."""
import numpy as np

U = 2.0 ** -53
SHAPES = [(4, 8, 8), (2, 6, 10), (8, 16, 48), (3, 5, 7), (1, 16, 16), (16, 32, 32)]
SPACING = (2.5, 1.0, 1.0)


def make_data(n, shape, seed, dtype=np.int16):
    """Integer-valued volumes in [-1024, 3072)."""
    return np.random.default_rng(seed).integers(-1024, 3072, size=(n,) + tuple(shape)).astype(dtype)


def bound(t, shape, cnt, S):
    """|got - S| <= 2 (2 e sqrt(cnt S) + cnt e^2 + cnt u S),  e = 1.01 (D + H + W + 6) u L1,  L1 = sum |t|: three matrix-vector
    products with |entries| <= 1 at gamma_n each plus 2u per matrix entry give |dF| <= e per coefficient; a bin of weighted
    count cnt and sum S = sum g |F|^2 then moves by at most sum g (2 |F| e + e^2) <= 2 e sqrt(cnt S) + cnt e^2 (Cauchy-Schwarz),
    plus cnt u S for the squares and the bin's own additions; the leading 2 covers the reference FFT's error."""
    e = 1.01 * (sum(shape) + 6) * U * float(np.abs(np.asarray(t, dtype=np.float64)).sum())
    cnt, S = np.asarray(cnt, dtype=np.float64), np.asarray(S, dtype=np.float64)
    return 2.0 * (2.0 * e * np.sqrt(cnt * S) + cnt * e * e + cnt * U * S)


def worst_ratio(got, ref, t, plan):
    """max |got - ref| / bound over the radial columns and the three profiles of ONE sample; got, ref: (radial, (d, h, w))."""
    worst = 0.0
    pairs = [(got[0], ref[0], plan.counts)] + [(g, r, c) for g, r, c in zip(got[1], ref[1], plan.axis_counts)]
    for g, r, c in pairs:
        g, r = np.asarray(g, dtype=np.float64), np.asarray(r, dtype=np.float64)
        b = bound(t, plan.shape, c, r)
        err = np.abs(g - r)
        assert np.all(np.isfinite(g))
        assert np.all((b > 0) | (err == 0))
        worst = max(worst, float(np.max(err / np.where(b > 0, b, 1.0))))
    return worst


def fold_reference(t, shape, spacing, bins):
    """(radial, (axis_d, axis_h, axis_w), counts): the FULL complex spectrum, every coefficient with weight 1, folded with
    explicit loops: a coefficient (kd, kh, kw), kw = 0 .. W - 1, lands where its mirror min(kw, W - kw) does."""
    d, h, w = shape
    f = np.fft.fftn(np.asarray(t, dtype=np.float64))
    fq = [[(min(k, n - k) / (n * sp)) ** 2 for k in range(n)] for n, sp in zip(shape, spacing)]
    top = (max(fq[0]) + max(fq[1])) + max(fq[2])
    edges2 = [(b * np.sqrt(top) / bins) ** 2 for b in range(bins)] + [top]
    radial, counts = np.zeros(bins + 1), np.zeros(bins + 1)
    axes = (np.zeros(d // 2 + 1), np.zeros(h // 2 + 1), np.zeros(w // 2 + 1))
    for kd in range(d):
        for kh in range(h):
            for kw in range(w):
                p = f[kd, kh, kw].real ** 2 + f[kd, kh, kw].imag ** 2
                r2 = (fq[0][kd] + fq[1][kh]) + fq[2][kw]
                col = 0 if r2 == 0 else min(1 + sum(1 for b in range(1, bins + 1) if edges2[b] <= r2), bins)
                radial[col] += p
                counts[col] += 1
                axes[0][min(kd, d - kd)] += p
                axes[1][min(kh, h - kh)] += p
                axes[2][min(kw, w - kw)] += p
    return radial, axes, counts


def matrix_spectrum(t, plan, mats=None, g=None, columns=None):
    """The statistic of one volume by the kernel's arithmetic: three one-axis passes of real matrix products (W, H, D) with the
    plan's transposed matrices, P = Fr^2 + Fi^2, the weights g and the column map -- each replaceable (the teeth)."""
    cd, sd, ch, sh, cw, sw = plan.mats if mats is None else mats
    g = plan.g if g is None else g
    columns = plan.columns() if columns is None else columns
    t = np.asarray(t, dtype=np.float64)
    yr, yi = t @ cw, -(t @ sw)
    mul = lambda m, x, spec: np.einsum(spec, m, x)
    zr = mul(ch, yr, 'jk,djw->dkw') + mul(sh, yi, 'jk,djw->dkw')
    zi = mul(ch, yi, 'jk,djw->dkw') - mul(sh, yr, 'jk,djw->dkw')
    fr = mul(cd, zr, 'jk,jhw->khw') + mul(sd, zi, 'jk,jhw->khw')
    fi = mul(cd, zi, 'jk,jhw->khw') - mul(sd, zr, 'jk,jhw->khw')
    p = (fr ** 2 + fi ** 2) * g[None, None, :]
    radial = np.zeros(plan.bins + 1)
    np.add.at(radial, columns.ravel(), p.ravel())
    axes = [np.zeros(m) for m in plan.axis_len]
    np.add.at(axes[0], plan.q[0], p.sum(axis=(1, 2)))
    np.add.at(axes[1], plan.q[1], p.sum(axis=(0, 2)))
    axes[2] += p.sum(axis=(0, 1))
    return radial, tuple(axes)
