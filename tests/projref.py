"""What the projection tests share: input makers, and an independent float64 statement of the multi-scale residual
loss and its gradient, written with plain reshapes and means -- it never calls the functional CPU path."""
import numpy as np
import torch

TABLE_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.uint16, torch.float16, torch.float32)
Y_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def make_table(rows, shape, dtype, seed):
    """A table [rows, c, d, h, w] of the stored type: integers of a few hundred counts (bytes: their whole range), halves and
    floats of a few units."""
    rng = np.random.default_rng([seed, 1])
    size = (rows,) + tuple(shape)
    if dtype == torch.uint8:
        a = rng.integers(0, 256, size).astype(np.uint8)
    elif dtype == torch.int8:
        a = rng.integers(-128, 128, size).astype(np.int8)
    elif dtype == torch.int16:
        a = rng.integers(-1000, 3000, size).astype(np.int16)
    elif dtype == torch.uint16:
        a = rng.integers(0, 4000, size).astype(np.uint16)
    elif dtype == torch.float16:
        a = (rng.standard_normal(size) * 3).astype(np.float16)
    else:
        a = (rng.standard_normal(size) * 3).astype(np.float32)
    return torch.from_numpy(a)


def make_y(n, shape, dtype, seed, channels_last=False):
    """y [n, c, d, h, w]: normal values of a few units, rounded to dtype."""
    rng = np.random.default_rng([seed, 2])
    y = torch.from_numpy((rng.standard_normal((n,) + tuple(shape)) * 2).astype(np.float32)).to(dtype)
    return y.contiguous(memory_format=torch.channels_last_3d) if channels_last else y


def make_integer_case(n, rows, shape, seed):
    """Integer-valued f32 y and int16 targets: with mean 0, stddev 1 and power-of-two weights every sum of the loss is exact."""
    rng = np.random.default_rng([seed, 3])
    y = torch.from_numpy(rng.integers(-40, 41, (n,) + tuple(shape)).astype(np.float32))
    table = torch.from_numpy(rng.integers(-40, 41, (rows,) + tuple(shape)).astype(np.int16))
    return y, table


def residual(y, table, pos, mean, stddev):
    """r = f32(y) - (f32(x) - mean) / stddev, the three float32 operations the definition names, as float64 [n, c, d, h, w]."""
    yf = y.float().numpy().astype(np.float32)
    x = table.numpy()[np.asarray(pos)].astype(np.float32)
    t = (x - np.float32(mean)) / np.float32(stddev)
    return (yf - t).astype(np.float64)


def upsample(m, e):
    return m.repeat(e, axis=2).repeat(e, axis=3).repeat(e, axis=4)


def reference(r, levels, lam, flip=False):
    """(loss [n], terms [n, levels], grad [n, c, d, h, w]) in float64 from the residuals r: loss = sum_l lam_l mean_B m_l(B)^2 with
    m_l the block means over cubes of edge 2^l, and its gradient sum_l lam_l (2 / N_l) m_l(B_l(v)) / 8^l.  flip=True evaluates the
    same sums on the mirrored volume (and mirrors the gradient back): numpy then adds in another order."""
    if flip:
        r = r[:, ::-1, ::-1, ::-1, ::-1]
    r = np.ascontiguousarray(r)
    n, c, d, h, w = r.shape
    terms, grad = np.empty((n, levels)), np.zeros_like(r)
    for l in range(levels):
        e = 2 ** l
        m = r.reshape(n, c, d // e, e, h // e, e, w // e, e).mean(axis=(3, 5, 7))
        count = m[0].size
        terms[:, l] = (m * m).reshape(n, -1).mean(axis=1)
        grad += float(lam[l]) * (2.0 / count) * upsample(m, e) / 8.0 ** l
    loss = sum(float(lam[l]) * terms[:, l] for l in range(levels))
    if flip:
        grad = np.ascontiguousarray(grad[:, ::-1, ::-1, ::-1, ::-1])
    return loss, terms, grad


def latent_step_scalar(z, m, v, g, loss, best_loss, z_best, best_step, lr, b1, b2, eps, step, sphere):
    """sg_latent_step's definition as a scalar Python loop over numpy float32 scalars; in place on the numpy arrays."""
    f = np.float32
    n, L = z.shape
    lr, b1, b2, eps = f(lr), f(b1), f(b2), f(eps)
    c1, c2 = f(1.0 - float(b1) ** step), f(1.0 - float(b2) ** step)
    with np.errstate(all='ignore'):
        for i in range(n):
            if loss[i] < best_loss[i]:
                best_loss[i], best_step[i] = loss[i], step
                for k in range(L):
                    z_best[i, k] = z[i, k]
            if lr == 0:
                continue
            for k in range(L):
                m[i, k] = f(b1 * m[i, k]) + f((f(1) - b1) * g[i, k])
                v[i, k] = f(b2 * v[i, k]) + f(f((f(1) - b2) * g[i, k]) * g[i, k])
                z[i, k] = z[i, k] - f(f(lr * f(m[i, k] / c1)) / f(np.sqrt(f(v[i, k] / c2)) + eps))
            if not sphere:
                continue
            part = [0.0] * 64
            for k in range(L):
                zk = float(z[i, k])
                part[k % 64] = part[k % 64] + zk * zk
            s = 32
            while s >= 1:
                part = [part[j] + part[j + s] for j in range(s)]
                s //= 2
            if part[0] > 0 and np.isfinite(part[0]):
                scale = float(np.sqrt(np.float64(L))) / float(np.sqrt(np.float64(part[0])))
                for k in range(L):
                    z[i, k] = f(float(z[i, k]) * scale)
