"""The memorisation audit's definitions restated in plain numpy int64 (metrics/memorisation.py), and the planted directories
the host and GPU tests share.  Nothing here imports the code under test."""
import math
import os

import numpy as np

SHAPE = (4, 8, 8)
N_TRAIN, N_FAKE, N_HOLDOUT = 40, 12, 10
COPY_OF, NOISY_OF = 5, 2      # fake 0 is a byte copy of training file 5, fake 1 is training file 2 plus +-1 noise


def sqdist(a, b):
    """int64 [ma, mb] by the definition: ((a[:, None] - b[None]) ** 2).sum(-1), one row at a time."""
    a, b = np.asarray(a), np.asarray(b)
    a64, b64 = a.reshape(a.shape[0], -1).astype(np.int64), b.reshape(b.shape[0], -1).astype(np.int64)
    return np.stack([((b64 - row[None]) ** 2).sum(-1) for row in a64])


def draw(rng, n, dtype, shape=SHAPE):
    if np.dtype(dtype) == np.int16:
        return rng.integers(-1024, 2048, size=(n,) + shape).astype(np.int16)
    if np.dtype(dtype) == np.uint16:
        return rng.integers(0, 65536, size=(n,) + shape).astype(np.uint16)
    if np.dtype(dtype) == np.uint8:
        return rng.integers(0, 256, size=(n,) + shape).astype(np.uint8)
    return rng.normal(size=(n,) + shape).astype(np.float32)


def planted(dtype=np.int16, seed=7):
    """(train, fakes, holdout) arrays with the two planted fakes."""
    rng = np.random.default_rng(seed)
    train, fakes, holdout = draw(rng, N_TRAIN, dtype), draw(rng, N_FAKE, dtype), draw(rng, N_HOLDOUT, dtype)
    fakes[0] = train[COPY_OF]
    noise = rng.choice(np.array([-1, 1]), size=SHAPE)
    if np.dtype(dtype).kind == 'f':
        fakes[1] = train[NOISY_OF] + np.float32(1e-3) * noise.astype(np.float32)
    else:
        info = np.iinfo(dtype)
        fakes[1] = np.clip(train[NOISY_OF].astype(np.int64) + noise, info.min, info.max).astype(dtype)
    return train, fakes, holdout


def write_dir(path, vols, prefix):
    os.makedirs(path, exist_ok=True)
    for i, v in enumerate(vols):
        np.save(os.path.join(path, f'{prefix}_{i:04d}.npy'), v)
    return path


def nearest(d, k, skip_self=False):
    """(d [m, k], id [m, k]) ascending by (distance, id) from the full matrix, by sorting pairs."""
    out_d, out_i = [], []
    for i, row in enumerate(d):
        pairs = sorted((int(x), j) for j, x in enumerate(row) if not (skip_self and j == i))[:k]
        out_d.append([p[0] for p in pairs])
        out_i.append([p[1] for p in pairs])
    return out_d, out_i


def expected_rows(queries, train, k, names):
    """The per-file rows of the report, from the definitions."""
    voxels = int(np.prod(train.shape[1:]))
    loo = [r[0] for r in nearest(sqdist(train, train), 1, skip_self=True)[0]]
    nd, ni = nearest(sqdist(queries, train), k)
    rows = []
    for d, ids in zip(nd, ni):
        rows.append({'nearest': [names[j] for j in ids], 'nearest_index': ids, 'd2': d, 'rms': [math.sqrt(x / voxels) for x in d],
                     'loo_of_nearest': loo[ids[0]], 'ratio': d[0] / loo[ids[0]] if loo[ids[0]] > 0 else None,
                     'duplicate': d[0] == 0, 'authentic': not d[0] < loo[ids[0]]})
    return rows, loo


def midrank_z(x, y):
    """Mann-Whitney z of x against y with mid-ranks, counted pair by pair: U = #{x > y} + #{x == y} / 2."""
    n, m = len(x), len(y)
    u = sum((1.0 if a > b else 0.5 if a == b else 0.0) for a in x for b in y)
    return (u - n * m / 2.0) / math.sqrt(n * m * (n + m + 1) / 12.0)


def strip(report):
    """A report without what may differ between runs of one audit: the timings and the command line."""
    return {k: v for k, v in report.items() if k not in ('seconds', 'arguments')}
