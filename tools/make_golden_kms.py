"""Writes tests/golden/kms_reference.npz: two small float32 sets, the intercept, the clip range and the value the reference's
kolmogorov_smirnov_distance (pgan_pytorch/metrics/kms.py) returns for them.  Data only; run on a host that has the reference
tree, never on the GPU machine:

    python tools/make_golden_kms.py /path/to/reference/pgan_pytorch/metrics/kms.py

The reference histograms each volume with np.histogram's AUTOMATIC range, [min, max] of that volume after the clip.  That is
the fixed grid of unit-wide bins over [lo, hi] only when lo >= 0 (its astype(int) truncates, the project floors: they differ
for negative values, which both then clip to lo) and every volume attains both clip bounds: one saturating low and one
saturating high voxel are planted per volume."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(path):
    spec = importlib.util.spec_from_file_location('reference_kms', path)
    kms = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kms)
    rng = np.random.default_rng(20240611)
    shape, intercept, clip_range = (5, 1, 4, 6, 7), 32, (0, 64)
    real = rng.normal(0.0, 0.45, shape).astype(np.float32)
    fake = rng.normal(0.1, 0.55, shape).astype(np.float32)
    for x in (real, fake):
        flat = x.reshape(shape[0], -1)
        flat[:, 0] = -2.0      # (-2 * 32 + 32 = -32: clipped to lo)
        flat[:, 1] = 3.0       # (3 * 32 + 32 = 128: clipped to hi)
    value = kms.kolmogorov_smirnov_distance(real.copy(), fake.copy(), intercept, clip_range)
    out = os.path.join(ROOT, 'tests', 'golden', 'kms_reference.npz')
    np.savez(out, real=real, fake=fake, intercept=np.int64(intercept), clip_range=np.array(clip_range, dtype=np.int64),
             value=np.float64(value))
    print(out, float(value))


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
