"""Download-free two-sample statistics of a set of real and a set of generated volumes (not in the reference, which has
FID only -- and FID needs the Inception graph it downloads):

  * kernel MMD^2, unbiased estimator with a Gaussian kernel (Gretton et al., "A kernel two-sample test", JMLR 2012);
  * leave-one-out 1-nearest-neighbour two-sample accuracy (Lopez-Paz & Oquab, "Revisiting classifier two-sample tests",
    ICLR 2017; Xu et al., "An empirical study on evaluation metrics of generative adversarial networks", 2018);
  * k-NN precision and recall (Kynkaanniemi et al., "Improved precision and recall metric for assessing generative
    models", NeurIPS 2019), in voxel space.

All three are reductions over ONE object: the [2n, 2n] matrix of squared distances of the pooled set Z = [reals; fakes].
That matrix is the GPU work (`sg_pairwise_sqdist`, csrc/pdist.hip: f32-input MFMAs, f64 across the voxels, deterministic);
the reductions are plain torch on a tiny f64 matrix and run wherever that matrix lives.

    python -m saragan_amd.metrics.sample_metrics REAL_DIR FAKE_DIR [--k 3] [--max_samples N] [--data_mean M --data_stddev S]

evaluates two directories of .npy volumes (e.g. generate_minimal's output against held-out data)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib


def _rows(x):
    if not torch.is_tensor(x) or not x.is_cuda:
        raise RuntimeError('saragan_amd.metrics run on the GPU only (no CPU fallback)')
    if x.dim() < 1 or x.shape[0] < 1:
        raise ValueError(f'pairwise_sqdist needs [m, ...] with m >= 1, got {tuple(x.shape)}')
    x = x.reshape(x.shape[0], -1).to(torch.float32).contiguous()
    if x.shape[1] < 1:
        raise ValueError('pairwise_sqdist: empty samples')
    return x


def pairwise_sqdist(a, b=None):
    """out[i][j] = max(0, |a_i|^2 + |b_j|^2 - 2 a_i.b_j) as an f64 device tensor [ma, mb]; a, b: device tensors [m, ...],
    flattened per sample.  b=None: the symmetric matrix of `a` with itself (upper triangle computed, mirrored, zero
    diagonal)."""
    a = _rows(a)
    b = a if b is None else _rows(b)
    if b.shape[1] != a.shape[1]:
        raise ValueError(f'pairwise_sqdist: {a.shape[1]} and {b.shape[1]} elements per sample')
    if b.device != a.device:
        raise ValueError('pairwise_sqdist: a and b on different devices')
    lib = _lib.load()
    ma, mb, v = a.shape[0], b.shape[0], a.shape[1]
    with torch.cuda.device(a.device):
        nbytes = lib.sg_pairwise_sqdist_workspace(ma, mb, v)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        out = torch.empty((ma, mb), dtype=torch.float64, device=a.device)
        _lib.check(lib.sg_pairwise_sqdist(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), C.c_void_p(out.data_ptr()), ma, mb,
                                          v, C.c_void_p(ws.data_ptr()), nbytes,
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'sg_pairwise_sqdist')
    return out


def _pooled(D, n):
    D = torch.as_tensor(D).to(torch.float64)
    if D.dim() != 2 or D.shape[0] != 2 * n or D.shape[1] != 2 * n:
        raise ValueError(f'expected the [2n, 2n] matrix of the pooled set with n = {n}, got {tuple(D.shape)}')
    return D


def mmd2(D, n, sigma2=None):
    """Unbiased MMD^2 with k = exp(-d^2 / (2 sigma^2)).  sigma2 defaults to the mean off-diagonal real-real squared distance:
    a bandwidth from the reals alone does not move with the generator."""
    if n < 2:
        raise ValueError(f'mmd2 needs n >= 2, got {n}')
    D = _pooled(D, n)
    off = ~torch.eye(n, dtype=torch.bool, device=D.device)
    rr, ff, rf = D[:n, :n], D[n:, n:], D[:n, n:]
    if sigma2 is None:
        sigma2 = float(rr[off].sum() / (n * (n - 1)))
    if not sigma2 > 0:
        raise ValueError(f'mmd2: the kernel bandwidth sigma^2 = {sigma2} is not positive (identical reals?)')
    k = lambda d: torch.exp(d * (-1.0 / (2.0 * sigma2)))
    return float(k(rr)[off].sum() / (n * (n - 1)) + k(ff)[off].sum() / (n * (n - 1)) - 2.0 * k(rf).sum() / (n * n))


def nn_accuracy(D, n):
    """Leave-one-out 1-NN accuracy (total, real, fake): the share of points whose nearest OTHER point (ties: lowest
    index) has their own label.  0.5 is the ideal; a fake-side value far under 0.5 means fakes sit on top of reals."""
    if n < 1:
        raise ValueError(f'nn_accuracy needs n >= 1, got {n}')
    D = _pooled(D, n).clone()
    D.fill_diagonal_(float('inf'))
    # argmin does not promise the first of equal minima: the lowest index among them, explicitly
    idx = torch.arange(2 * n, device=D.device)
    nearest = torch.where(D == D.min(dim=1, keepdim=True).values, idx[None, :], 2 * n).min(dim=1).values
    same = (nearest < n) == (idx < n)
    real, fake = int(same[:n].sum()), int(same[n:].sum())      # shares as count / size: one correctly rounded division
    return (real + fake) / (2 * n), real / n, fake / n


def precision_recall(D, n, k=3):
    """(precision, recall) of Kynkaanniemi et al. in voxel space: a fake is covered when it lies within some real's
    k-th-nearest-real radius, a real when it lies within some fake's k-th-nearest-fake radius."""
    if k < 1 or n < k + 1:
        raise ValueError(f'precision_recall needs n >= k + 1, got n = {n}, k = {k}')
    D = _pooled(D, n)
    inf = torch.full((n,), float('inf'), dtype=D.dtype, device=D.device)
    rad_r = (D[:n, :n] + torch.diag(inf)).kthvalue(k, dim=1).values      # k-th smallest distance to ANOTHER real
    rad_f = (D[n:, n:] + torch.diag(inf)).kthvalue(k, dim=1).values
    rf = D[:n, n:]                                                       # [real i, fake j]
    precision = int((rf <= rad_r[:, None]).any(dim=0).sum()) / n
    recall = int((rf <= rad_f[None, :]).any(dim=1).sum()) / n
    return precision, recall


def metrics_from_matrix(D, n, k=3, sigma2=None, which=('mmd', 'nn_accuracy', 'precision_recall')):
    """The dict of get_sample_metrics from a pooled matrix; `which` selects the statistics."""
    m = {}
    if 'mmd' in which:
        m['mmd'] = mmd2(D, n, sigma2)
    if 'nn_accuracy' in which:
        m['nn_accuracy'], m['nn_accuracy_real'], m['nn_accuracy_fake'] = nn_accuracy(D, n)
    if 'precision_recall' in which:
        m['precision'], m['recall'] = precision_recall(D, n, k)
    return m


def get_sample_metrics(real, fake, k=3, sigma2=None, keep=None):
    """real, fake: device tensors [n, ...] of equal shape.  One symmetric pairwise_sqdist over [real; fake]; keys mmd,
    nn_accuracy, nn_accuracy_real, nn_accuracy_fake, precision, recall.  `keep`: a list that receives the matrix (numpy)."""
    if tuple(real.shape) != tuple(fake.shape):
        raise ValueError(f'real {tuple(real.shape)} and fake {tuple(fake.shape)} differ in shape')
    n = real.shape[0]
    D = pairwise_sqdist(torch.cat((_rows(real), _rows(fake)), dim=0))
    if keep is not None:
        keep.append(D.cpu().numpy())
    return metrics_from_matrix(D, n, k, sigma2)


def format_lines(m, k):
    """The stdout lines of the statistics present in `m` (save_metrics and the command line print the same text)."""
    lines = []
    if 'mmd' in m:
        lines.append(f"MMD^2: {m['mmd']:.6g}")
    if 'nn_accuracy' in m:
        lines.append(f"1-NN accuracy (total real fake): {m['nn_accuracy']:.4f} {m['nn_accuracy_real']:.4f} "
                     f"{m['nn_accuracy_fake']:.4f}")
    if 'precision' in m:
        lines.append(f"Precision / recall (k={k}): {m['precision']:.4f} / {m['recall']:.4f}")
    return lines


def load_dir(path, max_samples=None):
    """The sorted .npy files of a directory as one float32 array [count, ...]; all of one shape."""
    import os
    names = sorted(f for f in os.listdir(path) if f.endswith('.npy'))
    if max_samples is not None:
        names = names[:max_samples]
    if not names:
        raise SystemExit(f'{path}: no .npy files')
    vols = [np.load(os.path.join(path, f)) for f in names]
    shapes = {v.shape for v in vols}
    if len(shapes) != 1:
        raise SystemExit(f'{path}: volumes of different shapes {sorted(shapes)}')
    return np.stack(vols).astype(np.float32)


def main(argv=None):
    import argparse
    p = argparse.ArgumentParser(prog='python -m saragan_amd.metrics.sample_metrics', description=__doc__.split('\n\n')[0])
    p.add_argument('real_dir')
    p.add_argument('fake_dir')
    p.add_argument('--k', type=int, default=3, help='neighbour rank of the precision / recall radii')
    p.add_argument('--max_samples', type=int, default=None)
    p.add_argument('--data_mean', type=float, default=None, help='with --data_stddev: (x - mean) / stddev on BOTH sets')
    p.add_argument('--data_stddev', type=float, default=None)
    args = p.parse_args(argv)
    real, fake = load_dir(args.real_dir, args.max_samples), load_dir(args.fake_dir, args.max_samples)
    if real.shape[1:] != fake.shape[1:]:
        raise SystemExit(f'volumes differ in shape: {args.real_dir} {real.shape[1:]}, {args.fake_dir} {fake.shape[1:]}')
    n = min(real.shape[0], fake.shape[0])
    if n < max(2, args.k + 1):
        raise SystemExit(f'{n} samples per set: MMD needs 2 and precision / recall k + 1 = {args.k + 1}')
    real, fake = real[:n], fake[:n]
    if (args.data_mean is None) != (args.data_stddev is None):
        raise SystemExit('--data_mean and --data_stddev go together')
    if args.data_mean is not None:
        real, fake = (real - args.data_mean) / args.data_stddev, (fake - args.data_mean) / args.data_stddev
    if not torch.cuda.is_available():
        raise RuntimeError('saragan_amd.metrics run on the GPU only (no CPU fallback)')
    print(f'{n} real and {n} generated volumes of shape {tuple(real.shape[1:])}')
    m = get_sample_metrics(torch.as_tensor(real, device='cuda'), torch.as_tensor(fake, device='cuda'), k=args.k)
    for line in format_lines(m, args.k):
        print(line)
    return m


if __name__ == '__main__':
    main()
