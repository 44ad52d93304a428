"""Mirror of SURFGAN_3D/metrics/save_metrics.py:19-300 (called from optuna_objective.py:500-506 every
--metrics_every_nsteps images and at :593-627 at the end of a phase): draw real batches from a data subset, generate fake
images with the CURRENT generator weights, evaluate the enabled metrics on the GPU (csrc/metrics.hip through
metrics/swd.py and metrics/skim_metrics.py), average over the batches and print them in the reference's stdout format.

What differs, and why: there is no tf.summary writer (TensorBoard is out of scope: `writer` is accepted and ignored);
MPI.COMM_WORLD.Gather of the ranks' fake images (save_metrics.py:117-131) is torch.distributed.gather to rank 0; FID needs
the Inception graph the reference downloads (metrics/fid_new.py:291-318): --compute_FID is answered with a printed notice at
every evaluation and no 'FID' key.  In its place (not in the reference): --compute_mmd, --compute_nn_accuracy and
--compute_precision_recall, three download-free two-sample statistics over the POOLED evaluated batches
(metrics/sample_metrics.py), and --compute_intensity_hist, the distances of the voxel-intensity histograms in data units
(metrics/intensity_metrics.py; the reference's metrics/kms.py, which its loop never calls), and --compute_power_spectrum, the
log-spectral distances and the high-frequency excess of the shell-binned power spectra (metrics/spectrum_metrics.py)."""
import time

import numpy as np
import torch

from .. import _lib
from ..dataset import normalize_numpy
from . import intensity_metrics as IM
from . import sample_metrics as SM
from . import skim_metrics as SK
from . import swd as SWD

SAMPLE_FLAGS = ('compute_mmd', 'compute_nn_accuracy', 'compute_precision_recall')


def get_compute_metrics_dict(args):
    """utils.py:267-277."""
    return {k: bool(getattr(args, k, False)) for k in
            ('compute_FID', 'compute_swds', 'compute_ssims', 'compute_psnrs', 'compute_mses', 'compute_nrmses') + SAMPLE_FLAGS
            + ('compute_intensity_hist', 'compute_power_spectrum')}


def _gather_to_rank0(fake, global_size):
    import torch.distributed as dist
    if dist.get_rank() == 0:
        parts = [torch.empty_like(fake) for _ in range(global_size)]
        dist.gather(fake, parts, dst=0)
        return torch.cat(parts, dim=0)
    dist.gather(fake, None, dst=0)
    return None


def save_metrics(writer, sess, npy_data, gen_sample, batch_size, global_size, global_step, imagesize_xy, horovod,
                 hyperparam_opt_inter_trial, compute_metrics, num_metric_samples, data_mean, data_stddev, verbose, suffix='',
                 keep=None, conditioning=None, pr_k=3, keep_sets=None, hist_range=None, hist_levels=1, keep_hists=None,
                 spectrum=None, keep_spectra=None):
    """Same arguments and return value as the reference (a dict with the keys swd, ssim, psnr, mse, nrmse of the enabled
    metrics).  `keep`: a list that receives (real_batch, fake_batch) of every evaluated batch (tests).  `conditioning` (not in
    the reference): the step graph's label placeholder -- the fakes are generated with the label rows of the real batch they
    are compared with (npy_data carries the table), sample i with row i, wrapping where the generator's batch overshoots.
    compute_mmd / compute_nn_accuracy / compute_precision_recall (not in the reference; metrics/sample_metrics.py) are set
    statistics: the evaluated batches stay on the device and are evaluated once, pooled, after the loop (keys mmd,
    nn_accuracy[_real|_fake], precision, recall).  `pr_k`: the neighbour rank of precision / recall.  `keep_sets`: a list
    that receives (n, distance matrix as numpy) when that evaluation ran (tests).
    compute_intensity_hist (metrics/intensity_metrics.py): every evaluated batch is counted into an IntensityAccumulator over
    `hist_range` = (lo, hi) in data units -- the batches are normalised, so the kernel maps them back with scale = data_stddev,
    shift = data_mean (1, 0 for data that is not normalised) -- on `hist_levels` levels; nothing is retained, the distances are
    read off the counts after the loop (keys intensity_ks, intensity_w1, intensity_gap: a list per level).  `keep_hists`: a
    list that receives the accumulator's level count and, per batch, the two Laplacian pyramids (tests).
    compute_power_spectrum (metrics/spectrum_metrics.py): every evaluated batch goes through a SpectrumAccumulator with the
    options `spectrum` = {'spacing': (d, h, w) in mm, 'bins': B or None, 'window': 'none' | 'hann'} (all optional) and the same
    map back to data units; only the two sum vectors are retained (keys spectrum_lsd, spectrum_lsd_d|h|w, spectrum_hf_excess,
    spectrum_skipped_columns).  `keep_spectra`: a list that receives the accumulator after the loop (tests)."""
    def log(s):
        if verbose:
            print(s)

    compute_metrics = dict(compute_metrics)
    if compute_metrics.get('compute_FID'):      # said every time, never silently dropped: the reference's example scripts pass it
        log('FID is NOT computed: it needs the Inception graph the reference downloads (metrics/fid_new.py:291-318)')
        compute_metrics['compute_FID'] = False
    metrics = {}
    batch_size = min(batch_size, num_metric_samples)                          # save_metrics.py:71
    sample_shape = np.load(npy_data.scratch_files[0], mmap_mode='r').shape    # (the reference reads npy_data.shape)
    compute_metrics['compute_swds'] = imagesize_xy >= 16 and compute_metrics.get('compute_swds', False)       # :78
    compute_metrics['compute_ssims'] = min(sample_shape) >= 16 and compute_metrics.get('compute_ssims', False)  # :79
    rank0 = (not horovod) or hyperparam_opt_inter_trial
    if horovod and not hyperparam_opt_inter_trial:
        import torch.distributed as dist
        rank0 = dist.get_rank() == 0
    swds_local, psnrs_local, mses_local, nrmses_local, ssims_local = [], [], [], [], []
    pool_sets = any(compute_metrics.get(f) for f in SAMPLE_FLAGS)
    reals_kept, fakes_kept = [], []
    hist = None
    if compute_metrics.get('compute_intensity_hist') and rank0:
        if hist_range is None:
            raise ValueError('compute_intensity_hist needs hist_range=(lo, hi) in data units (--hist_range LO,HI)')
        if isinstance(hist_range, str):      # (a namespace that did not go through main.finalize_args)
            hist_range = IM.parse_range(hist_range)
        normalised = data_mean is not None and data_stddev is not None
        hist = IM.IntensityAccumulator(hist_range[0], hist_range[1], data_stddev if normalised else 1.0,
                                       data_mean if normalised else 0.0, hist_levels)
    spec, spec_wanted = None, bool(compute_metrics.get('compute_power_spectrum')) and rank0
    if spec_wanted:
        from . import spectrum_metrics as SPM      # (only a run that asks for it imports it)
    counter = 0
    while True:
        real_batch = npy_data.batch_mpi(batch_size) if horovod else npy_data.batch(batch_size)      # :94-97
        real_batch = normalize_numpy(real_batch, data_mean, data_stddev, verbose)
        log('Generating fake images for metric computation...')
        start = time.time()
        rows, made = None, [0]
        if conditioning is not None:
            rows = npy_data.last_labels
            if rows is None or len(rows) == 0:
                raise ValueError('conditional metrics need a dataset with a label table (NumpyPathDataset.set_labels)')

        def generate():
            if rows is None:
                return sess.run(gen_sample).float()
            take = (np.arange(conditioning.shape[0]) + made[0]) % len(rows)
            made[0] += conditioning.shape[0]
            return sess.run(gen_sample, feed_dict={conditioning: rows[take]}).float()
        fake = generate()
        if horovod and not hyperparam_opt_inter_trial:
            while fake.shape[0] * global_size < batch_size:
                fake = torch.cat((fake, generate()))
            log(f'Each rank generated {fake.shape[0]} images')
            fake = _gather_to_rank0(fake.contiguous(), global_size)
            if rank0:
                log(f'Gathered a total of {fake.shape[0]} images')
        else:
            while fake.shape[0] < batch_size:
                fake = torch.cat((fake, generate()))
                log(f'Generated {fake.shape[0]} images')
        if rank0:
            fake = fake[0:batch_size, ...]
            if verbose:
                print(f"Generating fake images took {time.time() - start}")
            real = torch.as_tensor(np.ascontiguousarray(real_batch), device=fake.device)
            real = real[0:fake.shape[0]]        # (a short last draw of a subset smaller than the batch)
            fake = fake[0:real.shape[0]]
            if keep is not None:
                keep.append((real.cpu().numpy(), fake.cpu().numpy()))
            if pool_sets:
                reals_kept.append(real.reshape(real.shape[0], -1).to(torch.float32))
                fakes_kept.append(fake.reshape(fake.shape[0], -1).to(torch.float32))
            if hist is not None:
                hist.add(real, fake, keep=keep_hists)
            if spec_wanted:
                if spec is None:      # (the first batch gives the shape: [n, 1, d, h, w])
                    if real.dim() != 5 or real.shape[1] != 1:
                        raise ValueError(f'compute_power_spectrum reads [n, 1, d, h, w] volumes, got {tuple(real.shape)}')
                    normalised = data_mean is not None and data_stddev is not None
                    opts = dict(spectrum or {})
                    spec = SPM.SpectrumAccumulator(tuple(real.shape[2:]), opts.get('spacing', (1.0, 1.0, 1.0)), opts.get('bins'),
                                                   opts.get('window', 'none'), data_stddev if normalised else 1.0,
                                                   data_mean if normalised else 0.0)
                spec.add(real, fake)
            for flag, fn, dest, name in (('compute_swds', SWD.get_swd_for_volumes, swds_local, 'swds'),
                                         ('compute_psnrs', SK.get_psnr, psnrs_local, 'psnrs'),
                                         ('compute_ssims', SK.get_ssim, ssims_local, 'ssims'),
                                         ('compute_mses', SK.get_mean_squared_error, mses_local, 'mses'),
                                         ('compute_nrmses', SK.get_normalized_root_mse, nrmses_local, 'nrmses')):
                if compute_metrics.get(flag):
                    t0 = time.time()
                    dest.append(fn(real, fake))
                    print("%s took %s" % (name, time.time() - t0))
        counter += global_size * batch_size if horovod else batch_size
        if counter >= num_metric_samples:
            break
    if rank0:
        if compute_metrics.get('compute_psnrs'):
            metrics['psnr'] = np.mean(psnrs_local)
            log(f"PSNR: {metrics['psnr']:.4f}")
        if compute_metrics.get('compute_ssims'):
            metrics['ssim'] = np.mean(ssims_local)
            log(f"SSIM: {metrics['ssim']}")
        if compute_metrics.get('compute_mses'):
            metrics['mse'] = np.mean(mses_local)
            log(f"MSE: {metrics['mse']:.4f}")
        if compute_metrics.get('compute_nrmses'):
            metrics['nrmse'] = np.mean(nrmses_local)
            log(f"Normalized Root MSE: {metrics['nrmse']:.4f}")
        if compute_metrics.get('compute_swds'):
            metrics['swd'] = np.array(swds_local).mean(axis=0)
            log(f"SWDS: {metrics['swd']}")
        if pool_sets:
            metrics.update(_sample_set_metrics(reals_kept, fakes_kept, compute_metrics, pr_k, keep_sets, log))
        if hist is not None:
            m = hist.result()
            if keep_hists is not None:
                keep_hists.append(hist.levels)
            for line in IM.format_lines(m):
                log(line)
            metrics.update(m)
        if spec is not None:
            m = spec.result()
            if keep_spectra is not None:
                keep_spectra.append(spec)
            for line in SPM.format_lines(m):
                log(line)
            metrics.update(m)
    return metrics


def _sample_set_metrics(reals, fakes, compute_metrics, pr_k, keep_sets, log):
    """MMD^2, 1-NN accuracy and precision / recall of the pooled evaluated batches: ONE distance matrix.  Never raises for
    a set that is too small or too large: the statistic (or all three) is switched off with a printed notice."""
    n = sum(r.shape[0] for r in reals)
    which = []
    for flag, name, need, what in (('compute_mmd', 'mmd', 2, 'MMD'), ('compute_nn_accuracy', 'nn_accuracy', 1, '1-NN accuracy'),
                                   ('compute_precision_recall', 'precision_recall', pr_k + 1, f'Precision / recall (k={pr_k})')):
        if compute_metrics.get(flag):
            if n >= need and pr_k >= 1:
                which.append(name)
            else:
                print(f'{what} is switched off for this evaluation: {n} samples per set, it needs {need}')
    if not which:
        return {}
    v = reals[0].shape[1]
    need_bytes = 2 * n * v * 4 + (2 * n) ** 2 * 8 + _lib.load().sg_pairwise_sqdist_workspace(2 * n, 2 * n, v)
    free_bytes = torch.cuda.mem_get_info(reals[0].device)[0]
    if need_bytes > free_bytes:
        print(f'MMD / 1-NN accuracy / precision and recall are skipped for this evaluation: the pooled set of {2 * n} volumes '
              f'and its distance matrix need {need_bytes} bytes, {free_bytes} are free on the device')
        return {}
    t0 = time.time()
    D = SM.pairwise_sqdist(torch.cat(reals + fakes, dim=0))
    if keep_sets is not None:
        keep_sets.append((n, D.cpu().numpy()))
    try:
        m = SM.metrics_from_matrix(D, n, pr_k, None, which)
    except ValueError as e:      # (a degenerate set: all reals identical leaves MMD without a bandwidth)
        print(f'MMD / 1-NN accuracy / precision and recall are skipped for this evaluation: {e}')
        return {}
    print("sample metrics took %s" % (time.time() - t0))
    for line in SM.format_lines(m, pr_k):
        log(line)
    return m
