"""CLI with the flag names of SURFGAN_3D/main.py:234-355 (hot-path subset; optuna / metrics / summary flags are
accepted and ignored so that the reference's launch lines keep working).  Launch one process per GPU with
`python -m torch.distributed.run --nproc-per-node N -m saragan_amd.main pgan <data> --horovod ...`."""
import argparse
import json

from .networks.pgan.variables import preset_specs
from .utils import get_base_shape, get_num_phases, parse_tuple


def none_or_str(v):
    return None if v == 'None' else v


def none_or_float(v):
    return None if v == 'None' else float(v)


def _spec_loader(key):
    def load(value):
        with open(value) as f:
            return json.load(f)[key]
    return load


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('architecture', type=str)
    p.add_argument('dataset_path', type=str)
    p.add_argument('--start_shape', type=str, required=True)
    p.add_argument('--final_shape', type=str, required=True)
    p.add_argument('--starting_phase', type=int, required=True)
    p.add_argument('--ending_phase', type=int, required=True)
    p.add_argument('--scratch_path', type=str, default=None)
    p.add_argument('--base_batch_size', type=int, default=None)
    p.add_argument('--max_global_batch_size', type=int, default=None)
    p.add_argument('--mixing_nimg', type=int, default=2 ** 19)
    p.add_argument('--stabilizing_nimg', type=int, default=2 ** 19)
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--horovod', default=False, action='store_true')
    p.add_argument('--checkpoint_every_nsteps', default=20000, type=int)
    p.add_argument('--logdir', default=None, type=str)
    p.add_argument('--continue_path', default=None, type=str)
    p.add_argument('--starting_alpha', default=1, type=float)
    p.add_argument('--gpu', default=False, action='store_true')
    p.add_argument('--latent_dim', type=int, required=True)
    p.add_argument('--network_size', default=None, choices=['xxs', 'xs', 's', 'm', 'l', 'xl', 'xxl'])
    p.add_argument('--activation', type=str, default='leaky_relu')
    p.add_argument('--leakiness', type=float, default=0.2)
    p.add_argument('--kernel_spec', type=_spec_loader('kernel_spec'), default=None)
    p.add_argument('--filter_spec', type=_spec_loader('filter_spec'), default=None)
    p.add_argument('--g_lr', type=float, default=1e-3)
    p.add_argument('--d_lr', type=float, default=1e-3)
    for n in ('g', 'd'):
        p.add_argument(f'--{n}_lr_increase', type=none_or_str, choices=[None, 'linear', 'exponential'], default=None)
        p.add_argument(f'--{n}_lr_decrease', type=none_or_str, choices=[None, 'linear', 'exponential'], default=None)
        p.add_argument(f'--{n}_lr_rise_niter', type=int, default=None)
        p.add_argument(f'--{n}_lr_decay_niter', type=int, default=None)
        p.add_argument(f'--{n}_scaling', default='none', choices=['linear', 'sqrt', 'none'])
        p.add_argument(f'--{n}_clipping', default=False, type=bool)
    p.add_argument('--loss_fn', default='logistic', choices=['logistic', 'wgan'])
    p.add_argument('--gp_weight', type=float, default=1)
    p.add_argument('--optim_strategy', default='simultaneous', choices=['simultaneous', 'alternate'])
    p.add_argument('--use_adasum', default=False, action='store_true')
    p.add_argument('--hipgraph', default=False, action='store_true',
                   help='(not in the reference) always replay the training step as one hipGraph (SARAGAN_HIPGRAPH=1); by default a '
                        'phase is captured when its steps measure host-bound')
    p.add_argument('--no_hipgraph', default=False, action='store_true', help='(not in the reference) never capture: SARAGAN_HIPGRAPH=0')
    p.add_argument('--device_dataset_gib', type=float, default=0.0,
                   help='(not in the reference) keep a phase\'s whole .npy table in device memory, in the files\' dtype, and gather '
                        'each batch with one kernel launch instead of loading it through the host, when the table fits G GiB; '
                        '0 = off.  The budget is PER PROCESS: under --horovod every rank holds the whole table.  Decided per '
                        'phase: a phase whose table does not fit is streamed from the host as before.  DESIGN.md section 4.6')
    p.add_argument('--skip_nonfinite_steps', default=False, action='store_true',
                   help='(not in the reference) skip a network\'s update, on the device, when its gradient holds a NaN or Inf '
                        '(saragan_amd.set_nonfinite_guard); the skip counts are printed on a line of their own at each log point')
    p.add_argument('--max_consecutive_nonfinite', type=int, default=None,
                   help='(not in the reference) with --skip_nonfinite_steps: stop with an error after N consecutive skipped steps '
                        'of one network, without writing that phase\'s final checkpoint')
    # (not in the reference) discriminator augmentation (Karras et al. 2020) with pixel-blitting, fractional-geometry and
    # intensity transforms, drawn and applied on the device: DESIGN.md section 4
    p.add_argument('--augment', default='none', choices=['none', 'fixed', 'ada'],
                   help='(not in the reference) augment the real and generated batches before every use by the discriminator: '
                        'fixed = with probability --augment_p per transform, ada = the probability adapts to the sign of D\'s '
                        'real-sample logits (logistic loss only; under --horovod each rank adapts on its own shard)')
    p.add_argument('--augment_p', type=float, default=0.0,
                   help='(not in the reference) the fixed probability, or the initial one of --augment ada')
    p.add_argument('--augment_ops', type=str, default='flip_w,translate',
                   help='(not in the reference) comma list from flip_w,flip_h,flip_d,rot90,translate (pixel blitting; rot90 turns '
                        'the H x W plane and needs it square) and scale,rotate,shift,brightness,contrast (one trilinear resampling '
                        'pass: isotropic scale, rotation of the H x W plane by any angle, sub-voxel shift, additive brightness, '
                        'multiplicative contrast)')
    p.add_argument('--augment_max_shift', type=float, default=0.125,
                   help='(not in the reference) largest translation as a fraction of each extent')
    p.add_argument('--augment_max_scale', type=float, default=1.25,
                   help='(not in the reference) scale: the factor is log-uniform in [1/max, max], max in [1, 2]')
    p.add_argument('--augment_max_angle', type=float, default=180.0,
                   help='(not in the reference) rotate: the angle is uniform in [-max, max] degrees, max in [0, 180]')
    p.add_argument('--augment_max_brightness', type=float, default=0.2,
                   help='(not in the reference) brightness: the bias is uniform in [-max, max], in units of the normalised data')
    p.add_argument('--augment_max_contrast', type=float, default=1.5,
                   help='(not in the reference) contrast: the gain is log-uniform in [1/max, max], max in [1, 4]')
    p.add_argument('--augment_fill', type=float, default=0.0,
                   help='(not in the reference) value of the voxels a translation uncovers: the data\'s background value AFTER '
                        'normalisation (--data_mean / --data_stddev)')
    p.add_argument('--ada_target', type=float, default=None,
                   help='(not in the reference) --augment ada: set point of mean sign(D(real)) (default 0.6)')
    p.add_argument('--ada_interval', type=int, default=None,
                   help='(not in the reference) --augment ada: steps between two adjustments of p (default 4)')
    p.add_argument('--ada_kimg', type=float, default=None,
                   help='(not in the reference) --augment ada: thousands of images over which p can move from 0 to 1 (default 500): '
                        'an adjustment moves p by batch * interval / (ada_kimg * 1000)')
    p.add_argument('--ada_p_max', type=float, default=None,
                   help='(not in the reference) --augment ada: upper limit of p (default 0.8)')
    p.add_argument('--d_spectral_norm', default=False, action='store_true',
                   help='(not in the reference\'s flags; its networks/ops.py:80-127 defines the operation) spectral normalisation of '
                        'every discriminator weight -- conv, from_rgb, dense -- by batched on-device power iteration: DESIGN.md '
                        'section 4.2')
    p.add_argument('--sn_iterations', type=int, default=1,
                   help='(not in the reference) with --d_spectral_norm: power iterations per refresh (default 1)')
    p.add_argument('--d_mbstd_group', type=int, default=0,
                   help='(not in the reference, whose pgan/discriminator.py:50 is commented out) minibatch standard deviation in '
                        'front of the discriminator\'s last convolution, over groups of this many samples (0 = off; pgan only). '
                        'Groups are local to a rank: they are formed inside each process\'s own batch, which the group size must '
                        'divide in every phase, and never span ranks.  DESIGN.md section 4.3')
    p.add_argument('--conditioning_path', type=none_or_str, default=None,
                   help='(the reference\'s pgan refuses conditioning) conditional training: a float [F, L] .npy of label rows, '
                        'one-hot or continuous, row i for file i of every phase directory\'s sorted file table (F = the file '
                        'count of each of them).  Keep the file outside the phase directories, whose *.npy glob would read it as '
                        'a volume.  pgan only; a checkpoint written with the flag continues only with it.  DESIGN.md section 4.4')
    p.add_argument('--ema_beta', type=float, default=0.99)
    p.add_argument('--noise_stddev', type=float, required=True)
    p.add_argument('--optimizer', type=none_or_str, choices=[None, 'Adam', 'SGD', 'Momentum', 'Adadelta', 'LAMB', 'AdamW'], default='Adam')
    p.add_argument('--d_use_different_optimizer', default=False, action='store_true')
    p.add_argument('--d_optimizer', type=none_or_str, choices=[None, 'Adam', 'SGD', 'Momentum', 'Adadelta', 'LAMB', 'AdamW'], default='Adam')
    p.add_argument('--adam_beta1', type=none_or_float, default=0)
    p.add_argument('--d_use_different_beta1', default=False, action='store_true')
    p.add_argument('--d_adam_beta1', type=none_or_float, default=0)
    p.add_argument('--adam_beta2', type=none_or_float, default=0.9)
    p.add_argument('--d_use_different_beta2', default=False, action='store_true')
    p.add_argument('--d_adam_beta2', type=none_or_float, default=0.9)
    p.add_argument('--rho', type=none_or_float, default=0.95)
    p.add_argument('--d_use_different_rho', default=False, action='store_true')
    p.add_argument('--d_rho', type=none_or_float, default=0.95)
    p.add_argument('--momentum', type=none_or_float, default=0.9)
    p.add_argument('--d_use_different_momentum', default=False, action='store_true')
    p.add_argument('--d_momentum', type=none_or_float, default=0.9)
    p.add_argument('--weight_decay', type=none_or_float, default=0.0,
                   help='weight-decay rate of --optimizer LAMB / AdamW (SURFGAN_2D/optim.py:60-80); biases are not decayed')
    p.add_argument('--d_use_different_weight_decay', default=False, action='store_true')
    p.add_argument('--d_weight_decay', type=none_or_float, default=0.0)
    p.add_argument('--data_mean', default=None, type=float)
    p.add_argument('--data_stddev', default=None, type=float)
    # validation split and in-loop metrics (main.py:255-256,319-333); --compute_FID is accepted and refused (needs a download)
    p.add_argument('--validation_fraction', default=0.1, type=float)
    p.add_argument('--test_fraction', default=0.1, type=float)
    p.add_argument('--calc_metrics', default=False, action='store_true')
    p.add_argument('--compute_metrics_train', default=False, action='store_true')
    p.add_argument('--disable_compute_metrics_validation', dest='compute_metrics_validation', default=True, action='store_false')
    p.add_argument('--disable_compute_metrics_test', dest='compute_metrics_test', default=True, action='store_false')
    p.add_argument('--num_metric_samples', type=int, default=None)
    p.add_argument('--metrics_every_nsteps', default=128, type=int)
    p.add_argument('--metrics_batch_size', default=16, type=int)
    for m in ('FID', 'swds', 'ssims', 'psnrs', 'mses', 'nrmses'):
        p.add_argument(f'--compute_{m}', default=False, action='store_true')
    # (new flags) download-free set statistics over the pooled evaluated samples: metrics/sample_metrics.py
    p.add_argument('--compute_mmd', default=False, action='store_true', help='unbiased Gaussian-kernel MMD^2 of reals and fakes')
    p.add_argument('--compute_nn_accuracy', default=False, action='store_true',
                   help='leave-one-out 1-NN two-sample accuracy (0.5 is ideal)')
    p.add_argument('--compute_precision_recall', default=False, action='store_true',
                   help='k-NN precision (fidelity) and recall (coverage: low under mode collapse)')
    p.add_argument('--pr_k', default=3, type=int, help='neighbour rank of the precision / recall radii')
    # (new flags) voxel-intensity histogram distances in data units, counted on the device: metrics/intensity_metrics.py
    p.add_argument('--compute_intensity_hist', default=False, action='store_true',
                   help='KS, Wasserstein-1 and largest density gap between the intensity histograms of reals and fakes; needs '
                        '--hist_range')
    p.add_argument('--hist_range', type=none_or_str, default=None,
                   help='with --compute_intensity_hist: LO,HI in data units (for CT: Hounsfield units as stored), unit-wide bins '
                        'over [LO, HI]; values outside fall into the first and the last bin.  A negative LO is written '
                        '--hist_range=LO,HI')
    p.add_argument('--hist_levels', type=int, default=1,
                   help='with --compute_intensity_hist: 1 = the volumes; N = plus N - 1 detail levels of the Laplacian pyramid')
    # (new flags) power-spectrum distances, a direct 3-D DFT on f64 MFMAs: metrics/spectrum_metrics.py
    p.add_argument('--compute_power_spectrum', default=False, action='store_true',
                   help='log-spectral distance (radial and per axis) and high-frequency excess between the shell-binned power '
                        'spectra of reals and fakes, in dB')
    p.add_argument('--spectrum_spacing', type=str, default='1,1,1',
                   help='with --compute_power_spectrum: voxel spacing d,h,w in mm (frequencies are in cycles / mm)')
    p.add_argument('--spectrum_bins', type=int, default=None,
                   help='with --compute_power_spectrum: radial columns next to DC (default: the largest extent // 2)')
    p.add_argument('--spectrum_window', type=str, default='none', choices=['none', 'hann'],
                   help='with --compute_power_spectrum: hann tapers every axis (the mean is not removed: DC leaks into |k| <= 1)')
    # (not in the reference) sample previews: PNG contact sheets of fixed latents under <logdir>/previews (preview.py)
    p.add_argument('--preview_every_nsteps', type=int, default=0,
                   help='(not in the reference) write a sheet of the fixed latents every N images (0: off)')
    p.add_argument('--preview_samples', type=int, default=8, help='(not in the reference) fixed latents per sheet')
    p.add_argument('--preview_views', type=str, default='slice_d,slice_h,max_h',
                   help='(not in the reference) row bands of a sheet: slice_d|h|w[:INDEX], max_d|h|w, mean_d|h|w')
    p.add_argument('--preview_window', type=none_or_str, default=None,
                   help='(not in the reference) LO,HI in data units, drawn black to white; default: the reference\'s clip range '
                        '[-1, 2] of normalised values, data_mean - data_stddev,data_mean + 2 data_stddev.  A negative LO is '
                        'written --preview_window=LO,HI')
    p.add_argument('--preview_zoom_d', type=int, default=1,
                   help='(not in the reference) repeat the D rows of coronal and sagittal views (D is size / 4 in this data)')
    p.add_argument('--preview_interp', type=int, default=0,
                   help='(not in the reference) K > 1: a second sheet of K latents on the great arc between fixed latents 0 and 1')
    p.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'], help='activation / MFMA input type (new flag)')
    p.add_argument('--max_steps_per_phase', type=int, default=None, help='smoke runs: cap the steps per phase (new flag)')
    return p


ADA_DEFAULTS = {'ada_target': 0.6, 'ada_interval': 4, 'ada_kimg': 500.0, 'ada_p_max': 0.8}
AUGMENT_OPS = ('flip_w', 'flip_h', 'flip_d', 'rot90', 'translate', 'scale', 'rotate', 'shift', 'brightness', 'contrast')


def finalize_augment_args(args):
    """The --augment* / --ada_* flags: refusals first, then the defaults of the flags not given."""
    if not hasattr(args, 'augment'):      # a namespace built without the parser: augmentation off
        return args
    given = [k for k in ADA_DEFAULTS if getattr(args, k, None) is not None]
    if given and args.augment != 'ada':
        raise SystemExit(f'--{given[0]} needs --augment ada')
    if args.augment == 'ada' and args.loss_fn == 'wgan':
        raise SystemExit('--augment ada adapts on the sign of D\'s real-sample logits, which is defined for the logistic loss: '
                         'use --augment fixed with --loss_fn wgan')
    ops = [o for o in str(args.augment_ops).split(',') if o]
    for o in ops:
        if o not in AUGMENT_OPS:
            raise SystemExit(f'--augment_ops: unknown transform {o!r} (choose from {",".join(AUGMENT_OPS)})')
    if args.augment != 'none':
        shape = parse_tuple(args.final_shape)
        if 'rot90' in ops and shape[-2] != shape[-1]:
            raise SystemExit(f'--augment_ops rot90 turns the H x W plane and needs it square, got {shape[-2]} x {shape[-1]}')
        if not 0.0 <= args.augment_p <= 1.0:
            raise SystemExit('--augment_p is a probability')
        if not 0.0 <= args.augment_max_shift <= 1.0:
            raise SystemExit('--augment_max_shift is a fraction of the extent')
    # (the affine family's ranges are the ones sg_augment_affine_draw accepts: refused here whatever --augment is)
    if not 1.0 <= getattr(args, 'augment_max_scale', 1.25) <= 2.0:
        raise SystemExit('--augment_max_scale is a factor between 1 and 2')
    if not 0.0 <= getattr(args, 'augment_max_angle', 180.0) <= 180.0:
        raise SystemExit('--augment_max_angle is an angle between 0 and 180 degrees')
    if not 0.0 <= getattr(args, 'augment_max_brightness', 0.2) < float('inf'):
        raise SystemExit('--augment_max_brightness must be >= 0')
    if not 1.0 <= getattr(args, 'augment_max_contrast', 1.5) <= 4.0:
        raise SystemExit('--augment_max_contrast is a factor between 1 and 4')
    for k, v in ADA_DEFAULTS.items():
        if getattr(args, k, None) is None:
            setattr(args, k, v)
    if args.ada_interval < 1 or args.ada_kimg <= 0 or not 0.0 <= args.ada_p_max <= 1.0:
        raise SystemExit('--ada_interval must be >= 1, --ada_kimg > 0 and --ada_p_max a probability')
    args.augment_ops = ','.join(ops)
    return args


def phase_batch_size(args, phase, global_size=1):
    """The per-process batch of a phase (optuna_objective.py:127-136; train._run_training computes the same)."""
    batch_size = max(1, args.base_batch_size // (2 ** (phase - 1)))
    if args.max_global_batch_size is not None and batch_size > args.max_global_batch_size / global_size:
        batch_size = int(args.max_global_batch_size / global_size)
    return batch_size


def finalize_mbstd_args(args):
    """--d_mbstd_group: refused at start-up where the run could not use it."""
    group = getattr(args, 'd_mbstd_group', 0) or 0
    if group < 0:
        raise SystemExit('--d_mbstd_group must be >= 0 (0 turns the layer off)')
    if group == 0:
        return args
    if args.architecture != 'pgan':
        raise SystemExit(f'--d_mbstd_group is offered for the pgan architecture only, got {args.architecture!r}')
    if getattr(args, 'base_batch_size', None):
        import os
        world = int(os.environ.get('WORLD_SIZE', '1')) if getattr(args, 'horovod', False) else 1
        last = min(args.ending_phase, get_num_phases(args.start_shape, args.final_shape))
        for phase in range(args.starting_phase, last + 1):
            n = phase_batch_size(args, phase, world)
            if n < 1 or n % min(group, n) != 0:
                raise SystemExit(f'--d_mbstd_group {group} does not divide the per-process batch {n} of phase {phase}')
    return args


def finalize_hist_args(args):
    """--compute_intensity_hist: --hist_range 'LO,HI' becomes the tuple (lo, hi); refused at start-up where the run could not
    use it."""
    if not getattr(args, 'compute_intensity_hist', False):
        return args
    text = getattr(args, 'hist_range', None)
    if text is None:
        raise SystemExit('--compute_intensity_hist needs --hist_range LO,HI (the intensity range in data units)')
    if not isinstance(text, tuple):
        try:
            lo, hi = (int(v) for v in str(text).split(','))
        except ValueError:
            raise SystemExit(f'--hist_range: expected two integers LO,HI, got {text!r}')
        from ._lib import INTENSITY_HIST_MAX_BINS
        if not 1 <= hi - lo <= INTENSITY_HIST_MAX_BINS:
            raise SystemExit(f'--hist_range: HI - LO must lie in [1, {INTENSITY_HIST_MAX_BINS}], got {lo},{hi}')
        args.hist_range = (lo, hi)
    if getattr(args, 'hist_levels', 1) < 1:
        raise SystemExit('--hist_levels must be >= 1')
    return args


def finalize_spectrum_args(args):
    """--compute_power_spectrum: --spectrum_spacing 'd,h,w' becomes a tuple of three positive floats; refused at start-up
    where the run could not use it."""
    if not getattr(args, 'compute_power_spectrum', False):
        return args
    from ._lib import POWER_SPECTRUM_MAX_BINS, POWER_SPECTRUM_MAX_EXTENT
    text = getattr(args, 'spectrum_spacing', '1,1,1')
    if not isinstance(text, tuple):
        try:
            sp = tuple(float(v) for v in str(text).split(','))
        except ValueError:
            sp = ()
        if len(sp) != 3 or not all(v > 0 and v < float('inf') for v in sp):
            raise SystemExit(f'--spectrum_spacing: expected three positive numbers d,h,w (mm), got {text!r}')
        args.spectrum_spacing = sp
    bins = getattr(args, 'spectrum_bins', None)
    if bins is not None and not 1 <= bins <= POWER_SPECTRUM_MAX_BINS:
        raise SystemExit(f'--spectrum_bins must lie in [1, {POWER_SPECTRUM_MAX_BINS}], got {bins}')
    if getattr(args, 'spectrum_window', 'none') not in ('none', 'hann'):
        raise SystemExit(f'--spectrum_window is none or hann, got {args.spectrum_window!r}')
    shape = parse_tuple(args.final_shape) if getattr(args, 'final_shape', None) else ()
    if shape and shape[0] != 1:
        raise SystemExit(f'--compute_power_spectrum reads one channel, --final_shape has {shape[0]}')
    if shape and max(shape[1:]) > POWER_SPECTRUM_MAX_EXTENT:
        raise SystemExit(f'--compute_power_spectrum: extents above {POWER_SPECTRUM_MAX_EXTENT} are not supported, --final_shape '
                         f'is {args.final_shape}')
    return args


def finalize_preview_args(args):
    """--preview_*: the views and the window are parsed (args.preview_views: [(mode, axis, index)], args.preview_window: (lo,
    hi) in data units); refused at start-up where the run could not use them."""
    every = getattr(args, 'preview_every_nsteps', 0) or 0
    interp = getattr(args, 'preview_interp', 0) or 0
    if every < 0:
        raise SystemExit('--preview_every_nsteps must be >= 0 (0 turns the previews off)')
    if interp and not every:
        raise SystemExit('--preview_interp needs --preview_every_nsteps')
    if interp < 0 or interp == 1:
        raise SystemExit('--preview_interp is 0 (off) or the number K > 1 of interpolated latents')
    if not every:
        return args
    from . import preview
    if args.preview_samples < 1 or (interp and args.preview_samples < 2):
        raise SystemExit('--preview_samples must be >= 1 (>= 2 with --preview_interp: the arc runs from latent 0 to latent 1)')
    if args.preview_zoom_d < 1:
        raise SystemExit('--preview_zoom_d must be >= 1')
    try:
        args.preview_views = preview.parse_views(args.preview_views)
    except ValueError as e:
        raise SystemExit(f'--preview_views: {e}')
    if not isinstance(args.preview_window, tuple):
        try:
            args.preview_window = (preview.default_window(args.data_mean, args.data_stddev) if args.preview_window is None
                                   else preview.parse_window(args.preview_window))
        except ValueError as e:
            raise SystemExit(f'--preview_window: {e}')
    return args


def finalize_args(args):
    """main.py:384-411 post-parse defaults: the discriminator inherits the generator's optimiser settings unless
    the --d_use_different_* switches are given; presets fill missing kernel/filter specs."""
    if args.max_consecutive_nonfinite is not None:
        if not args.skip_nonfinite_steps:
            raise SystemExit('--max_consecutive_nonfinite needs --skip_nonfinite_steps')
        if args.max_consecutive_nonfinite < 1:
            raise SystemExit('--max_consecutive_nonfinite must be >= 1')
    finalize_augment_args(args)
    finalize_mbstd_args(args)
    finalize_hist_args(args)
    finalize_spectrum_args(args)
    finalize_preview_args(args)
    if getattr(args, 'conditioning_path', None) and args.architecture != 'pgan':
        raise SystemExit(f'--conditioning_path is offered for the pgan architecture only, got {args.architecture!r}')
    if getattr(args, 'sn_iterations', 1) != 1 and not getattr(args, 'd_spectral_norm', False):
        raise SystemExit('--sn_iterations needs --d_spectral_norm')
    if getattr(args, 'sn_iterations', 1) < 1:
        raise SystemExit('--sn_iterations must be >= 1')
    if getattr(args, 'd_spectral_norm', False) and getattr(args, 'use_adasum', False):
        raise SystemExit('--d_spectral_norm does not support --use_adasum (the ranks\' raw weights differ between the local step '
                         'and the combination): use the Average reduction')
    if not args.d_use_different_optimizer:
        args.d_optimizer = args.optimizer
    if not args.d_use_different_beta1:
        args.d_adam_beta1 = args.adam_beta1
    if not args.d_use_different_beta2:
        args.d_adam_beta2 = args.adam_beta2
    if not args.d_use_different_rho:
        args.d_rho = args.rho
    if not args.d_use_different_momentum:
        args.d_momentum = args.momentum
    if not args.d_use_different_weight_decay:
        args.d_weight_decay = args.weight_decay
    for n in ('g', 'd'):       # main.py:384-399: ramp lengths default to half the mixing / stabilising images
        if getattr(args, f'{n}_lr_increase') and not getattr(args, f'{n}_lr_rise_niter'):
            setattr(args, f'{n}_lr_rise_niter', int(args.mixing_nimg / 2))
        if getattr(args, f'{n}_lr_decrease') and not getattr(args, f'{n}_lr_decay_niter'):
            setattr(args, f'{n}_lr_decay_niter', int(args.stabilizing_nimg / 2))
    if args.kernel_spec is None or args.filter_spec is None:
        if args.network_size is None:
            raise SystemExit('give --kernel_spec and --filter_spec, or --network_size for the legacy presets')
        ks, fs = preset_specs(args.network_size, get_base_shape(args.start_shape),
                              max(8, get_num_phases(args.start_shape, args.final_shape)))
        args.kernel_spec = args.kernel_spec or ks
        args.filter_spec = args.filter_spec or fs
    return args


def main(argv=None):
    p = build_parser()
    args, unknown = p.parse_known_args(argv)
    if unknown:
        print(f'ignoring flags outside the hot path: {unknown}')
    args = finalize_args(args)
    if getattr(args, 'hipgraph', False) or getattr(args, 'no_hipgraph', False):
        import os
        os.environ['SARAGAN_HIPGRAPH'] = '1' if args.hipgraph else '0'
    from .train import run_training
    out = run_training(args, max_steps_per_phase=args.max_steps_per_phase)
    for ph, st in out['stats'].items():
        print(f"phase {ph}: {st['img_s']:.2f} img/s, batch {st['batch_size']}, steps {st['steps']}")


if __name__ == '__main__':
    main()
