"""Mirror of SURFGAN_3D/generate_minimal.py:13-64 on the HIP path: restore the generator's variables from a checkpoint,
sample `num_samples` volumes in batches of `batch_size`, undo the input normalisation and write
`<output_dir>/generated_images/fake_images_{phase}.npy`.  Same flag names (generate_minimal.py:76-96); the checkpoint is
the `{tf variable name: ndarray}` .npz that saragan_amd.utils.save_checkpoint writes (model_{phase})."""
import argparse
import importlib
import json
import os

import numpy as np
import torch

from . import dataset as data
from .utils import get_base_shape, get_current_input_shape, load_checkpoint
from .varstore import VariableStore, set_compute_dtype, use_store


def _spec_loader(key):
    def load(value):
        with open(value) as f:
            return json.load(f)[key]
    return load


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument('architecture', type=str)
    p.add_argument('--start_shape', type=str, required=True)
    p.add_argument('--final_shape', type=str, required=True)
    p.add_argument('--kernel_spec', type=_spec_loader('kernel_spec'), default=None)
    p.add_argument('--filter_spec', type=_spec_loader('filter_spec'), default=None)
    p.add_argument('--network_size', default=None, choices=['xxs', 'xs', 's', 'm', 'l', 'xl', 'xxl'], required=True)
    p.add_argument('--latent_dim', type=int, required=True)
    p.add_argument('--first_conv_nfilters', type=int, default=None)      # obsolete in the reference too (main.py:260-264)
    p.add_argument('--kernel_shape', default=[3, 3, 3])
    p.add_argument('--output_dir', type=str, default=None)
    p.add_argument('--model_path', type=str, required=True)
    p.add_argument('--num_samples', type=int, required=True)
    p.add_argument('--batch_size', default=1, type=int)
    p.add_argument('--phase', type=int, required=True)
    p.add_argument('--activation', type=str, default='leaky_relu')
    p.add_argument('--leakiness', type=float, default=0.2)
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--data_mean', default=None, type=float)
    p.add_argument('--data_stddev', default=None, type=float)
    p.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'], help='activation / MFMA input type (new flag)')
    p.add_argument('--conditioning', type=str, default=None,
                   help='(new flag) "v1,...,vL": the label row every sample is generated with; for checkpoints of conditional runs')
    p.add_argument('--conditioning_path', type=str, default=None,
                   help='(new flag) a float [num_samples, L] .npy: one label row per sample, in output order')
    p.add_argument('--png', default=False, action='store_true',
                   help='(new flag) also write fake_images_{phase}.png, a contact sheet of the samples (saragan_amd.preview)')
    p.add_argument('--preview_views', type=str, default='slice_d,slice_h,max_h', help='(new flag) with --png: the row bands')
    p.add_argument('--preview_window', type=str, default=None,
                   help='(new flag) with --png: LO,HI in data units; default data_mean - data_stddev,data_mean + 2 data_stddev')
    p.add_argument('--preview_zoom_d', type=int, default=1, help='(new flag) with --png: repeat the D rows of coronal / sagittal views')
    return p


def write_sheet(args, fake_batch, path, device):
    """--png: the sheet of the saved samples, re-normalised (what the generator gave) and mapped back by scale = stddev, shift =
    mean, as the training loop's previews are."""
    from . import preview
    window = (preview.default_window(args.data_mean, args.data_stddev) if args.preview_window is None
              else preview.parse_window(args.preview_window))
    x = np.ascontiguousarray(data.normalize_numpy(fake_batch, args.data_mean, args.data_stddev), dtype=np.float32)
    scale, shift = (1.0, 0.0) if args.data_mean is None else (float(args.data_stddev), float(args.data_mean))
    img = preview.sheet(torch.from_numpy(x).to(device), args.preview_views, window, scale, shift, args.preview_zoom_d)
    return preview.write_png(path, img, dict(phase=args.phase, views=args.preview_views, window=f'{window[0]},{window[1]}',
                                             seed=args.seed, model=args.model_path))


def label_rows(args):
    """The [num_samples, L] float32 label table of --conditioning / --conditioning_path, or None."""
    text, path = getattr(args, 'conditioning', None), getattr(args, 'conditioning_path', None)
    if text and path:
        raise ValueError('give --conditioning or --conditioning_path, not both')
    if text:
        row = np.array([float(v) for v in text.split(',')], dtype=np.float32)
        return np.tile(row, (args.num_samples, 1))
    if path:
        table = np.asarray(np.load(path), dtype=np.float32)
        if table.ndim != 2 or table.shape[0] != args.num_samples:
            raise ValueError(f'--conditioning_path {path}: expected [num_samples = {args.num_samples}, L], got {table.shape}')
        return table
    return None


def main(args, device='cuda'):
    """generate_minimal.py:13-64.  Returns the path of the written file."""
    if not torch.cuda.is_available():
        raise RuntimeError('saragan_amd generates on MI355X only: no CPU fallback')
    generator = importlib.import_module(f'saragan_amd.networks.{args.architecture}.generator').generator
    if args.kernel_spec is None or args.filter_spec is None:
        from .networks.pgan.variables import preset_specs
        ks, fs = preset_specs(args.network_size, get_base_shape(args.start_shape), 8)
        args.kernel_spec, args.filter_spec = args.kernel_spec or ks, args.filter_spec or fs
    phase = args.phase
    logdir = os.path.join(args.output_dir or '.', 'generated_images')
    os.makedirs(logdir, exist_ok=True)
    print("Arguments passed:")
    print(args)
    print(f"Saving files to {logdir}")
    set_compute_dtype(torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
    store = VariableStore(device, seed=args.seed)
    rng = torch.Generator(device=device).manual_seed(args.seed)
    shape = get_current_input_shape(args.phase, args.batch_size, args.start_shape)
    base_shape = get_base_shape(args.start_shape)
    alpha = 0.0                                  # generate_minimal.py:24-25: tf.Variable(0, name='alpha')
    labels = label_rows(args)
    made = [0]                                   # samples generated after the restore: sample i reads label row i

    def sample(count=True):
        z = torch.randn(shape[0], args.latent_dim, device=device, generator=rng)
        kw = {}
        if labels is not None:                   # (a last batch that overshoots num_samples repeats the last row)
            take = np.minimum(np.arange(shape[0]) + made[0], len(labels) - 1)
            kw['conditioning'] = torch.from_numpy(labels[take]).to(device)
            made[0] += shape[0] if count else 0
        with use_store(store), torch.no_grad():
            return generator(z, alpha, args.phase, base_shape, activation=args.activation, kernel_spec=args.kernel_spec,
                             filter_spec=args.filter_spec, param=args.leakiness, size=args.network_size, is_reuse=False, **kw)

    first = sample(count=False)                  # creates the generator's variables (tf.global_variables_initializer)
    print("Restoring variables...")
    sd = load_checkpoint(args.model_path)
    conditional = 'generator/conditioning/weight' in sd
    if conditional and labels is None:
        raise ValueError(f'checkpoint {args.model_path} was written with --conditioning_path: give --conditioning "v1,...,vL" or '
                         f'--conditioning_path')
    if labels is not None and not conditional:
        raise ValueError(f'checkpoint {args.model_path} was written without --conditioning_path: it takes no --conditioning')
    missing = store.load_state_dict({k: v for k, v in sd.items() if k.startswith('generator/')})
    if missing:
        raise KeyError(f'checkpoint {args.model_path} lacks generator variables {missing}')
    from . import functional as F
    F.clear_pack_cache()
    fake_batch = sample().float().cpu().numpy().astype(np.float32)
    del first
    i = 0
    while fake_batch.shape[0] < args.num_samples:
        i += 1
        print(f'Generating sample {i}')
        fake_batch = np.concatenate((fake_batch, sample().float().cpu().numpy().astype(np.float32)))
    print(f'Minimum of generated image 1 before inverting normalization: {np.min(fake_batch[0, ...])}')
    print(f'Maximum of generated image 1 before inverting normalization: {np.max(fake_batch[0, ...])}')
    fake_batch = data.invert_normalize_numpy(fake_batch, args.data_mean, args.data_stddev, True)
    print(f'Minimum of generated image 1 after inverting normalization: {np.min(fake_batch[0, ...])}')
    print(f'Maximum of generated image 1 after inverting normalization: {np.max(fake_batch[0, ...])}')
    out = os.path.join(logdir, f'fake_images_{phase}.npy')
    np.save(out, fake_batch)
    if getattr(args, 'png', False):
        write_sheet(args, fake_batch, os.path.join(logdir, f'fake_images_{phase}.png'), device)
    return out


if __name__ == '__main__':
    main(build_parser().parse_args())
