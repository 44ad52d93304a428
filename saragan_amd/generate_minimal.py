"""Mirror of SURFGAN_3D/generate_minimal.py:13-64 on the HIP path: restore the generator's variables from a checkpoint,
sample `num_samples` volumes in batches of `batch_size`, undo the input normalisation and write
`<output_dir>/generated_images/fake_images_{phase}.npy`.  Same flag names (generate_minimal.py:76-96); the checkpoint is
the `{tf variable name: ndarray}` .npz that saragan_amd.utils.save_checkpoint writes (model_{phase})."""
import argparse
import os

import numpy as np
import torch

from . import dataset as data
from .generation import RestoredGenerator, add_model_arguments, add_preview_arguments, label_rows  # noqa: F401


def build_parser():
    p = add_model_arguments(argparse.ArgumentParser())
    return add_preview_arguments(p, 'fake_images_{phase}.png')


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


def main(args, device='cuda'):
    """generate_minimal.py:13-64.  Returns the path of the written file."""
    if not torch.cuda.is_available():
        raise RuntimeError('saragan_amd generates on MI355X only: no CPU fallback')
    g = RestoredGenerator(args, device)
    phase = args.phase
    logdir = os.path.join(args.output_dir or '.', 'generated_images')
    os.makedirs(logdir, exist_ok=True)
    print("Arguments passed:")
    print(args)
    print(f"Saving files to {logdir}")
    rng = torch.Generator(device=device).manual_seed(args.seed)
    shape = g.shape
    labels = label_rows(args)
    made = [0]                                   # samples generated after the restore: sample i reads label row i

    def sample(count=True):
        z = torch.randn(shape[0], args.latent_dim, device=device, generator=rng)
        kw = {}
        if labels is not None:                   # (a last batch that overshoots num_samples repeats the last row)
            take = np.minimum(np.arange(shape[0]) + made[0], len(labels) - 1)
            kw['conditioning'] = torch.from_numpy(labels[take]).to(device)
            made[0] += shape[0] if count else 0
        return g(z, **kw)

    first = sample(count=False)                  # creates the generator's variables (tf.global_variables_initializer)
    print("Restoring variables...")
    g.restore(labels is not None)
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
