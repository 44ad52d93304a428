"""What the inference tools share (generate_minimal.py, generate.py): the model's command-line flags, the label table of
--conditioning / --conditioning_path, and a generator whose variables are created by one forward pass and then restored from a
training-side checkpoint (the `{tf variable name: ndarray}` .npz of saragan_amd.utils.save_checkpoint)."""
import importlib
import json

import numpy as np
import torch

from .utils import get_base_shape, get_current_input_shape, load_checkpoint
from .varstore import VariableStore, set_compute_dtype, use_store


def _spec_loader(key):
    def load(value):
        with open(value) as f:
            return json.load(f)[key]
    return load


def add_model_arguments(p):
    """generate_minimal.py:76-96 of the reference, flag for flag, and the flags both tools added to them."""
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
    return p


def optional_num_samples(p):
    """--num_samples stops being required: for the tools that can learn the count elsewhere (a latent table, a directory)."""
    for a in p._actions:
        if a.dest == 'num_samples':
            a.required, a.default = False, None
    return p


def add_preview_arguments(p, what):
    p.add_argument('--png', default=False, action='store_true',
                   help=f'(new flag) also write {what}, a contact sheet of the samples (saragan_amd.preview)')
    p.add_argument('--preview_views', type=str, default='slice_d,slice_h,max_h', help='(new flag) with --png: the row bands')
    p.add_argument('--preview_window', type=str, default=None,
                   help='(new flag) with --png: LO,HI in data units; default data_mean - data_stddev,data_mean + 2 data_stddev')
    p.add_argument('--preview_zoom_d', type=int, default=1, help='(new flag) with --png: repeat the D rows of coronal / sagittal views')
    return p


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


class RestoredGenerator:
    """The generator of args.architecture at args.phase on `device`, alpha = 0 (generate_minimal.py:24-25).  Call it once to create
    the variables (tf.global_variables_initializer), then restore(); from then on g(z, conditioning) samples the checkpoint."""

    def __init__(self, args, device):
        self.args, self.device = args, device
        self.generator = importlib.import_module(f'saragan_amd.networks.{args.architecture}.generator').generator
        if args.kernel_spec is None or args.filter_spec is None:
            from .networks.pgan.variables import preset_specs
            ks, fs = preset_specs(args.network_size, get_base_shape(args.start_shape), 8)
            args.kernel_spec, args.filter_spec = args.kernel_spec or ks, args.filter_spec or fs
        set_compute_dtype(torch.bfloat16 if args.dtype == 'bf16' else torch.float32)
        self.store = VariableStore(device, seed=args.seed)
        self.shape = get_current_input_shape(args.phase, args.batch_size, args.start_shape)
        self.base_shape = get_base_shape(args.start_shape)

    def __call__(self, z, conditioning=None, grad=False):
        """grad=True records the pass for autograd (project.py differentiates it with respect to z)."""
        a = self.args
        kw = {} if conditioning is None else {'conditioning': conditioning}
        with use_store(self.store), torch.set_grad_enabled(bool(grad)):
            return self.generator(z, 0.0, a.phase, self.base_shape, activation=a.activation, kernel_spec=a.kernel_spec,
                                  filter_spec=a.filter_spec, param=a.leakiness, size=a.network_size, is_reuse=False, **kw)

    def restore(self, labelled):
        """Loads the generator's variables from args.model_path; labelled: whether the caller has label rows."""
        a = self.args
        sd = load_checkpoint(a.model_path)
        conditional = 'generator/conditioning/weight' in sd
        if conditional and not labelled:
            raise ValueError(f'checkpoint {a.model_path} was written with --conditioning_path: give --conditioning "v1,...,vL" or '
                             f'--conditioning_path')
        if labelled and not conditional:
            raise ValueError(f'checkpoint {a.model_path} was written without --conditioning_path: it takes no --conditioning')
        missing = self.store.load_state_dict({k: v for k, v in sd.items() if k.startswith('generator/')})
        if missing:
            raise KeyError(f'checkpoint {a.model_path} lacks generator variables {missing}')
        from . import functional as F
        F.clear_pack_cache()
