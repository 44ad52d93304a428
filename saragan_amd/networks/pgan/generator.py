"""Mirror of SURFGAN_3D/networks/pgan/generator.py (same callables, argument order, variable scopes and
ValueError / NotImplementedError behaviour); the ops are saragan_amd.networks.ops (gfx950 kernels)."""
import numpy as np

from ..ops import *  # noqa: F401,F403  (the reference does `from networks.ops import *`)
from ..specs import filters, kernels
from ..ops import (act, apply_bias, conv3d, dense, label_embedding, label_rows, lerp, materialize, pixel_norm, to_rgb,
                   upscale3d, variable_scope)


def generator_in(x, shape, activation, kernel_spec, filter_spec, param=None):
    """pgan/generator.py:26-45."""
    with variable_scope('dense'):
        x = dense(x, int(np.prod(shape)) * filters(filter_spec, 0, 0), activation, param=param)
        x = apply_bias(x)
        x = act(x, activation, param=param)
    x = materialize(x).reshape([-1, filters(filter_spec, 0, 0)] + list(shape))
    with variable_scope('conv'):
        x = conv3d(x, filters(filter_spec, 0, 1), kernels(kernel_spec, 0, 1), activation,
                   param=param)
        x = apply_bias(x)
        x = act(x, activation, param=param)
        x = pixel_norm(x)
    return x


def generator_block(x, activation, kernel_spec, filter_spec, i, param=None):
    """pgan/generator.py:48-71."""
    with variable_scope('upsample'):
        x = upscale3d(x)
    with variable_scope('conv_1'):
        kernel = kernels(kernel_spec, i - 1, 0)
        x = conv3d(x, filters(filter_spec, i - 1, 0), kernel, activation, param=param)
        x = apply_bias(x)
        x = act(x, activation, param=param)
        x = pixel_norm(x)
    with variable_scope('conv_2'):
        kernel = kernels(kernel_spec, i - 1, 1)
        x = conv3d(x, filters(filter_spec, i - 1, 1), kernel, activation, param=param)
        x = apply_bias(x)
        x = act(x, activation, param=param)
        x = pixel_norm(x)
    return x


def generator(x, alpha, phase, base_shape, activation, kernel_spec, filter_spec, param=None, size='medium',
              is_reuse=False, conditioning=None):
    """pgan/generator.py:74-103.  conditioning (refused by the reference's pgan): a floating [N, L] tensor of label rows; their
    learned embedding is concatenated to the latents, as the reference's surfgan mapping network does."""
    conditioning = label_rows(conditioning)
    with variable_scope('generator', reuse=is_reuse):
        if conditioning is not None:
            x = label_embedding(x, conditioning)
        with variable_scope('generator_in'):
            x = generator_in(x, shape=base_shape[1:], activation=activation, kernel_spec=kernel_spec,
                             filter_spec=filter_spec, param=param)
        x_upsample = None
        for i in range(2, phase + 1):
            if i == phase:
                with variable_scope(f'to_rgb_{phase - 1}'):
                    x_upsample = upscale3d(to_rgb(x, channels=base_shape[0]))
            with variable_scope(f'generator_block_{i}'):
                x = generator_block(x, activation=activation, kernel_spec=kernel_spec, filter_spec=filter_spec, i=i,
                                    param=param)
        with variable_scope(f'to_rgb_{phase}'):
            x_out = to_rgb(x, channels=base_shape[0])
        if x_upsample is not None:
            x_out = lerp(x_upsample, x_out, alpha)     # alpha * x_upsample + (1 - alpha) * x_out
        return materialize(x_out)
