"""Mirror of the hot-path helpers of SURFGAN_3D/utils.py: shape/phase arithmetic, learning-rate scaling, the
stdout line format, and checkpoints keyed by the reference's TF variable names (tf.train.Saver stand-in)."""
import ast
import os
import time

import numpy as np
import torch


def parse_tuple(string):
    """utils.py: '(c, z, y, x)' strings from the CLI."""
    if isinstance(string, (tuple, list)):
        return tuple(string)
    s = ast.literal_eval(str(string))
    if not isinstance(s, tuple):
        raise ValueError(f'not a tuple: {string}')
    return s


def get_num_channels(start_shape):
    return parse_tuple(start_shape)[0]


def get_base_shape(start_shape):
    """utils.py:219-224."""
    s = parse_tuple(start_shape)
    return (s[0], s[1], s[2], s[3])


def get_num_phases(start_shape, final_shape):
    """utils.py:211-217."""
    return int(np.log2(parse_tuple(final_shape)[-1] / parse_tuple(start_shape)[-1]))


def get_current_input_shape(phase, batch_size, start_shape):
    """utils.py:163-168."""
    start_shape = parse_tuple(start_shape)
    return [batch_size, get_num_channels(start_shape), *[size * 2 ** (phase - 1) for size in get_base_shape(start_shape)[1:]]]


def get_xy_dim(phase, start_shape):
    """utils.py:188-193."""
    return parse_tuple(start_shape)[-1] * (2 ** (phase - 1))


def scale_lr(g_lr, d_lr, g_scaling, d_scaling, horovod, world_size=1):
    """utils.py:120-150 (hvd.size() -> world_size)."""
    def one(lr, how):
        if how == 'sqrt':
            return lr * np.sqrt(world_size)
        elif how == 'linear':
            return lr * world_size
        elif how == 'none':
            return lr
        raise ValueError(how)
    if horovod:
        g_lr, d_lr = one(g_lr, g_scaling), one(d_lr, d_scaling)
    return g_lr, d_lr


def get_num_metric_samples(num_metric_samples, batch_size, global_size):
    """utils.py:152-161."""
    if not num_metric_samples:
        return batch_size * global_size if batch_size > 1 else 2 * global_size
    return num_metric_samples


def format_summary_line(global_step, in_phase_step, img_s, local_img_s, d_loss, g_loss, d_lr_val, g_lr_val, alpha):
    """The stdout line of utils.py:62-73."""
    current_time = time.strftime("%Y-%m-%d_%H:%M:%S", time.gmtime())
    return (f"{current_time} \t"
            f"Step {global_step:09} \t"
            f"Step(phase) {in_phase_step:09} \t"
            f"img/s {img_s:.2f} \t "
            f"img/s/worker {local_img_s:.3f} \t"
            f"d_loss {d_loss:.4f} \t "
            f"g_loss {g_loss:.4f} \t "
            f"d_lr {d_lr_val:.5f} \t"
            f"g_lr {g_lr_val:.5f} \t"
            f"alpha {alpha:.2f}")


def print_summary_to_stdout(global_step, in_phase_step, img_s, local_img_s, d_loss, g_loss, d_lr_val, g_lr_val, alpha):
    a = float(alpha.eval()) if hasattr(alpha, 'eval') else float(alpha)
    print(format_summary_line(global_step, in_phase_step, img_s, local_img_s, d_loss, g_loss, d_lr_val, g_lr_val, a))


# ---- checkpoints: {tf variable name: ndarray}, the contract of tf.train.Saver(var_list) ---------------------
def save_checkpoint(store, path):
    """tf.train.Saver(var_list).save(sess, path): trainable G+D variables (no optimiser slots, no EMA) and the store's
    non-trainable state (spectral normalisation's u, which the reference's tf.global_variables saver would hold too)."""
    arrs = {k: v.detach().float().cpu().numpy() for k, v in store.vars.items()}
    arrs.update((k, v.detach().float().cpu().numpy()) for k, v in store.state.items())
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path if path.endswith('.npz') else path + '.npz', **arrs)


def load_checkpoint(path):
    z = np.load(path if path.endswith('.npz') else path + '.npz')
    return {k: z[k] for k in z.files}


MBSTD_SUFFIX = 'discriminator_out/mbstd/weight'
CONDITIONING_WEIGHT = 'generator/conditioning/weight'      # (networks/pgan/variables.py) present exactly in conditional graphs


def restore_variables(store, phase, starting_phase, logdir, continue_path, var_list, verbose, ema=None):
    """utils.py:75-118: restore by NAME the variables listed in var_list from model_{phase-1} (or continue_path),
    then set the EMA shadows to the restored values."""
    restore_path = None
    if phase > starting_phase:
        restore_path = os.path.join(logdir, f'model_{phase - 1}')
    elif continue_path and phase == starting_phase:
        restore_path = continue_path
    if verbose:
        print("Restoring variables from:", restore_path)
    sd = load_checkpoint(restore_path)
    names = [v if isinstance(v, str) else getattr(v, 'key', v.name.replace(':0', '')) for v in var_list]
    # (not in the reference) --conditioning_path: a conditional network's first dense layer and logit layer have other shapes,
    # so neither kind of checkpoint can start the other kind of run
    if CONDITIONING_WEIGHT in store.vars and CONDITIONING_WEIGHT not in sd:
        raise ValueError(f'checkpoint {restore_path} lacks {CONDITIONING_WEIGHT}: it was written without --conditioning_path and '
                         f'cannot start a conditional run; continue without --conditioning_path, or from a checkpoint written '
                         f'with it')
    if CONDITIONING_WEIGHT in sd and CONDITIONING_WEIGHT not in store.vars:
        raise ValueError(f'checkpoint {restore_path} holds {CONDITIONING_WEIGHT}: it was written with --conditioning_path; give '
                         f'the flag (optimize_step(..., conditioning=...)) to continue from it')
    if CONDITIONING_WEIGHT in sd and tuple(sd[CONDITIONING_WEIGHT].shape) != tuple(store.vars[CONDITIONING_WEIGHT].shape):
        raise ValueError(f'checkpoint {restore_path} was written with --conditioning_path rows of width '
                         f'{sd[CONDITIONING_WEIGHT].shape[0]}, this run\'s have {store.vars[CONDITIONING_WEIGHT].shape[0]}')
    missing = [n for n in names if n in store.vars and n not in sd]
    # (not in the reference) --d_mbstd_group: the statistic channel's filter.  A checkpoint written without the flag has none:
    # zeros leave the discriminator what the checkpoint's was (the term it scales vanishes), and training moves it from there
    zeroed = [n for n in missing if n.endswith(MBSTD_SUFFIX)]
    missing = [n for n in missing if n not in zeroed]
    if missing:
        raise KeyError(f'checkpoint {restore_path} lacks variables {missing}')
    extra = [k for k in sd if k.endswith(MBSTD_SUFFIX) and k not in store.vars]
    if extra:
        raise ValueError(f'checkpoint {restore_path} holds {extra[0]}: it was written with --d_mbstd_group; give the flag '
                         f'(networks.ops.set_minibatch_stddev) to continue from it')
    for n in zeroed:
        if n in store.effective:
            raise ValueError(f'checkpoint {restore_path} lacks {n}, and a zero filter cannot be spectrally normalised: continue '
                             f'without --d_spectral_norm, or from a checkpoint written with --d_mbstd_group')
        with torch.no_grad():
            store.vars[n].zero_()
        print(f'Checkpoint {restore_path} has no {n} (written without --d_mbstd_group): starting it from zeros')
    with torch.no_grad():
        for n in names:
            if n in store.vars and n not in zeroed:
                store.vars[n].copy_(torch.as_tensor(sd[n]).to(store.vars[n].device).reshape(store.vars[n].shape))
                u = store.u_name(n)      # the state of a normalised weight travels with it; a checkpoint without it: fresh u
                if n in store.effective and u in sd:
                    store.state[u].copy_(torch.as_tensor(sd[u]).to(store.state[u].device).reshape(store.state[u].shape))
    store.mark_rewritten()
    if ema is not None:
        ema.reset_to_variables()
    if verbose:
        print("Variables restored!")
