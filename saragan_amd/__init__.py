"""saragan_amd: MI355X-native (gfx950) engine for the SURFGAN_3D `pgan` generator + discriminator
training step of sara-nl/saraGAN.  HIP kernels + C ABI in csrc/ and include/saragan_hip.h; the Python
modules mirror the reference's interface (networks.ops, networks.pgan.*, networks.loss, optimization)."""
__version__ = '0.2.0'


def dropin_path():
    """Directory to put on sys.path so that the reference loop's module paths (`networks.pgan.generator`,
    `optimization`, `dataset`, ... as imported by SURFGAN_3D/optuna_objective.py:12-30,64-65) resolve to this package."""
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dropin')


def set_deterministic(on=True):
    """Reproducible mode of the library (SG_DETERMINISTIC): weight-gradient kernels store per-block slabs that are added in
    a fixed order instead of using float atomics, and the gradient-penalty row sums are ordered -- two runs from the same
    state produce bit-identical weights (tests/test_deterministic_gpu.py).  Costs workspace (one slab per block of the
    weight-gradient grids) and a few percent of the step; off by default."""
    import os
    from . import _lib
    os.environ['SG_DETERMINISTIC'] = '1' if on else '0'
    _lib.load().sg_config_reload()
    # the kept filter-gradient workspaces are clean only under the mode that used them last (the reproducible finalize pass does
    # not clear the slabs it read): none survives a switch
    from . import functional as F
    F.clear_kept_workspaces()


def set_nonfinite_guard(on=True, max_consecutive=None):
    """Non-finite step guard (not in the reference; off by default): a train op whose gradient, after the data-parallel
    reduction and before clipping, holds a NaN or +-Inf does nothing that step -- parameters, optimiser slots and the
    optimiser's step count stay as they were, the EMA update still runs -- decided on the device inside the (captured)
    step.  Applies to step graphs built afterwards (as SARAGAN_NONFINITE_GUARD=1 does); graph.skipped_steps counts the
    skips.  max_consecutive: graph.check_nonfinite raises NonFiniteStepsError once one network was skipped that many times
    in a row (train.py checks at its sync points)."""
    import os
    if max_consecutive is not None and not on:
        raise ValueError('max_consecutive needs the guard on')
    if max_consecutive is not None and int(max_consecutive) < 1:
        raise ValueError('max_consecutive must be >= 1')
    os.environ['SARAGAN_NONFINITE_GUARD'] = '1' if on else '0'
    if max_consecutive is None:
        os.environ.pop('SARAGAN_NONFINITE_MAX_CONSECUTIVE', None)
    else:
        os.environ['SARAGAN_NONFINITE_MAX_CONSECUTIVE'] = str(int(max_consecutive))
