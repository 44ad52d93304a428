"""fp64 references for the data-parallel step tests (tests/test_dp_step_gpu.py, tests/test_dp_premise_host.py): the oracle
replayed on the full batch or on one rank's slice of a golden fixture, with the update rule a variant names.  Host only."""
import torch

from oracle import pgan_oracle as O
from tests.lamb_rules import RULES

DECAY = 0.01                                       # weight decay of the LAMB / AdamW variants (tests/test_lamb_step_gpu.py)
LR = {'Adam': 1e-3, 'SGD': 2e-3, 'Momentum': 1e-3, 'Adadelta': 1.0, 'LAMB': 1e-3, 'AdamW': 1e-3}


def make_rule(kind, f32_error=None):
    """The oracle's rule for --optimizer `kind`, with the hyper-parameters the single-process twins use."""
    if kind == 'Adam':
        return O.TFAdam(0.0, 0.9)
    if kind == 'SGD':
        return O.TFSGD()
    if kind == 'Momentum':
        return O.TFMomentum(0.8, True)
    if kind == 'Adadelta':
        return O.TFAdadelta(0.9, 1e-7)
    return RULES[kind](0.0, 0.9, DECAY, f32_error=f32_error)


def rank_batch(fx, rank, world):
    """(rnd, real) of rank `rank`: its contiguous slice of the fixture's batch and injected randomness."""
    n = fx['real'].shape[0] // world
    sl = slice(rank * n, (rank + 1) * n)
    return {k: v[sl] for k, v in fx['rnd'].items()}, fx['real'][sl]


def scaled_p0(fx, scale):
    return {k: v * (scale if k.endswith('weight') else 1.0) for k, v in fx['p0'].items()}


def oracle_step(p, rule_g, rule_d, shadow, fx, strategy, rnd=None, real=None, freeze=None, clip=False, g_lr=1e-3, d_lr=1e-3):
    """One oracle step in place on (p, shadow); returns the oracle's fetches."""
    rnd = fx['rnd'] if rnd is None else rnd
    real = fx['real'] if real is None else real
    if strategy == 'simultaneous':
        return O.step_simultaneous(p, rule_g, rule_d, shadow, rnd, real, fx['alpha'], fx['cfg'], g_lr, d_lr, freeze=freeze,
                                   g_clipping=clip, d_clipping=clip)
    assert not clip
    return O.step_alternate(p, rule_g, rule_d, shadow, rnd, real, fx['alpha'], fx['cfg'], g_lr, d_lr, freeze=freeze)


def oracle_run(fx, strategy, kind, steps, p0=None, freeze=None, clip=False, f32_error=None, rank=None, world=1, d_kind=None, lr=None):
    """`steps` oracle steps from p0 (default: the fixture's) on the full batch, or on rank `rank`'s slice of it; lr overrides both learning
    rates.  Returns a list of dict(p=, shadow=, out=) snapshots, one per step."""
    p = {k: v.clone() for k, v in (fx['p0'] if p0 is None else p0).items()}
    shadow = {k: v.clone() for k, v in p.items()}
    rg, rd = make_rule(kind, f32_error), make_rule(d_kind or kind, f32_error)
    rnd, real = (None, None) if rank is None else rank_batch(fx, rank, world)
    snaps = []
    for _ in range(steps):
        out = oracle_step(p, rg, rd, shadow, fx, strategy, rnd, real, freeze, clip, LR[kind] if lr is None else lr,
                          LR[d_kind or kind] if lr is None else lr)
        snaps.append(dict(p=dict(p), shadow=dict(shadow), out=out))
    return snaps


def max_var_norm(grads):
    return max(float(torch.linalg.vector_norm(g)) for g in grads.values())
