"""Mirror of SURFGAN_3D/optimization.py: get_optimizer, minimize_with_clipping, optimize_step (same argument
order, same 20-tuple return order, optimization.py:221-224) and lr_update, for an eager runtime.

The reference builds TF1 graph ops and runs them with `sess.run(fetches, feed_dict)`.  Here optimize_step
returns lightweight handles bound to a StepGraph; `Session.run([...handles...], feed_dict={real_image_input:
batch})` executes ONE pass of the hot path for exactly the requested fetches: forward (4 discriminator passes,
gradient penalty), backward, gradient all-reduce (if the optimizer is wrapped by
parallel.DistributedOptimizer), optional global-norm clipping, and the fused TF-Adam(+EMA) kernel.

Not in the reference, off by default: the non-finite step guard (NonFiniteGuard; saragan_amd.set_nonfinite_guard,
SARAGAN_NONFINITE_GUARD=1).  A train op whose reduced gradient holds a NaN / Inf leaves its parameters, optimiser slots and
step count unchanged that step (the EMA update still runs), decided on the device so that a captured step stays a plain
replay.  Measured cost on BASELINE configs[2]: +0.06 % of the step."""
import importlib
import math
import os

import numpy as np
import torch

from . import _lib
from . import functional as F
from . import step_capture as SC
from .networks.loss import forward_discriminator, forward_generator, forward_simultaneous, linear_generator_link
from .networks.ops import Op, ScalarVariable
from .networks.pgan.variables import pgan_variable_shapes
from .varstore import compute_dtype, current_store, use_store


# ----------------------------------------------------------------------------------------------------
# optimizers (tf.train.* as used at optimization.py:16-37)
# ----------------------------------------------------------------------------------------------------
class _Optimizer:
    def __init__(self, learning_rate):
        self.lr = learning_rate
        self.t = 0
        self.state = {}          # prefix -> dict of flat state buffers
        self.distributed = None  # set by parallel.DistributedOptimizer
        self.t_dev = None        # non-finite guard: the step count on the device (authoritative while a guard holds it)

    def lr_value(self):
        return float(self.lr.eval()) if isinstance(self.lr, ScalarVariable) else float(self.lr)

    def step_size(self):
        """The scalar the update kernel multiplies with at the CURRENT step count (Adam: the bias-corrected lr_t)."""
        return self.lr_value()

    def next_step_size(self):
        """Captured step (StepGraph): advances the step count on the host and returns the scalar the replayed kernel reads
        from device memory (functional.DevScalars); `apply(..., lr_dev=...)` then leaves the count alone."""
        self.t += 1
        return self.step_size()

    def device_step_count(self, device):
        """The guard's device copy of the step count (int64 [1]), made from the host count on first use."""
        if self.t_dev is None:
            self.t_dev = torch.tensor([self.t], dtype=torch.int64, device=device)
        return self.t_dev

    def sync_step_count(self):
        """Host count <- device count (a sync: called only where the loop already waits for the device)."""
        if self.t_dev is not None:
            self.t = int(self.t_dev.item())
        return self.t

    def _guard_step(self, guard, adam=None):
        """Guarded step: the bookkeeping launch (device t, step size, skip counters); returns the device step size."""
        F.guard_step_(guard['flag'], self.t_dev, guard['counters'], guard['lr'], guard['lr_t'], adam=adam,
                      lr_dev=guard['lr_dev'])
        return guard['lr_t']

    def _slots(self, prefix, flat, names):
        st = self.state.get(prefix)
        if st is None or st['total'] != flat['total']:
            st = {n: torch.zeros_like(flat['param']) for n in names}
            st['total'] = flat['total']
            self.state[prefix] = st
        return st


class AdamOptimizer(_Optimizer):
    """tf.train.AdamOptimizer(learning_rate, beta1, beta2, epsilon=1e-8): SURVEY Appendix B."""

    def __init__(self, learning_rate, beta1=0.9, beta2=0.999, epsilon=1e-8):
        super().__init__(learning_rate)
        self.beta1, self.beta2, self.epsilon = float(beta1), float(beta2), float(epsilon)

    def step_size(self):
        return F.adam_step_size(self.lr_value(), self.beta1, self.beta2, self.t)

    def apply(self, prefix, flat, ranges, gscale, ema_flat, ema_decay, lr_dev=None, guard=None):
        st = self._slots(prefix, flat, ('m', 'v'))
        if guard is not None:       # skipped on the device when the gradient is not finite; t counts applied updates only
            lr_t = self._guard_step(guard, adam=(self.beta1, self.beta2))
            for (o, n) in ranges:
                F.adam_ema_(flat['param'][o:o + n], flat['grad'][o:o + n], st['m'][o:o + n], st['v'][o:o + n],
                            None if ema_flat is None else ema_flat[o:o + n], 0.0, self.beta1, self.beta2, 0, self.epsilon,
                            gscale, ema_decay, lr_dev=lr_t, skip=guard['flag'])
            return
        if lr_dev is None:
            self.t += 1
        lr = self.lr_value()
        for (o, n) in ranges:
            F.adam_ema_(flat['param'][o:o + n], flat['grad'][o:o + n], st['m'][o:o + n], st['v'][o:o + n],
                        None if ema_flat is None else ema_flat[o:o + n], lr, self.beta1, self.beta2, self.t,
                        self.epsilon, gscale, ema_decay, lr_dev=lr_dev)


class _FusedRule(_Optimizer):
    """Optimisers on sg_optim_step: one launch per contiguous range updates parameters, state and the EMA shadow."""
    KIND, SLOTS = None, ()

    def _hyper(self):
        return dict(h=0.0, eps=0.0, nesterov=False)

    def apply(self, prefix, flat, ranges, gscale, ema_flat, ema_decay, lr_dev=None, guard=None):
        st = self._slots(prefix, flat, self.SLOTS)
        if guard is not None:
            lr_dev = self._guard_step(guard)
        elif lr_dev is None:
            self.t += 1
        lr = self.lr_value()
        for (o, n) in ranges:
            s1 = st[self.SLOTS[0]][o:o + n] if len(self.SLOTS) > 0 else None
            s2 = st[self.SLOTS[1]][o:o + n] if len(self.SLOTS) > 1 else None
            F.optim_step_(self.KIND, flat['param'][o:o + n], flat['grad'][o:o + n], s1, s2,
                          None if ema_flat is None else ema_flat[o:o + n], lr, gscale=gscale, ema_decay=ema_decay,
                          lr_dev=lr_dev, skip=None if guard is None else guard['flag'], **self._hyper())


class GradientDescentOptimizer(_FusedRule):
    """tf.train.GradientDescentOptimizer(learning_rate): p -= lr * g (optimization.py:17-18,29-30)."""
    KIND = _lib.SG_OPT_SGD


class MomentumOptimizer(_FusedRule):
    """tf.train.MomentumOptimizer(learning_rate, momentum, use_nesterov): accum = momentum * accum + g;
    p -= lr * g + lr * momentum * accum (Nesterov, what optimization.py:21-22,34-35 asks for) or lr * accum."""
    KIND, SLOTS = _lib.SG_OPT_MOMENTUM, ('accum',)

    def __init__(self, learning_rate, momentum, use_nesterov=False):
        super().__init__(learning_rate)
        self.momentum, self.use_nesterov = float(momentum), bool(use_nesterov)

    def _hyper(self):
        return dict(h=self.momentum, eps=0.0, nesterov=self.use_nesterov)


class AdadeltaOptimizer(_FusedRule):
    """tf.train.AdadeltaOptimizer(learning_rate, rho, epsilon) (optimization.py:19-20,31-32: epsilon 1e-07)."""
    KIND, SLOTS = _lib.SG_OPT_ADADELTA, ('accum', 'accum_update')

    def __init__(self, learning_rate, rho=0.95, epsilon=1e-8):
        super().__init__(learning_rate)
        self.rho, self.epsilon = float(rho), float(epsilon)

    def _hyper(self):
        return dict(h=self.rho, eps=self.epsilon, nesterov=False)


def decays(name):
    """exclude_from_weight_decay of SURFGAN_2D/optim.py:70,79 as it applies to this project's variable names: biases are not
    decayed (its LayerNorm patterns match nothing here)."""
    return 'bias' not in name


class _SegmentedRule(_Optimizer):
    """Optimisers whose rule differs per variable (weight decay by name, LAMB's per-variable trust ratio): every launch
    covers all variables of the train op through a device table of their segments of the flat buffers
    (functional.SegmentTable), derived from flat['offsets'] restricted to `ranges` and cached per (prefix, ranges)."""

    def __init__(self, learning_rate, beta1=0.9, beta2=0.999, weight_decay_rate=0.0, epsilon=1e-6):
        super().__init__(learning_rate)
        self.beta1, self.beta2 = float(beta1), float(beta2)
        self.weight_decay_rate, self.epsilon = float(weight_decay_rate), float(epsilon)
        self.tables = {}

    def _slots(self, prefix, flat, names):
        st = self.state.get(prefix)
        if st is None or st['total'] != flat['total']:
            self.tables = {k: t for k, t in self.tables.items() if k[0] != prefix}      # (a new flat buffer: new tables)
        return super()._slots(prefix, flat, names)

    def _table(self, prefix, flat, ranges):
        """Allocated with the slots: the first apply of a (prefix, ranges) is never a captured one (StepGraph warms up
        eagerly), later ones only launch."""
        key = (prefix, tuple(ranges))
        tab = self.tables.get(key)
        if tab is None:
            segs = [(o, n, decays(name)) for name, (o, n) in flat['offsets'].items()
                    if any(lo <= o and o + n <= lo + ln for lo, ln in ranges)]
            tab = self.tables[key] = F.SegmentTable(segs, flat['total'], flat['param'].device)
        return tab

    def _launch(self, tab, flat, st, ema_flat, lr, gscale, ema_decay, lr_dev, skip):
        raise NotImplementedError

    def apply(self, prefix, flat, ranges, gscale, ema_flat, ema_decay, lr_dev=None, guard=None):
        st = self._slots(prefix, flat, ('m', 'v'))
        tab = self._table(prefix, flat, ranges)
        if guard is not None:      # t counts applied updates only: sg_guard_step advances the device count
            lr_dev = self._guard_step(guard)
        elif lr_dev is None:
            self.t += 1
        self._launch(tab, flat, st, ema_flat, self.lr_value(), gscale, ema_decay, lr_dev,
                     None if guard is None else guard['flag'])


class AdamWOptimizer(_SegmentedRule):
    """AdamWeightDecayOptimizer(learning_rate, weight_decay_rate, beta_1, beta_2, epsilon=1e-6) of SURFGAN_2D/optim.py:73-80
    (rule optim.py:246-267: Adam without bias correction, decay added to the update): one sg_adamw_ema launch per train op."""

    def _launch(self, tab, flat, st, ema_flat, lr, gscale, ema_decay, lr_dev, skip):
        F.adamw_ema_(tab, flat['param'], flat['grad'], st['m'], st['v'], ema_flat, lr, self.beta1, self.beta2, self.epsilon,
                     self.weight_decay_rate, gscale, ema_decay, lr_dev=lr_dev, skip=skip)


class LAMBOptimizer(_SegmentedRule):
    """LAMBOptimizer(learning_rate, weight_decay_rate, beta_1, beta_2, epsilon=1e-6) of SURFGAN_2D/optim.py:60-71 (rule
    optim.py:354-398): bias-corrected Adam direction plus decay, scaled per variable by the trust ratio |w| / |u|.  Three
    launches per train op (functional.lamb_ema_).  The bias corrections need t itself: it lives on the device
    (device_step_count), advanced there once per applied train op -- the captured step replays that -- with the host
    count alongside."""

    def _slots(self, prefix, flat, names):
        self.device_step_count(flat['param'].device)      # (made from the host count, before this apply advances it)
        return super()._slots(prefix, flat, names)

    def _launch(self, tab, flat, st, ema_flat, lr, gscale, ema_decay, lr_dev, skip):
        F.lamb_ema_(tab, flat['param'], flat['grad'], st['m'], st['v'], ema_flat, self.t_dev, lr, self.beta1, self.beta2,
                    self.epsilon, self.weight_decay_rate, gscale, ema_decay, lr_dev=lr_dev, skip=skip)


def get_optimizer(d_lr, g_lr, args):
    """optimization.py:6-45: Adam / SGD / Adadelta / Momentum (Nesterov), one per network; LAMB / AdamW as SURFGAN_2D/optim.py:60-80
    creates them."""
    def make(kind, lr, b1, b2, rho, momentum, decay):
        if kind == 'LAMB':
            return LAMBOptimizer(learning_rate=lr, beta1=b1, beta2=b2, weight_decay_rate=decay, epsilon=1e-6)
        elif kind == 'AdamW':
            return AdamWOptimizer(learning_rate=lr, beta1=b1, beta2=b2, weight_decay_rate=decay, epsilon=1e-6)
        elif kind == 'Adam':
            return AdamOptimizer(learning_rate=lr, beta1=b1, beta2=b2)
        elif kind == 'SGD':
            return GradientDescentOptimizer(learning_rate=lr)
        elif kind == 'Adadelta':
            return AdadeltaOptimizer(learning_rate=lr, rho=rho, epsilon=1e-07)
        elif kind == 'Momentum':
            return MomentumOptimizer(learning_rate=lr, momentum=momentum, use_nesterov=True)
        print(f"ERROR: optimizer argument {kind} not recognized or implemented")
        raise NotImplementedError
    rho, mom = getattr(args, 'rho', 0.95), getattr(args, 'momentum', 0.9)
    wd = getattr(args, 'weight_decay', 0.0)
    optimizer_gen = make(args.optimizer, g_lr, args.adam_beta1, args.adam_beta2, rho, mom, wd)
    optimizer_disc = make(args.d_optimizer, d_lr, args.d_adam_beta1, args.d_adam_beta2, getattr(args, 'd_rho', rho),
                          getattr(args, 'd_momentum', mom), getattr(args, 'd_weight_decay', wd))
    return optimizer_gen, optimizer_disc


# ----------------------------------------------------------------------------------------------------
# handles
# ----------------------------------------------------------------------------------------------------
class Placeholder:
    """tf.placeholder(shape, dtype): key of feed_dict (optuna_objective.py:147)."""

    def __init__(self, shape, dtype=torch.float32, name='real_image_input'):
        self.shape, self.dtype, self.name = list(shape), dtype, name


class Fetch:
    def __init__(self, graph, key, net=None, freeze=False):
        self.graph, self.key, self.net, self.freeze = graph, key, net, freeze

    def __repr__(self):
        return f'<Fetch {self.key}{"" if self.net is None else ":" + self.net}{"/freeze" if self.freeze else ""}>'


class VarRef:
    """What the reference's `variables` lists hold: something with a TF-style .name."""

    def __init__(self, name):
        self.name = name + ':0'
        self.key = name

    def __repr__(self):
        return f'<Variable {self.name}>'


def _key(v):
    n = v if isinstance(v, str) else getattr(v, 'key', None) or v.name
    return n[:-2] if n.endswith(':0') else n


def minimize_with_clipping(optimizer, loss, var_list, clipping):
    """optimization.py:47-75 -> (train_op, gradients, variables, max_norm) as deferred handles."""
    graph = loss.graph
    net = 'generator' if loss.key == 'gen_loss' else 'discriminator'
    names = [_key(v) for v in var_list]
    tid = graph.add_train(net, optimizer, names, clipping)
    return (Fetch(graph, 'train', tid), Fetch(graph, 'gradients', tid), [VarRef(n) for n in names],
            Fetch(graph, 'max_norm', tid))


# ----------------------------------------------------------------------------------------------------
# non-finite step guard (not in the reference)
# ----------------------------------------------------------------------------------------------------
class NonFiniteStepsError(RuntimeError):
    """A network's train op was skipped --max_consecutive_nonfinite times in a row."""


def nonfinite_guard_settings():
    """(on, max_consecutive) as saragan_amd.set_nonfinite_guard / SARAGAN_NONFINITE_GUARD=1 left them: read when a StepGraph
    is built."""
    on = os.environ.get('SARAGAN_NONFINITE_GUARD', '') == '1'
    mc = os.environ.get('SARAGAN_NONFINITE_MAX_CONSECUTIVE', '')
    return on, (int(mc) if on and mc else None)


class NonFiniteGuard:
    """Device state of a StepGraph's guard.  Each train op checks its network's gradient after the data-parallel reduction
    and before clipping (sg_nonfinite_flag, or fused into the clipping path's sg_segment_sumsq_flag); one bookkeeping thread
    (sg_guard_step) then advances the optimiser's device step count and writes the step size -- or counts a skip -- and the
    guarded update (sg_adam_ema_guarded / sg_optim_step_guarded) reads the flag: clear, exactly the unguarded update; set,
    the EMA-only update.  Nothing is read back: the host sees the counters only where it syncs anyway."""
    NETS = ('generator', 'discriminator')

    def __init__(self, max_consecutive=None):
        if max_consecutive is not None and int(max_consecutive) < 1:
            raise ValueError('max_consecutive must be >= 1')
        self.max_consecutive = None if max_consecutive is None else int(max_consecutive)
        self.device = None

    def prepare(self, graph, device):
        """Allocates the flags, step sizes and counters and the optimisers' device step counts (outside any capture)."""
        for tr in graph.trains:
            tr['optimizer'].device_step_count(device)
        if self.device is not None:
            return
        n = max(1, len(graph.trains))
        self.flags = torch.zeros(n, dtype=torch.int32, device=device)
        self.lr_t = torch.zeros(n, dtype=torch.float32, device=device)
        self.counters = {net: torch.zeros(3, dtype=torch.int64, device=device) for net in self.NETS}
        self.lr = F.DevScalars(device, n, dtype=torch.float64)     # base learning rates of a captured step (host-written)
        self.device = device

    def flag(self, tid):
        return self.flags[tid:tid + 1]

    def args(self, tid, net, optimizer, lr_dev=None):
        """What a guarded optimizer.apply launches with.  lr_dev: the captured step's device copy of the base learning rate
        (lr_coef); eager: the host value rides as a kernel argument."""
        return dict(flag=self.flag(tid), lr_t=self.lr_t[tid:tid + 1], counters=self.counters[net],
                    lr=optimizer.lr_value(), lr_dev=lr_dev)

    def lr_coef(self, tid, value):
        return self.lr.coef(tid, value)

    def read(self):
        """{net: (skipped, consecutive, longest run)}: one device-to-host copy (a sync)."""
        if self.device is None:
            return {net: (0, 0, 0) for net in self.NETS}
        c = torch.stack([self.counters[net] for net in self.NETS]).cpu().tolist()
        return {net: tuple(int(x) for x in row) for net, row in zip(self.NETS, c)}


class StepGraph:
    """Everything optimize_step was told, plus the machinery to execute it."""

    def __init__(self, store, cfg):
        self.store, self.cfg = store, cfg
        self.trains = []       # dicts: net, optimizer, names, clipping
        self.ema = None        # ExtendedEMA fused into the optimiser launches
        self.last = {}
        self.flat_ready = False
        self.allreduce = None  # parallel.GradientAllReducer
        self.world = 1
        self._cond = None      # the label rows of the step in flight (a conditional graph; run() sets them)
        on, max_consecutive = nonfinite_guard_settings()
        self.guard = NonFiniteGuard(max_consecutive) if on else None
        self._stepped, self._wanted = False, set()      # configure_guard: only before the first step; (key, net) of the step's fetches
        self._captures = {}    # capture key -> dict: eager, ratios, probes, decided, used and, once captured, graph (a CapturedStep)
        self._cap_clock, self._cap_pool = 0, None      # `used` of the entry touched last; the memory pool the captures share
        self._issue_log = None  # tests: a list here records the issue order of replayed segments and bucket collectives

    def add_train(self, net, optimizer, names, clipping):
        self.trains.append(dict(net=net, optimizer=optimizer, names=names, clipping=bool(clipping)))
        self._refuse_guard_with_adasum()
        self._refuse_spectral_with_adasum()
        return len(self.trains) - 1

    # -- spectral normalisation (not used by the reference's pgan; networks.ops.set_spectral_norm) ----------------------------
    def _refuse_spectral_with_adasum(self):
        for t in self.trains:
            if getattr(t['optimizer'].distributed, 'delta_form', False) and \
                    any(n in self.store.effective for n in t['names']):
                # Adasum combines the ranks' LOCAL weight deltas: their raw weights differ between the local step and the
                # combination, and so would u and the effective weights.  Refused rather than half-supported.
                raise ValueError('spectral normalisation does not support Adasum (--use_adasum): use the Average reduction '
                                 'or turn --d_spectral_norm off')

    def _refresh_effective(self, force=False):
        """Before a discriminator forward: W / sigma of the normalised weights -- a fixed number of launches on the current
        stream, eager or captured; every discriminator pass up to the next refresh shares the result.  A `simultaneous` step
        refreshes if the raw weights were rewritten since the last refresh (the optimiser step, a restore, a hand-off: every
        step of a training loop); an `alternate` step always does two, before forward_discriminator and before
        forward_generator."""
        if self.store.effective:
            self.store.refresh_effective('discriminator/', self.cfg.get('sn_iterations', 1), force=force)

    def _pull_back(self, info):
        """The flat buffer holds the gradient with respect to the effective weights in the raw weights' own slots: mapped in
        place to the gradient with respect to the raw weights (two launches).  Linear in the gradient with the same W / sigma,
        u, v, sigma on every rank: it commutes with the all-reduce sum and with gscale."""
        flat = info['flat']
        if flat.get('spectral') is not None and any(n in self.store.effective for n in info['names']):
            # the launches cover every normalised layer of the network: the slots of those outside this train op (frozen while
            # mixing) are cleared first, or what another train op left there would be divided by sigma again every step
            mine = set(info['names'])
            for n in flat['normalised']:
                if n not in mine:
                    o, cnt = flat['offsets'][n]
                    flat['grad'][o:o + cnt].zero_()
            F.spectral_pullback_(flat['spectral'], flat['grad'], flat['eff'])

    # -- non-finite step guard ------------------------------------------------------------------------------------------
    def configure_guard(self, on=True, max_consecutive=None):
        """Turns the non-finite step guard on (or off) for this step graph, before its first step."""
        if self._stepped:
            raise RuntimeError('configure_guard: call it before the first training step of the step graph')
        self.guard = NonFiniteGuard(max_consecutive) if on else None
        self._refuse_guard_with_adasum()

    def _refuse_guard_with_adasum(self):
        if self.guard is not None and any(getattr(t['optimizer'].distributed, 'delta_form', False) for t in self.trains):
            # Adasum combines each rank's LOCAL weight delta: the ranks' gradients (and flags) differ, and a skipped rank's
            # zero delta has no Adasum combination.  Refused rather than half-supported.
            raise ValueError('the non-finite step guard does not support Adasum (--use_adasum): use the Average reduction '
                             'or turn the guard off')

    @property
    def skipped_steps(self):
        """{'generator': n, 'discriminator': n} skipped train ops (reads the device: a host sync)."""
        rep = self.guard.read() if self.guard is not None else {n: (0, 0, 0) for n in NonFiniteGuard.NETS}
        return {net: c[0] for net, c in rep.items()}

    def guard_report(self):
        """{net: (skipped, consecutive, longest run)}, and the optimisers' host step counts brought in line with the device
        (a host sync: for the loop's existing sync points -- log line, checkpoint, phase end)."""
        if self.guard is None:
            return None
        for tr in self.trains:
            tr['optimizer'].sync_step_count()
        return self.guard.read()

    def check_nonfinite(self, global_step, report=None):
        """Raises NonFiniteStepsError if a network's train op was skipped max_consecutive times in a row."""
        if self.guard is None or self.guard.max_consecutive is None:
            return
        report = report or self.guard.read()
        for net, (_, _, longest) in report.items():
            if longest >= self.guard.max_consecutive:
                raise NonFiniteStepsError(f'{net}: {longest} consecutive training steps had a non-finite gradient and were '
                                          f'skipped (limit {self.guard.max_consecutive}) at global_step {global_step}')

    # -- flat buffers: frozen (previous-phase) variables first, new ones last -------------------------
    def _ensure_flat(self):
        if self.flat_ready:
            return
        fz = set(self.cfg['freeze_names'] or [])
        for prefix in ('generator/', 'discriminator/'):
            names = self.store.names(prefix)
            order = [n for n in names if n in fz] + [n for n in names if n not in fz]
            self.store.flatten(prefix, order)
        self.flat_ready = True

    def _ranges(self, prefix, names):
        """Contiguous (offset, length) runs in the flat buffer covering `names` (padding included)."""
        offs = self.store.flat[prefix]['offsets']
        want = set(names)
        runs, cur = [], None
        for k, (o, n) in offs.items():
            npad = (n + 3) // 4 * 4
            if k in want:
                if cur is not None and cur[0] + cur[1] == o:
                    cur[1] += npad
                else:
                    if cur is not None:
                        runs.append(tuple(cur))
                    cur = [o, npad]
        if cur is not None:
            runs.append(tuple(cur))
        return runs

    # -- execution ----------------------------------------------------------------------------------
    def _labels(self, cond, n):
        """The label rows of a step or a gen_sample fetch: None for an unconditional graph, else the fed [n, L] rows (f32, on
        the device)."""
        ph = self.cfg.get('conditioning')
        if ph is None:
            if cond is not None:
                raise ValueError('conditioning was fed to a step graph built without it (optimize_step(..., conditioning=...))')
            return None
        if cond is None:
            raise ValueError('conditioning must be fed')
        if tuple(cond.shape) != (int(n), int(ph.shape[1])):
            raise ValueError(f'conditioning: expected label rows of shape {(int(n), int(ph.shape[1]))}, got {tuple(cond.shape)}')
        return cond

    def _cond_kw(self):
        """conditioning=... for the loss builders of a conditional graph (none otherwise: their calls are what they were)."""
        return {} if self._cond is None else dict(conditioning=self._cond)

    def generate(self, z, cond=None):
        """The generator's forward alone, under the current weights and alpha, for the CALLER's latents z [n, latent_dim] (any
        n; cond: the [n, L] label rows of a conditional graph): no discriminator pass, no gradient, and no draw from any random
        stream -- what a gen_sample fetch runs on its own draw, and what the previews (preview.py) run on their fixed latents."""
        c = self.cfg
        self._ensure_flat()
        cond = self._labels(cond, z.shape[0])
        kw = {} if cond is None else dict(conditioning=cond.to(z.device))
        with use_store(self.store), torch.no_grad():
            alpha = float(c['alpha'].eval()) if isinstance(c['alpha'], ScalarVariable) else float(c['alpha'])
            sample = c['generator'](z, alpha, c['phase'], c['base_shape'], activation=c['activation'],
                                    kernel_spec=c['kernel_spec'], filter_spec=c['filter_spec'], param=c['leakiness'], **kw)
        return sample.detach()

    def run(self, fetches, feed, cond=None):
        c = self.cfg
        self._ensure_flat()
        train_ids = sorted({f.net for f in fetches if f.key in ('train', 'gradients', 'max_norm')})
        want_train = {f.net for f in fetches if f.key == 'train'}
        self._wanted = {(f.key, f.net) for f in fetches}
        real = feed
        if all(f.key == 'gen_sample' for f in fetches):
            # sess.run(gen_sample) (metrics/save_metrics.py:104: fake images for the validation metrics): TF prunes the graph
            # to the generator; so does this -- fresh latents, the current weights and alpha, no discriminator pass
            from .networks import loss as L
            n = c['placeholder'].shape[0]
            dev = self.store.device if real is None else real.device
            cond = self._labels(cond, n)
            sample = self.generate(L._rng(dev).latent(n, c['latent_dim'], dev), cond)
            return [sample for _ in fetches]
        self._cond = self._labels(cond, real.shape[0])
        self._stepped = True
        self._refuse_spectral_with_adasum()
        if self.guard is not None:
            self._refuse_guard_with_adasum()
            self.guard.prepare(self, real.device)
        with use_store(self.store), torch.enable_grad():
            alpha = float(c['alpha'].eval()) if isinstance(c['alpha'], ScalarVariable) else float(c['alpha'])
            net_args = (c['latent_dim'], alpha, c['phase'], c['base_shape'], c['kernel_spec'], c['filter_spec'],
                        c['activation'], c['leakiness'], c['loss_fn'])
            strategy = c['optim_strategy']      # alternate: D step, then G forward on the updated D (captured without a reducer only)
            no_dist = strategy == 'simultaneous' or all(self.trains[t]['optimizer'].distributed is None for t in train_ids)
            if no_dist and SC.capturable(self, train_ids, real):
                out = self._replay_or_capture(real, train_ids, want_train, net_args, alpha, strategy)
            else:
                out = self._eager_step(real, train_ids, want_train, net_args, strategy)
        static = out.pop('__static__', False)     # a replayed graph's outputs live in buffers the next replay overwrites
        self.last = None if static else out

        def own(v):       # what the caller gets is his to keep (the eager path returns fresh tensors each step)
            return v.clone() if static and torch.is_tensor(v) else v
        res = []
        for f in fetches:
            if f.key in ('train',):
                res.append(None)
            elif f.key == 'gradients':
                res.append(out[('gradients', f.net)])
            elif f.key == 'max_norm':
                res.append(own(out.get(('max_norm', f.net))))
            else:
                v = out[f.key]
                res.append(own(v.detach()) if torch.is_tensor(v) else v)
        return res

    def _compute_alternate(self, real, train_ids, want_train, net_args, out, lr_dev=None, marks=None):
        """One 'alternate' step (optimization.py:166-216 of the reference): the discriminator is updated from forward_discriminator's
        loss; the generator loss is then built on the UPDATED discriminator and the generator is updated."""
        c = self.cfg
        lr_dev = lr_dev or {}
        d_ids = [t for t in train_ids if self.trains[t]['net'] == 'discriminator']
        g_ids = [t for t in train_ids if self.trains[t]['net'] == 'generator']
        self._refresh_effective(force=True)
        disc_loss, gp_loss = forward_discriminator(c['generator'], c['discriminator'], real, *net_args,
                                                   c['gp_weight'], c['noise_stddev'], **self._cond_kw())
        out.update(disc_loss=disc_loss, gp_loss=gp_loss)
        for tid in d_ids:
            self._finish(tid, self._backward(tid, out), out, apply=tid in want_train, lr_dev=lr_dev.get(tid), marks=marks)
        self._refresh_effective(force=True)      # (the updated discriminator)
        gen_sample, gen_loss = forward_generator(c['generator'], c['discriminator'], real, *net_args,
                                                 c['noise_stddev'], is_reuse=True, **self._cond_kw())
        out.update(gen_sample=gen_sample, gen_loss=gen_loss)
        for tid in g_ids:
            self._finish(tid, self._backward(tid, out), out, apply=tid in want_train, lr_dev=lr_dev.get(tid), marks=marks)

    def _compute_simultaneous(self, real, train_ids, net_args, out, arm_dist=True, between=None):
        """Forward pass and both backward passes of a 'simultaneous' step (no optimizer): fills `out`, returns the per-net
        records `_finish` needs.  between(j): called between backward pass j and j + 1 (the segmented capture cuts there)."""
        c = self.cfg
        self._refresh_effective()
        nets = {self.trains[t]['net'] for t in train_ids}
        if nets >= {'generator', 'discriminator'}:
            with linear_generator_link():   # wgan: G's gradient through D comes out of D's own backward
                gen_loss, disc_loss, gp_loss, gen_sample = forward_simultaneous(
                    c['generator'], c['discriminator'], real, *net_args, c['gp_weight'], c['noise_stddev'], **self._cond_kw())
        else:
            gen_loss, disc_loss, gp_loss, gen_sample = forward_simultaneous(
                c['generator'], c['discriminator'], real, *net_args, c['gp_weight'], c['noise_stddev'], **self._cond_kw())
        out.update(gen_loss=gen_loss, disc_loss=disc_loss, gp_loss=gp_loss, gen_sample=gen_sample)
        if hasattr(gen_loss, 'sg_link'):    # the discriminator's backward must run first: it feeds G's
            train_ids = sorted(train_ids, key=lambda t: self.trains[t]['net'] != 'discriminator')
        pend = []
        for j, tid in enumerate(train_ids):   # both gradients at the pre-step weights (optimization.py:128-163)
            pend.append((tid, self._backward(tid, out, retain=j + 1 < len(train_ids), arm_dist=arm_dist)))
            if between is not None and j + 1 < len(train_ids):
                between(j)
        return pend

    # -- hipGraph capture of the step (step_capture.py: when a key is captured, and what a captured key owns and does) --------
    _MAX_CAPTURES = 4

    def _eager_step(self, real, train_ids, want_train, net_args, strategy):
        out = {}
        if strategy == 'alternate':
            self._compute_alternate(real, train_ids, want_train, net_args, out)
        else:
            for tid, info in self._compute_simultaneous(real, train_ids, net_args, out):
                self._finish(tid, info, out, apply=tid in want_train)
        return out

    def _replay_or_capture(self, real, train_ids, want_train, net_args, alpha, strategy):
        key = SC.capture_key(self, real, train_ids, want_train, alpha, strategy)
        ent = self._captures.get(key)
        if ent is None:
            ent = self._captures[key] = dict(eager=0, ratios=[])
        ent['used'] = self._cap_clock = self._cap_clock + 1
        if 'graph' in ent:
            ent['graph'].refill(real, self._cond, alpha)
        else:
            dist_ids = tuple(t for t in train_ids if self.trains[t]['optimizer'].distributed is not None)
            out = SC.warm_up(ent, lambda: self._eager_step(real, train_ids, want_train, net_args, strategy), bool(dist_ids), real.device)
            if out is not None:
                return out
            SC.evict(self._captures, self._MAX_CAPTURES)
            try:
                ent['graph'] = SC.CapturedStep(self, real, train_ids, want_train, net_args, alpha, strategy, dist_ids)
            except BaseException:      # this key stays on the eager path from now on
                ent['decided'] = 'eager'
                raise
        return ent['graph'].replay()

    def _backward(self, tid, out, retain=False, arm_dist=True):
        tr = self.trains[tid]
        prefix = tr['net'] + '/'
        flat = self.store.flat[prefix]
        names = [n for n in tr['names'] if n in flat['offsets']]
        ranges = self._ranges(prefix, names)
        for (o, n) in ranges:
            flat['grad'][o:o + n].zero_()
        # a normalised weight's effective leaf stands in for the raw parameter: the networks read it, and its gradient lands in
        # the raw parameter's own slot (same shape), where _finish pulls it back to the raw weight
        params = [self.store.stand_in(n) for n in names]
        slots = {}
        for p, n in zip(params, names):      # .grad views may have been replaced by autograd: re-point them
            o, cnt = flat['offsets'][n]
            p.grad = slots[id(p)] = flat['grad'][o:o + cnt].view(p.shape)
            if p is not self.store.vars[n]:
                self.store.vars[n].grad = slots[id(p)]
        loss = out['gen_loss'] if tr['net'] == 'generator' else out['disc_loss']
        dist = tr['optimizer'].distributed
        other = 'discriminator/' if tr['net'] == 'generator' else 'generator/'
        link = getattr(out['gen_loss'], 'sg_link', None) if 'gen_loss' in out else None
        if dist is not None and arm_dist:      # (a captured backward launches no collective: they follow the replay)
            roots = [link[0]] if (link is not None and tr['net'] == 'generator') else [loss]
            dist.land = lambda p: self._land(p, slots)      # (a bucket goes out from the hook of its last parameter)
            dist.begin(flat['grad'], ranges, params, roots if getattr(dist, 'world_size', 1) > 1 else None)
        # The kernels write the first gradient of every parameter straight into its slot of the (zeroed) flat buffer and
        # autograd adopts that tensor as .grad (F.grads_into): .grad starts out unset, and is checked afterwards (_land)
        for p in params:
            p.grad = None
        with F.grads_into({p.data_ptr(): slots[id(p)] for p in params}), \
                F.skip_param_grads(self.store.grad_leaves(other)):   # e.g. D's weights under the G loss
            if link is None:
                torch.autograd.backward(loss, inputs=params, retain_graph=retain)
            elif tr['net'] == 'discriminator':   # also deliver d disc_loss / d fake for the generator's backward
                link[1].grad = None
                torch.autograd.backward(loss, inputs=params + [link[1]], retain_graph=retain)
            else:
                start, leaf, factor = link
                if leaf.grad is None:
                    raise RuntimeError('linked generator backward before the discriminator backward')
                torch.autograd.backward(start, grad_tensors=leaf.grad * factor, inputs=params, retain_graph=retain)
        for p in params:
            self._land(p, slots)
        return dict(prefix=prefix, flat=flat, names=names, ranges=ranges, dist=dist)

    @staticmethod
    def _land(p, slots):
        """After backward: p.grad IS p's slot of the flat gradient buffer.  Unreached parameter: the zeros the slot was
        cleared to; a gradient autograd summed into a tensor of its own (more than one contribution): copied in."""
        slot = slots[id(p)]
        g = p.grad
        if g is None:
            F.GRAD_DEST_STATS['unreached'] += 1
        elif g.data_ptr() != slot.data_ptr() or g.dtype != slot.dtype:
            if p.data_ptr() in F.ACCUMULATED_IN_PLACE:
                raise RuntimeError('a gradient contribution was added in place to the flat-buffer slot of a parameter whose .grad '
                                   'autograd then assembled elsewhere: copying it in would drop that contribution '
                                   '(functional._grad_acc; SARAGAN_NO_GRAD_DEST=1 avoids the in-place path)')
            F.GRAD_DEST_STATS['copied'] += 1
            slot.copy_(g)
        elif g is not slot:
            F.GRAD_DEST_STATS['adopted'] += 1
        p.grad = slot

    def _finish(self, tid, info, out, apply, lr_dev=None, marks=None):
        tr = self.trains[tid]
        flat, ranges, names = info['flat'], info['ranges'], info['names']
        gscale = 1.0
        if info['dist'] is not None:
            info['dist'].finish()              # waits for the bucketed reductions
            gscale = info['dist'].grad_scale   # 1 / world after a SUM (the average is folded into the update kernel)
        self._pull_back(info)
        norms = tr['clipping'] or ('max_norm', tid) in self._wanted
        guard = None
        if apply and self.guard is not None:
            # the reduced gradient, before clipping (an Inf would make the clip scale 0 and the products NaN); with norms
            # wanted the test rides in their pass
            guard = self.guard.args(tid, tr['net'], tr['optimizer'], lr_dev)
            if not norms:
                for j, (o, n) in enumerate(ranges):
                    F.nonfinite_flag_(guard['flag'], flat['grad'][o:o + n], accumulate=j > 0)
        if norms:
            if 'bounds' not in tr:
                offs = flat['offsets']
                b = torch.tensor([[offs[n][0], offs[n][0] + offs[n][1]] for n in names], dtype=torch.int64)
                tr['bounds'] = b.reshape(-1).to(flat['grad'].device)
            # per-variable squared norms in ONE launch: offsets interleave [start_i, end_i); the odd segments
            # are the alignment padding between variables and are dropped
            sq = F.segment_sumsq(flat['grad'], tr['bounds'], tr['bounds'].numel() - 1,
                                 flag=None if guard is None else guard['flag'])[0::2] * (gscale * gscale)
            if tr['clipping']:                 # tf.clip_by_global_norm(gradients, 1.0), optimization.py:66-67
                scale = 1.0 / torch.clamp(torch.sqrt(sq.sum()), min=1.0)
                out[('max_norm', tid)] = torch.sqrt(sq).max() * scale
                # the clip factor stays on the device (reading it back would stall the host every step): the gradients
                # are scaled in place, which also makes the returned `gradients` the clipped ones, as the reference's are
                for (o, n) in ranges:
                    flat['grad'][o:o + n].mul_(scale * gscale)
                gscale = 1.0
            else:
                out[('max_norm', tid)] = torch.sqrt(sq).max()
        out[('gradients', tid)] = [self.store.vars[n].grad for n in names]
        if gscale != 1.0 and ('gradients', tid) in self._wanted:
            # unclipped, the flat buffer holds the SUM over ranks (the average is folded into the update kernel);
            # hvd.DistributedOptimizer.compute_gradients returns the average: scaled here, only where they are fetched
            out[('gradients', tid)] = [g * gscale for g in out[('gradients', tid)]]
        if apply and info['dist'] is not None and getattr(info['dist'], 'delta_form', False):
            # hvd.Adasum on a TF1 optimizer (parallel.AdasumReducer): local step, then the ranks' weight deltas are combined.
            # The EMA update must see the combined weights: it is left to ExtendedEMA.apply (these ranges stay unmarked).
            lo, hi = info['dist'].hull()
            start = flat['param'][lo:hi].clone()
            tr['optimizer'].apply(info['prefix'], flat, ranges, gscale, None, 0.0)
            info['dist'].combine_deltas(flat['param'], start)
            F.mark_packs_stale()
        elif apply:
            ema_flat = self.ema.shadow_flat(info['prefix']) if self.ema is not None else None
            ema_decay = self.ema.decay if self.ema is not None else 0.0
            tr['optimizer'].apply(info['prefix'], flat, ranges, gscale, ema_flat, ema_decay, lr_dev=lr_dev, guard=guard)
            self.store.mark_rewritten(info['prefix'])
            if self.ema is not None:
                self.ema.mark_updated(info['prefix'], ranges)
                if marks is not None:       # a replay repeats this bookkeeping (ExtendedEMA.apply skips the covered ranges)
                    marks.append((info['prefix'], ranges))


def optimize_step(optimizer_gen, optimizer_disc, generator, discriminator, real_image_input, latent_dim, alpha, phase,
                  base_shape, kernel_spec, filter_spec, activation, leakiness, loss_fn, gp_weight, optim_strategy,
                  g_clipping, d_clipping, noise_stddev, freeze_vars=None, conditioning=None):
    """optimization.py:77-224: returns the same 20-tuple (handles for Session.run).  conditioning (the reference keeps
    `# conditioning=real_label` at :182): a second Placeholder([N, L]) for the label rows of the real batch; Session.run reads
    them from feed_dict for every step and every gen_sample fetch of the graph (3-D pgan only)."""
    if optim_strategy not in ('simultaneous', 'alternate'):
        raise ValueError("Unknown optim strategy ", optim_strategy)
    if loss_fn not in ('wgan', 'logistic'):
        raise ValueError(f"Unknown loss function: {loss_fn}")
    store = current_store()
    # a new step graph (a new phase of the progressive run): the packed images and kept workspaces of the previous one are released
    # (the image cache holds its parameters; within a phase the images stay in place and are refreshed together, functional.py)
    F.clear_pack_cache()
    F.clear_kept_workspaces()
    # the architecture's own variable plan (networks/<arch>/variables.py), found from the generator's module the way
    # the reference finds the networks themselves (optuna_objective.py:64-65)
    arch_pkg = getattr(generator, '__module__', '').rsplit('.', 1)[0]
    try:
        plan = importlib.import_module(arch_pkg + '.variables').variable_shapes
    except (ImportError, AttributeError, ValueError):
        plan = pgan_variable_shapes
    if conditioning is not None:
        if not isinstance(conditioning, Placeholder) or len(conditioning.shape) != 2 or int(conditioning.shape[1]) < 1:
            raise ValueError('optimize_step: conditioning is a Placeholder([N, L]) with L >= 1')
        if int(conditioning.shape[0]) != int(real_image_input.shape[0]):
            raise ValueError(f'optimize_step: conditioning holds {conditioning.shape[0]} rows for a batch of '
                             f'{real_image_input.shape[0]}')
        if plan is not pgan_variable_shapes:
            raise NotImplementedError(f'conditioning is offered for the 3-D pgan architecture only, not for {arch_pkg}')
        shapes = plan(phase, base_shape, latent_dim, kernel_spec, filter_spec, label_dim=int(conditioning.shape[1]))
    else:
        shapes = plan(phase, base_shape, latent_dim, kernel_spec, filter_spec)
    for name, shp in shapes.items():           # create in the reference's order (weights N(0,1), biases 0)
        store.get(name, shp, 'normal' if name.endswith('weight') else 'zeros')
    from .networks import ops as nops
    for name in shapes:                        # (not in the reference) the weights networks.ops.set_spectral_norm names
        if nops.spectral_norm_applies(name):
            store.normalise(name)
    freeze_names = None if freeze_vars is None else [_key(v) for v in freeze_vars]
    cfg = dict(sn_iterations=nops.spectral_norm_settings()[1], generator=generator, discriminator=discriminator, latent_dim=latent_dim, alpha=alpha, phase=phase,
               base_shape=base_shape, kernel_spec=kernel_spec, filter_spec=filter_spec, activation=activation,
               leakiness=leakiness, loss_fn=loss_fn, gp_weight=gp_weight, optim_strategy=optim_strategy,
               noise_stddev=noise_stddev, freeze_names=freeze_names, placeholder=real_image_input, conditioning=conditioning)
    graph = StepGraph(store, cfg)
    gen_loss, disc_loss = Fetch(graph, 'gen_loss'), Fetch(graph, 'disc_loss')
    gp_loss, gen_sample = Fetch(graph, 'gp_loss'), Fetch(graph, 'gen_sample')

    gen_vars = [n for n in shapes if n.startswith('generator/')]
    disc_vars = [n for n in shapes if n.startswith('discriminator/')]
    train_gen, g_gradients, g_variables, max_g_norm = minimize_with_clipping(optimizer_gen, gen_loss, gen_vars, g_clipping)
    train_gen_freeze = g_gradients_freeze = g_variables_freeze = max_g_norm_freeze = None
    if freeze_names is not None:
        gen_vars_limited = [n for n in gen_vars if n not in set(freeze_names)]
        train_gen_freeze, g_gradients_freeze, g_variables_freeze, max_g_norm_freeze = minimize_with_clipping(
            optimizer_gen, gen_loss, gen_vars_limited, g_clipping)
    train_disc, d_gradients, d_variables, max_d_norm = minimize_with_clipping(optimizer_disc, disc_loss, disc_vars, d_clipping)
    train_disc_freeze = d_gradients_freeze = d_variables_freeze = max_d_norm_freeze = None
    if freeze_names is not None:
        disc_vars_limited = [n for n in disc_vars if n not in set(freeze_names)]
        train_disc_freeze, d_gradients_freeze, d_variables_freeze, max_d_norm_freeze = minimize_with_clipping(
            optimizer_disc, disc_loss, disc_vars_limited, d_clipping)

    return train_gen, train_disc, gen_loss, disc_loss, gp_loss, gen_sample, g_gradients, g_variables, \
        d_gradients, d_variables, max_g_norm, max_d_norm, \
        train_gen_freeze, g_gradients_freeze, g_variables_freeze, max_g_norm_freeze, \
        train_disc_freeze, d_gradients_freeze, d_variables_freeze, max_d_norm_freeze


def lr_update(lr, intra_phase_step, steps_per_phase, lr_max, lr_increase, lr_decrease, lr_rise_niter, lr_decay_niter):
    """optimization.py:227-296: returns the op that assigns the scheduled value to `lr` (f32 arithmetic)."""
    def val(v):
        return v.eval() if isinstance(v, ScalarVariable) else v

    def compute():
        step = int(val(intra_phase_step))
        total = int(val(steps_per_phase))
        lmax = np.float32(val(lr_max))
        new = lmax
        if lr_increase or lr_decrease:
            a = np.float32(lmax / np.float32(100))
            if lr_increase == 'linear':
                if step < lr_rise_niter:
                    new = np.float32(step / lr_rise_niter) * lmax
            elif lr_increase == 'exponential':
                if step < lr_rise_niter:
                    new = a * np.exp(np.float32(np.log(100) / lr_rise_niter) * np.float32(step), dtype=np.float32)
            if lr_decrease:
                step_decay_start = total - lr_decay_niter
                remaining = total - step
                if lr_decrease == 'linear':
                    if step > step_decay_start:
                        new = np.float32(remaining / lr_decay_niter) * lmax
                elif lr_decrease == 'exponential':
                    if step > step_decay_start:
                        new = a * np.exp(np.float32(np.log(100) / lr_decay_niter) * np.float32(remaining),
                                         dtype=np.float32)
        return lr.assign(new)
    return Op(compute, 'lr_update')


class Session:
    """Eager counterpart of tf.Session for this path: run(fetches, feed_dict) over Fetch handles and Ops."""

    def __init__(self, device='cuda'):
        self.device = torch.device(device)

    def run(self, fetches, feed_dict=None):
        single = not isinstance(fetches, (list, tuple))
        fl = [fetches] if single else list(fetches)
        results = [None] * len(fl)
        graphs = {}
        for i, f in enumerate(fl):
            if isinstance(f, Op):
                results[i] = f.run()
            elif isinstance(f, Fetch):
                graphs.setdefault(id(f.graph), (f.graph, []))[1].append(i)
            elif f is None:
                results[i] = None
            else:
                raise TypeError(f'cannot run {f!r}')
        for graph, idxs in graphs.values():
            ph = graph.cfg['placeholder']
            cond = None
            cph = graph.cfg.get('conditioning')
            if cph is not None and feed_dict is not None and cph in feed_dict:
                cond = feed_dict[cph]
                if not torch.is_tensor(cond):
                    cond = torch.from_numpy(np.ascontiguousarray(cond))
                cond = cond.to(self.device, torch.float32, non_blocking=True).contiguous()
            if all(fl[i].key == 'gen_sample' for i in idxs) and (feed_dict is None or ph not in feed_dict):
                vals = graph.run([fl[i] for i in idxs], None, cond)      # the generator alone needs no real batch
                for i, v in zip(idxs, vals):
                    results[i] = v
                continue
            if feed_dict is None or ph not in feed_dict:
                raise ValueError('real_image_input must be fed')
            batch = feed_dict[ph]
            if not torch.is_tensor(batch):
                batch = torch.from_numpy(np.ascontiguousarray(batch))
            batch = batch.to(self.device, torch.float32, non_blocking=True)
            vals = graph.run([fl[i] for i in idxs], batch, cond)
            for i, v in zip(idxs, vals):
                results[i] = v
        return results[0] if single else results
