"""Name-keyed variable store: the eager stand-in for TF1's variable scopes that the reference relies on
(`tf.variable_scope` / `tf.get_variable`, SURFGAN_3D/networks/ops.py:118,131 and pgan/*.py).  Variable names
are the reference's (without the ':0' suffix), so checkpoints, the phase hand-off and
the parameter-count KAT use the same keys.  Parameters are f32 masters; `flatten()` re-homes them in one flat
buffer per network so that the fused Adam/EMA kernel and the gradient all-reduce see contiguous memory."""
import contextlib
from collections import OrderedDict

import torch

_STATE = {'store': None, 'scope': []}
COMPUTE_DTYPE = {'dtype': torch.float32}


def set_compute_dtype(dtype):
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('compute dtype must be torch.float32 or torch.bfloat16')
    COMPUTE_DTYPE['dtype'] = dtype


def compute_dtype():
    return COMPUTE_DTYPE['dtype']


class VariableStore:
    def __init__(self, device='cuda', seed=0):
        self.device = torch.device(device)
        self.vars = OrderedDict()          # name -> nn.Parameter (f32)
        self.gen = torch.Generator().manual_seed(seed)
        self.flat = {}                     # prefix -> dict(param=, grad=, offsets={name:(off,numel)})
        self.state = OrderedDict()         # name -> non-trainable tensor (f32): in state_dict, never in trainable() / flat buffers
        self.effective = OrderedDict()     # name of a spectrally normalised weight -> its effective-weight leaf (W / sigma)
        self.rewritten = set()             # prefixes whose normalised raw weights changed since their last refresh

    # -- creation -----------------------------------------------------------------------------------
    def get(self, name, shape, init):
        p = self.vars.get(name)
        if p is not None:
            if tuple(p.shape) != tuple(shape):
                raise ValueError(f'variable {name} exists with shape {tuple(p.shape)}, requested {tuple(shape)}')
            return p
        if init == 'normal':
            t = torch.randn(tuple(shape), generator=self.gen, dtype=torch.float32)
        elif init == 'zeros':
            t = torch.zeros(tuple(shape), dtype=torch.float32)
        else:
            raise ValueError(init)
        p = torch.nn.Parameter(t.to(self.device))
        self.vars[name] = p
        return p

    def get_state(self, name, shape, init='normal'):
        """A persistent non-trainable variable (TF: trainable=False), e.g. spectral normalisation's `<scope>/u`."""
        t = self.state.get(name)
        if t is not None:
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f'state variable {name} exists with shape {tuple(t.shape)}, requested {tuple(shape)}')
            return t
        if init == 'normal':
            t = torch.randn(tuple(shape), generator=self.gen, dtype=torch.float32)
        elif init == 'zeros':
            t = torch.zeros(tuple(shape), dtype=torch.float32)
        else:
            raise ValueError(init)
        self.state[name] = t = t.to(self.device)
        return t

    # -- spectral normalisation -----------------------------------------------------------------------
    @staticmethod
    def u_name(weight_name):
        """`<weight's scope>/u`, the reference's name of the power-iteration state (networks/ops.py:83)."""
        return weight_name.rsplit('/', 1)[0] + '/u' if '/' in weight_name else 'u'

    def normalise(self, name):
        """Registers the weight `name` as spectrally normalised: creates its state u [1, cout] and its effective-weight leaf
        (a leaf tensor with requires_grad, shaped like the weight, that the networks convolve with; its values are W / sigma
        after functional.spectral_refresh_).  Must happen before the weight's network is flattened.  The leaf holds W / sigma
        only between a refresh and the next rewrite of the raw weights (StepGraph refreshes before every discriminator
        forward of a step); `effective_weight` is the checked way to read it.  Discriminator weights only: nothing refreshes
        any other network's."""
        eff = self.effective.get(name)
        if eff is not None:
            return eff
        if not name.startswith('discriminator/'):
            raise ValueError(f'spectral normalisation is offered for the discriminator only, got the weight {name!r}')
        p = self.vars[name]
        for prefix, flat in self.flat.items():
            if name in flat['offsets']:
                raise RuntimeError(f'{name} is already in the flat buffer of {prefix}: turn spectral normalisation on before the '
                                   f'step graph of this phase is built (networks.ops.set_spectral_norm)')
        self.get_state(self.u_name(name), [1, p.shape[-1]], 'normal')
        eff = self.effective[name] = torch.zeros_like(p.data).requires_grad_(True)
        return eff

    def effective_weight(self, name):
        """The effective-weight leaf of the normalised weight `name` for a forward pass: raises unless it holds W / sigma of
        the raw weights of the moment (it lives in the flat buffer and no rewrite is pending)."""
        eff = self.effective[name]
        prefix = name.split('/', 1)[0] + '/'
        flat = self.flat.get(prefix)
        if flat is None or flat.get('spectral') is None or name not in flat['normalised'] or prefix in self.rewritten:
            raise RuntimeError(f'the effective weight of {name} is not current: the raw weights were created or rewritten and not '
                               f'refreshed since (a training step refreshes; VariableStore.refresh_effective otherwise)')
        return eff

    def stand_in(self, name):
        """The leaf the networks read for variable `name`: the effective weight of a normalised one, else the parameter.  (For
        gradients and bookkeeping: no check that the leaf's values are current -- `effective_weight` has it.)"""
        eff = self.effective.get(name)
        return eff if eff is not None else self.vars[name]

    def grad_leaves(self, prefix=''):
        """Every leaf a backward Function may compute a gradient for under `prefix`: the parameters and the effective weights."""
        out = [v for k, v in self.vars.items() if k.startswith(prefix)]
        return out + [v for k, v in self.effective.items() if k.startswith(prefix)]

    def mark_rewritten(self, prefix=None):
        """The raw weights under `prefix` (None: everywhere) were rewritten: the next step refreshes their effective weights."""
        for k, flat in self.flat.items():
            if flat.get('spectral') is not None and (prefix is None or k == prefix):
                self.rewritten.add(k)

    def refresh_effective(self, prefix, iteration=1, force=False):
        """One power-iteration refresh of the effective weights under `prefix` if their raw weights were rewritten since the
        last one.  Plain launches on the current stream.  Returns whether it ran."""
        flat = self.flat.get(prefix)
        if flat is None or flat.get('spectral') is None or not (force or prefix in self.rewritten):
            return False
        from . import functional as F
        F.spectral_refresh_(flat['spectral'], flat['param'], flat['eff'], iteration)
        self.rewritten.discard(prefix)
        return True

    def names(self, prefix=''):
        return [k for k in self.vars if k.startswith(prefix)]

    def trainable(self, prefix=''):
        """tf.get_collection(tf.GraphKeys.TRAINABLE_VARIABLES, scope=prefix) in creation order."""
        return [(k, v) for k, v in self.vars.items() if k.startswith(prefix)]

    def count_parameters(self, prefix=''):
        return sum(v.numel() for k, v in self.vars.items() if k.startswith(prefix))

    # -- state dict (TF-name keyed) -----------------------------------------------------------------
    def state_dict(self):
        sd = OrderedDict((k, v.detach().clone()) for k, v in self.vars.items())
        sd.update((k, v.detach().clone()) for k, v in self.state.items())
        return sd

    def load_state_dict(self, sd, strict=False):
        missing = []
        for k, v in list(self.vars.items()) + list(self.state.items()):
            if k in sd:
                with torch.no_grad():
                    v.copy_(torch.as_tensor(sd[k]).to(v.device, torch.float32).reshape(v.shape))
            else:
                missing.append(k)      # (a state variable the checkpoint does not have keeps its fresh value)
        if strict and missing:
            raise KeyError(f'missing variables: {missing}')
        self.mark_rewritten()
        return missing

    def drop(self, names):
        for k in names:
            self.vars.pop(k, None)
            if self.effective.pop(k, None) is not None:
                self.state.pop(self.u_name(k), None)
        self.flat = {}
        self.rewritten = set()

    # -- flat buffers ---------------------------------------------------------------------------------
    def flatten(self, prefix, order=None):
        """Moves every variable under `prefix` into one flat f32 buffer (16-byte aligned segments, in
        `order`) and gives each a .grad view into a matching flat gradient buffer."""
        names = order if order is not None else self.names(prefix)
        offs, total = OrderedDict(), 0
        for k in names:
            n = self.vars[k].numel()
            offs[k] = (total, n)
            total += (n + 3) // 4 * 4
        flat_p = torch.zeros(total, device=self.device, dtype=torch.float32)
        flat_g = torch.zeros(total, device=self.device, dtype=torch.float32)
        for k in names:
            p = self.vars[k]
            o, n = offs[k]
            flat_p[o:o + n].copy_(p.data.reshape(-1))
            p.data = flat_p[o:o + n].view(p.shape)
            p.grad = flat_g[o:o + n].view(p.shape)
        self.flat[prefix] = dict(param=flat_p, grad=flat_g, offsets=offs, total=total)
        normalised = [k for k in names if k in self.effective]
        if normalised:
            self._flatten_effective(prefix, normalised)
        return self.flat[prefix]

    def _flatten_effective(self, prefix, names):
        """The flat effective-weight buffer of `prefix` (same offsets as the parameters; the leaves of `names` move into it) and
        the device table of its normalised segments, whose u buffer the state variables move into."""
        from . import functional as F
        flat = self.flat[prefix]
        order = sorted(names, key=lambda k: flat['offsets'][k][0])      # (the table sorts its segments by start)
        segs = []
        for k in order:
            shape = self.vars[k].shape
            segs.append((flat['offsets'][k][0], self.vars[k].numel() // shape[-1], shape[-1]))
        table = F.SpectralTable(segs, flat['total'], self.device)
        eff = torch.zeros(flat['total'], device=self.device, dtype=torch.float32)
        for s, k in enumerate(order):
            o, n = flat['offsets'][k]
            leaf = self.effective[k]
            eff[o:o + n].copy_(leaf.data.reshape(-1))
            leaf.data = eff[o:o + n].view(leaf.shape)
            u_view = table.views(s)[0]
            u_view.copy_(self.state[self.u_name(k)])
            self.state[self.u_name(k)] = u_view
        flat.update(eff=eff, spectral=table, normalised=order)
        self.rewritten.add(prefix)


@contextlib.contextmanager
def use_store(store):
    prev = _STATE['store']
    _STATE['store'] = store
    try:
        yield store
    finally:
        _STATE['store'] = prev


def current_store():
    if _STATE['store'] is None:
        raise RuntimeError('no active VariableStore: wrap network calls in `with use_store(store):`')
    return _STATE['store']


@contextlib.contextmanager
def variable_scope(name, reuse=None):
    """tf.variable_scope(name): nests by '/'.  `reuse` is accepted for signature parity; variables are
    always shared by name (the reference passes is_reuse=True for the 2nd..4th discriminator call)."""
    _STATE['scope'].append(name)
    try:
        yield
    finally:
        _STATE['scope'].pop()


def scope_name():
    return '/'.join(_STATE['scope'])


def get_variable(name, shape, initializer='normal'):
    full = (scope_name() + '/' + name) if _STATE['scope'] else name
    return current_store().get(full, shape, initializer)
