"""Who consumes the output of a masked data-gradient convolution (BackInfo).  Every autograd Function of the package counts itself
on its tensor inputs; only functional's convolutions ever register as pre-masking (functional._note_consumer)."""
import torch


class BackInfo:
    """ActInfo's bookkeeping (functional.py) one order up.  `t = M * conv(x)` (a data-gradient conv with a LeakyReLU mask in its
    epilogue, created while the gradient penalty's first backward builds its graph) has the backward gy -> M * gy, a full pass
    over the tensor.  Every Function that consumes `t` registers here (forward time); consumers that are able to return
    M * (their gradient) from their own kernel -- a conv's mask epilogue -- register as `premask`.  If all of them did,
    they do, and the producer skips its pass (decided at backward time, when all consumers are known).  Functions of this
    package are the only consumers of such tensors; all of them note themselves on their tensor inputs."""

    def __init__(self, bits, slope):
        self.bits, self.slope = bits, float(slope)
        self.n_consumers = 0
        self.n_premask = 0
        self._decision = None

    def all_premask(self):
        # decided once, by whoever asks first (a consumer's backward runs before the producer's): the backward itself
        # hands the tensor to further Functions (the weight gradient of the double backward), which must not change
        # what the consumers that already ran were told
        if self._decision is None:
            self._decision = self.n_consumers > 0 and self.n_consumers == self.n_premask
        return self._decision


def _note(t, premask):
    info = getattr(t, '_sg_back', None) if t is not None else None
    if info is not None and info._decision is None:
        info.n_consumers += 1
        if premask:
            info.n_premask += 1
    return info


def _note_all(*args):
    """A Function without a mask epilogue consuming the output of a masked conv: counted, never pre-masking."""
    for a in args:
        if isinstance(a, torch.Tensor):
            _note(a, False)
