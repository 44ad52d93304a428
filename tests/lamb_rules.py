"""The LAMB and AdamW rules in fp64 (torch, CPU), written from their statement -- per variable w, gradient g, moments m, v, t
counting applied updates from 1:

    m = b1*m + (1-b1)*g          v = b2*v + (1-b2)*g^2
    AdamW   u = m / (sqrt(v) + eps) + lam*w                               w -= lr*u
    LAMB    u = (m/(1-b1^t)) / (sqrt(v/(1-b2^t)) + eps) + lam*w           w -= lr*r*u
            r = |w| / |u| if |w| > 0 and |u| > 0 else 1     (2-norms over the whole variable, of w before the update)

lam is the decay rate, 0 for variables whose name contains `bias`; eps 1e-6.  The classes have the oracle optimisers'
`apply(params, grads, lr)` protocol (oracle.pgan_oracle.TFAdam), so step_simultaneous / step_alternate take them as they are.
f32_error (None, +1 or -1): the rule reads the gradient as an f32 computation would hand it over -- rounded to f32, then moved
by f32_error * 2^-24 * max|g| of its variable.  A gradient element is a sum of N terms of either sign; where they have size s the
sum has size about sqrt(N) s and f32 adds it with an error of about sqrt(N) s 2^-24, so the error goes with the size of the
variable's gradient elements, whatever an element's own value, and the largest element stands for that size.  The distance
between the exact run and the two moved runs measures how far f32 gradients alone move the result."""
import torch


def decays(name):
    return 'bias' not in name


def trust_ratio(w, u):
    wn, un = torch.linalg.vector_norm(w), torch.linalg.vector_norm(u)
    return float(wn / un) if float(wn) > 0.0 and float(un) > 0.0 else 1.0


class _Moments:
    def __init__(self, beta1=0.9, beta2=0.999, weight_decay_rate=0.0, epsilon=1e-6, f32_error=None):
        self.b1, self.b2, self.decay, self.eps, self.f32_error = beta1, beta2, weight_decay_rate, epsilon, f32_error
        self.t = 0
        self.m, self.v = {}, {}
        self.ratios = {}

    def _moments(self, name, w, g):
        if self.f32_error is not None:
            g = g.float().double() + self.f32_error * 2.0 ** -24 * g.abs().max()
        if name not in self.m:
            self.m[name], self.v[name] = torch.zeros_like(w), torch.zeros_like(w)
        self.m[name] = self.b1 * self.m[name] + (1 - self.b1) * g
        self.v[name] = self.b2 * self.v[name] + (1 - self.b2) * g * g
        return self.m[name], self.v[name], (self.decay if decays(name) else 0.0)


class AdamWRule(_Moments):
    def apply(self, params, grads, lr):
        self.t += 1
        for name, g in grads.items():
            w = params[name]
            m, v, lam = self._moments(name, w, g)
            params[name] = w - lr * (m / (torch.sqrt(v) + self.eps) + lam * w)


class LAMBRule(_Moments):
    def apply(self, params, grads, lr):
        self.t += 1
        for name, g in grads.items():
            w = params[name]
            m, v, lam = self._moments(name, w, g)
            u = (m / (1 - self.b1 ** self.t)) / (torch.sqrt(v / (1 - self.b2 ** self.t)) + self.eps) + lam * w
            r = self.ratios[name] = trust_ratio(w, u)
            params[name] = w - lr * r * u


RULES = {'LAMB': LAMBRule, 'AdamW': AdamWRule}
