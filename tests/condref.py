"""Helpers shared by tests/test_cond_gpu.py and tests/test_cond_host.py: an fp64 torch-CPU restatement of the conditional 3-D pgan
 on top of the unconditional oracle (oracle/pgan_oracle.py) -- the two label ops with their adjoints, the
conditional generator and discriminator, the three loss builders and one optimisation step.  The penalty's double backward is
autograd's.  Nothing here touches the GPU.

Definition (the reference's surfgan conditioning, networks/surfgan/g_mapping.py:20-25 and networks/surfgan/discriminator.py:68-69, on
its pgan): with label rows c [N, L],
  G(z, c) = G_pgan(concat([z, c @ W], 1))   W = generator/conditioning/weight [L, latent_dim], no equalised-LR coefficient;
                                            generator_in/dense/weight is [2 latent_dim, .] (fan-in 2 latent_dim)
  D(x, c) = sum_l D_pgan(x)[:, l] * c[:, l] as [N, 1]   with discriminator_out/dense_2 [latent_dim, L] / [L]."""
import torch

from oracle import pgan_oracle as O

CONDITIONING_WEIGHT = 'generator/conditioning/weight'
DENSE_IN = 'generator/generator_in/dense/weight'
DENSE_2 = 'discriminator/discriminator_out/dense_2/'


# ---- the two ops ---------------------------------------------------------------------------------------------------------------
def embed(z, c, w):
    return torch.cat([z, c @ w], dim=1)


def embed_adjoint(g, c):
    """(dz, dW) of embed for the gradient g [N, 2 Z] of its output."""
    zdim = g.shape[1] // 2
    return g[:, :zdim], c.t() @ g[:, zdim:]


def project(o, c):
    return (o * c).sum(dim=1, keepdim=True)


def project_adjoint(g, c):
    """do of project for the gradient g [N, 1] of its output."""
    return g * c


# ---- variables -----------------------------------------------------------------------------------------------------------------
def variable_shapes(phase, base_shape, latent_dim, kernel_spec, filter_spec, label_dim):
    """The unconditional plan with the three changes, the embedding first (the generator creates it before generator_in)."""
    plain = O.variable_shapes(phase, base_shape, latent_dim, kernel_spec, filter_spec)
    out = {CONDITIONING_WEIGHT: (label_dim, latent_dim)}
    for k, shp in plain.items():
        if k == DENSE_IN:
            shp = (2 * latent_dim, shp[1])
        elif k == DENSE_2 + 'weight':
            shp = (latent_dim, label_dim)
        elif k == DENSE_2 + 'bias':
            shp = (label_dim,)
        out[k] = tuple(shp)
    return out


def init_params(phase, base_shape, latent_dim, kernel_spec, filter_spec, label_dim, seed=0, bias_std=0.1):
    gen = torch.Generator().manual_seed(seed)
    p = {}
    for name, shape in variable_shapes(phase, base_shape, latent_dim, kernel_spec, filter_spec, label_dim).items():
        t = torch.randn(shape, generator=gen, dtype=torch.float64)
        p[name] = t if name.endswith('weight') else t * bias_std
    return p


# ---- networks ------------------------------------------------------------------------------------------------------------------
def generator(p, z, c, alpha, phase, base_shape, activation, kernel_spec, filter_spec, param=None):
    return O.generator(p, embed(z, c, p[CONDITIONING_WEIGHT]), alpha, phase, base_shape, activation, kernel_spec, filter_spec,
                       param=param)


def discriminator(p, x, c, alpha, phase, latent_dim, activation, kernel_spec, filter_spec, param=None):
    return project(O.discriminator(p, x, alpha, phase, latent_dim, activation, kernel_spec, filter_spec, param=param), c)


# ---- networks/loss.py with the same label rows in every pass -------------------------------------------------------------------
def _nets(p, c, alpha, cfg):
    net = dict(phase=cfg['phase'], activation=cfg['activation'], kernel_spec=cfg['kernel_spec'], filter_spec=cfg['filter_spec'],
               param=cfg['leakiness'])
    return (lambda z: generator(p, z, c, alpha, base_shape=cfg['base_shape'], **net),
            lambda x: discriminator(p, x, c, alpha, latent_dim=cfg['latent_dim'], **net))


def _penalty(D, interpolates, axes):
    d_int = D(interpolates)
    (gradients,) = torch.autograd.grad(d_int.sum(), interpolates, create_graph=True)
    return torch.sqrt(torch.sum(gradients * gradients, dim=axes))


def forward_simultaneous(p, real, c, rnd, alpha, cfg):
    """networks/loss.py:101-165 (quirk Q1: the slopes keep the W axis)."""
    G, D = _nets(p, c, alpha, cfg)
    gen_sample = G(rnd['z'])
    real_n = real + rnd['noise_real'] * cfg['noise_stddev']
    fake_n = gen_sample + rnd['noise_fake'] * cfg['noise_stddev']
    disc_fake_d = D(fake_n.detach())
    disc_real = D(real_n)
    interpolates = (rnd['gamma'] * real_n + (1 - rnd['gamma']) * fake_n.detach()).requires_grad_(True)
    slopes = _penalty(D, interpolates, (1, 2, 3))
    disc_fake_g = D(fake_n)
    if cfg['loss_fn'] == 'wgan':
        gp_loss = cfg['gp_weight'] * (slopes - 1) ** 2
        disc_loss = torch.mean((disc_fake_d - disc_real) + gp_loss + 1e-3 * disc_real ** 2)
        gen_loss = -torch.mean(disc_fake_g)
    else:
        gp_loss = cfg['gp_weight'] * torch.mean(slopes ** 2)
        disc_loss = torch.mean(O._softplus(disc_fake_d)) + torch.mean(O._softplus(-disc_real)) + gp_loss
        gen_loss = torch.mean(O._softplus(-disc_fake_g))
    return gen_loss, disc_loss, gp_loss, gen_sample


def forward_discriminator(p, real, c, rnd, alpha, cfg):
    """networks/loss.py:42-98 (the penalty over all of (c, d, h, w))."""
    G, D = _nets(p, c, alpha, cfg)
    gen_sample = G(rnd['z'])
    real_n = real + rnd['noise_real'] * cfg['noise_stddev']
    fake_n = gen_sample + rnd['noise_fake'] * cfg['noise_stddev']
    disc_fake_d = D(fake_n.detach())
    disc_real = D(real_n)
    interpolates = (rnd['gamma'] * real_n + (1 - rnd['gamma']) * fake_n.detach()).requires_grad_(True)
    slopes = _penalty(D, interpolates, (1, 2, 3, 4))
    if cfg['loss_fn'] == 'wgan':
        gp_loss = cfg['gp_weight'] * (slopes - 1) ** 2
        disc_loss = torch.mean((disc_fake_d - disc_real) + gp_loss + 1e-3 * disc_real ** 2)
    else:
        gp_loss = cfg['gp_weight'] * torch.mean(slopes ** 2)
        disc_loss = torch.mean(O._softplus(disc_fake_d)) + torch.mean(O._softplus(-disc_real)) + gp_loss
    return disc_loss, gp_loss


def forward_generator(p, real, c, rnd, alpha, cfg):
    """networks/loss.py:4-39."""
    G, D = _nets(p, c, alpha, cfg)
    gen_sample = G(rnd['z'])
    disc_fake_g = D(gen_sample + rnd['noise_fake'] * cfg['noise_stddev'])
    gen_loss = -torch.mean(disc_fake_g) if cfg['loss_fn'] == 'wgan' else torch.mean(O._softplus(-disc_fake_g))
    return gen_sample, gen_loss


def _leaves(p):
    return {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}


def step(p, c, rnd, real, alpha, cfg, strategy='simultaneous', lr=1e-3):
    """One optimisation step of every variable (TF-Adam beta1 0, beta2 0.9, as tests/test_step_gpu.py builds it); `p` is updated in
    place.  simultaneous: both gradients at the pre-step weights; alternate: the generator's on the updated discriminator."""
    gnames, dnames = O.split_vars(p)
    adam_g, adam_d = O.TFAdam(0.0, 0.9), O.TFAdam(0.0, 0.9)
    if strategy == 'simultaneous':
        w = _leaves(p)
        gen_loss, disc_loss, gp_loss, gen_sample = forward_simultaneous(w, real, c, rnd, alpha, cfg)
        gg = torch.autograd.grad(gen_loss, [w[k] for k in gnames], retain_graph=True)
        dg = torch.autograd.grad(disc_loss, [w[k] for k in dnames])
    else:
        w = _leaves(p)
        disc_loss, gp_loss = forward_discriminator(w, real, c, rnd, alpha, cfg)
        dg = torch.autograd.grad(disc_loss, [w[k] for k in dnames])
        adam_d.apply(p, dict(zip(dnames, [g.detach() for g in dg])), lr)
        w = _leaves(p)
        gen_sample, gen_loss = forward_generator(w, real, c, rnd, alpha, cfg)
        gg = torch.autograd.grad(gen_loss, [w[k] for k in gnames])
    g_grads = dict(zip(gnames, [g.detach() for g in gg]))
    d_grads = dict(zip(dnames, [g.detach() for g in dg]))
    adam_g.apply(p, g_grads, lr)
    if strategy == 'simultaneous':
        adam_d.apply(p, d_grads, lr)
    return dict(gen_loss=gen_loss.detach(), disc_loss=disc_loss.detach(), gp_loss=gp_loss.detach(), gen_sample=gen_sample.detach(),
                g_grads=g_grads, d_grads=d_grads)
