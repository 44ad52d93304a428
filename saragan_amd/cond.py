"""Label conditioning: the generator's embedding concatenated to the latents, the discriminator's label-weighted
sum of its outputs.  Both are linear in everything that carries a gradient; the labels themselves are data.  Re-exported by
functional."""
import torch

from . import _lib
from ._consumers import _note_all
from ._grad_dest import _f32_out, _wants
from ._launch import _dt, _ptr, _req_cuda, _stream
from ._lib import check


def _labels(c, n):
    if c.dim() != 2 or c.shape[0] != n or not c.is_floating_point():
        raise ValueError(f'conditioning: expected a floating [N, L] tensor with N = {n}, got {c.dtype} {tuple(c.shape)}')
    return c.detach().contiguous().float()


class _CondEmbed(torch.autograd.Function):
    """out = concat([z, c @ W], 1) (sg_cond_embed): z [N, Z], c f32 [N, L], W f32 [L, Z] (a raw variable: no coefficient).  The
    backward (the same entry point, adjoint = 1) writes dW straight into its slot of the flat gradient buffer (grads_into) and
    honours skip_param_grads; nothing differentiates the generator's backward."""

    @staticmethod
    def forward(ctx, z, c, W):
        _note_all(z)
        lib = _lib.load()
        _req_cuda(z, c, W)
        n, zdim = z.shape
        c = _labels(c, n)
        if W.dim() != 2 or W.shape != (c.shape[1], zdim) or W.dtype != torch.float32:
            raise ValueError(f'cond_embed: expected an f32 [{c.shape[1]}, {zdim}] embedding, got {W.dtype} {tuple(W.shape)}')
        z = z.contiguous()
        out = torch.empty((n, 2 * zdim), device=z.device, dtype=z.dtype)
        check(lib.sg_cond_embed(_ptr(z), _ptr(c), _ptr(W.detach().contiguous()), _ptr(out), n, zdim, c.shape[1], 0, _dt(z),
                                _stream()), 'sg_cond_embed')
        ctx.save_for_backward(c)
        ctx.w_ptr, ctx.w_shape = W.data_ptr(), tuple(W.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        lib = _lib.load()
        (c,) = ctx.saved_tensors
        want_z, want_w = ctx.needs_input_grad[0], _wants(ctx, 2, ctx.w_ptr)
        if not (want_z or want_w):
            return None, None, None
        g = g.contiguous()
        n, zdim = g.shape[0], g.shape[1] // 2
        dz = torch.empty((n, zdim), device=g.device, dtype=g.dtype) if want_z else None
        dW = _f32_out(ctx.w_ptr, ctx.w_shape, g.device) if want_w else None
        check(lib.sg_cond_embed(_ptr(dz), _ptr(c), _ptr(dW), _ptr(g), n, zdim, c.shape[1], 1, _dt(g), _stream()),
              'sg_cond_embed')
        return dz, None, dW


class _CondProject(torch.autograd.Function):
    """adjoint False: out[n, 0] = sum_l o[n, l] * c[n, l]; adjoint True: out[n, l] = o[n, 0] * c[n, l] (sg_cond_project).  The two
    are each other's backward, so the pair is differentiable to any order (the gradient penalty differentiates D's backward)."""

    @staticmethod
    def forward(ctx, o, c, adjoint):
        _note_all(o)
        lib = _lib.load()
        _req_cuda(o, c)
        c = _labels(c, o.shape[0])
        n, l = c.shape
        if o.dim() != 2 or o.shape[1] != (1 if adjoint else l):
            raise ValueError(f'cond_project: labels {tuple(c.shape)} do not fit the tensor {tuple(o.shape)}')
        o = o.contiguous()
        out = torch.empty((n, l if adjoint else 1), device=o.device, dtype=o.dtype)
        check(lib.sg_cond_project(_ptr(o), _ptr(c), _ptr(out), n, l, 1 if adjoint else 0, _dt(o), _stream()), 'sg_cond_project')
        ctx.save_for_backward(c)
        ctx.adjoint = adjoint
        return out

    @staticmethod
    def backward(ctx, g):
        (c,) = ctx.saved_tensors
        return _CondProject.apply(g, c, not ctx.adjoint), None, None


def cond_embed(z, c, W):
    """concat([z, c @ W], axis=1) for latents z [N, Z], labels c [N, L] and the embedding W [L, Z] (SURFGAN_3D's
    networks/surfgan/g_mapping.py:20-25): [N, 2 Z] of z's type, the product summed in f32."""
    return _CondEmbed.apply(z, c, W)


def cond_project(o, c):
    """sum_l o[n, l] * c[n, l] as [N, 1] (networks/surfgan/discriminator.py:69) of o's type, summed in f32.  Twice differentiable
    (and further) for o."""
    return _CondProject.apply(o, c, False)
