"""The training step as a differentiable PyTorch op: the loss lives in the caller's code, the hot path stays in the library's kernels.

    render = DifferentiableRender(trainer)                       # a Trainer, FlexTrainer or BranchTrainer
    color_pred, alpha_pred = render(rays_o, rays_d, t, parameters, cone_scale)
    total = my_loss(color_pred, alpha_pred, ...) + 1e-3 * parameters.square().sum()
    total.backward()                                             # weight gradients in the trainer, parameters.grad from both terms
    trainer.apply_gradients()

Every gradient of a step is linear in dL/d color_pred and dL/d alpha_pred, so autograd only has to hand those two cotangents to
`Trainer.backward` (`ntx_train_backward`, include/nerftex.h): the weight gradient is left in the trainer as `gradients_step` leaves it
(`gradients()`, `sync_gradients`, `apply_gradients`), and -- with `param_gradients=True` / "only" on a layer-by-layer trainer and
`parameters.requires_grad` -- dL/d parameters flows on into `parameters.grad` [rows, P], where other torch terms on `parameters` add up.

One backward per forward (the activations are the trainer's, not the graph's), first order only: nothing differentiates the backward.  A
data-parallel mean of the ranks' gradients is the gradient of their joint loss only when that loss is a mean over rays.  A coarse + fine
pair is two passes with two sets of cotangents and is not taken."""

from __future__ import annotations

import functools


class DifferentiableRender:
    def __init__(self, trainer) -> None:
        from .train import CoarseFineTrainer
        if isinstance(trainer, CoarseFineTrainer):
            raise TypeError("DifferentiableRender takes one pass (Trainer, FlexTrainer, BranchTrainer), not a coarse + fine pair")
        self.trainer = trainer

    def __call__(self, rays_o, rays_d, t, parameters, cone_scale, **kw):
        """`Trainer.forward`'s arguments; returns (color_pred [N,3], alpha_pred [N]) in the autograd graph."""
        import torch
        tr = self.trainer
        wants = isinstance(parameters, torch.Tensor) and parameters.requires_grad
        if wants and not getattr(tr, "param_gradients", False):
            raise ValueError("parameters.requires_grad, but the trainer takes no parameter gradients (FlexTrainer / BranchTrainer with param_gradients=True or \"only\"); "
                             "detach them, or their gradient would silently lack the render's term")
        # the anchor makes the outputs require grad also when `parameters` does not: the backward has to run for the weights' sake
        anchor = torch.zeros((), device=torch.device("cuda", tr.device), requires_grad=True)
        return _render_function().apply(anchor, parameters if wants else None, tr, (rays_o, rays_d, t, parameters, cone_scale), kw)


@functools.lru_cache(maxsize=None)
def _render_function():
    """The torch.autograd.Function behind `DifferentiableRender` (made at the first call: importing the package does not import torch)."""
    import torch

    class Render(torch.autograd.Function):
        @staticmethod
        def forward(ctx, anchor, held, trainer, args, kw):
            rays_o, rays_d, t, parameters, cone_scale = args
            if isinstance(parameters, torch.Tensor):
                parameters = parameters.detach()
            color, alpha = trainer.forward(rays_o, rays_d, t, parameters, cone_scale, **kw)
            ctx.trainer, ctx.serial, ctx.like = trainer, trainer._pending[0], (None if held is None else (tuple(held.shape), held.device, held.dtype))
            return color, alpha

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, d_color, d_alpha):
            tr = ctx.trainer
            pending = tr._pending
            if pending is None or pending[0] != ctx.serial:
                raise RuntimeError("DifferentiableRender: one backward per forward -- this forward's step has been taken back already, or the trainer has "
                                   "run another step since (its activations are the trainer's, not the graph's)")
            tr.backward(d_color, d_alpha)
            grad = None
            if ctx.like is not None:
                rows = tr.parameter_gradients()                       # [rows the step read, P]; rows of `parameters` behind them were not read
                shape, device, dtype = ctx.like
                grad = torch.zeros(shape, device=rows.device, dtype=rows.dtype)
                grad.reshape(-1)[:rows.numel()].copy_(rows.reshape(-1))
                grad = grad.to(device=device, dtype=dtype)
            return None, grad, None, None, None

    return Render
