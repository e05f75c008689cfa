"""The training step as a differentiable PyTorch op: the loss lives in the caller's code, the hot path stays in the library's kernels.

    render = DifferentiableRender(trainer)                       # a Trainer, FlexTrainer or BranchTrainer
    color_pred, alpha_pred = render(rays_o, rays_d, t, parameters, cone_scale)
    total = my_loss(color_pred, alpha_pred, ...) + 1e-3 * parameters.square().sum()
    total.backward()                                             # weight gradients in the trainer, parameters.grad from both terms
    trainer.apply_gradients()

Every gradient of a step is linear in dL/d color_pred and dL/d alpha_pred, so autograd only has to hand those two cotangents to
`Trainer.backward` (`ntx_train_backward`, include/nerftex.h): the weight gradient is left in the trainer as `gradients_step` leaves it
(`gradients()`, `sync_gradients`, `apply_gradients`), and -- with `param_gradients=True` / "only" on the trainer (a layer-by-layer one, or the fused
chain: `Trainer(..., param_gradients=)`) and `parameters.requires_grad` -- dL/d parameters flows on into `parameters.grad` [rows, P], where other torch terms on `parameters` add up.

With `input_gradients=True` / "only" on the trainer (either kind), `rays_o` / `rays_d` that require grad receive dL/d rays_o and dL/d rays_d
likewise (camera or pose refinement: the sample depths are constants), and the instanced op's `pts` / `rays_d_map` theirs; with it off, both ops
do what they do without it.

A loss that looks along the ray takes the compositing weights as a third differentiable output -- `DifferentiableRender(trainer,
weights=True)` returns (color_pred, alpha_pred, weights [N, S]), and their cotangent reaches the composite's adjoint through
`Trainer.backward(..., d_weights=)` (`ntx_trainer_weight_cotangent`):

    color_pred, alpha_pred, weights = DifferentiableRender(trainer, weights=True)(rays_o, rays_d, t, parameters, cone_scale, z_vals=z)
    (mse(color_pred, color) + 0.1 * mse(nerf_tex_amd.loss.expected_depth(weights, z), depth)).backward()

One backward per forward (the activations are the trainer's, not the graph's), first order only: nothing differentiates the backward.  A
data-parallel mean of the ranks' gradients is the gradient of their joint loss only when that loss is a mean over rays.  A coarse + fine
pair is two passes with two sets of cotangents and is not taken.

`DifferentiableInstanceRender` is the same op on the instanced render (InstanceRenderer's tail on an instancer's buffers), with the per-sample
parameter field `params_map` [N, S, P] in the place of `parameters`."""

from __future__ import annotations

import functools


class DifferentiableRender:
    def __init__(self, trainer, weights: bool = False) -> None:
        from .train import CoarseFineTrainer
        if isinstance(trainer, CoarseFineTrainer):
            raise TypeError("DifferentiableRender takes one pass (Trainer, FlexTrainer, BranchTrainer), not a coarse + fine pair")
        self.trainer, self.weights = trainer, bool(weights)

    def __call__(self, rays_o, rays_d, t, parameters, cone_scale, **kw):
        """`Trainer.forward`'s arguments; returns (color_pred [N,3], alpha_pred [N]) in the autograd graph -- with `weights=True` (color_pred,
        alpha_pred, weights [N,S])."""
        import torch
        tr = self.trainer
        wants = isinstance(parameters, torch.Tensor) and parameters.requires_grad
        if wants and not getattr(tr, "param_gradients", False):
            raise ValueError("parameters.requires_grad, but the trainer takes no parameter gradients (FlexTrainer / BranchTrainer with param_gradients=True or \"only\"); "
                             "detach them, or their gradient would silently lack the render's term")
        # the anchor makes the outputs require grad also when `parameters` does not: the backward has to run for the weights' sake
        anchor = torch.zeros((), device=torch.device("cuda", tr.device), requires_grad=True)
        # inputs that take a gradient reach the function as direct arguments: autograd does not look inside the tuple
        ins = [a if getattr(tr, "input_gradients", False) and isinstance(a, torch.Tensor) and a.requires_grad else None for a in (rays_o, rays_d)]
        return _render_function().apply(anchor, parameters if wants else None, ins[0], ins[1], tr, (rays_o, rays_d, t, parameters, cone_scale),
                                        dict(kw, return_weights=True) if self.weights else kw)


class DifferentiableInstanceRender:
    """The same op on the INSTANCED render (`Trainer.forward_instanced`, `ntx_train_forward_instanced`): fine-tune a network in the scene
    it is rendered in, or fit a parameter field to an image of the furred object.

        render = DifferentiableInstanceRender(trainer, patch_scale=0.09, density_scale=400.)   # a FlexTrainer or BranchTrainer, or Trainer(..., instanced=True)
        color_pred, alpha_pred = render(bufs, cone_scale, params_map=field)                    # bufs: the instancer's ten-tuple
        (my_loss(color_pred, alpha_pred) + 1e-3 * field.square().sum()).backward()             # field.grad [N,S,P] from both terms

    `params_map` (default: the tuple's) that requires grad receives the per-sample gradient (zero outside every patch); that needs
    `param_gradients` on.  The weight gradient stays in the trainer.  One backward per forward, as `DifferentiableRender`."""

    def __init__(self, trainer, patch_scale: float, density_scale: float = 1.0, density_reweighting: bool = True, weights: bool = False) -> None:
        if not hasattr(trainer, "forward_instanced"):
            raise TypeError("DifferentiableInstanceRender takes one pass (FlexTrainer, BranchTrainer, or Trainer with instanced=True), not a coarse + fine pair")
        self.trainer = trainer
        self.opts = dict(patch_scale=float(patch_scale), density_scale=float(density_scale), density_reweighting=bool(density_reweighting))
        if weights:                                                  # the third output: weights [N,S], 0 outside every patch (the appended sample's is not among them)
            self.opts["return_weights"] = True

    def __call__(self, bufs, cone_scale, params_map=None, **kw):
        """`Trainer.forward_instanced`'s arguments (composite_bkgd, bkgd_color, hit in `kw`); returns (color_pred [N,3], alpha_pred [N]) in
        the autograd graph."""
        import torch
        tr = self.trainer
        bufs = tuple(bufs)
        if params_map is None:
            params_map = bufs[9]
        wants = isinstance(params_map, torch.Tensor) and params_map.requires_grad
        if wants and not getattr(tr, "param_gradients", False):
            raise ValueError("params_map.requires_grad, but the trainer takes no parameter gradients (a trainer with param_gradients=True or \"only\"); "
                             "detach it, or its gradient would silently lack the render's term")
        anchor = torch.zeros((), device=torch.device("cuda", tr.device), requires_grad=True)
        ins = [a if getattr(tr, "input_gradients", False) and isinstance(a, torch.Tensor) and a.requires_grad else None for a in (bufs[1], bufs[0])]   # pts, rays_d_map
        return _render_function().apply(anchor, params_map if wants else None, ins[0], ins[1], tr, ("instanced", bufs[:9] + (params_map,), cone_scale),
                                        dict(self.opts, **kw))


def __getattr__(name):
    """`nerf_tex_amd.autograd.PosedRays` / `RayDistortion` / `RayInterlevel`: the torch.autograd.Functions of `ray_sampler.posed_rays`,
    `loss.distortion` and `loss.interlevel`, made at their first use."""
    if name == "PosedRays":
        return _posed_rays_function()
    if name == "RayDistortion":
        return _ray_distortion_function()
    if name == "RayInterlevel":
        return _ray_interlevel_function()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


@functools.lru_cache(maxsize=None)
def _posed_rays_function():
    """The torch.autograd.Function in front of the render op when the CAMERAS are the unknowns: rays from device poses
    (`ntx_generate_rays_posed`) forward, `ntx_generate_rays_posed_adjoint` backward.

        rays_o, rays_d, t, cone_scale = PosedRays.apply(poses [B,3,4], focal [B], image_plane_loc [N,2], rays_per_pose, consts)

    with consts = (height, width, mode, b_0, b_1, near, far) (`ray_sampler.posed_rays` builds them).  All tensors float32, contiguous, on one
    GPU; both launches go to the current stream.  `poses` and `focal` receive gradients when they require them; t and cone_scale are marked
    non-differentiable (the depths and the cone take no gradient anywhere in the step: include/nerftex.h).  First order only."""
    import torch
    from . import _lib

    class PosedRays(torch.autograd.Function):
        @staticmethod
        def forward(ctx, poses, focal, loc, rays_per_pose, consts):
            height, width, mode, b0, b1, near, far = consts
            n, dev = int(loc.shape[0]), poses.device
            poses, focal = poses.detach(), focal.detach()
            rays_o, rays_d = torch.empty((n, 3), device=dev, dtype=torch.float32), torch.empty((n, 3), device=dev, dtype=torch.float32)
            t, cone = torch.empty((n, 2), device=dev, dtype=torch.float32), torch.empty((n, 1), device=dev, dtype=torch.float32)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib.ntx_generate_rays_posed(poses.data_ptr(), focal.data_ptr(), int(poses.shape[0]), height, width, loc.data_ptr(), n, int(rays_per_pose), mode,
                                                            _lib.f3(b0) if b0 is not None else None, _lib.f3(b1) if b1 is not None else None, near, far,
                                                            rays_o.data_ptr(), rays_d.data_ptr(), t.data_ptr(), cone.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
            ctx.save_for_backward(poses, focal, loc)
            ctx.call = (height, width, int(rays_per_pose), mode)
            ctx.mark_non_differentiable(t, cone)
            return rays_o, rays_d, t, cone

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, d_rays_o, d_rays_d, _d_t, _d_cone):
            poses, focal, loc = ctx.saved_tensors
            height, width, rays_per_pose, mode = ctx.call
            n, dev = int(loc.shape[0]), poses.device
            d_rays_o, d_rays_d = d_rays_o.to(torch.float32).contiguous(), d_rays_d.to(torch.float32).contiguous()
            d_poses, d_focal = torch.empty_like(poses), torch.empty_like(focal)
            with torch.cuda.device(dev):
                _lib.check(_lib.lib.ntx_generate_rays_posed_adjoint(poses.data_ptr(), focal.data_ptr(), int(poses.shape[0]), height, width, loc.data_ptr(), n, rays_per_pose, mode,
                                                                    d_rays_o.data_ptr(), d_rays_d.data_ptr(), d_poses.data_ptr(), d_focal.data_ptr(),
                                                                    torch.cuda.current_stream(dev).cuda_stream))
            return (d_poses if ctx.needs_input_grad[0] else None), (d_focal if ctx.needs_input_grad[1] else None), None, None, None

    return PosedRays


@functools.lru_cache(maxsize=None)
def _ray_distortion_function():
    """The torch.autograd.Function behind `loss.distortion`: `ntx_ray_distortion` once in the forward -- one launch writes the per-ray values
    and their gradient at the weights, which is saved -- and `grad_out[:, None] * saved` in the backward.

        per_ray = RayDistortion.apply(weights [N,S], z_vals [N,S], widths or None, live or None, ray_scale or None)

    Differentiable in `weights` alone (the depths, widths and factors are constants).  First order only: a double backward raises."""
    import torch
    from . import loss as _loss

    class RayDistortion(torch.autograd.Function):
        @staticmethod
        def forward(ctx, weights, z_vals, widths, live, ray_scale):
            val, grad = _loss.ray_distortion(weights, z_vals, widths, live, ray_scale, with_grad=True)
            ctx.save_for_backward(grad)
            ctx.like = weights.dtype
            return val

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, d_val):
            (grad,) = ctx.saved_tensors
            return (d_val.to(grad.dtype)[:, None] * grad).to(ctx.like), None, None, None, None

    return RayDistortion


@functools.lru_cache(maxsize=None)
def _ray_interlevel_function():
    """The torch.autograd.Function behind `loss.interlevel`: `ntx_ray_interlevel` once in the forward -- one launch writes the per-ray values
    and their gradients at both sets of weights, which are saved -- and `grad_out[:, None] * saved` in the backward, for whichever of the two
    requires grad.

        per_ray = RayInterlevel.apply(weights [N,S], z_vals [N,S], weights_prop [N,S_p], z_prop [N,S_p], ray_scale or None, eps)

    Differentiable in `weights_prop` and `weights` (the depths and factors are constants).  First order only: a double backward raises."""
    import torch
    from . import loss as _loss

    class RayInterlevel(torch.autograd.Function):
        @staticmethod
        def forward(ctx, weights, z_vals, weights_prop, z_prop, ray_scale, eps):
            val, grad_prop, grad_fine = _loss.ray_interlevel(weights, z_vals, weights_prop, z_prop, ray_scale, eps, with_grad=True)
            ctx.save_for_backward(grad_prop, grad_fine)
            ctx.like = (weights.dtype, weights_prop.dtype)
            return val

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, d_val):
            grad_prop, grad_fine = ctx.saved_tensors
            d = d_val.to(grad_prop.dtype)[:, None]
            d_fine = (d * grad_fine).to(ctx.like[0]) if ctx.needs_input_grad[0] else None
            d_prop = (d * grad_prop).to(ctx.like[1]) if ctx.needs_input_grad[2] else None
            return d_fine, None, d_prop, None, None, None

    return RayInterlevel


@functools.lru_cache(maxsize=None)
def _render_function():
    """The torch.autograd.Function behind `DifferentiableRender` (made at the first call: importing the package does not import torch)."""
    import torch

    class Render(torch.autograd.Function):
        @staticmethod
        def forward(ctx, anchor, held, in_a, in_b, trainer, args, kw):
            ctx.instanced = len(args) == 3 and isinstance(args[0], str)
            if ctx.instanced:                                        # ("instanced", the instancer's ten buffers, cone_scale)
                _, bufs, cone_scale = args
                bufs = tuple(b.detach() if isinstance(b, torch.Tensor) else b for b in bufs)
                outs = trainer.forward_instanced(bufs, cone_scale, **kw)
            else:
                rays_o, rays_d, t, parameters, cone_scale = (a.detach() if isinstance(a, torch.Tensor) else a for a in args)
                outs = trainer.forward(rays_o, rays_d, t, parameters, cone_scale, **kw)
            like = lambda x: None if x is None else (tuple(x.shape), x.device, x.dtype)
            ctx.trainer, ctx.serial, ctx.like, ctx.like_in = trainer, trainer._pending[0], like(held), (like(in_a), like(in_b))
            if len(outs) == 3:                                       # with the weights: an output the loss does not use hands back None, not zeros
                ctx.set_materialize_grads(False)
                ctx.color_like = like(outs[0])
            return outs

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, d_color, d_alpha, d_weights=None):
            tr = ctx.trainer
            pending = tr._pending
            if pending is None or pending[0] != ctx.serial:
                raise RuntimeError("DifferentiableRender: one backward per forward -- this forward's step has been taken back already, or the trainer has "
                                   "run another step since (its activations are the trainer's, not the graph's)")
            if d_color is None:                                      # (only where the weights are an output: a loss of alpha_pred / the weights alone)
                d_color = torch.zeros(ctx.color_like[0], device=ctx.color_like[1], dtype=ctx.color_like[2])
            tr.backward(d_color, d_alpha) if d_weights is None else tr.backward(d_color, d_alpha, d_weights)
            grad = None
            if ctx.like is not None and ctx.instanced:
                shape, device, dtype = ctx.like
                grad = tr.sample_parameter_gradients().reshape(shape).to(device=device, dtype=dtype)   # [N, S, P], zero outside every patch
            elif ctx.like is not None:
                rows = tr.parameter_gradients()                      # [rows the step read, P]; rows of `parameters` behind them were not read
                shape, device, dtype = ctx.like
                grad = torch.zeros(shape, device=rows.device, dtype=rows.dtype)
                grad.reshape(-1)[:rows.numel()].copy_(rows.reshape(-1))
                grad = grad.to(device=device, dtype=dtype)
            ins = [None, None]
            if any(l is not None for l in ctx.like_in):              # (rays_o, rays_d) of a plain step, (pts, rays_d_map) of an instanced one
                got = tr.sample_input_gradients() if ctx.instanced else tr.ray_gradients()
                ins = [None if l is None else g.reshape(l[0]).to(device=l[1], dtype=l[2]) for g, l in zip(got, ctx.like_in)]
            return None, grad, ins[0], ins[1], None, None, None

    return Render
