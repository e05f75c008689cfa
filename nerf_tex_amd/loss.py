"""network/loss.py of the reference, as descriptions the training step evaluates on the GPU (`ntx_train_step_gradients`, include/nerftex.h).

Same names, same constructor keywords: a training config's `loss_config` ({'module': 'network.loss.AlphaLoss', 'loss_fn':
'network.loss.smape', 'alpha_loss_fn': 'network.loss.mse'}, configs/config_carpet_train.py:95-99) instantiates these through
`util.remap_reference_config`.  A loss object is not called on tensors here -- value and gradient come out of the fused step -- it carries
`desc()`, the `ntx_loss_desc` of its settings.

Any OTHER loss is written in PyTorch: `Trainer.gradients_step`, `Train` and `ParameterFitter.fit` take an object without `desc()` as a callable
`loss(color_true=, alpha_true=, color_pred=, alpha_pred=) -> scalar tensor` (the reference's call, loss.py:12, 30; a `loss_config` names its
class by module path) and run the step as `ntx_train_forward`, the loss and its two cotangents in torch, `ntx_train_backward`
(`nerf_tex_amd.autograd` is the same as a differentiable op).  A callable whose signature also names `weights` (and `z_vals`) is a loss ALONG
the ray: it receives the compositing weights [N, S] (and the step's depths) and its gradient at the weights goes back through
`ntx_trainer_weight_cotangent`; `expected_depth` below is the helper such a loss starts from, and `Distortion` wraps any loss with the
distortion regulariser of mip-NeRF 360 on those weights (`ntx_ray_distortion`: the formula is stated at the entry in include/nerftex.h).
`ray_interlevel` / `interlevel` are the same paper's interlevel loss between the weights of two passes (`ntx_ray_interlevel`, stated at its
entry too): the loss `train.ProposalTrainer` trains a sampler's network with; `Interlevel` is the config key that asks for it."""

from __future__ import annotations

import ctypes as C

from . import _lib

_FNS = {"mse": _lib.LOSS_MSE, "smape": _lib.LOSS_SMAPE}


def _fn(path: str) -> int:
    name = path.rsplit(".", 1)[-1]
    if name not in _FNS:
        raise _lib.NtxError(_lib.NTX_E_UNSUPPORTED, f"loss function {path!r}: mse and smape (loss.py:51-59) are built")
    return _FNS[name]


def mse(*_a, **_k):
    """network.loss.mse (loss.py:51-54): evaluated inside the training step; here only a name to point a config at."""
    raise TypeError("nerf_tex_amd.loss.mse is evaluated inside ntx_train_step_gradients")


def smape(*_a, **_k):
    """network.loss.smape (loss.py:56-59)."""
    raise TypeError("nerf_tex_amd.loss.smape is evaluated inside ntx_train_step_gradients")


class NerfLoss:
    """network.loss.NerfLoss (loss.py:6-19): loss_fn(color_true, color_pred)."""

    def __init__(self, loss_fn: str = "network.loss.mse") -> None:
        self.kind, self.loss_fn, self.alpha_loss_fn = _lib.LOSS_NERF, _fn(loss_fn), _fn(loss_fn)
        self.gamma, self.filter_color_loss, self.use_hard_mask = 1.0, False, False

    def desc(self) -> "_lib.LossDesc":
        return _lib.LossDesc(C.sizeof(_lib.LossDesc), self.kind, self.loss_fn, self.alpha_loss_fn, float(self.gamma), int(self.filter_color_loss), int(self.use_hard_mask))


class AlphaLoss(NerfLoss):
    """network.loss.AlphaLoss (loss.py:21-49): colours masked by alpha_true (hard: alpha_true > 0), + gamma * alpha_loss_fn(alpha_true, alpha_pred)."""

    def __init__(self, loss_fn: str = "network.loss.mse", alpha_loss_fn: str = None, gamma: float = 1, filter_color_loss: bool = True,
                 use_hard_mask: bool = True) -> None:
        self.kind, self.loss_fn = _lib.LOSS_ALPHA, _fn(loss_fn)
        self.alpha_loss_fn = self.loss_fn if alpha_loss_fn is None else _fn(alpha_loss_fn)
        self.gamma, self.filter_color_loss, self.use_hard_mask = gamma, filter_color_loss, use_hard_mask


def expected_depth(weights, z_vals):
    """The depth a ray's composite expects: sum_s w_s z_s over the compositing weights `weights` [N, S] (`Trainer.forward(...,
    return_weights=True)`, `DifferentiableRender(trainer, weights=True)`) and the sample depths `z_vals` [N, S] -- a torch expression, so a
    loss built on it reaches the network through `backward(..., d_weights=)`.  A ray's samples that are not finite (a ray that misses the
    proxy: depths inf, weights 0) count 0, not 0 * inf."""
    import torch
    z = torch.as_tensor(z_vals, device=weights.device, dtype=weights.dtype)
    return (weights * torch.where(torch.isfinite(z), z, torch.zeros_like(z))).sum(-1)


def as_callable(descriptor):
    """A descriptor loss (`NerfLoss` / `AlphaLoss` over mse / smape) as a callable `loss(color_true=, alpha_true=, color_pred=, alpha_pred=)` on
    torch tensors: the formulas the fused step evaluates (include/nerftex.h at `ntx_loss_desc`; network/loss.py:6-59), restated in torch so
    that the same loss can take the callable route -- alone, or as the base of `Distortion`.  mse = mean((t - p)^2), smape = mean(|t - p| /
    (t + p + 1e-2)); AlphaLoss multiplies both colours by alpha_true (`use_hard_mask`: by alpha_true > 0) when `filter_color_loss`, and adds
    gamma * alpha_loss_fn(alpha_true, alpha_pred)."""
    d = descriptor.desc()
    fns = {_lib.LOSS_MSE: lambda t, p: ((t - p) ** 2).mean(), _lib.LOSS_SMAPE: lambda t, p: ((t - p).abs() / (t + p + 1e-2)).mean()}
    fn, alpha_fn = fns[d.loss_fn], fns[d.alpha_loss_fn]
    alpha_kind, gamma, filtered, hard = d.kind == _lib.LOSS_ALPHA, float(descriptor.gamma), bool(d.filter_color_loss), bool(d.use_hard_mask)   # (gamma unrounded)

    def loss(color_true=None, alpha_true=None, color_pred=None, alpha_pred=None):
        if not alpha_kind:
            return fn(color_true, color_pred)
        if filtered:
            mask = alpha_true[..., None]
            if hard:
                mask = (mask > 0).to(color_pred.dtype)
            color_true, color_pred = color_true * mask, color_pred * mask
        return fn(color_true, color_pred) + gamma * alpha_fn(alpha_true, alpha_pred)
    return loss


def _ray_tensors(weights, z_vals, widths, live, ray_scale):
    """The device tensors `ntx_ray_distortion` reads, float32 and contiguous on the weights' GPU, and (N, S)."""
    import torch
    if weights.dim() != 2 or not weights.is_cuda:
        raise ValueError("weights: a [N, S] tensor on the GPU")
    n, S = (int(v) for v in weights.shape)
    to = lambda a: None if a is None else torch.as_tensor(a).detach().to(device=weights.device, dtype=torch.float32).contiguous()
    w, z, widths, live, ray_scale = to(weights), to(z_vals), to(widths), to(live), to(ray_scale)
    for name, x, numel in (("z_vals", z, n * S), ("widths", widths, n * S), ("live", live, n * S), ("ray_scale", ray_scale, n)):
        if x is not None and x.numel() != numel:
            raise ValueError(f"{name} holds {x.numel()} floats, not {numel} ({n} rays x {S} samples)")
    return (w, z, widths, live, ray_scale), n, S


def ray_distortion(weights, z_vals, widths=None, live=None, ray_scale=None, with_grad: bool = False):
    """`ntx_ray_distortion` on device tensors, on the current stream: the distortion loss of every ray (include/nerftex.h has the formula, the
    liveness rule and the limits) from weights [N, S], depths z_vals [N, S], optional interval widths [N, S] (None: the differences of the
    depths), an optional `live` [N, S] (a sample counts iff live > 0; needs `widths`) and an optional per-ray factor ray_scale [N].  Returns
    loss [N], or (loss [N], grad [N, S] = d loss / d weights) with `with_grad`.  Nothing here is in the autograd graph: `distortion` is."""
    import torch
    (w, z, widths, live, ray_scale), n, S = _ray_tensors(weights, z_vals, widths, live, ray_scale)
    loss = torch.empty((n,), device=w.device, dtype=torch.float32)
    grad = torch.empty((n, S), device=w.device, dtype=torch.float32) if with_grad else None
    ptr = lambda x: None if x is None else x.data_ptr()
    with torch.cuda.device(w.device):
        _lib.check(_lib.lib.ntx_ray_distortion(ptr(w), ptr(z), ptr(widths), ptr(live), ptr(ray_scale), n, S, ptr(loss), ptr(grad),
                                               torch.cuda.current_stream(w.device).cuda_stream))
    return (loss, grad) if with_grad else loss


def distortion(weights, z_vals, widths=None, live=None, ray_scale=None):
    """`ray_distortion` as a differentiable op (`nerf_tex_amd.autograd.RayDistortion`): per-ray values [N], differentiable in `weights` alone
    (the depths are constants, as everywhere in the trainers), first order only.  After a whole-ray step: `distortion(weights, z_vals)`; after an
    instanced one, on the instancer's buffers: `distortion(weights, bufs[2], widths=bufs[3], live=bufs[3])` -- t and dists; the appended closing
    sample has no depth and is not part of the sum."""
    from . import autograd
    return autograd.RayDistortion.apply(weights, z_vals, widths, live, ray_scale)


def ray_interlevel(weights, z_vals, weights_prop, z_prop, ray_scale=None, eps: float = 2.0 ** -23, with_grad: bool = False):
    """`ntx_ray_interlevel` on device tensors, on the current stream: the interlevel loss of every ray (include/nerftex.h has the formula, the
    liveness rule and the limits) between the fine histogram -- weights [N, S] at depths z_vals [N, S] -- and the proposal one -- weights_prop
    [N, S_p] at z_prop [N, S_p] -- with an optional per-ray factor ray_scale [N].  Returns loss [N], or (loss [N], grad_prop [N, S_p] = d loss /
    d weights_prop, grad_fine [N, S] = d loss / d weights) with `with_grad`.  Nothing here is in the autograd graph: `interlevel` is."""
    import torch
    (w, z, _, _, ray_scale), n, S = _ray_tensors(weights, z_vals, None, None, ray_scale)
    if not isinstance(weights_prop, torch.Tensor) or weights_prop.dim() != 2 or int(weights_prop.shape[0]) != n:
        raise ValueError(f"weights_prop: a [N, S_p] tensor with the weights' {n} rays")
    (wp, zp, _, _, _), _, Sp = _ray_tensors(weights_prop, z_prop, None, None, None)
    if wp.device != w.device:
        raise ValueError("weights and weights_prop live on different devices")
    loss = torch.empty((n,), device=w.device, dtype=torch.float32)
    grad_prop = torch.empty((n, Sp), device=w.device, dtype=torch.float32) if with_grad else None
    grad_fine = torch.empty((n, S), device=w.device, dtype=torch.float32) if with_grad else None
    ptr = lambda x: None if x is None else x.data_ptr()
    with torch.cuda.device(w.device):
        _lib.check(_lib.lib.ntx_ray_interlevel(ptr(w), ptr(z), S, ptr(wp), ptr(zp), Sp, ptr(ray_scale), float(eps), n, ptr(loss), ptr(grad_prop), ptr(grad_fine),
                                               torch.cuda.current_stream(w.device).cuda_stream))
    return (loss, grad_prop, grad_fine) if with_grad else loss


def interlevel(weights, z_vals, weights_prop, z_prop, ray_scale=None, eps: float = 2.0 ** -23):
    """`ray_interlevel` as a differentiable op (`nerf_tex_amd.autograd.RayInterlevel`): per-ray values [N], differentiable in `weights_prop` and
    in `weights`, for whichever requires grad (the depths are constants), first order only.  The mip-NeRF 360 use detaches the fine weights:
    `interlevel(weights.detach(), z_all, weights_prop, z_prop).mean()` trains the sampler alone."""
    from . import autograd
    return autograd.RayInterlevel.apply(weights, z_vals, weights_prop, z_prop, ray_scale, float(eps))


class Interlevel:
    """The `sampler_loss` block of a training config: {'module': 'nerf_tex_amd.loss.Interlevel', 'weight': 1.0} makes `Trainer.from_config`
    build a `train.ProposalTrainer`, whose first network learns from `weight` * mean_n(interlevel_n) alone.  It holds the two numbers; the
    trainer calls `ray_interlevel`."""

    def __init__(self, weight: float = 1.0, eps: float = 2.0 ** -23) -> None:
        self.weight, self.eps = float(weight), float(eps)
        if not self.eps > 0:
            raise ValueError("eps must be > 0")


class Distortion:
    """`base` + weight * mean_n(distortion_n * s_n): any loss with the distortion regulariser on the compositing weights, as a callable loss
    along the ray -- its signature names `weights` and `z_vals`, so `gradients_step` / `Train` / `ParameterFitter.fit` hand it
    the step's weights and depths (the callable route; the fused-loss step does not take it).  Called without them it raises TypeError:
    `TextureFitter` hands a loss the predictions alone, and an instanced step needs `live` -- there, use `distortion(w, t, widths=dists,
    live=dists)` by hand behind `DifferentiableInstanceRender(..., weights=True)`.  `base`: a callable loss, a descriptor loss
    (`NerfLoss` / `AlphaLoss`: through `as_callable`), or a `loss_config` dict for `util.instantiate` -- so a training config may say
    {'module': 'nerf_tex_amd.loss.Distortion', 'weight': 0.01, 'base': {'module': 'network.loss.AlphaLoss', 'loss_fn': 'network.loss.smape',
    'alpha_loss_fn': 'network.loss.mse'}}.  `normalize`: s_n = 1 / (z_vals[n, -1] - z_vals[n, 0]), the span the ray's samples cover (else 1); a
    ray whose span is not positive and finite (one that missed its proxy: depths inf; a single sample) counts 0."""

    def __init__(self, base, weight: float = 0.01, normalize: bool = True) -> None:
        from . import util
        if isinstance(base, dict):
            base = util.instantiate(base)
        if hasattr(base, "desc"):
            base = as_callable(base)
        if not callable(base):
            raise TypeError("Distortion(base): a callable loss, a NerfLoss / AlphaLoss, or a loss_config dict")
        self.base, self.weight, self.normalize = base, float(weight), bool(normalize)
        self._base_names = util.loss_keywords(base) & {"weights", "z_vals"}

    def __call__(self, color_true=None, alpha_true=None, color_pred=None, alpha_pred=None, weights=None, z_vals=None):
        import torch
        if weights is None or z_vals is None:
            raise TypeError("Distortion needs the step's compositing weights and depths (weights=, z_vals=): `gradients_step`, `Train` and `ParameterFitter.fit` "
                            "hand them to a loss that names them; a caller that passes the predictions alone (`TextureFitter`) uses `loss.distortion` by hand")
        more = {k: v for k, v in (("weights", weights), ("z_vals", z_vals)) if k in self._base_names}
        val = self.base(color_true=color_true, alpha_true=alpha_true, color_pred=color_pred, alpha_pred=alpha_pred, **more)
        z = torch.as_tensor(z_vals, device=weights.device, dtype=torch.float32)
        scale = None
        if self.normalize:                                                        # 0 where the span is not positive and finite (a missed ray, a single sample)
            span = z[:, -1] - z[:, 0]
            scale = torch.where(torch.isfinite(span) & (span > 0), 1.0 / span, torch.zeros_like(span))
        return val + self.weight * distortion(weights, z, ray_scale=scale).mean()
