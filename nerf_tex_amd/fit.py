"""Fitting material parameters to images: the inverse use of a parameter-conditioned texture.  A trained `ParamNerf` renders a material at
any parameters (`n_parameters = [geometry, appearance]`, model.py:58-101); `ParameterFitter` goes the other way -- given the texture and
target images it finds the parameters that reproduce them, by gradient descent on the training step's own loss with the weights fixed.

    fitter = ParameterFitter(model, n_samples=64, max_rays=2 * 1024, lrate=1e-2, bounds=(0.0, 2.0))
    params, history = fitter.fit(batch, AlphaLoss(...), init=[[0.5] * 5] * 2, n_iters=200)

The gradient is the layer-by-layer trainer's dL/d parameters in its parameters-only mode (`ntx_trainer_enable_param_gradients` mode 2: the
forward pass, the composite's adjoint and the way back through the activations, no weight gradient) -- or, with `fused=True` and a model of the
fused chain's 8 x 256 shape, the chain's (`ntx_trainer_enable_gradients`); the update of the handful of parameters is `torch.optim.Adam` on the
device.  Positions and directions take no gradient; an IPE model and a coarse + fine pair are not
taken.  `loss`: a `nerf_tex_amd.loss` object, or any callable `loss(color_true=, alpha_true=, color_pred=, alpha_pred=)` on torch tensors that
returns a scalar -- a robust loss for photographs, say (`Trainer.gradients_step`).

`TextureFitter` fits what varies OVER a surface: the texels of the parameter textures of an instanced scene (instancer.cpp:640-667), from the
instanced step's dL/d params_map, the texture coordinates `Instancer.sample_uv` gives per sample and the lookup restated in torch
(`texture_lookup`, `apply_textures`).

`PoseFitter` fits the CAMERAS: the poses (and optionally the focal lengths) the images were taken from, from the trainers' dL/d rays_o and
dL/d rays_d through the adjoint of the ray generator (`ray_sampler.posed_rays`, `autograd.PosedRays`, `compose_poses`)."""

from __future__ import annotations

from typing import Optional


class ParameterFitter:
    def __init__(self, model, n_samples: int, max_rays: int, blur_idx: Optional[int] = None, perturb: bool = False, raw_noise_std: float = 0, map_exr: bool = False,
                 lrate: float = 1e-2, bounds=None, device: int = 0, fused: bool = False, precision: str = "float32") -> None:
        """`model`: the trained Nerf-Tex (`nerf_tex_amd.model.ParamNerf` container; its blob gives the weights, which never change);
        `n_samples`, `blur_idx`, `perturb`, `raw_noise_std`, `map_exr`: the renderer's, as the model was trained; `max_rays`: the largest batch
        (images x rays per image); `lrate`: Adam's; `bounds`: None or (low, high), scalars or one value per parameter -- the parameters are
        clamped to them after every update; `fused`: an 8 x 256 / skips [4] / color_depth 1 FourierFeatures model keeps the fused chain
        (`trainer_for(..., fused=True)`), every other model trains layer by layer as without it; `precision`: "float32" or "bf16x6", the
        layer-by-layer trainer's (`Trainer.set_precision`; not together with `fused`)."""
        from .train import trainer_for
        if getattr(model, "n_params", 0) < 1:
            raise ValueError("the model has no parameters to fit (a Nerf, or n_parameters [0, 0])")
        self.model, self.lrate, self.bounds, self.device = model, float(lrate), bounds, int(device)
        self.trainer = trainer_for(model, param_gradients="only", max_rays=int(max_rays), n_samples=int(n_samples), blur_idx=blur_idx, perturb=perturb,
                                   raw_noise_std=raw_noise_std, map_exr=map_exr, device=device, fused=fused, precision=precision)

    def step(self, batch: dict, loss, parameters, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.), seed: Optional[int] = None):
        """The loss of `batch` at `parameters` [B, P] and its gradient [B, P] (GPU tensors): `batch` as `Train` takes it -- rays_o / rays_d
        [B,R,3], t [B,R,2], cone_scale [B,R,1], color [B,R,3], alpha [B,R] -- one parameter row per image (`rays_per_param_row = R`); a
        'parameters' entry of the batch is not read."""
        import torch
        as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(a)
        ro = as_t(batch["rays_o"]); B, R = int(ro.shape[0]), int(ro.shape[1])
        flat = lambda k, w: as_t(batch[k]).reshape(B * R, w) if w else as_t(batch[k]).reshape(B * R)
        alpha = flat("alpha", 0) if batch.get("alpha") is not None else None
        cone = flat("cone_scale", 0) if batch.get("cone_scale") is not None else None
        val, _, _ = self.trainer.gradients_step(flat("rays_o", 3), flat("rays_d", 3), flat("t", 2), as_t(parameters).reshape(B, -1), cone, flat("color", 3), alpha, loss,
                                                composite_bkgd=composite_bkgd, bkgd_color=bkgd_color, seed=seed, rays_per_param_row=R)
        return val, self.trainer.parameter_gradients()

    def fit(self, batches, loss, init, n_iters: int, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.)):
        """`n_iters` Adam steps on the parameters from `init` [B, P].  `batches`: one batch dict (every step takes it) or an iterable of them
        over the SAME images (taken in turn, again from the start when it runs out).  Returns (parameters [B, P] as a GPU tensor, the loss of
        every step -- taken BEFORE its update -- as a list of floats)."""
        import torch
        dev = torch.device("cuda", self.device)
        params = torch.as_tensor(init, dtype=torch.float32).to(dev).clone().contiguous()
        if params.dim() != 2:
            raise ValueError("init must be [B, P]: one parameter row per image")
        if params.shape[1] != self.model.n_params:
            raise ValueError(f"init has {params.shape[1]} columns, the model takes {self.model.n_params} parameters")
        params.requires_grad_(True)
        params.grad = torch.zeros_like(params)
        opt = torch.optim.Adam([params], lr=self.lrate)
        low = high = None
        if self.bounds is not None:
            low, high = (torch.as_tensor(b, dtype=torch.float32).to(dev) for b in self.bounds)
        cycle = [batches] if isinstance(batches, dict) else list(batches)
        history = []
        for it in range(int(n_iters)):
            val, grad = self.step(cycle[it % len(cycle)], loss, params.detach(), composite_bkgd=composite_bkgd, bkgd_color=bkgd_color)
            params.grad.copy_(grad)
            opt.step()
            if low is not None:
                with torch.no_grad():
                    params.copy_(torch.minimum(torch.maximum(params, low), high))
            history.append(val)
        values = torch.cat([v.reshape(1) for v in history]).cpu().tolist() if history else []
        return params.detach(), values

    def weights(self):
        """The trainer's weights (they are the model's: no step changes them)."""
        return self.trainer.weights()


# ---- camera poses: where was a photograph of a known material taken from? ----------------------------------------------------------------------

def hat(omega):
    """The skew matrices [B,3,3] of `omega` [B,3]: hat(w) x = w cross x."""
    import torch
    zero = torch.zeros_like(omega[:, 0])
    x, y, z = omega.unbind(-1)
    return torch.stack([torch.stack([zero, -z, y], -1), torch.stack([z, zero, -x], -1), torch.stack([-y, x, zero], -1)], -2)


def compose_poses(c2w0, omega, tau):
    """c2w_i = [exp(hat(omega_i)) R0_i | T0_i + tau_i], [B,4,4] in `c2w0`'s dtype: a rotation applied on the left of the initial one and a
    shift of the camera centre.  exp is `torch.linalg.matrix_exp`, which torch differentiates, so the 3x3 block stays a rotation at every
    omega; omega = tau = 0 gives `c2w0`'s top three rows back exactly (exp(0) is the identity matrix, and 1 * x + 0 * y = x).  The exponential
    of the B 3x3 matrices is taken in float64 and rounded once: in float32 its scaling and squaring leaves 3e-6 of non-orthonormality at
    |omega| of a few radians, in float64 the rounding of the result is all there is.  The last row is (0, 0, 0, 1)."""
    import torch
    R = torch.linalg.matrix_exp(hat(omega).to(torch.float64)).to(c2w0.dtype) @ c2w0[:, :3, :3]
    top = torch.cat([R, (c2w0[:, :3, 3] + tau)[..., None]], -1)
    last = torch.zeros_like(top[:, :1, :])
    last[:, 0, 3] = 1.0
    return torch.cat([top, last], 1)


class PoseFitter:
    """Fits CAMERA POSES (and, with `fit_focal`, focal lengths) to images of a known material: the third inverse use of a trained texture,
    beside `ParameterFitter` (material parameters) and `TextureFitter` (parameter textures).  Finds where photographs were taken from, or
    corrects noisy dataset poses.

        fitter = PoseFitter(model, height, width, focal, proxy=AABB(b_0, b_1), n_samples=64, max_rays=4 * 256, lrate=1e-3)
        c2w, focal, history = fitter.fit(batch, my_loss, init_c2w, n_iters=200)

    An iteration: `compose_poses` (torch), `ray_sampler.posed_rays` (the rays of every image in one launch, from the poses on the device),
    `DifferentiableRender` on an inputs-only trainer (`trainer_for(model, input_gradients="only", fused=fused)`: dL/d rays_o and dL/d rays_d,
    no weight gradient), the loss, `backward` -- the trainer's ray gradients, `ntx_generate_rays_posed_adjoint`, torch through the matrix
    exponential -- and Adam on omega, tau [B,3] (and log f).  Nothing of the pose passes through the host; the host work of an iteration is
    what `DifferentiableRender` does already.
    What is differentiated: rays_o and rays_d.  The depths (`t`, the proxy's range), `cone_scale` and the focal's part in them are constants,
    as everywhere in the trainer's input gradients.  Not taken: IPE models, a coarse + fine pair, instanced scenes, lens distortion."""

    def __init__(self, model, height: int, width: int, focal, proxy=None, near=None, far=None, n_samples: int = 64, max_rays: int = 1024, blur_idx: Optional[int] = None,
                 perturb: bool = False, raw_noise_std: float = 0, map_exr: bool = False, lrate: float = 1e-3, fit_focal: bool = False, device: int = 0, fused: bool = False,
                 precision: str = "float32") -> None:
        """`model`: the trained Nerf-Tex (a Nerf or ParamNerf container; the weights never change); `height`, `width`, `focal` (a float, or
        one value per image): the cameras' intrinsics, `focal` the start when `fit_focal`; `proxy` (an AABB: `ray_sampler.Proxy`'s rays) or
        `near` and `far` (`Frustum`'s); `n_samples`, `blur_idx`, `perturb`, `raw_noise_std`, `map_exr`, `fused`, `precision`, `max_rays`: as
        `ParameterFitter` takes them; `lrate`: Adam's, for omega (radians), tau (scene units) and log f alike."""
        from .autograd import DifferentiableRender
        from .train import trainer_for
        if isinstance(model, dict) or not hasattr(model, "get_blob"):
            raise TypeError("PoseFitter takes one model (a Nerf or ParamNerf container), not a coarse + fine pair: two passes are two sets of ray gradients")
        if getattr(model, "pos_encoding", "fourier") == "ipe":
            raise TypeError("PoseFitter takes a FourierFeatures model: the derivative of the cone gaussians of an IPE model in the rays is not written")
        if (proxy is None) == (near is None and far is None) or (near is None) != (far is None):
            raise ValueError("give either proxy (an AABB) or near and far, not both and not neither")
        self.model, self.height, self.width, self.focal = model, int(height), int(width), focal
        self.proxy, self.near, self.far = proxy, near, far
        self.lrate, self.fit_focal, self.device = float(lrate), bool(fit_focal), int(device)
        self.trainer = trainer_for(model, input_gradients="only", max_rays=int(max_rays), n_samples=int(n_samples), blur_idx=blur_idx, perturb=perturb,
                                   raw_noise_std=raw_noise_std, map_exr=map_exr, device=device, fused=fused, precision=precision)
        self.render = DifferentiableRender(self.trainer)

    def rays(self, image_plane_loc, c2w, focal):
        """`ray_sampler.posed_rays` under the fitter's intrinsics and proxy / frustum."""
        from .ray_sampler import posed_rays
        return posed_rays(image_plane_loc, c2w, focal, self.height, self.width, proxy=self.proxy, near=self.near, far=self.far)

    def step(self, batch: dict, loss, c2w, focal, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.), seed: Optional[int] = None):
        """The loss [1] of `batch` at the poses `c2w` [B,4,4] / [B,3,4] and `focal` [B] (GPU tensors, any torch expression of the caller's
        leaves), and its `backward()`: the leaves that require grad have their `.grad` (added to what it holds).  `batch`: image_plane_loc
        [B,R,2], color [B,R,3], alpha [B,R], and parameters [B,P] for a ParamNerf -- one row per image."""
        import torch
        if hasattr(loss, "desc"):
            raise TypeError("PoseFitter takes a callable loss(color_true=, alpha_true=, color_pred=, alpha_pred=) on torch tensors")
        dev = torch.device("cuda", self.device)
        to = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(a)).to(device=dev, dtype=torch.float32)
        loc = to(batch["image_plane_loc"])
        B, R = int(loc.shape[0]), int(loc.shape[1])
        rays_o, rays_d, t, cone = self.rays(loc, c2w, focal)
        params = to(batch["parameters"]).reshape(B, -1) if getattr(self.model, "n_params", 0) > 0 else None
        color, alpha = self.render(rays_o, rays_d, t, params, cone.reshape(-1), composite_bkgd=composite_bkgd, bkgd_color=bkgd_color, seed=seed, rays_per_param_row=R)
        val = loss(color_true=to(batch["color"]).reshape(B * R, 3), alpha_true=to(batch["alpha"]).reshape(B * R), color_pred=color, alpha_pred=alpha)
        if not isinstance(val, torch.Tensor) or val.numel() != 1:
            raise TypeError("the loss must return a scalar tensor")
        val.reshape(()).backward()
        return val.detach().reshape(1)

    def fit(self, batches, loss, init_c2w, n_iters: int, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.), callback=None):
        """`n_iters` Adam steps from the poses `init_c2w` [B,4,4] (or [B,3,4]).  `batches`: one batch dict (every step takes it) or an iterable
        of them over the SAME images, taken in turn.  Returns (c2w [B,4,4], focal [B], history): GPU tensors and the loss of every step --
        taken BEFORE its update -- as a list of floats.  `callback(it, c2w, focal)`: called before step `it` with the poses it starts from
        (detached GPU tensors), to follow a fit; what it does with them -- a copy to the host, say -- is its own cost."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.device)
        c2w0 = torch.as_tensor(np.asarray(init_c2w, np.float32) if not isinstance(init_c2w, torch.Tensor) else init_c2w).to(device=dev, dtype=torch.float32)
        if c2w0.dim() != 3 or tuple(c2w0.shape[1:]) not in ((4, 4), (3, 4)):
            raise ValueError(f"init_c2w must be [B,4,4] or [B,3,4], got {tuple(c2w0.shape)}")
        B = int(c2w0.shape[0])
        omega, tau = (torch.zeros((B, 3), device=dev, requires_grad=True) for _ in range(2))
        f0 = torch.as_tensor(np.broadcast_to(np.asarray(self.focal, np.float32), (B,)).copy()).to(dev)
        log_f = torch.log(f0).requires_grad_(self.fit_focal)
        opt = torch.optim.Adam([omega, tau] + ([log_f] if self.fit_focal else []), lr=self.lrate)
        up = lambda b: {k: (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).to(device=dev, dtype=torch.float32).contiguous() for k, v in b.items()
                        if k in ("image_plane_loc", "color", "alpha", "parameters")}
        cycle = [up(b) for b in ([batches] if isinstance(batches, dict) else list(batches))]                                # uploaded once
        focal_now = lambda: torch.exp(log_f) if self.fit_focal else f0
        history = []
        for it in range(int(n_iters)):
            opt.zero_grad(set_to_none=True)
            c2w = compose_poses(c2w0, omega, tau)
            if callback is not None:
                callback(it, c2w.detach(), focal_now().detach())
            history.append(self.step(cycle[it % len(cycle)], loss, c2w, focal_now(), composite_bkgd=composite_bkgd, bkgd_color=bkgd_color))
            opt.step()
        values = torch.cat(history).cpu().tolist() if history else []
        with torch.no_grad():
            return compose_poses(c2w0, omega, tau), focal_now().clone(), values


# ---- learnable parameter textures: a material parameter that varies over the instancer mesh ---------------------------------------------------

def texture_lookup(texels, uv, found):
    """interpolate2d (ntx_instancer.hip, instancer.cpp:605-625) of one channel matrix `texels` [rows, cols] at the texture coordinates `uv`
    [..., 2], as a torch expression: x = u (rows - 1), v (cols - 1); indices by truncation, weights x - floor(x), both indices clamped to the
    matrix, and the device's sum order ((y00 (1 - w0)(1 - w1) + y01 (1 - w0) w1) + y10 w0 (1 - w1)) + y11 w0 w1 -- in float32 the device's value
    bit for bit.  1 where `found` [...] is false (nothing of the mesh within reach: the parameter stays as it is).  `texels` follows
    `nerf_tex_amd.instancer.load_texture`: row = image column, column = image row counted from the bottom.
    The arithmetic runs in `texels`' dtype.  `texels.grad` is torch autograd's: the backward of the four gathers is a scatter-add whose sum
    order is torch's (atomic on a GPU), so the gradient is reproducible to rounding only, not bit for bit."""
    import torch
    rows, cols = int(texels.shape[0]), int(texels.shape[1])
    uv = uv.to(texels.dtype)
    x0, x1 = uv[..., 0] * (rows - 1.0), uv[..., 1] * (cols - 1.0)
    w0, w1 = x0 - torch.floor(x0), x1 - torch.floor(x1)
    # (int)x, then min(max(., 0), n - 1) on the index and on the index + 1: anything beyond [-1, n] clamps like -1 or n
    i, j = torch.trunc(x0).clamp(-1, rows).to(torch.int64), torch.trunc(x1).clamp(-1, cols).to(torch.int64)
    i0, i1, j0, j1 = i.clamp(0, rows - 1), (i + 1).clamp(0, rows - 1), j.clamp(0, cols - 1), (j + 1).clamp(0, cols - 1)
    flat = texels.reshape(-1)
    take = lambda k: flat.index_select(0, k.reshape(-1)).reshape(k.shape)       # (its backward is index_add_: atomic adds, no sort of the indices)
    y00, y01, y10, y11 = take(i0 * cols + j0), take(i0 * cols + j1), take(i1 * cols + j0), take(i1 * cols + j1)
    val = ((y00 * (1.0 - w0) * (1.0 - w1) + y01 * (1.0 - w0) * w1) + y10 * w0 * (1.0 - w1)) + y11 * w0 * w1
    return torch.where(found.to(torch.bool), val, torch.ones_like(val))


def apply_textures(params_map, parameter_idx, textures, uv, found):
    """getParameters' product (instancer.cpp:656-662) outside the instancer: a NEW params_map [N, S, P] whose column `parameter_idx[i]` is the
    given one times `texture_lookup(textures[i], uv, found)`; every other column is copied bit for bit.  On the `params_map` of an instancer
    whose image entries are `neutral_texture()` and `uv`, `found` of its `sample_uv`, this is the textured instancer's per-step lookup."""
    import torch
    if len(parameter_idx) != len(textures):
        raise ValueError(f"{len(textures)} textures for {len(parameter_idx)} parameter columns")
    cols = list(params_map.unbind(-1))
    for idx, tex in zip(parameter_idx, textures):
        cols[int(idx)] = cols[int(idx)] * texture_lookup(tex, uv, found)
    return torch.stack(cols, -1)


class TextureFitter:
    """Fits the parameter TEXTURES of an instanced scene to images: the texels of one channel matrix per image entry of the instancer's
    `textures` list, by torch Adam on the loss of the instanced render with the network's weights fixed.

        inst = Instancer(b_0, b_1, textures=[neutral_texture(), "", "light"], mesh_path=..., n_texture_samples=10 ** 6)
        trainer = trainer_for(model, param_gradients="only", instanced=True, max_rays=1024, n_samples=256)
        fitter = TextureFitter(trainer, inst, shapes=[(12, 16)], patch_scale=0.09, density_scale=400., step_size=0.002)
        textures, history = fitter.fit(batches, my_loss, init=0.5, n_iters=200)

    An iteration: `get_model_input` under a fixed seed per batch, `sample_uv`, `apply_textures`, `DifferentiableInstanceRender`, the loss,
    `backward` (the trainer's dL/d params_map, then torch's scatter-add into the texels), Adam, a clamp to `bounds`.  The texture coordinates
    depend on the rays and the seed alone and are kept per batch after its first pass.
    EVERY sample is looked up at its own point -- what the instancer does when `n_texture_samples` is large.  This is NOT the interpolation
    along the ray between a few texture samples (instancer.cpp:910-923) that a small `n_texture_samples` selects: a texture fitted here
    renders exactly as fitted with a large `n_texture_samples`, and approximately with a small one.  Out of scope: gradients to uv or the
    mesh, albedo textures of auxiliary meshes, light entries, IPE trainers, a deterministic scatter-add, data-parallel fitting."""

    def __init__(self, trainer, instancer, shapes, lrate: float = 1e-2, bounds=(0., 1.), patch_scale: float = 1.0, density_scale: float = 1.0,
                 step_size: float = 1.0, density_reweighting: bool = True, seed: int = 0) -> None:
        """`trainer`: a FlexTrainer, a BranchTrainer or a Trainer(instanced=True), with param_gradients="only"; `instancer`: an `Instancer`
        with image entries (usually `neutral_texture()`: an entry's own texture multiplies on top of the fitted one); `shapes`: one (rows,
        cols) per image entry, in `load_texture`'s convention (rows = image width); `patch_scale`, `density_scale`,
        `density_reweighting`: InstanceRenderer's; `step_size`: the march's; `seed`: batch k marches under seed + k."""
        if not hasattr(trainer, "forward_instanced") or getattr(trainer, "mip", False):
            raise TypeError("TextureFitter takes one pass that runs instanced steps (FlexTrainer, BranchTrainer, Trainer(instanced=True)); IPE trainers and coarse + fine pairs are not taken")
        if getattr(trainer, "param_gradients", False) != "only":
            raise ValueError('TextureFitter needs a trainer with param_gradients="only": the weights are fixed, the gradient wanted is dL/d params_map')
        n_tex = len(getattr(instancer, "tex_idx", ()))
        if n_tex == 0 or getattr(instancer, "inst_mesh", None) is None:
            raise ValueError("the instancer has no image entry in `textures` on an instancer mesh: nothing to look up (neutral_texture() is an entry that changes nothing)")
        self.shapes = [(int(r), int(c)) for r, c in shapes]
        if len(self.shapes) != n_tex or any(r < 1 or c < 1 for r, c in self.shapes):
            raise ValueError(f"shapes must give one (rows, cols) >= 1 per image entry of the instancer: {n_tex} entries, got {list(shapes)!r}")
        from .autograd import DifferentiableInstanceRender
        self.trainer, self.instancer, self.lrate, self.bounds = trainer, instancer, float(lrate), bounds
        self.step_size, self.seed = float(step_size), int(seed)
        self.render = DifferentiableInstanceRender(trainer, patch_scale=patch_scale, density_scale=density_scale, density_reweighting=density_reweighting)
        self._uv = {}                                                 # batch index -> (uv, found)

    def step(self, batch: dict, loss, textures, key=0, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.)):
        """The loss of `batch` at `textures` (a list of tensors [rows, cols] on the GPU; the ones that require grad receive `.grad`, added to
        what it holds).  `batch`: rays_o / rays_d [N,3], parameters [N,P], cone_scale [N], color_true [N,3], alpha_true [N]; `key` names the
        batch for the seed and the kept texture coordinates."""
        import torch
        if hasattr(loss, "desc"):
            raise TypeError("TextureFitter takes a callable loss(color_true=, alpha_true=, color_pred=, alpha_pred=) on torch tensors")
        inst, tr = self.instancer, self.trainer
        dev = torch.device("cuda", tr.device)
        to = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(a)).to(device=dev, dtype=torch.float32)
        rays_o, rays_d = to(batch["rays_o"]).reshape(-1, 3), to(batch["rays_d"]).reshape(-1, 3)
        bufs = inst.get_model_input(rays_o, rays_d, batch["parameters"], tr.n_samples, self.step_size, seed=self.seed + int(key))
        if key not in self._uv:
            self._uv[key] = inst.sample_uv(rays_o, rays_d, bufs, self.step_size)
        uv, found = self._uv[key]
        field = apply_textures(bufs[9], inst.tex_idx, textures, uv, found)
        color, alpha = self.render(bufs, to(batch["cone_scale"]).reshape(-1), params_map=field, hit=inst.last_hit, composite_bkgd=composite_bkgd, bkgd_color=bkgd_color)
        val = loss(color_true=to(batch["color_true"]), alpha_true=to(batch["alpha_true"]), color_pred=color, alpha_pred=alpha)
        if not isinstance(val, torch.Tensor) or val.numel() != 1:
            raise TypeError("the loss must return a scalar tensor")
        val.reshape(()).backward()
        return val.detach().reshape(1)

    def fit(self, batches, loss, init=None, n_iters: int = 100, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.)):
        """`n_iters` Adam steps on the textures.  `batches`: one batch dict or a list of them, taken in turn (batch k always under seed + k).
        `init`: None (every texel 1: the untextured scene), a number, or one array [rows, cols] per texture.  Returns (the textures as a
        list of GPU tensors [rows, cols], the loss of every step -- taken BEFORE its update -- as a list of floats)."""
        import numpy as np
        import torch
        dev = torch.device("cuda", self.trainer.device)
        if init is None or np.isscalar(init):
            start = [torch.full(s, 1.0 if init is None else float(init), dtype=torch.float32, device=dev) for s in self.shapes]
        else:
            start = [torch.as_tensor(np.asarray(a, np.float32)).to(dev).clone().contiguous() for a in init]
        if [tuple(t.shape) for t in start] != self.shapes:
            raise ValueError(f"init must hold one array per texture of shapes {self.shapes}")
        textures = [t.requires_grad_(True) for t in start]
        opt = torch.optim.Adam(textures, lr=self.lrate)
        low = high = None
        if self.bounds is not None:
            low, high = (float(b) for b in self.bounds)
        names = ("rays_o", "rays_d", "parameters", "cone_scale", "color_true", "alpha_true")
        up = lambda a: (a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))).to(device=dev, dtype=torch.float32).contiguous()
        cycle = [{k: up(b[k]) for k in names} for b in ([batches] if isinstance(batches, dict) else list(batches))]      # uploaded once
        self._uv = {}
        history = []
        for it in range(int(n_iters)):
            opt.zero_grad(set_to_none=True)
            history.append(self.step(cycle[it % len(cycle)], loss, textures, key=it % len(cycle), composite_bkgd=composite_bkgd, bkgd_color=bkgd_color))
            opt.step()
            if low is not None:
                with torch.no_grad():
                    for t in textures:
                        t.clamp_(low, high)
        values = torch.cat(history).cpu().tolist() if history else []
        return [t.detach() for t in textures], values
