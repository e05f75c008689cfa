"""The training step of the reference on the GPU (network/train.py:49-70): `Trainer` owns the weights, Adam's state and every layer's
activations behind the C ABI (`ntx_trainer_*`, include/nerftex.h); `step(...)` is the body of the reference's loop -- forward under a
tape, loss, gradients, `optimizer.apply_gradients`.

    trainer = Trainer(model, max_rays=1024, n_samples=256, lrate=5e-4, lrate_decay=500)       # config_carpet_train.py:100-109
    loss = trainer.step(rays_o, rays_d, t, parameters, cone_scale, color, alpha, loss_fn)      # one iteration of train.py:61-67

`Train(...)` is the reference's function of that name (train.py:7-70): the datasets (`nerf_tex_amd.dataset`; or any iterable of batch
dicts), model, loss, schedule and renderer from the config blocks, the loop, and what its Logger does every i_img / i_checkpoint steps (logger.py:57-86) -- the validation
views rendered through the inference path with the trainer's weights handed over on the device, checkpoints in TensorFlow's bundle format
with model + step + optimizer (train.py:55-57) that `Trainer.restore` resumes from.

`Trainer` is built for the ParamNerf architecture of the shipped training configs (8 x 256, skips [4], color_depth 1; narrower widths inside
it), with FourierFeatures under the Renderer or -- an IntegratedPositionalEncoding model (n_pos 6) -- under the MipRenderer
(renderer.py:356-473): three fused passes over the layer chain.  `FlexTrainer` trains every other Nerf / ParamNerf the renderer's flex family
takes (FourierFeatures; depth 1..24, width 2..256, color_depth 0..4, skips below depth-1, no parameter branches) layer by layer: one
contraction per Dense layer and pass (`ntx_trainer_create_flex`); `BranchTrainer` is the same step for a ParamNerf with parameter branches
(param_depth 1..4, param_width 2..128: `ntx_trainer_create_flex_ex`).  `trainer_for(model, ...)` picks between them, and
`Trainer.from_config`, `CoarseFineTrainer` and `Train` build their trainers through it.  The layer-by-layer trainers also take the one
gradient a training step otherwise leaves out, dL/d material parameters (`param_gradients=`, `parameter_gradients()`); `nerf_tex_amd.fit`
fits parameters to target images with it.  The fused chain takes the same two keywords for a FourierFeatures model (`set_gradients`,
`ntx_trainer_enable_gradients`), and `trainer_for(model, ..., fused=True)` keeps such a model on it when a gradient is asked for.
The losses of `nerf_tex_amd.loss` are evaluated inside the step; any other loss is a callable on
torch tensors, and the step runs as `forward(...)`, the loss and its two cotangents in torch, `backward(d_color, d_alpha)`
(`nerf_tex_amd.autograd.DifferentiableRender`: the same pair as a differentiable op).  A loss that looks ALONG the ray -- an expected depth
(`nerf_tex_amd.loss.expected_depth`), an entropy or distortion term -- takes the compositing weights too: `forward(..., return_weights=True)`
hands them out, `backward(d_color, d_alpha, d_weights)` takes their cotangent (`ntx_trainer_weight_cotangent`), and a callable loss that
names `weights` (and `z_vals`) in its signature receives them.  Every trainer also takes the step through
the INSTANCED render (`forward_instanced(bufs, ...)` on an instancer's buffers, then the same `backward`; `DifferentiableInstanceRender`):
the layer-by-layer ones as they are, the fused chain for a FourierFeatures model once asked (`instanced=True`, `enable_instanced()`).
The layer-by-layer trainers run their contractions in float32 or, opt-in, as six bf16 products on the 16-bit matrix cores, float32-grade at
every scale of the cotangents (`precision="bf16x6"`, `set_precision`, `ntx_trainer_set_precision`; `trainer_for(model, precision="bf16x6")`
names them also for the chain's shape); weights, gradients, Adam and checkpoints are float32 either way."""

from __future__ import annotations

import ctypes as C
from typing import Optional

from . import _lib


class Trainer:
    def __init__(self, model, max_rays: int, n_samples: int, lrate: float = 5e-4, lrate_decay: float = 0, perturb: bool = True, blur_idx: Optional[int] = None,
                 map_exr: bool = False, raw_noise_std: float = 0.0, beta_1: float = 0.9, beta_2: float = 0.999, epsilon: float = 1e-7, device: int = 0,
                 param_gradients=False, input_gradients=False, instanced: bool = False, precision: str = "float32") -> None:
        """`model`: a nerf_tex_amd.model.ParamNerf container (its blob gives the initial weights); `lrate`, `lrate_decay` as train.py:49-50
        (ExponentialDecay(lrate, decay_steps=lrate_decay * 1e3, decay_rate=0.1) when lrate_decay > 0); `perturb`, `blur_idx`, `map_exr`: the
        renderer's (renderer.py:34); `raw_noise_std`: the density regulariser of map_model_output (renderer.py:190-192; config_grass_filtered_train.py:99
        trains with 0.1), drawn per (seed, ray, sample) like the jitter.  An IPE model (pos_encoding 'ipe', n_pos 6) trains as the MipRenderer
        renders it (renderer.py:365-444): `n_samples` cone segments between n_samples + 1 depths, the parameter rows hold the blur parameter at
        `blur_idx` (required) -- its product with cone_scale is the cone's radius, and the model sees the other parameters.
        `param_gradients` / `input_gradients`: False, True or "only" (`set_gradients`), for a FourierFeatures model.  `instanced`: the trainer
        also takes steps through the instanced render (`enable_instanced`, `forward_instanced`), for a FourierFeatures model.  `precision`:
        "float32", or "bf16x6" (`set_precision`) on the layer-by-layer trainers; the fused chain refuses it (NTX_E_UNSUPPORTED)."""
        import numpy as np
        _train_precision(precision)
        self.mip = getattr(model, "pos_encoding", "fourier") == "ipe"
        if self.mip and blur_idx is None:
            raise ValueError("an IPE model trains as the MipRenderer renders it, which needs blur_idx (renderer.py:385 indexes the parameters with it)")
        self.model = model
        self.device = int(device)
        self.n_samples, self.max_rays = int(n_samples), int(max_rays)
        self.lrate, self.lrate_decay = float(lrate), float(lrate_decay)
        self.perturb, self.blur_idx, self.map_exr = bool(perturb), blur_idx, bool(map_exr)
        self.raw_noise_std = float(raw_noise_std)
        if self.raw_noise_std < 0:
            raise ValueError("raw_noise_std must be >= 0")
        self.beta_1, self.beta_2, self.epsilon = float(beta_1), float(beta_2), float(epsilon)
        blob = np.ascontiguousarray(model.get_blob(), dtype=np.float32)
        self._h = C.c_void_p()
        self._pad = None
        wide = self._widen(model)
        if wide is not None:                                                    # a narrower network trains inside the 256-wide one (see _widened)
            self._pad = _narrow_in_wide(model, wide)
            full = np.zeros(wide.n_weight_floats(), np.float32)
            full[self._pad] = blob
            blob = full
        desc = (wide or model).desc()
        _lib.check(self._create(C.byref(desc), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, self.device, self.max_rays, self.n_samples, C.byref(self._h)))
        self._n_native = int(_lib.lib.ntx_trainer_weight_count(self._h))
        self.n_weights = self._n_native if self._pad is None else int(self._pad.size)
        self._calls = 0
        self._last_rays = 0
        self._pending, self._forwards = None, 0                                 # (serial, rays, device tensors, samples a ray) of a `forward` whose `backward` has not run
        self.param_gradients = self.input_gradients = False
        self.precision = "float32"
        if precision != "float32":
            self.set_precision(precision)
        if param_gradients is not False or input_gradients is not False:
            self.set_gradients(param_gradients, input_gradients)
        if instanced:
            self.enable_instanced()

    _create = staticmethod(lambda *a: _lib.lib.ntx_trainer_create(*a))           # the entry that makes the native trainer
    _widen = staticmethod(lambda model: _widened(model))                           # a narrower network inside the 256-wide one

    @classmethod
    def from_config(cls, config: dict, max_rays: Optional[int] = None, device: int = 0, weights=None):
        """The trainer and the loss a reference TRAINING config asks for, from its own blocks as written (train.py:20-52): `model_config`
        (network.model.ParamNerf ...), `loss_config`, `lrate`, `lrate_decay`, `renderer_config` (n_samples, perturb, raw_noise_std, blur_idx,
        map_exr; render_chunk / net_chunk / downsampling_factor have no meaning here: a step is one batch), and this package's own top-level
        keys `precision`, `sampler_loss` ({'module': 'nerf_tex_amd.loss.Interlevel', 'weight': 1.0}: a `ProposalTrainer` instead of a
        `CoarseFineTrainer`; it needs a CoarseFine model block and n_importance > 0) and `proposal_model_config` (with `sampler_loss`: a block
        that replaces the first network's with a smaller one).  `max_rays` defaults to the config's batch --
        `train_dataset_config.batchsize` images x `pixel_sampler_config.n_samples` rays -- when the config says it.  Returns (trainer, loss).
        The data side (`nerf_tex_amd.dataset`) and the loop around the step are `Train`'s."""
        from . import util
        cfg = util.remap_reference_config(config)
        models = util.instantiate(dict(cfg["model_config"]))                     # {'model': ...} or CoarseFine's {'model': ..., 'model_fine': ...}
        model = models["model"] if "model" in models else next(iter(models.values()))
        if weights is not None:
            model.set_weights(weights) if isinstance(weights, (list, tuple)) else model.set_blob(weights)
        loss = util.instantiate(dict(cfg["loss_config"]))
        r = dict(cfg["renderer_config"])
        mip = _is_mip(r)
        for k in ("module", "render_chunk", "net_chunk", "downsampling_factor"):
            r.pop(k, None)
        n_samples = int(r.pop("n_samples", 64))                                   # renderer.py:34 default
        known = {k: r.pop(k) for k in ("perturb", "raw_noise_std", "blur_idx", "map_exr") if k in r}
        n_importance = int(r.pop("n_importance", 0))
        if r:
            raise TypeError(f"renderer_config keys without a meaning in a training step: {sorted(r)}")
        if max_rays is None:
            ds = cfg.get("train_dataset_config") or {}
            max_rays = int(cfg.get("batchsize", ds.get("batchsize", 1))) * int(cfg.get("rays_per_image", (ds.get("pixel_sampler_config") or {}).get("n_samples", 1024)))
        kw = dict(max_rays=max_rays, n_samples=n_samples, lrate=cfg.get("lrate", 5e-4), lrate_decay=cfg.get("lrate_decay", 0), device=device, **known)
        if cfg.get("precision") not in (None, "float32"):                          # a top-level key of the config: "bf16x6" trains layer by layer
            kw["precision"] = cfg["precision"]
        if mip and n_importance > 0:
            raise NotImplementedError("Importance sampling for mip-NeRF style rendering is not implemented in the reference either (renderer.py:403-404)")
        if mip != (getattr(model, "pos_encoding", "fourier") == "ipe"):             # the render side's pairing (renderer.py:71, :338)
            raise _lib.NtxError(_lib.NTX_E_UNSUPPORTED, "IPE models train under MipRenderer, FourierFeatures models under Renderer")
        sampler = cfg.get("sampler_loss")                                        # a top-level key of the config: the proposal pair
        if sampler is not None:
            sampler = util.instantiate(dict(sampler))
            fine = models.get(model.name + "_fine")
            if not hasattr(sampler, "weight") or fine is None or n_importance < 1:
                raise ValueError("sampler_loss (nerf_tex_amd.loss.Interlevel) needs a CoarseFine model block and n_importance > 0")
            if cfg.get("proposal_model_config") is not None:                       # a smaller first network, under the first network's name
                made = util.instantiate(dict(cfg["proposal_model_config"], name=model.name))
                model = made[model.name] if isinstance(made, dict) else made
            return ProposalTrainer(model, fine, n_importance=n_importance, interlevel_weight=sampler.weight, interlevel_eps=sampler.eps, **kw), loss
        if n_importance > 0:                                                    # renderer.py:125-138: a coarse and a fine pass
            return CoarseFineTrainer(model, models.get(model.name + "_fine"), n_importance=n_importance, **kw), loss
        return (trainer_for if cls is Trainer else cls)(model, **kw), loss      # the chain where it takes the model, layer by layer otherwise

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value and _lib is not None and getattr(_lib, "lib", None) is not None:
            _lib.lib.ntx_trainer_destroy(h)
            self._h = None

    def set_precision(self, name: str) -> None:
        """The arithmetic of the layer-by-layer trainers' contractions from the next step on (`ntx_trainer_set_precision`): "float32", or
        "bf16x6" -- both operands of every Dense layer's product, forward and backward, as three bf16 terms and six products on the 16-bit
        matrix cores, float32-grade at every scale of the cotangents.  Weights, gradients, Adam and checkpoints are float32 either way.
        Refused by the fused chain (NTX_E_UNSUPPORTED) and between a `forward` and its `backward` (NTX_E_INVALID); the trainer keeps what
        it had."""
        _lib.check(_lib.lib.ntx_trainer_set_precision(self._h, _train_precision(name)))
        self.precision = str(name)

    def _vector(self, what: int):
        import numpy as np
        out = np.empty(self._n_native, np.float32)
        _lib.check(_lib.lib.ntx_trainer_get(self._h, what, out.ctypes.data_as(C.POINTER(C.c_float)), out.size))
        return out if self._pad is None else np.ascontiguousarray(out[self._pad])

    def weights(self):
        """The weights as one float32 vector in `get_weights()` order (hand it to `model.set_blob` to render with them)."""
        return self._vector(_lib.TRAINER_WEIGHTS)

    def gradients(self):
        return self._vector(_lib.TRAINER_GRADIENTS)

    def adam_state(self):
        return self._vector(_lib.TRAINER_ADAM_M), self._vector(_lib.TRAINER_ADAM_V)

    def activation(self, layer: int, n_samples_total: int):
        """What the last step kept of layer 0-7 (trunk), 8 / 9 (colour layers), 10 (raw density), 11 (raw colour), or -- 20-27, 28, 29 -- the
        gradient at the outputs of the trunk layers, the first colour layer, the feature layer, 30 the composite's adjoint (dL/d raw colour,
        dL/d raw density), 40 / 41 the gradient at pos_map / dir_map of a step under `set_gradients`: [n_samples_total, width] float32 (tests)."""
        import numpy as np
        width = {9: 128, 10: 1, 11: 3, 30: 4, 40: self.model.pos_map_dim, 41: self.model.dir_map_dim}.get(int(layer), 256)
        out = np.empty((int(n_samples_total), width), np.float32)
        _lib.check(_lib.lib.ntx_trainer_activation(self._h, int(layer), int(n_samples_total), out.ctypes.data_as(C.POINTER(C.c_float))))
        if self._pad is not None and width > 4 and int(layer) < 40:             # the narrow network's own columns
            out = np.ascontiguousarray(out[:, :self.model.width // (2 if layer == 9 else 1)])
        return out

    def set_weights(self, blob) -> None:
        """New weights (waits for what is in flight on the device); Adam's moments and iteration count stay as they are."""
        self._set(_lib.TRAINER_WEIGHTS, blob)

    def _set(self, what: int, values) -> None:
        import numpy as np
        b = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        if self._pad is not None:
            if b.size != self._pad.size:
                raise ValueError(f"{b.size} floats given, the model has {self._pad.size}")
            full = np.zeros(self._n_native, np.float32)
            full[self._pad] = b
            b = full
        _lib.check(_lib.lib.ntx_trainer_set(self._h, what, b.ctypes.data_as(C.POINTER(C.c_float)), b.size))

    @property
    def iterations(self) -> int:
        return int(_lib.lib.ntx_trainer_iterations(self._h))

    # ---- resuming (train.py:55-60, logger.py:30-39, 84-86) -------------------------------------------------------------------------
    def state_dict(self) -> dict:
        """Everything a resumed run needs to continue bit for bit: weights, Adam's moments and iteration count (its bias correction and
        the ExponentialDecay schedule run on it), and the counter the default jitter / noise seeds come from."""
        m, v = self.adam_state()
        return {"weights": self.weights(), "adam_m": m, "adam_v": v, "iterations": self.iterations, "calls": self._calls}

    def load_state_dict(self, state: dict) -> None:
        self._set(_lib.TRAINER_WEIGHTS, state["weights"])
        self._set(_lib.TRAINER_ADAM_M, state["adam_m"]); self._set(_lib.TRAINER_ADAM_V, state["adam_v"])
        _lib.check(_lib.lib.ntx_trainer_set_iterations(self._h, int(state["iterations"])))
        self._calls = int(state.get("calls", state["iterations"]))

    def save(self, prefix: str, step: int = None, root: str = None) -> str:
        """`checkpoint_manager.save(checkpoint_number=step)` (logger.py:84-86): a TensorBundle `<prefix>.index` / `.data-00000-of-00001` with
        the keys of `tf.train.Checkpoint(**{model.name: model}, step=step, optimizer=optimizer)` (train.py:55-57; nerf_tex_amd/checkpoint.py)."""
        import numpy as np
        from . import checkpoint
        table = self.model.layer_table()
        split = lambda blob: _split_blob(table, blob)
        st = self.state_dict()
        hyper = {"beta_1": self.beta_1, "beta_2": self.beta_2, "decay": 0.0}
        if not self.lrate_decay > 0:
            hyper["learning_rate"] = self.lrate                  # (under a schedule Keras has no such variable)
        return checkpoint.write_checkpoint(prefix, table, split(st["weights"]), split(st["adam_m"]), split(st["adam_v"]), iterations=st["iterations"],
                                           step=st["iterations"] if step is None else int(step), hyper=hyper, root=root or self.model.name)

    def restore(self, path: str, root: str = None, verify: bool = True) -> dict:
        """`checkpoint.restore(manager.latest_checkpoint)` (logger.py:39): `path` is a checkpoint prefix or a directory of `ckpt-<n>`.  Weights,
        Adam's slots and iteration count when the bundle holds them (a bundle with weights alone restarts the optimiser, as TensorFlow's
        `expect_partial()` restore would).  Returns {'prefix', 'step', 'iterations'}."""
        import os
        import numpy as np
        from . import checkpoint
        prefix = checkpoint.latest_checkpoint(path) if os.path.isdir(path) else path
        st = checkpoint.training_state_from_bundle(checkpoint.read_bundle(prefix, verify), self.model.layer_table(), root or self.model.name)
        flat = lambda arrs: np.concatenate([np.asarray(a, np.float32).ravel() for a in arrs])
        self._set(_lib.TRAINER_WEIGHTS, flat(st["weights"]))
        zeros = np.zeros(self.n_weights, np.float32)
        self._set(_lib.TRAINER_ADAM_M, zeros if st["m"] is None else flat(st["m"])); self._set(_lib.TRAINER_ADAM_V, zeros if st["v"] is None else flat(st["v"]))
        it = st["iterations"] if st["iterations"] is not None and st["m"] is not None else 0
        _lib.check(_lib.lib.ntx_trainer_set_iterations(self._h, int(it)))
        self._calls = int(it)
        return {"prefix": prefix, "step": st["step"], "iterations": it}

    def gradients_step(self, rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, loss, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.),
                       seed: Optional[int] = None, z_vals=None, rays_per_param_row: int = 1, n_samples: Optional[int] = None):
        """Forward + loss + gradients (train.py:61-66): rays_o / rays_d [N,3], t [N,2] (inf for a ray that misses the proxy: it predicts 0 / the
        background and counts in the loss, renderer.py:58-86), parameters [rows,P],
        cone_scale [N] or [N,1], color_true [N,3], alpha_true [N]; `loss`: a nerf_tex_amd.loss object (the fused step), or any callable
        `loss(color_true=, alpha_true=, color_pred=, alpha_pred=)` on torch tensors that returns a scalar (`forward`, torch, `backward`: the same
        gradients for ANY differentiable loss of the predictions; a callable whose signature names `weights` also receives the compositing
        weights [N,S], and -- if it names `z_vals` too -- the step's depths [N,S]: a loss along the ray).  Returns (loss [1], color_pred [N,3],
        alpha_pred [N]) as GPU tensors; the gradients stay in the trainer.  `z_vals` [N, n_samples]: given sample depths (`n_samples` of them,
        default the trainer's) instead of the ones placed between t.  An IPE trainer (MipRenderer): parameters [rows, P + 1] with the blur parameter
        at blur_idx, `z_vals` [N, n_samples + 1] segment edges."""
        import torch
        if not hasattr(loss, "desc"):                                          # a loss written in PyTorch: forward, the loss and its cotangents in torch, backward
            return self._callable_loss_step(rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, loss, composite_bkgd=composite_bkgd, bkgd_color=bkgd_color,
                                            seed=seed, z_vals=z_vals, rays_per_param_row=rays_per_param_row, n_samples=n_samples)
        self._pending = None                                                   # (the fused step drops a forward left open)
        dev, to, ptr = self._device_tools()
        color_true, alpha_true = to(color_true), to(alpha_true)
        n, head, tail, keep = self._step_inputs(rays_o, rays_d, t, parameters, cone_scale, composite_bkgd, bkgd_color, seed, z_vals, rays_per_param_row, n_samples)   # keep: alive over the call
        color = torch.empty((n, 3), device=dev); alpha = torch.empty((n,), device=dev); val = torch.empty((1,), device=dev)
        desc = loss.desc()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.ntx_train_step_gradients(self._h, *head, *tail, ptr(color_true), ptr(alpha_true), C.byref(desc), ptr(color), ptr(alpha), ptr(val),
                                                         torch.cuda.current_stream(dev).cuda_stream))
        return val, color, alpha

    def _device_tools(self):
        import torch
        dev = torch.device("cuda", self.device)
        to = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a)).to(device=dev, dtype=torch.float32).contiguous()
        ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None
        return dev, to, ptr

    def _step_inputs(self, rays_o, rays_d, t, parameters, cone_scale, composite_bkgd, bkgd_color, seed, z_vals, rays_per_param_row, n_samples):
        """What `ntx_train_step_gradients` and `ntx_train_forward` share: the number of rays, the arguments up to blur_idx (`head`) and from the
        flags to z_vals (`tail`), and the device tensors behind the pointers (to be kept while the library reads them).  Counts the call: the
        default jitter / noise seed is the number of steps taken."""
        _, to, ptr = self._device_tools()
        rays_o, rays_d, t, parameters, cone_scale, z_vals = (to(a) for a in (rays_o, rays_d, t, parameters, cone_scale, z_vals))
        n = rays_o.reshape(-1, 3).shape[0]
        P_in = int(getattr(self.model, "n_params", 0)) + (1 if self.mip else 0)
        if P_in > 0 and parameters is not None:                                # the kernels read row ray // rays_per_param_row of it unasked: a count of floats, no shape test
            need = -(-n // max(1, int(rays_per_param_row))) * P_in
            if parameters.numel() < need:
                raise ValueError(f"parameters holds {parameters.numel()} floats, the step reads {need}: ceil({n} rays / {max(1, int(rays_per_param_row))} rays a row) rows "
                                 f"of {P_in}")
        self._last_rays = n
        flags = (_lib.FLAG_PERTURB if self.perturb else 0) | (_lib.FLAG_MAP_EXR if self.map_exr else 0) | (_lib.FLAG_COMPOSITE_BKGD if composite_bkgd else 0)
        opts = None
        if self.raw_noise_std > 0:
            flags |= _lib.FLAG_RAW_NOISE
            opts = C.byref(_lib.render_opts(raw_noise_std=self.raw_noise_std))
        if seed is None:
            seed = self._calls
        self._calls += 1
        head = (ptr(rays_o), ptr(rays_d), ptr(t), ptr(parameters), int(rays_per_param_row), ptr(cone_scale), n, int(n_samples or self.n_samples),
                -1 if self.blur_idx is None else int(self.blur_idx))
        tail = (flags, _lib.f3(bkgd_color), int(seed) & (2 ** 64 - 1), opts, ptr(z_vals))
        return n, head, tail, (rays_o, rays_d, t, parameters, cone_scale, z_vals)

    def forward(self, rays_o, rays_d, t, parameters, cone_scale, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.), seed: Optional[int] = None, z_vals=None,
                rays_per_param_row: int = 1, n_samples: Optional[int] = None, return_weights: bool = False):
        """The first half of a step under any loss (`ntx_train_forward`): `gradients_step`'s arguments less the targets and the loss; returns
        (color_pred [N,3], alpha_pred [N]) as GPU tensors -- bit for bit `gradients_step`'s -- and leaves the step pending until
        `backward(d_color, d_alpha)`.  The trainer keeps the batch's device tensors until then; a tensor handed in that is already float32,
        contiguous and on the device is read in place and must not be written before the backward.  `return_weights`: returns (color_pred,
        alpha_pred, weights [N, S]) -- the composite's weights a_s T_s, for a loss that looks along the ray (`backward(..., d_weights=)`); an
        IPE trainer hands out none (NTX_E_UNSUPPORTED)."""
        import torch
        dev, _, ptr = self._device_tools()
        self._pending = None
        n, head, tail, keep = self._step_inputs(rays_o, rays_d, t, parameters, cone_scale, composite_bkgd, bkgd_color, seed, z_vals, rays_per_param_row, n_samples)
        S = int(n_samples or self.n_samples)
        color = torch.empty((n, 3), device=dev); alpha = torch.empty((n,), device=dev)
        weights = torch.empty((n, S), device=dev) if return_weights else None
        with torch.cuda.device(dev), self._weights_into(weights):
            _lib.check(_lib.lib.ntx_train_forward(self._h, *head, *tail, ptr(color), ptr(alpha), torch.cuda.current_stream(dev).cuda_stream))
        self._forwards += 1
        self._pending = (self._forwards, n, keep, S)
        return (color, alpha, weights) if return_weights else (color, alpha)

    def _weights_into(self, weights):
        """A context in which the forward fills `weights` [N, S] (`ntx_trainer_composite_weights`, taken back on the way out); None: nothing."""
        import contextlib
        if weights is None:
            return contextlib.nullcontext()

        @contextlib.contextmanager
        def registered():
            _lib.check(_lib.lib.ntx_trainer_composite_weights(self._h, weights.data_ptr()))
            try:
                yield
            finally:
                _lib.check(_lib.lib.ntx_trainer_composite_weights(self._h, None))
        return registered()

    def backward(self, d_color, d_alpha=None, d_weights=None) -> None:
        """The second half (`ntx_train_backward`): `d_color` [N,3] = dL/d color_pred and `d_alpha` [N] = dL/d alpha_pred (None: 0) of the pending
        `forward` -> the gradients of L, left in the trainer exactly as `gradients_step` leaves them (`gradients()`, `sync_gradients`,
        `apply_gradients`, `parameter_gradients()`).  One backward per forward: NTX_E_INVALID without a pending forward, or after a
        `gradients_step` in between.  Every gradient is linear in the two cotangents, so L is any differentiable function of the predictions;
        a data-parallel mean of gradients (`sync_gradients`) is the gradient of the ranks' joint loss only if L is a mean over rays.
        `d_weights` [N, S] = dL/d weights of the pending forward's compositing weights (`return_weights=True`; None: no such term, and the
        backward is bit for bit what it is without the keyword): registered for this backward alone (`ntx_trainer_weight_cotangent`)."""
        import torch
        dev, to, ptr = self._device_tools()
        pending, self._pending = self._pending, None
        d_color, d_alpha, d_weights = to(d_color), to(d_alpha), to(d_weights)
        if pending is not None and d_color is not None:
            n = pending[1]
            if d_color.numel() != 3 * n or (d_alpha is not None and d_alpha.numel() != n):
                self._pending = pending
                raise ValueError(f"d_color / d_alpha hold {d_color.numel()} / {None if d_alpha is None else d_alpha.numel()} floats, the pending forward has {n} rays")
            if d_weights is not None and d_weights.numel() != n * pending[3]:
                self._pending = pending
                raise ValueError(f"d_weights holds {d_weights.numel()} floats, the pending forward has {n} rays x {pending[3]} samples")
        if d_weights is not None and d_color is not None:
            rc = _lib.lib.ntx_trainer_weight_cotangent(self._h, ptr(d_weights))
            if rc != _lib.NTX_OK:
                self._pending = pending
                _lib.check(rc)
        with torch.cuda.device(dev):
            rc = _lib.lib.ntx_train_backward(self._h, d_color.data_ptr() if d_color is not None else None, ptr(d_alpha), torch.cuda.current_stream(dev).cuda_stream)
        if rc != _lib.NTX_OK and d_color is None:
            self._pending = pending                                            # (the library keeps the forward open on a NULL d_color)
        _lib.check(rc)

    def _callable_loss_step(self, rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, loss, **kw):
        """`gradients_step` for a loss without `desc()`: any callable `loss(color_true=, alpha_true=, color_pred=, alpha_pred=)` on torch tensors
        that returns a scalar (the reference's call, loss.py:12, 30).  Its value and its gradient at the predictions come from torch's autograd,
        everything else from the native forward and backward."""
        import torch
        _, to, _ = self._device_tools()
        color_true, alpha_true = to(color_true), to(alpha_true)
        names = _loss_keywords(loss)
        if "weights" not in names:                                             # a loss of the predictions alone: today's call
            color, alpha = self.forward(rays_o, rays_d, t, parameters, cone_scale, **kw)
            c, a = color.detach().requires_grad_(True), alpha.detach().requires_grad_(True)
            with torch.enable_grad():
                val = loss(color_true=color_true, alpha_true=alpha_true, color_pred=c, alpha_pred=a)
                if not isinstance(val, torch.Tensor) or val.numel() != 1:
                    raise TypeError("a loss without desc() must return a scalar tensor")
                d_color, d_alpha = torch.autograd.grad(val.reshape(()), (c, a), allow_unused=True)
            self.backward(torch.zeros_like(color) if d_color is None else d_color, d_alpha)
            return val.detach().reshape(1), color, alpha
        # a loss along the ray: it names `weights`, and -- where it also names `z_vals` -- receives the step's depths, placed here exactly as the
        # step would place them (`ntx_sample_depths` under the step's flags and seed) and handed to the forward as z_vals
        more = {}
        if "z_vals" in names:
            if kw.get("z_vals") is None:
                kw = dict(kw, z_vals=self._sample_depths(t, kw.get("seed"), kw.get("n_samples")), seed=self._calls if kw.get("seed") is None else kw.get("seed"))
            more["z_vals"] = to(kw["z_vals"])
        color, alpha, weights = self.forward(rays_o, rays_d, t, parameters, cone_scale, return_weights=True, **kw)
        c, a, w = (x.detach().requires_grad_(True) for x in (color, alpha, weights))
        with torch.enable_grad():
            val = loss(color_true=color_true, alpha_true=alpha_true, color_pred=c, alpha_pred=a, weights=w, **more)
            if not isinstance(val, torch.Tensor) or val.numel() != 1:
                raise TypeError("a loss without desc() must return a scalar tensor")
            d_color, d_alpha, d_weights = torch.autograd.grad(val.reshape(()), (c, a, w), allow_unused=True)
        self.backward(torch.zeros_like(color) if d_color is None else d_color, d_alpha, d_weights)
        return val.detach().reshape(1), color, alpha

    def _sample_depths(self, t, seed, n_samples):
        """The depths [N, S] the next step would place between `t` under the trainer's `perturb` and `seed` (default: the step counter), as a
        device tensor: `ntx_sample_depths`, the entry the step itself calls -- a step handed these as `z_vals` is that step bit for bit."""
        import torch
        dev, to, ptr = self._device_tools()
        t = to(t)
        n, S = t.reshape(-1, 2).shape[0], int(n_samples or self.n_samples)
        if self.mip:
            raise _lib.NtxError(_lib.NTX_E_UNSUPPORTED, "an IPE trainer hands out no composite weights, so a loss on them has no depths to take")
        z = torch.empty((n, S), device=dev)
        seed = self._calls if seed is None else seed
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.ntx_sample_depths(ptr(t), n, S, _lib.FLAG_PERTURB if self.perturb else 0, int(seed) & (2 ** 64 - 1), None, ptr(z),
                                                  torch.cuda.current_stream(dev).cuda_stream))
        return z

    def set_gradients(self, param_gradients=False, input_gradients=False) -> None:
        """Both gradient modes for the following steps, each False / True / "only" (`ntx_trainer_enable_gradients`; the buffers are placed
        at the first True or "only"): True -- every step also leaves dL/d parameters (`parameter_gradients()`) or dL/d rays_o, rays_d
        (`ray_gradients()`), loss, predictions and weight gradients bit for bit as without it; "only" -- the same gradients and no weight
        gradient at all (`gradients()` keeps what it held; `apply_gradients` raises NTX_E_INVALID) while either is "only".  On the fused chain
        for a FourierFeatures model (an IPE model: NTX_E_UNSUPPORTED); set them before a `forward`, a change drops the pending one."""
        modes = {False: 0, True: 1, "only": 2}
        native = []
        for name, mode in (("param_gradients", param_gradients), ("input_gradients", input_gradients)):
            if not (isinstance(mode, (int, str)) and mode in modes):
                raise ValueError(f'{name} must be False, True or "only", not {mode!r}')
            native.append(modes[mode])
        import torch
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.ntx_trainer_enable_gradients(self._h, native[0], native[1]))
        self.param_gradients, self.input_gradients = ("only" if m == 2 else bool(m) for m in native)

    def enable_instanced(self) -> None:
        """From here on the trainer takes `forward_instanced` (`ntx_trainer_enable_instanced`): the fused chain places the compaction's maps
        for its capacity, once; plain steps stay bit for bit what they were.  A layer-by-layer trainer takes instanced steps as it is and
        nothing changes; an IPE model: NTX_E_UNSUPPORTED."""
        import torch
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.ntx_trainer_enable_instanced(self._h))

    def _device_copies(self, ptrs, shape):
        """Copies of the trainer's device results `ptrs` as torch tensors of `shape`, in the current stream's order."""
        import torch
        dev = torch.device("cuda", self.device)
        outs = tuple(torch.empty(shape, device=dev, dtype=torch.float32) for _ in ptrs)
        with torch.cuda.device(dev):
            for out, ptr in zip(outs, ptrs):
                if out.numel():
                    _lib.copy_device_async(out.data_ptr(), ptr.value, out.numel() * 4, torch.cuda.current_stream(dev).cuda_stream)
        return outs

    def ray_gradients(self):
        """(dL/d rays_o, dL/d rays_d) of the last plain step: torch tensors [N, 3] on the trainer's device, copies in the current stream's
        order.  The sample depths are constants; a ray that misses has exact zeros."""
        o, d, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _lib.check(_lib.lib.ntx_trainer_ray_gradients(self._h, C.byref(o), C.byref(d), C.byref(n)))
        return self._device_copies((o, d), (int(n.value), 3))

    def parameter_gradients(self):
        """dL/d parameters of the last step: a torch tensor [rows, P] on the trainer's device (rows = the step's parameter rows,
        ceil(n_rays / rays_per_param_row); geometry columns first), a copy in the current stream's order."""
        import torch
        ptr, rows, n = C.c_void_p(), C.c_int64(), C.c_int()
        _lib.check(_lib.lib.ntx_trainer_param_gradients(self._h, C.byref(ptr), C.byref(rows), C.byref(n)))
        dev = torch.device("cuda", self.device)
        out = torch.empty((int(rows.value), int(n.value)), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.copy_device_async(out.data_ptr(), ptr.value, out.numel() * 4, torch.cuda.current_stream(dev).cuda_stream)
        return out

    def sample_input_gradients(self):
        """(dL/d pts, dL/d rays_d_map) of the last INSTANCED step: torch tensors [N, S, 3] on the trainer's device (exact zeros at samples
        outside every patch), copies in the current stream's order."""
        p, d, n, s = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int()
        _lib.check(_lib.lib.ntx_trainer_sample_input_gradients(self._h, C.byref(p), C.byref(d), C.byref(n), C.byref(s)))
        return self._device_copies((p, d), (int(n.value), int(s.value), 3))

    def forward_instanced(self, bufs, cone_scale, *, patch_scale: float, density_scale: float = 1.0, density_reweighting: bool = True, composite_bkgd: bool = False,
                          bkgd_color=(1., 1., 1.), hit=None, return_weights: bool = False):
        """The first half of a step on the INSTANCED render (`ntx_train_forward_instanced`): InstanceRenderer's tail (renderer.py:247-354) with
        every activation kept, the network on the in-patch samples alone.  `bufs`: the ten-tuple of an instancer's `get_model_input` --
        rays_d_map [N,S,3], pts [N,S,3], t [N,S], dists [N,S], color_last [N,1,3], alpha_last [N,1], alpha_weight [N,S], instance_id (unused),
        idxs (indices of the hit rays [k,1] or a bool mask [N]), params_map [N,S,P] -- as numpy arrays or tensors; `hit` [N] (the native
        instancer's `last_hit`) takes the place of idxs.  `cone_scale` [N] (read with blur_idx only).  Returns (color_pred [N,3], alpha_pred
        [N]) as GPU tensors and leaves the step pending until `backward(d_color, d_alpha)`, exactly as `forward` does; `self.last_live` is
        the number of in-patch samples the network ran on (reading it back is the step's one synchronisation).  Float32, contiguous device
        tensors are read in place and must not be written before the backward.  `return_weights`: returns (color_pred, alpha_pred, weights
        [N, S]) -- (1 - el) T at the in-patch samples, exactly 0 elsewhere and on rays that hit nothing; the appended sample's weight is
        alpha_pred - weights.sum(-1) -- for `backward(..., d_weights=)`."""
        import numpy as np
        import torch
        dev, to, ptr = self._device_tools()
        self._pending = None
        rays_d_map, pts, tt, dists, color_last, alpha_last, alpha_weight, _, idxs, params_map = bufs
        dists = to(dists)
        n, S = int(dists.shape[0]), int(dists.shape[1])
        if hit is None:
            idxs = idxs.detach().cpu().numpy() if isinstance(idxs, torch.Tensor) else np.asarray(idxs)
            mask = np.zeros(n, np.uint8)
            mask[idxs.reshape(-1) if idxs.dtype == np.bool_ else idxs.reshape(-1).astype(np.int64)] = 1
            hit = mask
        hit = (hit if isinstance(hit, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(hit))).to(device=dev).ne(0).to(torch.uint8).contiguous()
        P = int(getattr(self.model, "n_params", 0))
        keep = dict(rd=to(rays_d_map), pts=to(pts), t=to(tt), dists=dists, cl=to(color_last), al=to(alpha_last), aw=to(alpha_weight) if density_reweighting else None, hit=hit,
                    pm=to(params_map) if P > 0 else None, cone=to(cone_scale))
        sizes = dict(rd=3 * n * S, pts=3 * n * S, t=n * S, cl=3 * n, al=n, aw=n * S, hit=n, pm=n * S * P, cone=n)
        for k, want in sizes.items():
            if keep[k] is not None and keep[k].numel() != want:
                raise ValueError(f"forward_instanced: buffer '{k}' holds {keep[k].numel()} elements, {n} rays x {S} samples need {want}")
        flags = (_lib.FLAG_MAP_EXR if self.map_exr else 0) | (_lib.FLAG_COMPOSITE_BKGD if composite_bkgd else 0)
        color = torch.empty((n, 3), device=dev); alpha = torch.empty((n,), device=dev)
        live = C.c_int64(0)
        weights = torch.empty((n, S), device=dev) if return_weights else None
        with torch.cuda.device(dev), self._weights_into(weights):
            _lib.check(_lib.lib.ntx_train_forward_instanced(
                self._h, ptr(keep["rd"]), ptr(keep["pts"]), ptr(keep["t"]), ptr(dists), ptr(keep["cl"]), ptr(keep["al"]), ptr(keep["aw"]), ptr(hit), ptr(keep["pm"]),
                ptr(keep["cone"]), n, S, -1 if self.blur_idx is None else int(self.blur_idx), float(patch_scale), float(density_scale), flags, _lib.f3(bkgd_color),
                ptr(color), ptr(alpha), C.byref(live), torch.cuda.current_stream(dev).cuda_stream))
        self.last_live = int(live.value)
        self._last_rays = n
        self._forwards += 1
        self._pending = (self._forwards, n, keep, S)
        return (color, alpha, weights) if return_weights else (color, alpha)

    def sample_parameter_gradients(self):
        """dL/d params_map of the last INSTANCED step: a torch tensor [N, S, P] on the trainer's device (geometry columns first, exact zeros at
        samples outside every patch), a copy in the current stream's order."""
        import torch
        ptr, n, s, p = C.c_void_p(), C.c_int64(), C.c_int(), C.c_int()
        _lib.check(_lib.lib.ntx_trainer_sample_param_gradients(self._h, C.byref(ptr), C.byref(n), C.byref(s), C.byref(p)))
        dev = torch.device("cuda", self.device)
        out = torch.empty((int(n.value), int(s.value), int(p.value)), device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            _lib.copy_device_async(out.data_ptr(), ptr.value, out.numel() * 4, torch.cuda.current_stream(dev).cuda_stream)
        return out

    def apply_gradients(self) -> None:
        """optimizer.apply_gradients (train.py:67): Adam under the learning-rate schedule of train.py:49-52."""
        import torch
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.ntx_trainer_adam_step(self._h, self.lrate, self.lrate_decay * 1e3 if self.lrate_decay > 0 else 0.0, 0.1, self.beta_1, self.beta_2,
                                                      self.epsilon, torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream))

    def train_step(self, data: dict, loss, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.), comm=None, group=None, seed: Optional[int] = None) -> dict:
        """The body of the reference's loop on ITS batch dict (train.py:61-67: `pred = renderer(**data, composite_bkgd=..., bkgd_color=...)`,
        `loss_fn(color_true=data['color'], alpha_true=data['alpha'], **pred)`, gradients, `apply_gradients`): `data` as network/dataset.py maps it
        -- rays_o / rays_d [B,R,3], t [B,R,2], cone_scale [B,R,1], parameters [B,P] (one row per image: renderer.py:54), color [B,R,3],
        alpha [B,R].  Returns {'loss', 'color_pred' [B,R,3], 'alpha_pred' [B,R]} (GPU tensors)."""
        import torch
        as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(a)
        ro = as_t(data["rays_o"]); B, R = int(ro.shape[0]), int(ro.shape[1])
        flat = lambda k, w: as_t(data[k]).reshape(B * R, w) if w else as_t(data[k]).reshape(B * R)
        alpha = flat("alpha", 0) if data.get("alpha") is not None else None
        val, c, a = self.gradients_step(flat("rays_o", 3), flat("rays_d", 3), flat("t", 2), as_t(data["parameters"]).reshape(B, -1), flat("cone_scale", 0),
                                        flat("color", 3), alpha, loss, composite_bkgd=composite_bkgd, bkgd_color=bkgd_color, seed=seed, rays_per_param_row=R)
        if comm is not None or (torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size(group) > 1):
            self.sync_gradients(comm, group)
        self.apply_gradients()
        return {"loss": val, "color_pred": c.reshape(B, R, 3), "alpha_pred": a.reshape(B, R)}

    def sync_gradients(self, comm=None, group=None) -> None:
        """Data-parallel training (one process per GPU, every rank on its own rays -- equally many): the gradient becomes the mean over the
        ranks, which is the gradient of the loss over all their rays (the losses of loss.py are means over rays).  `comm`: a
        nerf_tex_amd.dist.Comm -- ONE ncclAllReduce of the 2.7 MB over xGMI behind the C ABI (`ntx_trainer_allreduce_gradients`), on the current
        stream.  Without one, the same mean through torch.distributed on host memory (gloo: the CPU-side tests, ranks sharing a GPU)."""
        import torch
        import torch.distributed as dist
        on_device = dist.is_available() and dist.is_initialized() and dist.get_backend(group) == "nccl"
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1 and not (on_device and getattr(self, "_shards_agreed", False)):
            # the mean of the ranks' means is the batch's gradient only when every rank brought as many rays (the losses are means over rays).
            # Over gloo (host tensors) this is asked every step; over nccl it costs a device sync, so it is asked at the first step only.
            self._shards_agreed = True
            mine = torch.tensor([self._last_rays], dtype=torch.int64, device=torch.device("cuda", self.device) if on_device else "cpu")
            counts = [torch.empty_like(mine) for _ in range(dist.get_world_size(group))]
            dist.all_gather(counts, mine, group=group)
            if len({int(c.item()) for c in counts}) != 1:
                raise ValueError(f"data-parallel step with unequal shards ({[int(c.item()) for c in counts]} rays): the mean of per-rank gradients would be wrong")
        if comm is not None:
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib.ntx_trainer_allreduce_gradients(self._h, comm.handle, torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream))
            return
        g = allreduce_mean_host(self.gradients(), group)
        _lib.check(_lib.lib.ntx_trainer_set(self._h, _lib.TRAINER_GRADIENTS, g.ctypes.data_as(C.POINTER(C.c_float)), g.size))

    def step(self, *args, comm=None, group=None, **kwargs):
        """One iteration of the reference's loop (train.py:61-67); returns the loss (a GPU tensor; with several ranks: this rank's).
        `comm` / `group`: data-parallel (see `sync_gradients`)."""
        import torch.distributed as dist
        val, _, _ = self.gradients_step(*args, **kwargs)
        if comm is not None or (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
            self.sync_gradients(comm, group)
        self.apply_gradients()
        return val


class FlexTrainer(Trainer):
    """`Trainer` for the architectures the fused chain does not take: any Nerf / ParamNerf of the renderer's flex family (FourierFeatures on
    n_pos 3, depth 1..24, width 2..256, color_depth 0..4, skips below depth-1, param_depth 0 -- the chain's own 8 x 256 shape included), one
    contraction per Dense layer and pass behind `ntx_trainer_create_flex`.  Same constructor, same steps, state, checkpoints and all-reduce;
    weights and gradients in `get_weights()` order."""

    _create = staticmethod(lambda *a: _lib.lib.ntx_trainer_create_flex(*a))
    _widen = staticmethod(lambda model: None)                                      # every width trains as it is

    def __init__(self, model, *args, param_gradients=False, input_gradients=False, instanced: bool = False, **kw) -> None:
        """`Trainer`'s arguments (`instanced` is accepted and changes nothing: this trainer takes instanced steps as it is), and
        `param_gradients`: False, True -- every `gradients_step` also leaves dL/d parameters (`parameter_gradients()`), the weight gradients bit for bit as without it -- or "only": the same parameter gradients and no weight
        gradient at all (`gradients()` keeps what it held; `apply_gradients` raises NTX_E_INVALID).  For a model with parameters
        (`ntx_trainer_enable_param_gradients`).  `input_gradients`: the same three values for dL/d rays_o, rays_d (`ray_gradients()`) and,
        of an instanced step, dL/d pts, rays_d_map (`sample_input_gradients()`), for any model (`ntx_trainer_enable_input_gradients`); no
        weight gradient is taken while either is "only"."""
        super().__init__(model, *args, **kw)
        self.param_gradients = False
        self.input_gradients = False
        if param_gradients is not False:
            self.set_param_gradients(param_gradients)
        if input_gradients is not False:
            self.set_input_gradients(input_gradients)

    def set_param_gradients(self, mode) -> None:
        """False / True / "only" for the following steps (the buffers are placed at the first True or "only")."""
        modes = {False: 0, True: 1, "only": 2}
        if isinstance(mode, (int, str)) and mode in modes:
            native = modes[mode]
        else:
            raise ValueError(f'param_gradients must be False, True or "only", not {mode!r}')
        import torch
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.ntx_trainer_enable_param_gradients(self._h, native))
        self.param_gradients = "only" if native == 2 else bool(native)

    def set_input_gradients(self, mode) -> None:
        """False / True / "only" for the following steps (the buffers are placed at the first True or "only")."""
        modes = {False: 0, True: 1, "only": 2}
        if isinstance(mode, (int, str)) and mode in modes:
            native = modes[mode]
        else:
            raise ValueError(f'input_gradients must be False, True or "only", not {mode!r}')
        import torch
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib.ntx_trainer_enable_input_gradients(self._h, native))
        self.input_gradients = "only" if native == 2 else bool(native)

    def relu_widths(self):
        """Widths of the ReLU layers in the order of `activation`'s indices (and of the oracle's masks): trunk, colour layers, colour half."""
        m = self.model
        cd = m.color_depth if m.kind == 0 else 0
        return [m.width] * (m.depth + cd) + [m.width // 2]

    def activation(self, layer: int, n_samples_total: int):
        """What the last step kept: `layer` 0 .. n_relu - 1 the output of the k-th ReLU layer (trunk 0 .. depth-1, colour hidden layers, colour
        half layer), 64 the raw density, 65 the raw colour, 30 the composite's adjoint (dL/d raw colour, dL/d raw density): [n_samples_total,
        width] float32 (tests)."""
        import numpy as np
        widths = self.relu_widths()
        width = {64: 1, 65: 3, 30: 4}.get(int(layer)) or (widths[int(layer)] if 0 <= int(layer) < len(widths) else 1)
        out = np.empty((int(n_samples_total), width), np.float32)
        _lib.check(_lib.lib.ntx_trainer_activation(self._h, int(layer), int(n_samples_total), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out


class BranchTrainer(FlexTrainer):
    """`FlexTrainer` for a ParamNerf with parameter branches (model.py:88-101: `param_depth` Dense(param_width, relu) layers on the Fourier
    features of the geometry parameters and, separately, of the appearance parameters; param_depth 0..4, param_width 2..128) behind
    `ntx_trainer_create_flex_ex`.  The branches are evaluated per sample, their layers train like the trunk's, and their weights sit where
    `get_weights()` has them.  With param_depth 0 (or a model without parameters) the step is `FlexTrainer`'s bit for bit."""

    @staticmethod
    def _create(desc_ref, *a):
        desc = desc_ref._obj
        desc.kind = _lib.KIND_PARAMNERF_EX                                       # the extended descriptor, also when param_depth is 0
        return _lib.lib.ntx_trainer_create_flex_ex(C.byref(desc), *a)

    def branch_widths(self):
        """Widths of the branch ReLU layers in the order of the oracle's `branch_masks`: geometry layers (`activation` 32 + j), then
        appearance layers (48 + j); a branch exists where the model has parameters of its kind."""
        m = self.model
        return [m.param_width] * (m.param_depth * ((m.n_geo > 0) + (m.n_app > 0)))

    def activation(self, layer: int, n_samples_total: int):
        """`FlexTrainer.activation`, and `layer` 32 + j / 48 + j: the kept output of layer j of the geometry / appearance branch,
        [n_samples_total, param_width] float32 (tests)."""
        import numpy as np
        if not 32 <= int(layer) < 64:
            return super().activation(layer, n_samples_total)
        out = np.empty((int(n_samples_total), self.model.param_width), np.float32)
        _lib.check(_lib.lib.ntx_trainer_activation(self._h, int(layer), int(n_samples_total), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out


def _train_precision(name) -> int:
    """The ntx_precision of a trainer's precision name."""
    if not isinstance(name, str) or name not in _lib.TRAIN_PRECISIONS:
        if name == "fp16x3":
            raise _lib.NtxError(_lib.NTX_E_UNSUPPORTED, "training in fp16x3: the cotangents of a mean loss lie below the range of an IEEE half; \"bf16x6\" keeps float32's exponents")
        raise ValueError(f"precision must be one of {sorted(_lib.TRAIN_PRECISIONS)}, not {name!r}")
    return _lib.TRAIN_PRECISIONS[name]


def _chain_takes(model) -> bool:
    """Whether `Trainer` (the fused chain, `ntx_trainer_create`) trains `model`: ParamNerf 8 x 256 / skips [4] / color_depth 1 with Fourier
    features or IPE and encodings of at most 96 features, or a narrower Fourier network that `_widened` pads into it."""
    from .model import KIND_PARAMNERF
    live = sorted({int(i) for i in model.skips if 0 <= int(i) < model.depth})
    if not (model.kind == KIND_PARAMNERF and model.depth == 8 and live == [4] and model.color_depth == 1 and model.param_depth == 0):
        return False
    if max(model.pos_map_dim, model.dir_map_dim) > 96:
        return False
    ipe = model.pos_encoding == "ipe"
    if model.width == 256:
        return model.n_pos == (6 if ipe else 3)
    return _widened(model) is not None and model.n_pos == 3


def trainer_class_for(model, branches: bool = False, param_gradients=False, input_gradients=False, fused: bool = False, precision: str = "float32"):
    """The class that trains `model`, without creating anything (no device is asked for): `Trainer` where the fused chain takes it,
    `FlexTrainer` for any other model `ntx_trainer_create_flex` accepts; the library's NTX_E_UNSUPPORTED otherwise -- which is what a
    model with parameter branches gets unless `branches` is set: then a model with param_depth > 0 and at least one parameter gets
    `BranchTrainer`, if `ntx_trainer_create_flex_ex` accepts it.  `param_gradients` / `input_gradients` (True or "only"): the layer-by-layer class also
    where the chain would take the model, unless `fused` is set: then a FourierFeatures model the chain takes keeps `Trainer`, which takes both
    gradients through `ntx_trainer_enable_gradients` (an IPE model: the library's NTX_E_UNSUPPORTED -- the cone gaussians' derivative is not
    written, and the layer-by-layer trainer takes no IPE model).  `precision` "bf16x6": the layer-by-layer class also for the chain's own
    8 x 256 shape (the chain runs on its own float32 kernels); together with `fused` it raises NTX_E_UNSUPPORTED."""
    import numpy as np
    wants = param_gradients is not False or input_gradients is not False
    if _train_precision(precision) != _lib.PRECISION_F32:
        if fused:
            raise _lib.NtxError(_lib.NTX_E_UNSUPPORTED, f"precision {precision!r} on the fused chain (fused=True): the chain runs on its own float32 kernels; the "
                                "layer-by-layer trainer takes the same model")
        wants = True
    if _chain_takes(model) and (not wants or fused):
        if wants and model.pos_encoding == "ipe":
            raise _lib.NtxError(_lib.NTX_E_UNSUPPORTED, "parameter / input gradients of an IPE model on the fused chain: the cone gaussians' derivative is not written")
        return Trainer
    cls = BranchTrainer if branches and model.param_depth > 0 and model.n_params > 0 else FlexTrainer
    desc, h = model.desc(), C.c_void_p()
    blob = np.zeros(max(1, model.n_weight_floats()), np.float32)
    # the entry checks the architecture first (NTX_E_UNSUPPORTED) and max_rays = 0 next (NTX_E_INVALID), before anything is created
    rc = cls._create(C.byref(desc), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, 0, 0, 0, C.byref(h))
    if rc != _lib.NTX_E_INVALID:                                                   # NTX_E_UNSUPPORTED, with the library's own words
        _lib.check(rc)
    return cls


def trainer_for(model, **kw):
    """`Trainer(model, **kw)`, `FlexTrainer(model, **kw)` or `BranchTrainer(model, **kw)`, whichever `trainer_class_for(model, branches=True)`
    names; with `param_gradients` or `input_gradients` True / "only" the layer-by-layer class -- or, with `fused=True` and a FourierFeatures
    model the chain takes, the fused chain with the same two keywords.  `instanced=True` goes on to the class: the chain then takes instanced
    steps too (the layer-by-layer classes always do)."""
    fused = bool(kw.pop("fused", False))
    cls = trainer_class_for(model, branches=True, param_gradients=kw.get("param_gradients", False), input_gradients=kw.get("input_gradients", False), fused=fused,
                            precision=kw.get("precision", "float32"))
    if cls is Trainer and not fused:
        kw.pop("param_gradients", None)                                        # (False: the chain has no such argument)
        kw.pop("input_gradients", None)
    return cls(model, **kw)


class CoarseFineTrainer:
    """Training with `n_importance > 0` (renderer.py:125-138, loss.py:15-16, 41-47, model.py:47-56): a coarse pass on `n_samples` depths, the
    importance sampler on its composite weights (sample_pdf, no gradient through it: `tf.stop_gradient`, :129), a fine pass on the
    n_samples + n_importance merged depths by `model_fine` -- or by the same network when there is none (:132) -- and the loss of both
    passes added up.  Two networks take one step each, on their own gradients; one network takes one step on the sum of the two passes'.
    Every piece is the C ABI's: two `ntx_train_step_gradients` (the coarse one also leaves the weights: `ntx_trainer_composite_weights`),
    `ntx_sample_pdf` between them, `ntx_trainer_stash_gradients` for the shared network.  Input gradients (`input_gradients=`) are out of
    scope here: two steps give two results to add, and each pass's trainer holds only its own."""

    def __init__(self, model, model_fine=None, max_rays: int = 1024, n_samples: int = 64, n_importance: int = 64, **kw) -> None:
        self.n_samples, self.n_importance, self.shared = int(n_samples), int(n_importance), model_fine is None
        if self.n_importance < 1:
            raise ValueError("n_importance must be >= 1 (a plain Trainer otherwise)")
        total = self.n_samples + self.n_importance
        self.fine = trainer_for(model if self.shared else model_fine, max_rays=max_rays, n_samples=total, **kw)
        self.coarse = self.fine if self.shared else trainer_for(model, max_rays=max_rays, n_samples=self.n_samples, **kw)
        self.model, self.model_fine, self.device, self.perturb = model, model_fine, self.fine.device, self.fine.perturb
        self._calls = 0

    @property
    def trainers(self):
        return (self.fine,) if self.shared else (self.coarse, self.fine)

    @property
    def iterations(self) -> int:
        return self.fine.iterations

    def gradients_step(self, rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, loss, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.),
                       seed: Optional[int] = None, rays_per_param_row: int = 1, u=None, on_coarse=None):
        """Both passes and their gradients.  Returns (loss [1] = fine + coarse, color_pred, alpha_pred, color_pred_coarse, alpha_pred_coarse).
        `u` [N, n_importance]: the sampler's uniform draws when perturb is off (renderer.py:128 `det=self.perturb`: with perturb they are
        tf.linspace); default: torch's generator under `seed`.  `on_coarse()`: called between the passes (tests read the coarse activations)."""
        import torch
        if not hasattr(loss, "desc"):
            raise TypeError("a coarse + fine step takes a nerf_tex_amd.loss object: a loss written in PyTorch would need the cotangents of two passes "
                            "(Trainer.forward / backward and nerf_tex_amd.autograd.DifferentiableRender are one pass)")
        dev = torch.device("cuda", self.device)
        to = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a)).to(device=dev, dtype=torch.float32).contiguous()
        rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true = (to(a) for a in (rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true))
        n, S, NI = rays_o.reshape(-1, 3).shape[0], self.n_samples, self.n_importance
        if seed is None:
            seed = self._calls
        self._calls += 1
        wts = torch.empty((n, S), device=dev)
        _lib.check(_lib.lib.ntx_trainer_composite_weights(self.coarse._h, wts.data_ptr()))
        try:
            val_c, cc, ac = self.coarse.gradients_step(rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, loss, composite_bkgd=composite_bkgd,
                                                       bkgd_color=bkgd_color, seed=seed, rays_per_param_row=rays_per_param_row, n_samples=S)
        finally:
            _lib.check(_lib.lib.ntx_trainer_composite_weights(self.coarse._h, None))
        if on_coarse is not None:
            on_coarse()
        if not self.perturb and u is None:
            u = torch.rand((n, NI), device=dev, generator=torch.Generator(device=dev).manual_seed(int(seed) & (2 ** 63 - 1)))
        u = None if self.perturb else to(u).reshape(n, NI).contiguous()
        z_all = torch.empty((n, S + NI), device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.ntx_sample_pdf(t.data_ptr(), None, wts.data_ptr(), u.data_ptr() if u is not None else None, n, S, NI,
                                               _lib.FLAG_PERTURB if self.perturb else 0, int(seed) & (2 ** 64 - 1), None, z_all.data_ptr(), stream))
            if self.shared:
                _lib.check(_lib.lib.ntx_trainer_stash_gradients(self.fine._h, 0, stream))
        val_f, cf, af = self.fine.gradients_step(rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, loss, composite_bkgd=composite_bkgd,
                                                 bkgd_color=bkgd_color, seed=seed, z_vals=z_all, rays_per_param_row=rays_per_param_row, n_samples=S + NI)
        if self.shared:
            with torch.cuda.device(dev):
                _lib.check(_lib.lib.ntx_trainer_stash_gradients(self.fine._h, 1, stream))
        self.last_z = z_all
        return val_f + val_c, cf, af, cc, ac

    def apply_gradients(self) -> None:
        for tr in self.trainers:
            tr.apply_gradients()

    # ---- resuming: ONE checkpoint holds both networks under one optimizer (train.py:55: dict(model, step=..., optimizer=...)) --------------
    def save(self, prefix: str, step: int = None) -> str:
        from . import checkpoint
        parts = []
        for tr in self.trainers:
            st, table = tr.state_dict(), tr.model.layer_table()
            parts.append((tr.model.name, table, _split_blob(table, st["weights"]), _split_blob(table, st["adam_m"]), _split_blob(table, st["adam_v"])))
        f = self.fine
        hyper = {"beta_1": f.beta_1, "beta_2": f.beta_2, "decay": 0.0}
        if not f.lrate_decay > 0:
            hyper["learning_rate"] = f.lrate
        root, table, w, m, v = parts[0]
        return checkpoint.write_checkpoint(prefix, table, w, m, v, iterations=self.iterations, step=self.iterations if step is None else int(step), hyper=hyper,
                                           root=root, more=parts[1:])

    def restore(self, path: str, verify: bool = True) -> dict:
        """As `Trainer.restore`, every network from its own root of the one bundle."""
        import os
        from . import checkpoint
        prefix = checkpoint.latest_checkpoint(path) if os.path.isdir(path) else path
        info = {}
        for tr in self.trainers:
            info = tr.restore(prefix, root=tr.model.name, verify=verify)
        self._calls = int(info.get("iterations") or 0)
        return info

    def hand_weights_to_models(self) -> None:
        """Both networks' render contexts take the trainers' weights on the device (`NerfModel.set_weights_from_trainer`)."""
        for tr in self.trainers:
            tr.model.set_weights_from_trainer(tr)

    def step(self, *args, **kwargs):
        val = self.gradients_step(*args, **kwargs)[0]
        self.apply_gradients()
        return val

    def train_step(self, data: dict, loss, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.), seed: Optional[int] = None) -> dict:
        """`Trainer.train_step` on the reference's batch dict; the predictions carry the coarse pass's too, as Renderer.render_rays returns them (:138)."""
        import torch
        as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.as_tensor(a)
        ro = as_t(data["rays_o"]); B, R = int(ro.shape[0]), int(ro.shape[1])
        flat = lambda k, w: as_t(data[k]).reshape(B * R, w) if w else as_t(data[k]).reshape(B * R)
        alpha = flat("alpha", 0) if data.get("alpha") is not None else None
        val, c, a, cc, ac = self.gradients_step(flat("rays_o", 3), flat("rays_d", 3), flat("t", 2), as_t(data["parameters"]).reshape(B, -1), flat("cone_scale", 0),
                                                flat("color", 3), alpha, loss, composite_bkgd=composite_bkgd, bkgd_color=bkgd_color, seed=seed, rays_per_param_row=R)
        self.apply_gradients()
        return {"loss": val, "color_pred": c.reshape(B, R, 3), "alpha_pred": a.reshape(B, R), "color_pred_coarse": cc.reshape(B, R, 3), "alpha_pred_coarse": ac.reshape(B, R)}


class ProposalTrainer(CoarseFineTrainer):
    """A proposal network and a fine network under the interlevel loss of mip-NeRF 360 (`ntx_ray_interlevel`: the formula is stated at the
    entry in include/nerftex.h): the first network only places the fine pass's samples, and learns from the fine pass's weights alone --
    it is never asked for a colour, so it may be much smaller than the fine one.  A step: `proposal.forward(return_weights=True)` on the
    depths the step would place itself; `ntx_sample_pdf` on its weights (the `u`, seed and perturb rule of `CoarseFineTrainer`); the fine
    network's whole step on the merged depths under the caller's loss (a descriptor object or any callable the fine trainer takes);
    `ray_interlevel(w_fine, z_all, w_prop, z_prop, ray_scale=interlevel_weight / N)` -- N counts every ray of the batch, missed ones
    too; `proposal.backward(zeros, None, d_weights=grad_prop)`.  The image loss never reaches the proposal network (its colour layers take
    exact zeros) and the interlevel term never reaches the fine one.  Always two networks, each through `trainer_for` (their architectures
    may differ); an IPE model hands out no weights (NTX_E_UNSUPPORTED).  Everything else -- `apply_gradients`, `save` / `restore`,
    `hand_weights_to_models`, `step`, `train_step` -- is the parent's.  Out of scope: shared-network and data-parallel pairs, more than one
    proposal level, instanced steps, `input_gradients=`."""

    def __init__(self, proposal_model, model, max_rays: int = 1024, n_samples: int = 64, n_importance: int = 64, interlevel_weight: float = 1.0,
                 interlevel_eps: float = 2.0 ** -23, **kw) -> None:
        if model is None or model is proposal_model:
            raise ValueError("ProposalTrainer holds two networks: a proposal model and a fine model of its own (a shared network has nothing to propose to)")
        for m in (proposal_model, model):
            if getattr(m, "pos_encoding", "fourier") == "ipe":
                raise _lib.NtxError(_lib.NTX_E_UNSUPPORTED, "an IPE trainer hands out no composite weights, so the interlevel loss has nothing to compare")
        super().__init__(proposal_model, model, max_rays=max_rays, n_samples=n_samples, n_importance=n_importance, **kw)
        self.interlevel_weight, self.interlevel_eps = float(interlevel_weight), float(interlevel_eps)
        self.last_interlevel = None

    proposal = property(lambda self: self.coarse)

    def gradients_step(self, rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, loss, composite_bkgd: bool = False, bkgd_color=(1., 1., 1.),
                       seed: Optional[int] = None, rays_per_param_row: int = 1, u=None, on_coarse=None):
        """Both networks' gradients.  Returns (loss [1] = fine loss + interlevel_weight * mean interlevel, color_pred, alpha_pred,
        color_pred_prop, alpha_pred_prop); `last_interlevel` [1] holds the interlevel term alone, `last_z` the merged depths.  `u`, `seed`,
        `on_coarse`: as in `CoarseFineTrainer.gradients_step` (`on_coarse()` runs after the proposal's forward)."""
        import torch
        from . import loss as _loss
        dev = torch.device("cuda", self.device)
        to = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.as_tensor(a)).to(device=dev, dtype=torch.float32).contiguous()
        rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true = (to(a) for a in (rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true))
        n, S, NI = rays_o.reshape(-1, 3).shape[0], self.n_samples, self.n_importance
        if seed is None:
            seed = self._calls
        self._calls += 1
        step = dict(composite_bkgd=composite_bkgd, bkgd_color=bkgd_color, seed=seed, rays_per_param_row=rays_per_param_row)
        z_prop = self.coarse._sample_depths(t, seed, S)                        # the depths the forward would place itself
        cp, ap, w_prop = self.coarse.forward(rays_o, rays_d, t, parameters, cone_scale, z_vals=z_prop, n_samples=S, return_weights=True, **step)
        if on_coarse is not None:
            on_coarse()
        if not self.perturb and u is None:
            u = torch.rand((n, NI), device=dev, generator=torch.Generator(device=dev).manual_seed(int(seed) & (2 ** 63 - 1)))
        u = None if self.perturb else to(u).reshape(n, NI).contiguous()
        z_all = torch.empty((n, S + NI), device=dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.ntx_sample_pdf(t.data_ptr(), None, w_prop.data_ptr(), u.data_ptr() if u is not None else None, n, S, NI,
                                               _lib.FLAG_PERTURB if self.perturb else 0, int(seed) & (2 ** 64 - 1), None, z_all.data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream))
        fine_step = lambda fn: self.fine.gradients_step(rays_o, rays_d, t, parameters, cone_scale, color_true, alpha_true, fn, z_vals=z_all, n_samples=S + NI, **step)
        if hasattr(loss, "desc"):                                              # the fused-loss step leaves its weights where they are registered
            w_fine = torch.empty((n, S + NI), device=dev)
            with self.fine._weights_into(w_fine):
                val_f, cf, af = fine_step(loss)
        else:                                                                  # a callable: the fine trainer's forward hands the weights to a loss that names them
            names, seen = _loss_keywords(loss), {}

            def along(color_true=None, alpha_true=None, color_pred=None, alpha_pred=None, weights=None, z_vals=None):
                seen["weights"] = weights.detach()
                more = {k: v for k, v in (("weights", weights), ("z_vals", z_vals)) if k in names}
                return loss(color_true=color_true, alpha_true=alpha_true, color_pred=color_pred, alpha_pred=alpha_pred, **more)
            val_f, cf, af = fine_step(along)
            w_fine = seen["weights"]
        scale = torch.full((n,), self.interlevel_weight / n, device=dev)
        per_ray, grad_prop, _ = _loss.ray_interlevel(w_fine, z_all, w_prop, z_prop, ray_scale=scale, eps=self.interlevel_eps, with_grad=True)
        self.coarse.backward(torch.zeros_like(cp), None, d_weights=grad_prop)
        self.last_interlevel, self.last_z = per_ray.sum().reshape(1), z_all
        return val_f + self.last_interlevel, cf, af, cp, ap


def _loss_keywords(loss) -> set:
    """`util.loss_keywords`: the keyword names a callable loss's signature spells out."""
    from . import util
    return util.loss_keywords(loss)


def _is_mip(renderer_config) -> bool:
    """Whether a renderer_config block names the MipRenderer (as the reference's module path or this package's)."""
    return str((renderer_config or {}).get("module") or "").rsplit(".", 1)[-1] == "MipRenderer"


def _widened(model):
    """Training is built for 8 x 256.  A ParamNerf of the same shape but NARROWER (`width` < 256, even) trains inside it:
    its kernels sit in the top-left corners of the 256-wide ones (behind the encoding rows of the skip and colour layers), everything else is
    zero and STAYS zero -- a padded unit's pre-activation is exactly 0, its ReLU gate is shut, so no gradient reaches its incoming weights, and
    its outgoing weights see an activation of exactly 0; Adam leaves a weight whose gradient was always 0 where it is.  The step is then the
    narrow network's, value for value (adding exact zeros changes no float32 sum), at the 256-wide network's cost -- as the flex render
    family does.  Returns the 256-wide twin, or None if `model` is not such a network (256 itself included)."""
    from .model import KIND_PARAMNERF, NerfModel
    if not (model.kind == KIND_PARAMNERF and model.width < 256 and model.width >= 2 and model.width % 2 == 0 and model.depth == 8 and tuple(model.skips) == (4,)
            and model.color_depth == 1 and model.param_depth == 0 and model.pos_encoding == "fourier"):
        return None
    return NerfModel(model.kind, [model.n_geo, model.n_app], model.n_pos, model.pos_freq, model.dir_freq, model.param_freq, 8, 256, (4,), 1, model.name)


def _narrow_in_wide(narrow, wide):
    """Index of every float of `narrow`'s weight blob inside `wide`'s (both in `get_weights()` order): a layer's input rows are
    [encoding rows (the same in both) | hidden rows 0 .. w-1 of the wide layer's 256 (128 for the last colour layer)], its columns 0 .. out-1."""
    import numpy as np
    idx, at = [], 0
    for (name, i_n, o_n), (name_w, i_w, o_w) in zip(narrow.layer_table(), wide.layer_table()):
        assert name == name_w
        hidden_n = 0 if name == "trunk0" else narrow.width // 2 if name == "color" else narrow.width     # the rows that come from a hidden layer
        hidden_w = 0 if name == "trunk0" else 128 if name == "color" else 256
        assert i_n - hidden_n == i_w - hidden_w and i_n >= hidden_n, (name, i_n, i_w)                # the pos_map / dir_map rows in front of them (model.py:107, 115)
        rows = np.arange(i_n)                                                 # narrow row r -> wide row r: the hidden rows follow the encoding rows in both
        kernel = at + rows[:, None] * o_w + np.arange(o_n)[None, :]
        idx += [kernel.reshape(-1), at + i_w * o_w + np.arange(o_n)]
        at += i_w * o_w + o_w
    return np.concatenate(idx).astype(np.int64)


def allreduce_mean_host(values, group=None):
    """The mean over the ranks of a float32 vector, through torch.distributed on host memory (sum in the backend's order, then / world)."""
    import numpy as np
    import torch
    import torch.distributed as dist
    v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).copy())
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(v, op=dist.ReduceOp.SUM, group=group)
        v /= dist.get_world_size(group)
    return v.numpy()


def _split_blob(table, blob):
    import numpy as np
    out, p = [], 0
    b = np.asarray(blob, np.float32).ravel()
    for _, i, o in table:
        out.append(b[p:p + i * o].reshape(i, o)); p += i * o
        out.append(b[p:p + o]); p += o
    return out


def Train(target_path: str, train_dataset=None, val_dataset=None, model_config: dict = None, loss_config: dict = None, n_iters: int = 1000, lrate: float = 5e-4,
          lrate_decay: float = 0, renderer_config: dict = None, logger_config: dict = None, max_rays: int = None, device: int = 0, weights=None,
          composite_bkgd: bool = None, bkgd_color=None, train_dataset_config: dict = None, val_dataset_config: dict = None, precision: str = "float32",
          **kwargs) -> dict:
    """network.train.Train (train.py:7-70).  The data side either as the reference's blocks -- `train_dataset_config` / `val_dataset_config`
    (`network.dataset.Dataset` over `TFRecord` / `FileFolder` / `GenerateData`, instantiated here as train.py:23-26 does, `n_parameters` of the
    model defaulting to the dataset's, :29) -- or handed in: `train_dataset` any iterable of batch dicts as network/dataset.py maps them
    (rays_o / rays_d [B,R,3], t [B,R,2], cone_scale [B,R,1], parameters [B,P], color [B,R,3], alpha [B,R]), `val_dataset` a
    `nerf_tex_amd.dataset.Dataset` (or any iterable of ray batch dicts with height / width / composite_bkgd / bkgd_color) whose views are
    rendered every `i_img` steps.  The other arguments are the reference's: `model_config` / `loss_config` /
    `renderer_config` blocks, `n_iters`, `lrate`, `lrate_decay`, and of `logger_config` (logger.py:14) `i_print`, `i_img`, `i_checkpoint`,
    `max_to_keep`; `precision` (this package's; a config's top-level key): "float32", or "bf16x6" -- the layer-by-layer trainer with its
    contractions on the 16-bit matrix cores (`Trainer.set_precision`).  What the reference's Logger does at its cadences happens here: a checkpoint `checkpoints/ckpt-<step>` under `target_path`
    (model + step + optimizer, train.py:55-57) every `i_checkpoint` steps, the validation views through `Renderer` (`MipRenderer` for a mip run) -- the inference path, the
    trainer's weights handed over on the device -- every `i_img` steps; a run whose `target_path` holds checkpoints resumes from the newest and
    takes `n_iters - step` batches (train.py:60).  Returns {'trainer', 'renderer', 'loss' [(step, value)], 'images' {step: [RGBA [H,W,4]]},
    'checkpoints' [prefix], 'step'}."""
    import os
    import torch
    from . import checkpoint, util
    from .renderer import MipRenderer, Renderer
    import torch.distributed as dist
    rank, world = (dist.get_rank(), dist.get_world_size()) if dist.is_available() and dist.is_initialized() else (0, 1)
    if train_dataset is None:
        if train_dataset_config is None:
            raise TypeError("Train needs train_dataset_config (the reference's block) or train_dataset (an iterable of batches)")
        block = dict(util.remap_reference_config(train_dataset_config), device=torch.device("cuda", device))
        if world > 1 and block.get("seed") is not None:
            block["seed"] = int(block["seed"]) + rank                         # every rank its own views and pixels
        train_dataset = util.instantiate(block)
    if val_dataset is None and val_dataset_config is not None:
        val_dataset = util.instantiate(dict(util.remap_reference_config(val_dataset_config), device=torch.device("cuda", device)))
    if model_config is not None and hasattr(train_dataset, "n_parameters"):
        model_config = dict(model_config)
        model_config.setdefault("n_parameters", train_dataset.n_parameters)     # train.py:29
    cfg = util.remap_reference_config(dict(model_config=model_config, loss_config=loss_config, renderer_config=renderer_config or {}, lrate=lrate,
                                           lrate_decay=lrate_decay, precision=precision))
    if max_rays is None:
        if hasattr(train_dataset, "batchsize") and hasattr(train_dataset, "n_samples"):
            max_rays = int(train_dataset.batchsize) * int(train_dataset.n_samples)
        else:
            first = next(iter(train_dataset))
            max_rays = int(first["rays_o"].shape[0]) * int(first["rays_o"].shape[1])
    trainer, loss_fn = Trainer.from_config(cfg, max_rays=max_rays, device=device, weights=weights)
    model = trainer.model
    rcfg = {k: v for k, v in dict(cfg["renderer_config"]).items() if k != "module"}
    two = isinstance(trainer, CoarseFineTrainer)                  # n_importance > 0: render.py:24 hands the renderer every model of the dict
    if rank == 0 and (logger_config or {}).get("print_model_summary", True):
        for m in ([trainer.coarse.model, trainer.fine.model] if two and not trainer.shared else [model]):      # train.py:35-36 (plot_model needs graphviz: not drawn)
            m.summary()
    if _is_mip(cfg["renderer_config"]):                           # a mip run validates as it trains (renderer.py:356)
        renderer = MipRenderer(model=model, **rcfg)
    else:
        renderer = Renderer(model=model, model_fine=trainer.model_fine if two else None, **rcfg)
    lg = dict(i_summary=10, i_print=100, i_img=5e3, i_checkpoint=1e3, max_to_keep=3, keep_every_n_hours=12)
    lg.update({k: v for k, v in (logger_config or {}).items() if k in lg})
    i_print, i_img, i_ckpt, keep, i_summary = int(lg["i_print"]), int(lg["i_img"]), int(lg["i_checkpoint"]), int(lg["max_to_keep"]), int(lg["i_summary"])
    ckpt_dir = os.path.join((logger_config or {}).get("source_path") or target_path, "checkpoints")     # logger.py:15, 30
    os.makedirs(ckpt_dir, exist_ok=True)
    step = 0
    try:                                                          # logger.py:39: restore the newest checkpoint if there is one
        info = trainer.restore(ckpt_dir)
        step = int(info["step"] if info["step"] is not None else info["iterations"])
        print(f"Restored model & optimizer from {info['prefix']}.")
    except FileNotFoundError:
        pass
    dp_comm = None
    if world > 1:
        # Data parallel (one process per GPU; the reference has one): every rank on its own batches, the gradient their mean
        # (`Trainer.train_step` -> `sync_gradients`), so the ranks must start from ONE state -- rank 0's, restored or freshly drawn --
        # and only rank 0 keeps the Logger's files.
        if two:
            raise NotImplementedError("data-parallel coarse + fine training")
        state = [dict(trainer.state_dict(), step=step) if rank == 0 else None]
        with torch.cuda.device(device):
            dist.broadcast_object_list(state, src=0)
        trainer.load_state_dict({k: v for k, v in state[0].items() if k != "step"})
        step = int(state[0]["step"])
        if rank != 0:
            i_print = i_img = i_ckpt = i_summary = 0
        if dist.get_backend() == "nccl":                           # one ncclAllReduce of the gradients a step on the device
            from .dist import Comm
            dp_comm = Comm(device)
    cb = getattr(train_dataset, "composite_bkgd", False) if composite_bkgd is None else composite_bkgd
    bc = getattr(train_dataset, "bkgd_color", (1., 1., 1.)) if bkgd_color is None else bkgd_color
    # CheckpointManager keeps the list of checkpoints it still rotates in the directory's `checkpoint` file (all_model_checkpoint_paths): a
    # resumed run goes on rotating THOSE.  A checkpoint kept for good (keep_every_n_hours) is not in the list and is never deleted; without
    # the file, the newest max_to_keep found are taken as the list (never more: nothing this run cannot account for is removed).
    import re
    listed = [p for p in checkpoint.read_manager_state(ckpt_dir) if os.path.exists(p + ".index")]
    if listed:
        found = [(0, p) for p in listed]
    else:
        found = sorted((int(m.group(1)), os.path.join(ckpt_dir, f[:-6])) for f in os.listdir(ckpt_dir) for m in [re.fullmatch(r"ckpt-(\d+)\.index", f)] if m)
        found = found[-keep:] if keep > 0 else found
    out = {"trainer": trainer, "renderer": renderer, "loss": [], "images": {}, "checkpoints": [p for _, p in found] if rank == 0 else [], "step": step}
    if step >= n_iters:
        if dp_comm is not None:
            dp_comm.close()
        return out
    todo = int(n_iters) - step
    import time
    t_print = time.perf_counter()
    # logger.py:41-44, 60-64, 79-81: the loss every i_summary steps and the validation images as TensorBoard summaries in target_path.  The
    # loss stays on the device until the loop next waits for it anyway (a print, a checkpoint, the end): asking every 10 steps would stall it.
    writer, pending = None, []
    saved_at, kept_for_good = {}, [time.time()]
    if i_summary > 0:
        from .summary import FileWriter
        writer = FileWriter(target_path)

    def flush_summaries():
        for st, value, wall in pending:
            writer.scalar("Loss", float(value.item()), st, wall)
        pending.clear()
        writer.flush()

    for data in train_dataset:                                    # train.py:60: train_dataset.take(n_iters - logger.step)
        if todo <= 0:
            break
        todo -= 1
        pred = trainer.train_step(data, loss_fn, composite_bkgd=cb, bkgd_color=bc, **({"seed": step * world + rank, "comm": dp_comm} if world > 1 else {}))
        step += 1
        if writer is not None and step % i_summary == 0:
            pending.append((step, pred["loss"], time.time()))
            if len(pending) >= 256:
                flush_summaries()
        if i_print > 0 and step % i_print == 0:
            val = float(pred["loss"].item())
            out["loss"].append((step, val))
            now = time.perf_counter()
            print(f"Step {step} | Loss {val:.3g} | Duration {now - t_print:.3g}")      # logger.py:68-73
            t_print = now
        if val_dataset is not None and i_img > 0 and step % i_img == 0:      # logger.py:76-81
            from .render import render_image
            trainer.hand_weights_to_models() if two else model.set_weights_from_trainer(trainer)
            out["images"][step] = [render_image(renderer, val_dataset, view)[0] for view in val_dataset]
            from .render import write_images, util_format                 # logger.py:76-78: media/validation/<step padded to n_iters>/<view>.png
            vdir = os.path.join(target_path, "media", "validation", util_format(step, int(n_iters))[:-4])
            for k, im in enumerate(out["images"][step]):
                write_images(vdir, im[None], k, len(out["images"][step]), int((logger_config or {}).get("downsampling_factor", 1)),
                             bool((logger_config or {}).get("write_exr", False)))
            if writer is not None:
                from .render import image_epilogue
                flush_summaries()
                u8 = [image_epilogue(im, int((logger_config or {}).get("downsampling_factor", 1)), uint8=True)[1] for im in out["images"][step][:3]]
                writer.image("Validation Rendering", torch.stack(u8).cpu().numpy(), step)
        if i_ckpt > 0 and step % i_ckpt == 0:                               # logger.py:84-86
            out["checkpoints"].append(trainer.save(os.path.join(ckpt_dir, f"ckpt-{step}"), step=step))
            saved_at[out["checkpoints"][-1]] = time.time()
            for old in out["checkpoints"][:-keep] if keep > 0 else []:
                # CheckpointManager(keep_checkpoint_every_n_hours=...): one that falls out of the newest `max_to_keep` stays for good if it was
                # saved that long after the last one kept this way (counted from the start of the run)
                if saved_at.get(old, 0.0) - kept_for_good[0] >= 3600.0 * float(lg["keep_every_n_hours"]):
                    kept_for_good[0] = saved_at[old]
                    continue
                for suffix in (".index", ".data-00000-of-00001"):
                    if os.path.exists(old + suffix):
                        os.remove(old + suffix)
            out["checkpoints"] = out["checkpoints"][-keep:] if keep > 0 else out["checkpoints"]
            checkpoint.write_manager_state(ckpt_dir, out["checkpoints"])
            if writer is not None:
                flush_summaries()
    if writer is not None:
        flush_summaries()
        writer.close()
        out["events"] = writer.path
    out["step"] = step
    torch.cuda.synchronize(torch.device("cuda", device))
    if dp_comm is not None:
        dp_comm.close()
    return out
