"""What fitting a parameter texture costs: the bench scene of the instancer (48 x 48 patches on a waving sheet that is also the instancer mesh,
patch box x 0.09, 'nearest', steps of 0.002) with a neutral parameter texture and a lookup per step, 1024 rays of the carpet config's first camera
x 256 samples, the carpet model on the fused chain with param_gradients="only".  HIP events, all sides in ONE process on the same buffers:
    model_input   `Instancer.get_model_input` with the texture's per-step lookups (the march)
    sample_uv     `Instancer.sample_uv` on its t and dists (`ntx_instancer_sample_uv`)
    step          `forward_instanced` + `backward` of the trainer on those buffers, cotangents given: the plain instanced step
    fit_iter      one iteration of `TextureFitter.fit` (12 x 16 texels): the march, apply_textures, the same step through
                  DifferentiableInstanceRender, an MSE loss in torch, the scatter-add into the texels, Adam, the clamp -- timed as one `fit` call of
                  `--steps` iterations (its single sample_uv and the optimiser's construction are in the window)
The sides alternate over `--rounds` rounds; a side's figure is the MEDIAN of its windows (min and max beside it).
    python tools/bench_texture_fit.py [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/texture_fit/bench.json]
One JSON line."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_train_custom_loss import time_steps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--side", type=int, default=32, help="the rays are a side x side window of the 800 x 800 grid")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.dataset import look_at
    from nerf_tex_amd.fit import TextureFitter
    from nerf_tex_amd.instancer import Instancer, neutral_texture
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.proxy import AABB
    from nerf_tex_amd.ray_sampler import Proxy
    from nerf_tex_amd.train import Trainer
    dev = torch.device("cuda", 0)
    fam = synthetic.FAMILIES["carpet"]
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    model = ParamNerf(emb(10), emb(4), emb(4), list(fam["n_parameters"]))["model"]
    model.set_blob(synthetic.synthetic_weights(model.layer_table(), seed=0))
    side, S, step_size, patch_scale, density_scale, shape = a.side, a.samples, 0.002, 0.09, 400.0, (12, 16)
    n = side * side
    tr_, v, f = synthetic.patch_sheet(48)
    uv = ((v[:, :2] + 1.5) / 3.0).astype(np.float32)
    b_0, b_1 = synthetic.PATCH_BOX
    inst = Instancer(b_0, b_1, textures=[neutral_texture(), "", "", "", "light"], transformations=tr_, instance_sampling_method="nearest", instancer_mesh=(v, f, uv),
                     patch_scale=patch_scale, n_texture_samples=10 ** 6, min_texture_samples=8)
    focal = 800 / np.tan(fam["angle"] / 2) / 2
    r0 = (800 - side) // 2
    rows, cols = np.meshgrid(np.arange(r0, r0 + side), np.arange(r0, r0 + side), indexing="ij")
    loc = torch.as_tensor(np.stack([rows.ravel(), cols.ravel()], -1).astype(np.float32), device=dev)
    ro, rd, t, cone = Proxy(800, 800, focal, AABB([-1.7, -1.7, -.3], [1.7, 1.7, .4]))(loc, look_at(np.asarray(fam["cam"], np.float32)), device=dev)
    params = torch.as_tensor(np.asarray([fam["params"]], np.float32), device=dev).repeat(n, 1).contiguous()
    cone = cone.reshape(n).contiguous()
    trainer = Trainer(model, max_rays=n, n_samples=S, perturb=False, param_gradients="only", instanced=True)
    fitter = TextureFitter(trainer, inst, [shape], lrate=1e-2, patch_scale=patch_scale, density_scale=density_scale, step_size=step_size, seed=1)
    rng = np.random.default_rng(0)
    d_color, d_alpha = (torch.as_tensor(x, device=dev) for x in (rng.normal(size=(n, 3)).astype(np.float32) / n, rng.normal(size=n).astype(np.float32) / n))
    bufs = inst.get_model_input(ro, rd, params, S, step_size, seed=1)
    found = inst.sample_uv(ro, rd, bufs, step_size)[1]
    color, alpha = trainer.forward_instanced(bufs, cone, patch_scale=patch_scale, density_scale=density_scale, hit=inst.last_hit)
    batch = dict(rays_o=ro, rays_d=rd, parameters=params, cone_scale=cone, color_true=(0.9 * color).clone(), alpha_true=(0.9 * alpha).clone())
    mse = lambda color_true, alpha_true, color_pred, alpha_pred: torch.mean((color_pred - color_true) ** 2) + torch.mean((alpha_pred - alpha_true) ** 2)

    def step():
        trainer.forward_instanced(bufs, cone, patch_scale=patch_scale, density_scale=density_scale, hit=inst.last_hit)
        trainer.backward(d_color, d_alpha)

    sides = {"model_input": (lambda: inst.get_model_input(ro, rd, params, S, step_size, seed=1), a.steps),
             "sample_uv": (lambda: inst.sample_uv(ro, rd, bufs, step_size), a.steps),
             "step": (step, a.steps),
             "fit_iter": (lambda: fitter.fit(batch, mse, init=0.5, n_iters=a.steps), 1)}
    windows = {k: [] for k in sides}
    for rnd in range(a.rounds):
        for key, (one, reps) in sides.items():
            warm = (a.warmup if rnd == 0 else 1) if reps > 1 else 1
            windows[key].append(1e3 * time_steps(one, reps, warm) / (1 if reps > 1 else a.steps))
    stat = lambda w: {"ms_median": float(np.median(w)), "ms_min": float(min(w)), "ms_max": float(max(w))}
    out = {"what": f"bench scene (48 x 48 patches, {f.shape[0]} triangles), {n} rays x {S} samples, step {step_size}: the march with a neutral texture's per-step lookups, "
                   "ntx_instancer_sample_uv, forward_instanced + backward on the fused chain (param_gradients only), one TextureFitter iteration (12 x 16 texels); HIP events, "
                   "median of the rounds' windows",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "rays": n, "samples": S,
           "in_patch_samples": int((bufs[3] > 0).sum().item()), "found_samples": int(found.sum().item()), "live": int(trainer.last_live),
           "sides": {k: stat(w) for k, w in windows.items()}}
    med = lambda k: out["sides"][k]["ms_median"]
    out["sample_uv_over_model_input"] = med("sample_uv") / med("model_input")
    out["fit_iter_over_step"] = med("fit_iter") / med("step")
    out["fit_iter_less_march_and_step_ms"] = med("fit_iter") - med("model_input") - med("step")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
