"""What fitting camera poses costs: the carpet model, 4 poses x 256 rays x 256 samples, look-at cameras around the carpet family's box, an MSE loss
in torch.  HIP events, all sides in ONE process on the same buffers, for the fused chain and for the layer-by-layer trainer (both
input_gradients="only"):
    posed_rays    `ray_sampler.posed_rays` alone (`ntx_generate_rays_posed`: the rays of the four images in one launch)
    adjoint       `ntx_generate_rays_posed_adjoint` alone, on given cotangents
    step          the plain `forward` + `backward` of the inputs-only trainer on fixed rays, cotangents given
    fit_iter      one iteration of `PoseFitter.fit`: compose_poses, posed_rays, the same step through DifferentiableRender, the loss in torch, the
                  trainer's ray gradients, the adjoint, torch through the matrix exponential, Adam -- timed as one `fit` call of `--steps`
                  iterations (the optimiser's construction and the batch's upload are in the window)
The sides alternate over `--rounds` rounds; a side's figure is the MEDIAN of its windows (min and max beside it).
    python tools/bench_pose_fit.py [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/pose_fit/bench.json]
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
    ap.add_argument("--poses", type=int, default=4)
    ap.add_argument("--rays", type=int, default=256, help="rays per pose")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import _lib, synthetic
    from nerf_tex_amd.dataset import look_at
    from nerf_tex_amd.fit import PoseFitter
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.proxy import AABB
    dev = torch.device("cuda", 0)
    fam = synthetic.FAMILIES["carpet"]
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    model = ParamNerf(emb(10), emb(4), emb(4), list(fam["n_parameters"]))["model"]
    model.set_blob(synthetic.synthetic_weights(model.layer_table(), seed=0, dense_media=True))
    B, R, S, H, W = a.poses, a.rays, a.samples, 800, 800
    n = B * R
    rng = np.random.default_rng(0)
    cam = np.asarray(fam["cam"], np.float64)
    turn = lambda k: np.asarray([[np.cos(k), -np.sin(k), 0], [np.sin(k), np.cos(k), 0], [0, 0, 1]])
    c2w = np.stack([look_at((turn(2 * np.pi * k / B) @ cam).astype(np.float32)) for k in range(B)]).astype(np.float32)
    focal = np.full(B, W / np.tan(fam["angle"] / 2) / 2, np.float32)
    side = int(np.ceil(np.sqrt(R)))
    r0 = (H - side) // 2                                                          # a window at the image centre: every ray hits the box
    rows, cols = np.meshgrid(np.arange(r0, r0 + side), np.arange(r0, r0 + side), indexing="ij")
    loc = np.tile(np.stack([rows.ravel(), cols.ravel()], -1)[None, :R].astype(np.float32), (B, 1, 1))
    params = np.tile(np.asarray([fam["params"]], np.float32), (B, 1))
    up = lambda x: torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(dev)
    mse = lambda color_true, alpha_true, color_pred, alpha_pred: torch.mean((color_pred - color_true) ** 2) + torch.mean((alpha_pred - alpha_true) ** 2)
    d_color, d_alpha = up(rng.normal(size=(n, 3)) / n), up(rng.normal(size=n) / n)
    g_o, g_d = up(rng.normal(size=(n, 3))), up(rng.normal(size=(n, 3)))
    loc_d, c2w_d, focal_d, params_d = up(loc), up(c2w), up(focal), up(params)
    poses34 = c2w_d[:, :3, :].contiguous()
    d_poses, d_focal = torch.empty((B, 3, 4), device=dev), torch.empty((B,), device=dev)
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream

    def adjoint():
        _lib.check(_lib.lib.ntx_generate_rays_posed_adjoint(poses34.data_ptr(), focal_d.data_ptr(), B, H, W, loc_d.data_ptr(), n, R, 0, g_o.data_ptr(), g_d.data_ptr(),
                                                            d_poses.data_ptr(), d_focal.data_ptr(), stream()))

    out = {"what": f"carpet model, {B} poses x {R} rays x {S} samples, input_gradients only: posed_rays and its adjoint alone, the plain forward + backward of the trainer, one "
                   "PoseFitter iteration; HIP events, median of the rounds' windows",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "poses": B, "rays_per_pose": R, "samples": S, "trainers": {}}
    for name, fused in (("fused_chain", True), ("layer_by_layer", False)):
        fitter = PoseFitter(model, H, W, focal, proxy=AABB(fam["b_0"], fam["b_1"]), n_samples=S, max_rays=n, lrate=1e-4, fused=fused)
        with torch.no_grad():
            ro, rd, t, cone = fitter.rays(loc_d, c2w_d, focal_d)
            hits = int(torch.isfinite(t[:, 0]).sum().item())
            cone1 = cone.reshape(-1).contiguous()
            color, alpha = fitter.trainer.forward(ro, rd, t, params_d, cone1, rays_per_param_row=R)
        batch = dict(image_plane_loc=loc_d, parameters=params_d, color=(0.9 * color).reshape(B, R, 3).clone(), alpha=(0.9 * alpha).reshape(B, R).clone())

        def step():
            fitter.trainer.forward(ro, rd, t, params_d, cone1, rays_per_param_row=R)
            fitter.trainer.backward(d_color, d_alpha)

        sides = {"posed_rays": (lambda: fitter.rays(loc_d, c2w_d, focal_d), a.steps), "adjoint": (adjoint, a.steps), "step": (step, a.steps),
                 "fit_iter": (lambda: fitter.fit(batch, mse, c2w_d, n_iters=a.steps), 1)}
        windows = {k: [] for k in sides}
        for rnd in range(a.rounds):
            for key, (one, reps) in sides.items():
                warm = (a.warmup if rnd == 0 else 1) if reps > 1 else 1
                windows[key].append(1e3 * time_steps(one, reps, warm) / (1 if reps > 1 else a.steps))
        stat = lambda w: {"ms_median": float(np.median(w)), "ms_min": float(min(w)), "ms_max": float(max(w))}
        res = {"trainer": type(fitter.trainer).__name__, "rays_that_hit": hits, "sides": {k: stat(w) for k, w in windows.items()}}
        med = lambda k: res["sides"][k]["ms_median"]
        res["fit_iter_over_step"] = med("fit_iter") / med("step")
        res["fit_iter_less_step_ms"] = med("fit_iter") - med("step")
        out["trainers"][name] = res
        del fitter
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
