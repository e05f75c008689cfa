"""What a loss on the compositing weights costs a training step: the carpet model (ParamNerf [1, 6], 8 x 256, skips [4], color_depth 1) at 1024
rays x 256 samples, perturb, gradients only (no Adam), timed with HIP events, both sides in ONE run on the same trainer:
    B  `forward` + torch mse on the predictions + torch autograd for the two cotangents + `backward` (tools/bench_train_custom_loss.py's side B:
       a step under a loss of the predictions, as it was before the weights could take one)
    W  the same with the weights: the step's depths placed first (`ntx_sample_depths`), `forward(return_weights=True)`, torch mse +
       0.1 * mse(`expected_depth`, a depth target) and autograd for three cotangents, `backward(d_color, d_alpha, d_weights)` -- two more [N][S]
       float arrays through the composite (the weights out, their cotangent in) and torch's kernels on them
for the fused chain (`Trainer`) and layer by layer (`FlexTrainer`).  Both sides go through `gradients_step` with a callable loss; B and W alternate
over `--rounds` rounds, a window is `--steps` whole steps between two events after `--warmup` steps, a side's figure is the MEDIAN of its windows
(min and max beside it).
    python tools/bench_train_weight_loss.py [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/weight_losses/bench.json]
One JSON line: per trainer and side ms a step (median, min, max) and W / B."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_train_custom_loss import time_steps, torch_mse  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.loss import expected_depth
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.train import FlexTrainer, Trainer
    B, R, S = 4, 256, 256
    n = B * R
    f = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    rng = np.random.default_rng(0)
    color = rng.uniform(0, 1, (n, 3)).astype(np.float32); alpha = rng.uniform(0, 1, n).astype(np.float32)
    params = np.asarray([f["params"]] * B, np.float32) * rng.uniform(0.8, 1.2, (B, 7)).astype(np.float32)
    depth = (t[:, 0] + rng.uniform(0.2, 0.8, n) * (t[:, 1] - t[:, 0])).astype(np.float32)
    dev = torch.device("cuda", 0)
    d = lambda x: torch.as_tensor(x, device=dev)
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    carpet = ParamNerf(emb(10), emb(4), emb(4), [1, 6])["model"]
    carpet.set_blob(synthetic.synthetic_weights(carpet.layer_table(), seed=0, dense_media=True))
    batch = (d(ro), d(rd), d(t), d(params), d(cone), d(color), d(alpha))
    depth_true = d(depth)

    def mse_and_depth(color_true, alpha_true, color_pred, alpha_pred, weights, z_vals):
        return torch.mean((color_true - color_pred) ** 2) + 0.1 * torch.mean((expected_depth(weights, z_vals) - depth_true) ** 2)

    out = {"what": "gradients of one step, carpet model, 1024 rays x 256 samples, perturb; B forward + torch mse + backward, W the same with return_weights and "
                   "mse + 0.1 mse(expected_depth, target) + the weight cotangent; HIP events, median of the rounds' windows",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "trainers": {}}
    for cls in (Trainer, FlexTrainer):
        tr = cls(carpet, max_rays=n, n_samples=S, perturb=True)
        sides = {"B": lambda seed=None: tr.gradients_step(*batch, torch_mse, rays_per_param_row=R, seed=seed),
                 "W": lambda seed=None: tr.gradients_step(*batch, mse_and_depth, rays_per_param_row=R, seed=seed)}
        windows = {k: [] for k in sides}
        for rnd in range(a.rounds):
            for key, one in sides.items():
                windows[key].append(1e3 * time_steps(one, a.steps, a.warmup if rnd == 0 else 1))
        res = {k: {"ms_step_median": float(np.median(w)), "ms_step_min": float(min(w)), "ms_step_max": float(max(w))} for k, w in windows.items()}
        res["W_over_B"] = res["W"]["ms_step_median"] / res["B"]["ms_step_median"]
        # the depth term is a real share of the gradient, and a step that never names the weights is the step it was
        sides["B"](5); gb = tr.gradients()
        sides["W"](5); gw = tr.gradients()
        sides["B"](5); gb2 = tr.gradients()
        res["depth_term_rel_linf"] = float(np.abs(gw - gb).max() / np.abs(gb).max())
        res["B_reproduced_after_W"] = bool(np.array_equal(gb, gb2))
        out["trainers"][cls.__name__] = res
        del tr
        torch.cuda.synchronize()
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
