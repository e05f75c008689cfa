"""What a loss written in PyTorch costs a training step: the carpet model (ParamNerf [1, 6], 8 x 256, skips [4], color_depth 1) at 1024 rays x 256
samples, perturb, gradients only (no Adam: both sides leave the same gradient), timed with HIP events:
    A  `gradients_step` with NerfLoss(mse): the fused composite + loss + adjoint kernel
    B  `forward` + torch mse on the predictions + torch autograd for the two cotangents + `backward`: a second pass over the composite
       (composite_adjoint_kernel recomputes the transmittance) and torch's small kernels between the two native halves
for the fused chain (`Trainer`) and layer by layer (`FlexTrainer`).  A and B alternate twice in one process so that clock drift shows
(tools/bench_train_flex.py's conventions: 5 + 20 steps, whole steps between two events).
    python tools/bench_train_custom_loss.py [--steps 20] [--warmup 5] [--only A] [--out profiles/custom_loss/bench.json]
One JSON line: per run ms a step and ray-samples/s, and B / A per trainer.  `--only A`: what a library from before the two entries can run too
(NERFTEX_LIB, or this file in the parent's tree): the yardstick B / A is read against."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def torch_mse(color_true, alpha_true, color_pred, alpha_pred):
    return torch.mean((color_true - color_pred) ** 2)


def time_steps(one, steps, warmup):
    for _ in range(warmup):
        one()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        one()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["A"], help="the fused side alone, twice")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.loss import NerfLoss
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.train import FlexTrainer, Trainer
    B, R, S = 4, 256, 256
    n = B * R
    f = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    rng = np.random.default_rng(0)
    color = rng.uniform(0, 1, (n, 3)).astype(np.float32); alpha = rng.uniform(0, 1, n).astype(np.float32)
    params = np.asarray([f["params"]] * B, np.float32) * rng.uniform(0.8, 1.2, (B, 7)).astype(np.float32)
    dev = torch.device("cuda", 0)
    d = lambda x: torch.as_tensor(x, device=dev)
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    carpet = ParamNerf(emb(10), emb(4), emb(4), [1, 6])["model"]
    carpet.set_blob(synthetic.synthetic_weights(carpet.layer_table(), seed=0, dense_media=True))
    batch = (d(ro), d(rd), d(t), d(params), d(cone), d(color), d(alpha))
    fused = NerfLoss("network.loss.mse")
    out = {"what": "gradients of one step, carpet model, 1024 rays x 256 samples, perturb; A fused NerfLoss(mse), B forward + torch mse + backward; HIP events",
           "steps": a.steps, "warmup": a.warmup, "runs": []}
    for cls in (Trainer, FlexTrainer):
        tr = cls(carpet, max_rays=n, n_samples=S, perturb=True)
        sides = {"A": lambda seed=None: tr.gradients_step(*batch, fused, rays_per_param_row=R, seed=seed),
                 "B": lambda seed=None: tr.gradients_step(*batch, torch_mse, rays_per_param_row=R, seed=seed)}
        for key in ("A", "A") if a.only else ("A", "B", "A", "B"):
            sec = time_steps(sides[key], a.steps, a.warmup)
            out["runs"].append({"run": key, "trainer": cls.__name__, "ms_step": 1e3 * sec, "ray_samples_per_s": n * S / sec})
        if a.only:
            continue
        ms = lambda k: [r["ms_step"] for r in out["runs"] if r["run"] == k and r["trainer"] == cls.__name__]
        out[f"B_over_A_{cls.__name__}"] = float(np.mean(ms("B")) / np.mean(ms("A")))
        # the two ways leave one gradient on one jitter seed (torch forms mse's cotangents in another order than the fused kernel: the last bits;
        # with the kernel's own order tests/test_gpu_custom_loss.py holds the two to the same bits)
        sides["A"](5); ga = tr.gradients()
        sides["B"](5); gb = tr.gradients()
        out[f"gradients_rel_linf_{cls.__name__}"] = float(np.abs(ga - gb).max() / np.abs(ga).max())
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
