"""What the distortion loss on the compositing weights costs, on an MI355X, timed with HIP events; every side of a comparison in ONE run,
alternating over `--rounds` rounds, a window is `--steps` calls between two events, a side's figure is the MEDIAN of its windows (min and max
beside it) -- tools/bench_train_weight_loss.py's protocol.  Peak memory of a side: `torch.cuda.max_memory_allocated` over its windows, less
what was allocated before them.
  (a) loss + gradient at the weights at 1024 x 256 and 256 x 1024, three statements of the same numbers:
        entry     `nerf_tex_amd.loss.ray_distortion(..., with_grad=True)`: one launch of `ntx_ray_distortion`
        pairwise  the textbook torch expression with [N, S, S] intermediates + torch.autograd.grad
        cumsum    the O(S) form with `torch.cumsum` (shifted by the first depth) + torch.autograd.grad
  (b) `gradients_step` of the fused chain on the carpet model at 1024 x 256, perturb, under
        mse         `as_callable(NerfLoss())`
        distortion  `Distortion(that, weight=0.01)`
        pairwise    the same loss with the pairwise torch term
    python tools/bench_ray_distortion.py [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/ray_distortion/bench.json]
One JSON line.  No ratio is promised: the entry is bound by launch and memory latency (a call at 1024 x 256 moves 3 MB)."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_train_custom_loss import time_steps  # noqa: E402


def rays(n, S, seed=0):
    """(w, z) float32: jittered depths on rays of length 0.5 - 2 from 2 - 6, the composite's weights of a smooth random density."""
    rng = np.random.default_rng(seed)
    lo, sp = rng.uniform(2, 6, (n, 1)), rng.uniform(0.5, 2, (n, 1))
    z = lo + sp * (np.arange(S)[None] + rng.uniform(0.05, 0.95, (n, S))) / S
    d = np.diff(z, axis=1); d = np.concatenate([d, d[:, -1:]], 1)
    sigma = rng.uniform(0.5, 4, (n, 1)) / sp * np.exp(-(((z - lo) / sp - rng.uniform(0.3, 0.7, (n, 1))) / 0.35) ** 2) * rng.uniform(0.5, 1.5, (n, S))
    a = 1 - np.exp(-sigma * d)
    T = np.cumprod(1 - a + 1e-10, 1)
    return (a * np.concatenate([np.ones((n, 1)), T[:, :-1]], 1)).astype(np.float32), z.astype(np.float32)


def widths_of(z):
    d = z[:, 1:] - z[:, :-1]
    return torch.cat([d, d[:, -1:]], 1)


def pairwise(w, z):
    return (w[:, :, None] * w[:, None, :] * (z[:, :, None] - z[:, None, :]).abs()).sum((1, 2)) + (w * w * widths_of(z)).sum(1) / 3.0


def by_cumsum(w, z):
    m = z - z[:, :1]
    wm = w * m
    W_lt, M_lt = torch.cumsum(w, 1) - w, torch.cumsum(wm, 1) - wm
    return 2.0 * (w * (m * W_lt - M_lt)).sum(1) + (w * w * widths_of(z)).sum(1) / 3.0


def with_autograd(fn):
    def one(w, z):
        leaf = w.detach().requires_grad_(True)
        val = fn(leaf, z)
        (g,) = torch.autograd.grad(val.sum(), leaf)
        return val.detach(), g
    return one


def measure(sides, steps, warmup, rounds):
    """{side: ms median / min / max, peak MB} of callables that alternate over the rounds."""
    windows, peak = {k: [] for k in sides}, {k: 0 for k in sides}
    for rnd in range(rounds):
        for key, one in sides.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            windows[key].append(1e3 * time_steps(one, steps, warmup if rnd == 0 else 1))
            peak[key] = max(peak[key], torch.cuda.max_memory_allocated() - base)
    return {k: {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "peak_mb": peak[k] / 2 ** 20} for k, v in windows.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.loss import Distortion, NerfLoss, as_callable, ray_distortion
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.train import Trainer
    dev = torch.device("cuda", 0)
    d = lambda x: torch.as_tensor(x, device=dev)
    rel = lambda x, ref: float((x.double() - ref.double()).abs().max() / ref.double().abs().max())
    out = {"what": "the distortion loss on the compositing weights: (a) loss + gradient by the entry, by the pairwise torch expression and by a torch.cumsum expression, "
                   "both with autograd; (b) gradients_step of the fused chain, carpet model, 1024 x 256, perturb, under mse, Distortion(mse) and mse + the pairwise term; "
                   "HIP events, medians of the rounds' windows, peak memory by torch.cuda.max_memory_allocated",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "entry": {}, "step": {}}
    for n, S in ((1024, 256), (256, 1024)):
        w, z = (d(x) for x in rays(n, S))
        sides = {"entry": lambda: ray_distortion(w, z, with_grad=True), "pairwise": lambda: with_autograd(pairwise)(w, z), "cumsum": lambda: with_autograd(by_cumsum)(w, z)}
        res = measure(sides, a.steps, a.warmup, a.rounds)
        got = {k: one() for k, one in sides.items()}
        ref = with_autograd(pairwise)(w.double(), z.double())
        for k in sides:
            res[k]["loss_rel_linf_vs_float64"], res[k]["grad_rel_linf_vs_float64"] = rel(got[k][0], ref[0]), rel(got[k][1], ref[1])
        res["bytes_moved_by_the_entry"] = 4 * (3 * n * S + n)
        out["entry"][f"{n}x{S}"] = res
        del got, ref
    B, R, S = 4, 256, 256
    n = B * R
    f = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    rng = np.random.default_rng(0)
    color, alpha = rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    params = np.asarray([f["params"]] * B, np.float32) * rng.uniform(0.8, 1.2, (B, 7)).astype(np.float32)
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    carpet = ParamNerf(emb(10), emb(4), emb(4), [1, 6])["model"]
    carpet.set_blob(synthetic.synthetic_weights(carpet.layer_table(), seed=0, dense_media=True))
    batch = (d(ro), d(rd), d(t), d(params), d(cone), d(color), d(alpha))
    mse = as_callable(NerfLoss())

    def with_pairwise(color_true, alpha_true, color_pred, alpha_pred, weights, z_vals):
        return mse(color_true=color_true, alpha_true=alpha_true, color_pred=color_pred, alpha_pred=alpha_pred) + \
            0.01 * (pairwise(weights, z_vals) / (z_vals[:, -1] - z_vals[:, 0])).mean()
    losses = {"mse": mse, "distortion": Distortion(mse, weight=0.01), "pairwise": with_pairwise}
    tr = Trainer(carpet, max_rays=n, n_samples=S, perturb=True)
    sides = {k: (lambda loss=loss, seed=None: tr.gradients_step(*batch, loss, rays_per_param_row=R, seed=seed)) for k, loss in losses.items()}
    res = measure(sides, a.steps, a.warmup, a.rounds)
    grads = {}
    for k, one in sides.items():
        val = one(seed=5)[0]
        torch.cuda.synchronize()
        grads[k] = tr.gradients().copy()
        res[k]["loss"] = float(val.item())
    res["distortion_over_mse"] = res["distortion"]["ms_median"] / res["mse"]["ms_median"]
    res["pairwise_over_mse"] = res["pairwise"]["ms_median"] / res["mse"]["ms_median"]
    res["gradient_rel_linf_distortion_vs_pairwise"] = float(np.abs(grads["distortion"] - grads["pairwise"]).max() / np.abs(grads["pairwise"]).max())
    res["term_moves_the_gradient_by"] = float(np.abs(grads["distortion"] - grads["mse"]).max() / np.abs(grads["mse"]).max())
    out["step"]["Trainer_1024x256"] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
