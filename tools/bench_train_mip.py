"""One training step of an IPE ParamNerf [1, 3] under the MipRenderer (4 images x 256 rays x 256 cone segments, perturb, raw_noise_std 0.1,
blur_idx 0, AlphaLoss(smape, mse)) beside the Fourier step of config_grass_filtered_train.py on the same batch shape.  Both on one synthetic
batch, 10 warm steps each, timed as a whole on the device.
    python tools/bench_train_mip.py [--steps 10] [--warmup 3]
One JSON line: ms a step of each and the fraction of the f32 matrix cores' peak the FLOPs of each step take."""

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PEAK_F32_MFMA = 157.3e12          # MI355X: 256 CUs x 256 f32 matrix FLOPs a clock x 2.4 GHz


def step_flops(table, samples):
    """The FLOPs a step NEEDS: the forward and the weight gradients of every layer, the input gradients of all but the
    encoded inputs (layer 0, the skip's pos_map rows and the first colour layer's dir_map rows take none)."""
    macs = sum(i * o for _, i, o in table)
    rows = dict((name, i) for name, i, _ in table)
    kp, kd = rows["trunk0"], rows["color_hidden0"] - 256
    return 2.0 * samples * (2 * macs + macs - 256 * (2 * kp + kd))


def time_steps(tr, args, loss, steps, warmup, **kw):
    for _ in range(warmup):
        tr.step(*args, loss, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(*args, loss, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.loss import AlphaLoss
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.train import Trainer
    B, R, S = 4, 256, 256
    n = B * R
    f = synthetic.FAMILIES["grass_filtered"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    rng = np.random.default_rng(0)
    color = rng.uniform(0, 1, (n, 3)).astype(np.float32); alpha = rng.uniform(0, 1, n).astype(np.float32)
    dev = torch.device("cuda", 0)
    d = lambda x: torch.as_tensor(x, device=dev)
    loss = AlphaLoss(loss_fn="network.loss.smape", alpha_loss_fn="network.loss.mse")
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    ipe = {"module": "network.layer.IntegratedPositionalEncoding", "n_freq_bands": 10}
    out = {"what": "training step, 4 x 256 rays x 256 samples, perturb, raw_noise_std 0.1, blur_idx 0, AlphaLoss(smape, mse) + Adam", "steps": a.steps}
    for name, model, P in (("fourier_grass_filtered", ParamNerf(emb(10), emb(4), emb(4), [2, 3])["model"], 5),
                           ("ipe_mip_1_3", ParamNerf(ipe, emb(4), emb(4), [1, 3], n_pos=6)["model"], 5)):
        model.set_blob(synthetic.synthetic_weights(model.layer_table(), seed=0, dense_media=True))
        params = rng.uniform(0.2, 1.5, (B, P)).astype(np.float32)
        tr = Trainer(model, max_rays=n, n_samples=S, lrate=5e-4, lrate_decay=500, perturb=True, blur_idx=0, raw_noise_std=0.1)
        batch = (d(ro), d(rd), d(t), d(params), d(cone), d(color), d(alpha))
        sec = time_steps(tr, batch, loss, a.steps, a.warmup, rays_per_param_row=R)
        fl = step_flops(model.layer_table(), n * S)
        out[name] = {"ms_step": 1e3 * sec, "gflop_step": fl / 1e9, "fraction_of_f32_mfma_peak": fl / sec / PEAK_F32_MFMA}
    out["ipe_over_fourier"] = out["ipe_mip_1_3"]["ms_step"] / out["fourier_grass_filtered"]["ms_step"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
