"""The layer-by-layer training step (`FlexTrainer`, ntx_trainer_create_flex) beside the fused chain (`Trainer`), 1024 rays x 256 samples, perturb,
AlphaLoss(smape, mse) + Adam, timed with HIP events over whole steps:
    A  the carpet model (ParamNerf [1, 6], 8 x 256, skips [4], color_depth 1) through Trainer
    B  the same model through FlexTrainer      (B / A on one model is the ratio that matters)
    C  a plain Nerf 8 x 256 through FlexTrainer
    D  a ParamNerf [1, 6] of width 128, depth 4 through FlexTrainer
    E  the carpet model with param_depth 2 (two Dense(128) layers per parameter branch) through BranchTrainer   (E / B: what the branches cost)
    P0 P1 P2  the carpet model through FlexTrainer with parameter gradients off / beside the weight gradients / alone (`param_gradients=False, True,
              "only"`): P0 is B's step again; P2 has no weight gradient, so no Adam step -- it is `gradients_step` alone, and P0g is P0's
              `gradients_step` alone beside it (P2 / P0g: what the weight gradients are of a step)
    I0 I1 I2  the same with input gradients (dL/d rays_o, rays_d: `input_gradients=False, True, "only"`): I0 is B's step again, I0g its
              `gradients_step` alone, I2 has no weight gradient and no Adam step.  Nothing of the new path has been tuned.
A and B alternate twice in one process so that clock drift shows, and so do the P and the I runs.
    python tools/bench_train_flex.py [--steps 20] [--warmup 5] [--only B] [--out profiles/train_flex/bench.json]
    python tools/bench_train_flex.py --only P --out profiles/train_flex/bench_param_gradients.json
    python tools/bench_train_flex.py --only I --out profiles/input_gradients/bench.json
One JSON line: per run ms a step, ray-samples/s and the fraction of the f32 matrix cores' peak the FLOPs a step needs take (bench.py's
convention for training: 2 x forward + forward less the encoded inputs' rows)."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

PEAK_F32_MFMA = 157.3e12          # MI355X: 256 CUs x 256 f32 matrix FLOPs a clock x 2.4 GHz


def step_flops(model, samples):
    """Forward and weight gradients of every layer, input gradients of all rows but the encoded inputs' (layer 0, pos_map behind a skip, dir_map
    behind the feature layer)."""
    table = model.layer_table()
    macs = model.macs_per_sample()
    names = [name for name, _, _ in table]
    behind_feature = names[names.index("feature") + 1]
    enc = sum((i if name == "trunk0" else i - model.width) * o for name, i, o in table if name.startswith("trunk") or name == behind_feature)
    return 2.0 * samples * (3 * macs - enc)


def param_flops(model, samples, only):
    """`step_flops` with the readers' terms of dL/d parameters (dY . W[parameter-feature rows]^T: trunk layer 0 and the layers behind a skip, the
    layer behind the feature layer); `only`: forward + dX alone, no weight gradient."""
    table = model.layer_table()
    names = [name for name, _, _ in table]
    behind_feature = names[names.index("feature") + 1]
    kq = 1 + 2 * model.param_freq
    terms = sum((model.n_geo if name.startswith("trunk") else model.n_app) * kq * o for name, i, o in table
                if (name.startswith("trunk") and (name == "trunk0" or i > model.width)) or name == behind_feature)
    return step_flops(model, samples) + 2.0 * samples * (terms - (model.macs_per_sample() if only else 0))


def input_flops(model, samples, only):
    """`step_flops` with the readers' terms of dL/d rays (dY . W[first K3 rows]^T: 3 (1 + 2 pos_freq) = 63 columns at trunk layer 0 and the layers
    behind a skip, 3 (1 + 2 dir_freq) = 27 at the layer behind the feature layer); `only`: forward + dX alone, no weight gradient."""
    table = model.layer_table()
    names = [name for name, _, _ in table]
    behind_feature = names[names.index("feature") + 1]
    k3p, k3d = 3 * (1 + 2 * model.pos_freq), 3 * (1 + 2 * model.dir_freq)
    terms = sum((k3p if name.startswith("trunk") else k3d) * o for name, i, o in table
                if (name.startswith("trunk") and (name == "trunk0" or i > model.width)) or name == behind_feature)
    return step_flops(model, samples) + 2.0 * samples * (terms - (model.macs_per_sample() if only else 0))


def time_steps(tr, args, loss, steps, warmup, gradients_only=False, **kw):
    one = tr.gradients_step if gradients_only else tr.step
    for _ in range(warmup):
        one(*args, loss, **kw)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        one(*args, loss, **kw)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, help="one of A B C D E (a profiler's run), P: the parameter-gradient runs, or I: the input-gradient runs")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.loss import AlphaLoss
    from nerf_tex_amd.model import Nerf, ParamNerf
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer, Trainer
    B, R, S = 4, 256, 256
    n = B * R
    f = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    rng = np.random.default_rng(0)
    color = rng.uniform(0, 1, (n, 3)).astype(np.float32); alpha = rng.uniform(0, 1, n).astype(np.float32)
    params = np.asarray([f["params"]] * B, np.float32) * rng.uniform(0.8, 1.2, (B, 7)).astype(np.float32)
    dev = torch.device("cuda", 0)
    d = lambda x: torch.as_tensor(x, device=dev)
    loss = AlphaLoss(loss_fn="network.loss.smape", alpha_loss_fn="network.loss.mse")
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    seeded = lambda m: (m.set_blob(synthetic.synthetic_weights(m.layer_table(), seed=0, dense_media=True)), m)[1]
    carpet = seeded(ParamNerf(emb(10), emb(4), emb(4), [1, 6])["model"])
    runs = {"A": (Trainer, carpet), "B": (FlexTrainer, carpet), "C": (FlexTrainer, seeded(Nerf(emb(10), emb(4))["model"])),
            "D": (FlexTrainer, seeded(ParamNerf(emb(10), emb(4), emb(4), [1, 6], width=128, depth=4)["model"])),
            "E": (BranchTrainer, seeded(ParamNerf(emb(10), emb(4), emb(4), [1, 6], param_depth=2)["model"]))}
    modes = {"P0": False, "P0g": False, "P1": True, "P2": "only"}
    runs.update({k: (FlexTrainer, carpet) for k in modes})
    imodes = {"I0": False, "I0g": False, "I1": True, "I2": "only"}
    runs.update({k: (FlexTrainer, carpet) for k in imodes})
    p_order, i_order = ["P0", "P0g", "P1", "P2"] * 2, ["I0", "I0g", "I1", "I2"] * 2
    order = p_order if a.only == "P" else i_order if a.only == "I" else [a.only] if a.only else ["A", "B", "A", "B", "C", "D", "E", "B", "E"] + p_order
    out = {"what": "training step, 1024 rays x 256 samples, perturb, AlphaLoss(smape, mse) + Adam; HIP events", "steps": a.steps, "warmup": a.warmup, "runs": []}
    trainers = {}
    for key in order:
        cls, model = runs[key]
        if key not in trainers:
            trainers[key] = cls(model, max_rays=n, n_samples=S, lrate=5e-4, lrate_decay=500, perturb=True, **({"param_gradients": modes[key]} if modes.get(key) else {}),
                                **({"input_gradients": imodes[key]} if imodes.get(key) else {}))
        batch = (d(ro), d(rd), d(t), d(params) if model.n_params else None, d(cone), d(color), d(alpha))
        sec = time_steps(trainers[key], batch, loss, a.steps, a.warmup, gradients_only=key in ("P0g", "P2", "I0g", "I2"), rays_per_param_row=R)
        fl = param_flops(model, n * S, key == "P2") if modes.get(key) else input_flops(model, n * S, key == "I2") if imodes.get(key) else step_flops(model, n * S)
        out["runs"].append({"run": key, "trainer": cls.__name__,
                            "model": f"{'Nerf' if model.kind else 'ParamNerf'} {model.depth} x {model.width}" + (f" param_depth {model.param_depth}" if model.param_depth else ""), "ms_step": 1e3 * sec,
                            "ray_samples_per_s": n * S / sec, "gflop_step": fl / 1e9, "fraction_of_f32_mfma_peak": fl / sec / PEAK_F32_MFMA})
    ms = lambda k: [r["ms_step"] for r in out["runs"] if r["run"] == k]
    if ms("A") and ms("B"):
        out["B_over_A"] = float(np.mean(ms("B")) / np.mean(ms("A")))
    if ms("B") and ms("E"):
        out["E_over_B"] = float(np.mean(ms("E")) / np.mean(ms("B")[-len(ms("E")):]))      # the B runs next to the E runs
    if ms("P0") and ms("P1") and ms("P2"):
        out["P1_over_P0"] = float(np.mean(ms("P1")) / np.mean(ms("P0")))
        out["P2_over_P0g"] = float(np.mean(ms("P2")) / np.mean(ms("P0g")))
        out["weight_gradient_share_of_flops"] = float(1.0 - param_flops(carpet, n * S, True) / param_flops(carpet, n * S, False))
    if ms("I0") and ms("I1") and ms("I2"):
        out["I1_over_I0"] = float(np.mean(ms("I1")) / np.mean(ms("I0")))
        out["I2_over_I0g"] = float(np.mean(ms("I2")) / np.mean(ms("I0g")))
        out["input_gradient_gflop_step"] = float((input_flops(carpet, n * S, False) - step_flops(carpet, n * S)) / 1e9)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
