"""Parameter and ray gradients on the fused chain (`Trainer(param_gradients=, input_gradients=)`, ntx_trainer_enable_gradients) beside the
layer-by-layer trainer's (`FlexTrainer`), the carpet model (ParamNerf [1, 6], 8 x 256, skips [4], color_depth 1) at 1024 rays x 256 samples,
perturb, AlphaLoss(smape, mse), timed with HIP events over whole steps (tools/bench_train_flex.py's protocol):
    Z      the chain with nothing asked for, `Trainer(model, ...)` as a library from before the entry makes it: step + Adam
    CP0 CP0g CP1 CP2   the chain with parameter gradients off / off, `gradients_step` alone / beside the weight gradients / alone ("only": no
                       weight gradient, so no Adam step -- `gradients_step` alone, as CP0g)
    CI0 CI0g CI1 CI2   the same with input gradients (dL/d rays_o, rays_d)
    FP1 FP2 FI1 FI2    `FlexTrainer` on the same model in modes 1 and 2 of either, beside them
Every run comes twice, the runs alternating in one process so that clock drift shows.
    python tools/bench_train_fused_gradients.py [--steps 20] [--warmup 5] [--out profiles/fused_gradients/bench.json]
    python tools/bench_train_fused_gradients.py --only Z          # also runs on a tree from before the entry: mode 0 against the parent
    python tools/bench_train_fused_gradients.py --only CP2        # a profiler's run
One JSON line: per run ms a step and ray-samples/s; the ratios the chain's modes are held to."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


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
    ap.add_argument("--only", default=None, help="one run (Z, CP0 .. CI2, FP1 .. FI2), twice")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.loss import AlphaLoss
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
    loss = AlphaLoss(loss_fn="network.loss.smape", alpha_loss_fn="network.loss.mse")
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    carpet = ParamNerf(emb(10), emb(4), emb(4), [1, 6])["model"]
    carpet.set_blob(synthetic.synthetic_weights(carpet.layer_table(), seed=0, dense_media=True))
    # run -> (class, keywords, `gradients_step` alone)
    runs = {"Z": (Trainer, {}, False)}
    for tag, key in (("P", "param_gradients"), ("I", "input_gradients")):
        runs.update({f"C{tag}0": (Trainer, {key: False}, False), f"C{tag}0g": (Trainer, {key: False}, True), f"C{tag}1": (Trainer, {key: True}, False),
                     f"C{tag}2": (Trainer, {key: "only"}, True), f"F{tag}1": (FlexTrainer, {key: True}, False), f"F{tag}2": (FlexTrainer, {key: "only"}, True)})
    p_order, i_order = ["CP0", "CP0g", "CP1", "CP2", "FP1", "FP2"], ["CI0", "CI0g", "CI1", "CI2", "FI1", "FI2"]
    order = [a.only] * 2 if a.only else ["Z"] + p_order + ["Z"] + p_order + i_order * 2
    out = {"what": "carpet model, 1024 rays x 256 samples, perturb, AlphaLoss(smape, mse); step + Adam, or gradients_step alone (runs ending in g or 2); HIP events",
           "steps": a.steps, "warmup": a.warmup, "runs": []}
    batch = (d(ro), d(rd), d(t), d(params), d(cone), d(color), d(alpha))
    for key in order:
        cls, kw, alone = runs[key]
        tr = cls(carpet, max_rays=n, n_samples=S, lrate=5e-4, lrate_decay=500, perturb=True, **kw)      # a fresh trainer a run: one set of activations on the device at a time
        sec = time_steps(tr, batch, loss, a.steps, a.warmup, gradients_only=alone, rays_per_param_row=R)
        out["runs"].append({"run": key, "trainer": cls.__name__, "modes": kw, "gradients_step_alone": alone, "ms_step": 1e3 * sec, "ray_samples_per_s": n * S / sec})
        del tr
    ms = lambda k: [r["ms_step"] for r in out["runs"] if r["run"] == k]
    mean = lambda k: float(np.mean(ms(k)))
    if not a.only:
        for tag in ("P", "I"):
            out[f"C{tag}1_over_C{tag}0"] = mean(f"C{tag}1") / mean(f"C{tag}0")
            out[f"C{tag}2_over_C{tag}0g"] = mean(f"C{tag}2") / mean(f"C{tag}0g")
            out[f"C{tag}1_over_F{tag}1"] = mean(f"C{tag}1") / mean(f"F{tag}1")
            out[f"C{tag}2_over_F{tag}2"] = mean(f"C{tag}2") / mean(f"F{tag}2")
        out["CP0_over_Z"] = mean("CP0") / mean("Z")
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
