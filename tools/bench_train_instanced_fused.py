"""What an instanced training step costs on the fused 8 x 256 chain beside the layer-by-layer trainer's: the carpet model (ParamNerf [1, 6],
8 x 256, skips [4], color_depth 1) at 1024 rays x 256 samples on run-structured synthetic instancer buffers (`FakeInstancer(run_len=24)`),
gradients only (no Adam), timed with HIP events, both trainers on the SAME device buffers in the SAME process:
    chain@f   `forward_instanced` + `backward` on `Trainer(instanced=True)` at live fractions f = 1.0, 0.35, 0.1
    flex@f    the same step on `FlexTrainer`
    chain     the chain's plain `forward` + `backward` (the proxy render: the network on all 262 144 samples, the direction hoist on)
The sides alternate over `--rounds` rounds; every side is warmed up before its first window, a window is `--steps` whole steps between two
events, and a side's figure is the MEDIAN of its windows (min and max beside it).  Everything is then repeated once with
`param_gradients="only"` on both trainers (a parameter field fitted at fixed weights: no weight gradient).
    python tools/bench_train_instanced_fused.py [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/train_instanced_fused/bench.json]
One JSON line: per mode and side ms a step (median, min, max) and the live rows; per fraction flex / chain."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_train_custom_loss import time_steps  # noqa: E402

FRACTIONS = (1.0, 0.35, 0.1)


def measure(mode, a, carpet, batch, cotangents, held, n, S, R):
    from nerf_tex_amd.train import FlexTrainer, Trainer
    d_color, d_alpha = cotangents
    chain = Trainer(carpet, max_rays=n, n_samples=S, perturb=False, param_gradients=mode, instanced=True)
    flex = FlexTrainer(carpet, max_rays=n, n_samples=S, perturb=False, param_gradients=mode)

    def plain():
        chain.forward(*batch, rays_per_param_row=R)
        chain.backward(d_color, d_alpha)

    def instanced(tr, bufs, dh):
        def one():
            tr.forward_instanced(bufs, batch[4], patch_scale=0.09, density_scale=400.0, hit=dh)
            tr.backward(d_color, d_alpha)
        return one
    sides, live = {"chain": plain}, {}
    for frac, (bufs, dh) in held.items():
        sides[f"chain@{frac}"] = instanced(chain, bufs, dh)
        sides[f"flex@{frac}"] = instanced(flex, bufs, dh)
    windows = {k: [] for k in sides}
    for rnd in range(a.rounds):
        for key, one in sides.items():
            windows[key].append(1e3 * time_steps(one, a.steps, a.warmup if rnd == 0 else 1))
            if "@" in key:
                live[key] = (chain if key.startswith("chain") else flex).last_live
    out = {"param_gradients": mode, "sides": {}}
    for key, w in windows.items():
        out["sides"][key] = {"ms_step_median": float(np.median(w)), "ms_step_min": float(min(w)), "ms_step_max": float(max(w))}
        if key in live:
            out["sides"][key].update(live=live[key], live_fraction=live[key] / (n * S))
    med = lambda k: out["sides"][k]["ms_step_median"]
    for frac in FRACTIONS:
        assert live[f"chain@{frac}"] == live[f"flex@{frac}"]
        out[f"flex_over_chain@{frac}"] = med(f"flex@{frac}") / med(f"chain@{frac}")
    out["chain@1.0_over_chain_plain"] = med("chain@1.0") / med("chain")
    del chain, flex
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rays", type=int, default=256, help="rays per image (4 images a batch)")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.model import ParamNerf
    from tests.test_gpu_instance import FakeInstancer
    B, R, S = 4, a.rays, a.samples
    n = B * R
    f = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    rng = np.random.default_rng(0)
    params = np.asarray([f["params"]] * B, np.float32) * rng.uniform(0.8, 1.2, (B, 7)).astype(np.float32)
    dev = torch.device("cuda", 0)
    d = lambda x: torch.as_tensor(x, device=dev)
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    carpet = ParamNerf(emb(10), emb(4), emb(4), [1, 6])["model"]
    carpet.set_blob(synthetic.synthetic_weights(carpet.layer_table(), seed=0, dense_media=True))
    batch = (d(ro), d(rd), d(t), d(params), d(cone))
    cotangents = (d(rng.normal(size=(n, 3)).astype(np.float32) / n), d(rng.normal(size=n).astype(np.float32) / n))
    held = {}
    for frac in FRACTIONS:
        inst = FakeInstancer(7, seed=int(100 * frac), p_hit=1.0, p_in=frac, run_len=24)
        bufs = inst.get_model_input(ro, rd, np.repeat(params, R, 0), S, 0.002)
        if frac == 1.0:
            bufs = bufs[:3] + (np.abs(bufs[3]) + np.float32(0.002),) + bufs[4:]                      # every sample of every ray in a patch
        held[frac] = (tuple(b if i in (7, 8) else d(np.ascontiguousarray(b, np.float32)) for i, b in enumerate(bufs)), d(np.ones(n, np.uint8)))
    out = {"what": f"gradients of one step, carpet model, {n} rays x {S} samples, run-structured buffers (run_len 24): forward_instanced + backward on the fused chain "
                   "(chain@f) and on FlexTrainer (flex@f) at live fraction f, the chain's plain forward + backward (chain); HIP events, median of the rounds' windows",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "modes": [measure(mode, a, carpet, batch, cotangents, held, n, S, R) for mode in (False, "only")]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
