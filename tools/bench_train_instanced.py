"""What a differentiable instanced step costs beside a plain one: the carpet model (ParamNerf [1, 6], 8 x 256, skips [4], color_depth 1) on
`FlexTrainer` at 1024 rays x 256 samples, gradients only (no Adam), timed with HIP events:
    A      `forward` + `backward` of the proxy render: the network on all 262 144 samples
    B@f    `forward_instanced` + `backward` on run-structured synthetic instancer buffers (`FakeInstancer(run_len=24)`: runs of 1 .. 24 samples, in
           or out of a patch as a whole) at live fractions f = 1.0, 0.35, 0.1: the compaction (a pass over dists, two int32 maps, one 8-byte copy
           to the host and the wait for it), the encoder's gather, the network on the M' live rows alone, the instanced composite and its adjoint
A and the B's alternate twice in one process so that clock drift shows as A / A (tools/bench_train_custom_loss.py's conventions: 5 + 20 steps,
whole steps between two events).
    python tools/bench_train_instanced.py [--steps 20] [--warmup 5] [--only A] [--out profiles/train_instanced/bench.json]
One JSON line: per run ms a step and M'; per fraction time / (live fraction x A) -- 1.0 means the step costs what its live rows cost in a plain
step.  `--only A`: what a library from before the entry can run too (NERFTEX_LIB, or this file in the parent's tree)."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_train_custom_loss import time_steps  # noqa: E402

FRACTIONS = (1.0, 0.35, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["A"], help="the plain side alone, twice")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.train import FlexTrainer
    B, R, S = 4, 256, 256
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
    d_color, d_alpha = d(rng.normal(size=(n, 3)).astype(np.float32) / n), d(rng.normal(size=n).astype(np.float32) / n)
    tr = FlexTrainer(carpet, max_rays=n, n_samples=S, perturb=False)

    def plain():
        tr.forward(*batch, rays_per_param_row=R)
        tr.backward(d_color, d_alpha)

    sides, live = {"A": plain}, {}
    if not a.only:
        from tests.test_gpu_instance import FakeInstancer
        for frac in FRACTIONS:
            inst = FakeInstancer(7, seed=int(100 * frac), p_hit=1.0, p_in=frac, run_len=24)
            bufs = inst.get_model_input(ro, rd, np.repeat(params, R, 0), S, 0.002)
            hit = np.ones(n, np.uint8)
            if frac == 1.0:
                bufs = bufs[:3] + (np.abs(bufs[3]) + np.float32(0.002),) + bufs[4:]              # every sample of every ray in a patch
            held = tuple(b if i in (7, 8) else d(np.ascontiguousarray(b, np.float32)) for i, b in enumerate(bufs))
            dh = d(hit)

            def instanced(held=held, dh=dh):
                tr.forward_instanced(held, batch[4], patch_scale=0.09, density_scale=400.0, hit=dh)
                tr.backward(d_color, d_alpha)
            sides[f"B@{frac}"] = instanced
    out = {"what": "gradients of one step, carpet model on FlexTrainer, 1024 rays x 256 samples; A forward + backward (proxy render), B@f forward_instanced + backward at "
                   "live fraction f (run-structured buffers, run_len 24); HIP events", "steps": a.steps, "warmup": a.warmup, "runs": []}
    order = ("A", "A") if a.only else ("A",) + tuple(k for k in sides if k != "A") + ("A",) + tuple(k for k in sides if k != "A")
    for key in order:
        sec = time_steps(sides[key], a.steps, a.warmup)
        run = {"run": key, "ms_step": 1e3 * sec}
        if key != "A":
            live[key] = tr.last_live
            run.update(live=tr.last_live, live_fraction=tr.last_live / (n * S))
        out["runs"].append(run)
    ms = lambda k: [r["ms_step"] for r in out["runs"] if r["run"] == k]
    A = ms("A")
    out["A_ms"] = float(np.mean(A)); out["A_over_A_drift"] = float(max(A) / min(A))
    for key in sides:
        if key != "A":
            out[f"{key}_ms"] = float(np.mean(ms(key)))
            out[f"{key}_over_fraction_x_A"] = float(np.mean(ms(key)) / (live[key] / (n * S) * np.mean(A)))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
