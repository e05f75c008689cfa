"""Opt-in bf16x6 training beside float32, timed with HIP events in ONE process (same-run comparisons only):
  * the contraction alone at 262 144 x 256 x 256 on random glorot-scale operands (not zeros: the 16-bit matrix pipe throttles under toggling
    data, and zero data hides that): the k-contiguous form with bias + ReLU (a trunk layer's forward) and the dW form with 128 ranges of 2048
    and column sums (a layer's weight and bias gradient), `ntx_gemm_f32_ex` and `ntx_gemm_bf16x6_ex` alternating, medians of 5 windows;
  * the carpet step at 1024 rays x 256 samples (perturb, AlphaLoss(smape, mse)): `FlexTrainer` float32, `FlexTrainer` bf16x6 and the fused
    chain (`Trainer`) alternating, medians of 5 windows of 20 steps, gradients only (`gradients_step`) and with Adam (`step`).
    python tools/bench_train_bf16x6.py [--windows 5] [--steps 20] [--warmup 5] [--out profiles/bf16x6/bench.json]
One JSON line.  `faster` says whether bf16x6 beat float32 in this run for each pair; nothing here is a bar."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from tools.bench_train_flex import time_steps                 # noqa: E402


def time_calls(call, reps, warmup):
    for _ in range(warmup):
        call()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        call()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / reps                      # ms


def contraction(windows, reps, warmup):
    from nerf_tex_amd import _lib
    dev = torch.device("cuda", 0)
    M, K, N, split = 262144, 256, 256, 2048
    g = torch.Generator(device=dev).manual_seed(0)
    glorot = lambda rows, cols, fan: (torch.rand((rows, cols), device=dev, generator=g) * 2 - 1) * float(np.sqrt(6.0 / fan))
    X = torch.relu(glorot(M, K, 2))                           # activations: O(1), half of them zero
    W, bias = glorot(K, N, K + N), glorot(1, N, N)
    dY = glorot(M, N, 2) * 1e-6                               # cotangents of a mean loss
    Y = torch.empty((M, N), device=dev)
    n_split = M // split
    partial, colsum = torch.empty((n_split, K, N), device=dev), torch.empty((n_split, N), device=dev)
    p = lambda t: t.data_ptr()
    null = None                                               # both entries on the null stream: the bf16x6 one takes no other
    forms = {
        "k_contiguous_bias_relu": lambda fn, tail: fn(p(X), K, 1, p(W), N, p(Y), N, M, N, K, p(bias), 1, None, 0, 0, 1, 0, 0, None, *tail),
        "dw_128_ranges_colsum": lambda fn, tail: fn(p(X), K, 0, p(dY), N, p(partial), N, K, N, M, None, 0, None, 0, 0, n_split, split, K * N, p(colsum), *tail)}
    out = {}
    for name, form in forms.items():
        calls = {"float32": lambda form=form: _lib.check(form(_lib.lib.ntx_gemm_f32_ex, (null,))),
                 "bf16x6": lambda form=form: _lib.check(form(_lib.lib.ntx_gemm_bf16x6_ex, ()))}
        ms = {k: [] for k in calls}
        for _ in range(windows):
            for k, call in calls.items():                     # alternating: clock drift hits both
                ms[k].append(time_calls(call, reps, warmup))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        flop = 2.0 * M * K * N
        out[name] = {"ms_windows": ms, "ms_median": med, "tflops": {k: flop / (v * 1e-3) / 1e12 for k, v in med.items()},
                     "bf16x6_over_float32": med["bf16x6"] / med["float32"], "faster": bool(med["bf16x6"] < med["float32"])}
    return {"M": M, "K": K, "N": N, "operand_bytes_read_written": 4 * (M * K + K * N + M * N), "forms": out}


def carpet_step(windows, steps, warmup):
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
    kw = dict(max_rays=n, n_samples=S, lrate=5e-4, lrate_decay=500, perturb=True)
    trainers = {"flex_float32": FlexTrainer(carpet, **kw), "flex_bf16x6": FlexTrainer(carpet, precision="bf16x6", **kw), "fused_chain": Trainer(carpet, **kw)}
    batch = (d(ro), d(rd), d(t), d(params), d(cone), d(color), d(alpha))
    out = {}
    for mode, gradients_only in (("gradients_only", True), ("with_adam", False)):
        ms = {k: [] for k in trainers}
        for _ in range(windows):
            for k, tr in trainers.items():
                ms[k].append(1e3 * time_steps(tr, batch, loss, steps, warmup, gradients_only=gradients_only, rays_per_param_row=R))
        med = {k: float(np.median(v)) for k, v in ms.items()}
        out[mode] = {"ms_windows": ms, "ms_median": med, "bf16x6_over_flex_float32": med["flex_bf16x6"] / med["flex_float32"],
                     "bf16x6_over_fused_chain": med["flex_bf16x6"] / med["fused_chain"], "faster": bool(med["flex_bf16x6"] < med["flex_float32"])}
    return {"rays": n, "samples": S, "modes": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    out = {"what": "bf16x6 beside float32: the contraction alone (random glorot-scale operands) and the carpet training step; HIP events, one process, alternating, medians",
           "windows": a.windows, "steps": a.steps, "warmup": a.warmup,
           "contraction": contraction(a.windows, a.steps, a.warmup), "carpet_step": carpet_step(a.windows, a.steps, a.warmup)}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
