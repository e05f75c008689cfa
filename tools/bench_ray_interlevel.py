"""What the interlevel loss between a proposal and a fine histogram costs, on an MI355X, timed with HIP events; every side of a comparison in
ONE run, alternating over `--rounds` rounds, a window is `--steps` calls between two events, a side's figure is the MEDIAN of its windows (min
and max beside it) -- tools/bench_ray_distortion.py's protocol and its `measure`.
  (a) loss + both gradients at 1024 x (64 -> 128) and 256 x (256 -> 512) (rays x (proposal -> fine samples), the fine depths being the
      proposal's merged with as many draws inside the span):
        entry         `nerf_tex_amd.loss.ray_interlevel(..., with_grad=True)`: one launch of `ntx_ray_interlevel`
        searchsorted  a torch statement -- `torch.searchsorted` twice, the bound as a difference of prefix sums -- + torch.autograd.grad
      with the error of each against float64 autograd of the dense [N, S, S_p] mask statement
  (b) one `gradients_step` at 1024 rays, 64 + 64 samples, perturb, under NerfLoss, of
        proposal      `ProposalTrainer`: a 4 x 128 ParamNerf proposal and the carpet model (8 x 256)
        coarse_fine   `CoarseFineTrainer` of two carpet models
    python tools/bench_ray_interlevel.py [--steps 20] [--warmup 5] [--rounds 5] [--out profiles/ray_interlevel/bench.json]
One JSON line.  Measured, no ratio promised."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tools.bench_ray_distortion import measure, rays  # noqa: E402

EPS = 2.0 ** -23


def histograms(n, Sp, S, seed=0):
    """(w, z, wp, zp) float32: `rays` for the proposal set; the fine depths are those merged with S - Sp uniform draws inside the span; the fine
    weights are the composite's weights of another smooth density."""
    wp, zp = rays(n, Sp, seed)
    rng = np.random.default_rng(seed + 1)
    lo, sp = zp[:, :1].astype(np.float64), (zp[:, -1:] - zp[:, :1]).astype(np.float64)
    z = np.sort(np.concatenate([zp, (lo + sp * rng.uniform(0.02, 0.98, (n, S - Sp))).astype(np.float32)], 1), 1)
    z64 = z.astype(np.float64)
    d = np.diff(z64, axis=1); d = np.concatenate([d, d[:, -1:]], 1)
    sigma = rng.uniform(2, 8, (n, 1)) / sp * np.exp(-(((z64 - lo) / sp - rng.uniform(0.3, 0.7, (n, 1))) / 0.15) ** 2) * rng.uniform(0.5, 1.5, (n, S))
    a = 1 - np.exp(-sigma * d)
    T = np.cumprod(1 - a + 1e-10, 1)
    return (a * np.concatenate([np.ones((n, 1)), T[:, :-1]], 1)).astype(np.float32), z, wp, zp


def ends(x):
    return torch.cat([x[:, 1:], x[:, -1:] + (x[:, -1:] - x[:, -2:-1])], 1)


def by_searchsorted(w, z, wp, zp):
    b, bp = ends(z), ends(zp)
    lo, hi = torch.searchsorted(bp, z, right=True), torch.searchsorted(zp, b, right=False)
    csum = torch.cat([torch.zeros_like(wp[:, :1]), torch.cumsum(wp, 1)], 1)
    bound = torch.where(hi > lo, torch.gather(csum, 1, hi) - torch.gather(csum, 1, lo), torch.zeros_like(w))
    res = torch.relu(w - bound)
    return (res * res / (w + EPS)).sum(1)


def dense(w, z, wp, zp):
    b, bp = ends(z), ends(zp)
    mask = (zp[:, None, :] < b[:, :, None]) & (bp[:, None, :] > z[:, :, None])
    res = torch.relu(w - (mask.to(wp.dtype) * wp[:, None, :]).sum(-1))
    return (res * res / (w + EPS)).sum(1)


def with_autograd(fn):
    def one(w, z, wp, zp):
        lw, lp = w.detach().requires_grad_(True), wp.detach().requires_grad_(True)
        val = fn(lw, z, lp, zp)
        gf, gp = torch.autograd.grad(val.sum(), (lw, lp))
        return val.detach(), gp, gf
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.loss import NerfLoss, ray_interlevel
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.train import CoarseFineTrainer, ProposalTrainer
    dev = torch.device("cuda", 0)
    d = lambda x: torch.as_tensor(x, device=dev)
    rel = lambda x, ref: float((x.double() - ref.double()).abs().max() / ref.double().abs().max())
    out = {"what": "the interlevel loss: (a) loss + both gradients by the entry and by a torch.searchsorted + prefix-difference statement with autograd, errors against "
                   "float64 autograd of the dense mask statement; (b) gradients_step of ProposalTrainer (4 x 128 proposal + carpet model) beside CoarseFineTrainer (two carpet "
                   "models), 1024 rays, 64 + 64 samples, perturb, NerfLoss; HIP events, medians of the rounds' windows, peak memory by torch.cuda.max_memory_allocated",
           "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "entry": {}, "step": {}}
    for n, Sp, S in ((1024, 64, 128), (256, 256, 512)):
        w, z, wp, zp = (d(x) for x in histograms(n, Sp, S))
        sides = {"entry": lambda: ray_interlevel(w, z, wp, zp, with_grad=True), "searchsorted": lambda: with_autograd(by_searchsorted)(w, z, wp, zp)}
        res = measure(sides, a.steps, a.warmup, a.rounds)
        got = {k: one() for k, one in sides.items()}
        ref = with_autograd(dense)(w.double(), z.double(), wp.double(), zp.double())
        for k in sides:
            res[k]["loss_rel_linf_vs_float64"], res[k]["grad_prop_rel_linf_vs_float64"], res[k]["grad_fine_rel_linf_vs_float64"] = (rel(got[k][i], ref[i]) for i in range(3))
        res["bytes_moved_by_the_entry"] = 4 * (3 * n * S + 3 * n * Sp + n)
        out["entry"][f"{n}x({Sp}->{S})"] = res
        del got, ref
    B, R, S, NI = 4, 256, 64, 64
    n = B * R
    f = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    rng = np.random.default_rng(0)
    color, alpha = rng.uniform(0, 1, (n, 3)).astype(np.float32), rng.uniform(0, 1, n).astype(np.float32)
    params = np.asarray([f["params"]] * B, np.float32) * rng.uniform(0.8, 1.2, (B, 7)).astype(np.float32)
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}

    def model(seed, **arch):
        m = ParamNerf(emb(10), emb(4), emb(4), [1, 6], **arch)["model"]
        m.set_blob(synthetic.synthetic_weights(m.layer_table(), seed=seed, dense_media=True))
        return m
    batch = (d(ro), d(rd), d(t), d(params), d(cone), d(color), d(alpha))
    kw = dict(max_rays=n, n_samples=S, n_importance=NI, perturb=True)
    pair = {"proposal": ProposalTrainer(model(0, depth=4, width=128), model(1), **kw), "coarse_fine": CoarseFineTrainer(model(0), model(1), **kw)}
    loss = NerfLoss()
    sides = {k: (lambda tr=tr, seed=None: tr.gradients_step(*batch, loss, rays_per_param_row=R, seed=seed)) for k, tr in pair.items()}
    res = measure(sides, a.steps, a.warmup, a.rounds)
    for k, one in sides.items():
        val = one(seed=5)[0]
        torch.cuda.synchronize()
        res[k]["loss"] = float(val.item())
        res[k]["trainers"] = [type(x).__name__ for x in pair[k].trainers]
    res["proposal"]["interlevel_term"] = float(pair["proposal"].last_interlevel.item())
    res["proposal_over_coarse_fine"] = res["proposal"]["ms_median"] / res["coarse_fine"]["ms_median"]
    out["step"]["1024x(64+64)"] = res
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
