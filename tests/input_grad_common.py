"""What the tests of dL/d rays_o, rays_d and dL/d pts, rays_d_map share (tests/test_input_gradients.py on the CPU, tests/test_gpu_input_gradients.py
on the GPU): the yardsticks -- float64 torch autograd of the restated step with the RAYS as leaves (plain step), of the restated instanced
step with the SAMPLE POINTS and DIRECTIONS as leaves --, the cases the GPU file runs, and the project's standing bar per output column.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED as the rest of the training oracle: the plain forward pass is oracle/train_oracle.py's `render` +
`_loss` (tests/train_branch_oracle.py's `render` with parameter branches), both differentiable in the rays with the depths given; the
instanced one is the short restatement below on `oracle.torch_cpu.fourier_features` / `mlp` and `tests.train_branch_oracle.mlp`
(`tests.instanced_train_common.restated` builds pts / rays_d_map as constants).  tests/test_input_gradients.py holds both against central
finite differences of the same loss."""

import numpy as np
import torch

from oracle import torch_cpu as tcpu
from oracle import train_oracle as tro
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests import train_branch_oracle as tbo
from tests.train_common import BKGD, F, step_depths, step_noise

MARGIN = 2.0                                                                     # how far inside `pgc.fair`'s guards every GPU case sits on the CPU


def restated_ray_gradients(w_np, spec, rays_o, rays_d, z, rows, rays_per_param_row, cone_scale, color_true, alpha_true, loss, blur_idx=None, map_exr=False,
                           composite_bkgd=False, bkgd=(1., 1., 1.), dtype=torch.float64, masks=None, branch_masks=None, sigma_mask=None, noise=None):
    """(loss, [color | alpha], dL/d rays_o [n, 3], dL/d rays_d [n, 3]) of one step: `pgc.restated_param_gradients` with the weights and the
    parameter rows held, the depths given and rays_o / rays_d as the leaves.  Rays whose depths are not finite are filtered out (their
    rows of both results are exactly 0), the loss runs over ALL rays (renderer.py:58-86)."""
    z = np.asarray(z)
    n, S = z.shape
    hit = np.isfinite(z).all(1)
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    sub = lambda x: None if x is None else t_(np.asarray(x)[hit])
    per_sample = lambda ms: None if ms is None else [sub(m.reshape(n, S, -1)).flatten(0, 1) for m in map(np.asarray, ms)]
    lo = torch.tensor(np.asarray(rays_o), dtype=dtype, requires_grad=True)
    ld = torch.tensor(np.asarray(rays_d), dtype=dtype, requires_grad=True)
    per_ray = t_(np.repeat(np.asarray(rows), int(rays_per_param_row), 0)[:n])
    w = [t_(a) for a in w_np]
    c = torch.zeros((n, 3), dtype=dtype); a = torch.zeros((n,), dtype=dtype)
    if hit.any():
        idx = torch.as_tensor(np.nonzero(hit)[0])
        args = (w, spec, lo[idx], ld[idx], sub(z), per_ray[idx], sub(cone_scale), blur_idx, map_exr, composite_bkgd, bkgd, per_sample(masks))
        if pgc.has_branches(spec):
            ch, ah = tbo.render(*args, per_sample(branch_masks), sub(sigma_mask), sub(noise))
        else:
            ch, ah = tro.render(*args, sub(sigma_mask), sub(noise))
        c = c.index_put((idx,), ch); a = a.index_put((idx,), ah)
    if composite_bkgd:
        c = c + torch.as_tensor((~hit)[:, None] * np.asarray(bkgd, np.float64)[None, :], dtype=dtype)
    val = tro._loss(loss, t_(color_true), t_(alpha_true), c, a)
    if val.requires_grad:
        val.backward()
    g = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().astype(np.float64)
    return float(val.detach()), np.concatenate([c.detach().numpy(), a.detach().numpy()[:, None]], -1), g(lo), g(ld)


# ---- the cases of tests/test_gpu_input_gradients.py, in `pgc`'s form: (id, n_parameters, arch, freqs, family, knobs, (step seed, batch seed)).
# Knobs beyond `pgc.DEFAULTS`: kind ("Nerf": a model without parameters).  Every batch has its rays_d scaled per ray by a factor in [0.5, 2]
# (`unnormalised`): with unit directions the normalisation and |d| terms are never exercised.  Seeds are chosen on the CPU
# (tests/test_input_gradients.py::test_the_gpu_cases_are_fair).
_BR = dict(width=128, depth=4, skips=[1], param_depth=2, param_width=64)
ARCH_CASES = [
    ("one_skip", *pgc.SMALL, dict(), (11, 3)),
    ("w98_d5_skips13", (1, 6), dict(width=98, depth=5, skips=[1, 3]), None, "carpet", dict(), (11, 3)),          # three readers of FF(xyz)
    ("color_depth0", (1, 4), dict(color_depth=0), None, "grass", dict(), (11, 3)),                              # the half layer reads dir_map
    ("chain_arch", (1, 6), None, None, "carpet", dict(), (11, 3)),
    ("branches_pd2_pw64", (1, 6), _BR, None, "carpet", dict(), (11, 3)),
    ("branch_geometry_only", (2, 0), _BR, None, "carpet", dict(), (11, 3)),
    ("branch_appearance_only", (0, 3), _BR, None, "carpet", dict(), (11, 3)),
    ("nerf", (0, 0), dict(width=64, depth=3, skips=[1]), None, "carpet", dict(kind="Nerf", loss_name="nerf_mse"), (11, 3)),
    ("pos_dir_freq0", (1, 6), dict(width=64, depth=3, skips=[1]), (0, 0, 4), "carpet", dict(), (11, 3)),         # identity rows only
    ("w128_d4_blur_geo", (2, 3), dict(width=128, depth=4, skips=[]), None, "grass_filtered", dict(blur=0), (11, 3)),
    ("w128_d4_blur_app", (2, 3), dict(width=128, depth=4, skips=[]), None, "grass_filtered", dict(blur=3), (11, 3)),
]
OPTION_CASES = [
    ("perturb_noise_alpha_smape", *pgc.SMALL, dict(perturb=True, noise_std=0.1, loss_name="alpha_smape"), (11, 5)),   # the noise enters the |d| term
    ("map_exr", *pgc.SMALL, dict(map_exr=True), (11, 3)),
    ("nerf_mse_bkgd", *pgc.SMALL, dict(loss_name="nerf_mse", bkgd=True), (11, 3)),
    ("callers_depths", *pgc.SMALL, dict(n=10, S=40, NI=27, z="merged", rpr=5), (11, 7)),
    ("a_row_per_ray", *pgc.SMALL, dict(rpr=1), (11, 3)),
]
# The fold's trips along a ray (lane l takes the samples l, l + 64, ...), and one ray in all.  Batch seeds other than 3 (here and above): the
# ones whose float32 floors are the lowest of 3 .. 8 where seed 3 sits less than 2x inside the floor guard (samples_6x65: 1.2e-4 at 3, 3.7e-5 at 6)
SAMPLE_CASES = [(f"samples_{n}x{S}", *pgc.SMALL, dict(n=n, S=S, rpr=r), (11, bs)) for n, S, r, bs in ((10, 2, 5, 5), (5, 3, 2, 3), (6, 64, 3, 3), (6, 65, 3, 6), (6, 129, 3, 3),
                                                                                                  (9, 256, 4, 3), (1, 33, 1, 3))]
MISS_CASES = [("rays_that_miss", *pgc.SMALL, dict(rpr=35, miss=pgc.MISS_RAYS, perturb=True), (11, 5)),
              ("rays_that_miss_blur", (2, 3), dict(width=64, depth=3, skips=[1]), None, "grass_filtered", dict(rpr=35, miss=pgc.MISS_RAYS, miss_cone="nan_inf", perturb=True, blur=0),
               (11, 5))]                                                           # (batch seeds 3 and 4 sit less than 2x inside the floor guard here)
ALL_CASES = ARCH_CASES + OPTION_CASES + SAMPLE_CASES + MISS_CASES


def unnormalised(rays_d, seed):
    """Each ray's direction scaled by a factor in [0.5, 2]."""
    scale = np.random.default_rng(seed + 77).uniform(0.5, 2.0, size=(len(rays_d), 1))
    return np.ascontiguousarray(rays_d * scale, F)


def case_setup(case):
    """`pgc.case_setup` (a model without parameters: a Nerf) with un-normalised rays_d."""
    from tests.common import make_model
    cid, npar, arch, freqs, fam, knobs, (seed, batch_seed) = case
    kind = knobs.get("kind", "ParamNerf")
    plain = (cid, npar, arch, freqs, fam, {k: v for k, v in knobs.items() if k != "kind"}, (seed, batch_seed))
    if kind == "Nerf":                                                             # (`pgc.case_setup` makes ParamNerfs: the same batch on the Nerf)
        model, spec, wts = make_model(npar, kind="Nerf", dense_media=True, arch=arch, freqs=freqs)
        _, pspec, _, batch, kn, seed = pgc.case_setup((cid, (1, 6), arch, freqs, fam, plain[5], (seed, batch_seed)))
        ro, rd, t, cone, rows, color, alpha = batch
        batch = (ro, rd, t, cone, np.zeros((rows.shape[0], 0), F), color, alpha)
    else:
        model, spec, wts, batch, kn, seed = pgc.case_setup(plain)
    ro, rd, t, cone, rows, color, alpha = batch
    return model, spec, wts, (ro, unnormalised(rd, batch_seed), t, cone, rows, color, alpha), kn, seed


def restate(spec, wts, batch, kn, seed, dtype, masks, branch_masks, sigma_mask):
    """`restated_ray_gradients` of a case's step on the depths and the noise the step places itself, or on the case's own depths."""
    from tests.train_common import LOSSES
    ro, rd, t, cone, rows, color, alpha = batch
    z, noise = pgc._depths(t, kn, seed, kn["miss"]), step_noise(len(t), kn["S"], seed, kn["noise_std"])
    return restated_ray_gradients(wts, spec, ro, rd, z, rows, kn["rpr"], pgc._cone(cone), color, alpha, LOSSES[kn["loss_name"]][0], blur_idx=kn["blur"],
                                  map_exr=kn["map_exr"], composite_bkgd=kn["bkgd"], bkgd=BKGD, dtype=dtype, masks=masks, branch_masks=branch_masks, sigma_mask=sigma_mask,
                                  noise=noise)


def columns(d_a, d_b):
    """[.., 3] and [.., 3] as six columns over the rows: x, y, z of each of the two results."""
    return np.concatenate([np.asarray(d_a, np.float64).reshape(-1, 3), np.asarray(d_b, np.float64).reshape(-1, 3)], 1)


def check_input_gradients(got, want, f32, report=print, rows=None):
    """The project's standing bar per output column (x, y, z of each of the two results over `rows`, default all): rel-Linf <= max(1e-4, 4 x
    floor) under the guards floor <= 5e-4 and max |grad| > 1e-6 -- `pgc.check_param_gradients` on the six columns.  Every figure is printed
    before it is gated."""
    return pgc.check_param_gradients(columns(*got), columns(*want), columns(*f32), report, rows)


# ---- the instanced step: InstanceRenderer.evaluate_model + map_model_output (renderer.py:247-354) on the live samples, as
# `itc.restated`, with pts and rays_d_map of the live samples as the leaves and the weights and params_map held ----------------------------
def restated_sample_gradients(w_np, spec, bufs, hit, cone, head, *, blur_idx=None, patch_scale=itc.PATCH_SCALE, density_scale=1.0, density_reweighting=True, map_exr=False,
                              composite_bkgd=False, bkgd=BKGD, dtype=torch.float64, masks=None, branch_masks=None, sigma_mask=None, pts=None, dirs=None):
    """(loss, pred [n, 4], dL/d pts [n, S, 3], dL/d rays_d_map [n, S, 3]) of one instanced step under `head(color_pred, alpha_pred)`; zeros at
    samples that are not live, where nothing is read.  `masks` / `branch_masks` / `sigma_mask`: GIVEN ReLU patterns in compact row order
    (None: free).  `pts` / `dirs`: other values than the buffers' (finite differences)."""
    rays_d_map, pts_b, tt, dists, color_last, alpha_last, alpha_weight, _, _, params_map = [np.asarray(b) for b in bufs]
    n, S = dists.shape
    P = params_map.shape[-1]
    hit = np.asarray(hit, bool)
    live = itc.live_order(hit, dists)
    li = torch.as_tensor(live)
    t_ = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    at_live = lambda a, w: t_(np.nan_to_num(np.asarray(a, np.float64)).reshape(n * S, *([w] if w else []))[live])
    lp = at_live(pts_b if pts is None else pts, 3).requires_grad_(True)
    ld = at_live(rays_d_map if dirs is None else dirs, 3).requires_grad_(True)
    w = [t_(a) for a in w_np]
    par = at_live(params_map, P)
    if blur_idx is not None:                                                                                     # renderer.py:259-263
        scale = (t_(np.repeat(np.asarray(cone).reshape(n, 1), S, 1).reshape(-1)[live]) * at_live(tt, 0) / patch_scale)[:, None]
        par = torch.cat([par[:, :blur_idx], par[:, blur_idx, None] * scale, par[:, blur_idx + 1:]], -1)
    m_ = lambda ms: None if ms is None else [t_(np.asarray(m)) for m in ms]
    pos_map = tcpu.fourier_features(lp, spec.pos_freq)
    if len(live) == 0:
        raw, sg = torch.zeros((0, 3), dtype=dtype), torch.zeros((0, 1), dtype=dtype)
    elif pgc.has_branches(spec):
        raw, sg = tbo.mlp(w, spec, pos_map, ld, par, m_(masks), m_(branch_masks))
    else:
        raw, sg = tcpu.mlp(w, spec, pos_map, ld, par, m_(masks))
    sp = sg[:, 0] * (at_live(alpha_weight, 0) if density_reweighting else 1.0) * density_scale                  # :300
    gate = torch.relu(sp) if sigma_mask is None else sp * t_(np.asarray(sigma_mask))
    a_live = 1.0 - torch.exp(-gate * at_live(dists, 0) / patch_scale)                                            # :339
    rgb_live = torch.nn.functional.elu(raw) + 1 if map_exr else torch.sigmoid(raw)                               # :325-330
    am = torch.zeros(n * S, dtype=dtype).index_put((li,), a_live).reshape(n, S)
    rgb = torch.zeros((n * S, 3), dtype=dtype).index_put((li,), rgb_live).reshape(n, S, 3)
    am = torch.cat([am, t_(alpha_last).reshape(n, 1)], 1)                                                        # :331, :339
    rgb = torch.cat([rgb, t_(color_last).reshape(n, 1, 3)], 1)
    trans = torch.cumprod(1.0 - am + 1e-10, -1)
    wts = am * torch.cat([torch.ones_like(trans[:, :1]), trans[:, :-1]], -1)                                     # :342
    c = torch.sum(wts[..., None] * rgb, -2); a = torch.sum(wts, -1)
    if composite_bkgd:                                                                                           # :351-352
        c = c + (1.0 - a[..., None]) * torch.as_tensor(bkgd, dtype=dtype)
    h_ = torch.as_tensor(hit)
    c = torch.where(h_[:, None], c, torch.zeros_like(c)); a = torch.where(h_, a, torch.zeros_like(a))             # :313-314
    val = head(c, a)
    if val.requires_grad:
        val.backward()
    out = []
    for leaf in (lp, ld):
        full = np.zeros((n * S, 3))
        if leaf.grad is not None:
            full[live] = leaf.grad.numpy().astype(np.float64)
        out.append(full.reshape(n, S, 3))
    return float(val.detach()), np.concatenate([c.detach().numpy(), a.detach().numpy()[:, None]], -1), out[0], out[1]


# The instanced edges: live counts around a wave's rows and the contraction's 2048-row range, sample counts around the composite's chunk
INST_EDGES = [(f"S{S}", "S", S) for S in (1, 64, 65)] + [(f"live{K}", "live", K) for K in (0, 1, 32, 33, 2047, 2049)]
INST_EDGE_IDS = [e[0] for e in INST_EDGES]


def own_instanced_patterns(spec, w, bufs, hit, cone, okw):
    """The ReLU patterns of a float32 forward pass of `itc.restated` itself, in compact row order: the CPU's stand-in for a trainer's."""
    out = itc.restated(w, spec, bufs, hit, cone, None, dtype=torch.float32, **okw)
    return dict(masks=out.masks, branch_masks=out.branch_masks, sigma_mask=out.sigma_mask)
