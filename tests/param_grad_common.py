"""What the tests of dL/d parameters share (tests/test_param_gradients.py on the CPU, tests/test_gpu_param_gradients.py on the GPU): the
yardstick -- float64 torch autograd of the restated step with the PARAMETER ROWS as the leaf --, the cases the GPU file runs, and the bars of
tests/train_flex_common.check_against_float64 restated per parameter column.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED as the rest of the training oracle: the forward pass is oracle/train_oracle.py's `render` + `_loss`
(tests/train_branch_oracle.py's `render` for a model with parameter branches: its forward takes torch parameters as they come), the gradient is what
autograd derives from it.  tests/test_param_gradients.py holds it against central finite differences of the same loss."""

from types import SimpleNamespace

import numpy as np
import torch

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro
from tests import train_branch_oracle as tbo
from tests.train_common import BKGD, F, step_depths, step_noise
from tests.train_flex_common import n_relu

N_RAYS, N_SAMPLES = 70, 33        # 2310 samples: across one range of 2048 of the weight gradients; 70 is no multiple of a wave, 33 none of 32 or 4


def has_branches(spec):
    return spec.param_layers > 0 and spec.n_params > 0


def restated_param_gradients(w_np, spec, rays_o, rays_d, z, rows, rays_per_param_row, cone_scale, color_true, alpha_true, loss, blur_idx=None, map_exr=False,
                             composite_bkgd=False, bkgd=(1., 1., 1.), dtype=torch.float64, masks=None, branch_masks=None, sigma_mask=None, noise=None):
    """(loss, [color | alpha], dL/d rows [n_rows, P]) of one step: `tro.step_gradients` with the weights held and the parameter rows as the
    leaf -- ray r reads `rows.repeat_interleave(rays_per_param_row, 0)[r]`.  Rays whose depths are not finite are filtered out, the rest
    rendered, the results scattered back into zeros (plus the background when compositing), the loss over ALL rays (renderer.py:58-86).
    `masks` / `sigma_mask` / `noise` as `tro.step_gradients` takes them, `branch_masks` as tests/train_branch_oracle.step_gradients."""
    z = np.asarray(z)
    n, S = z.shape
    hit = np.isfinite(z).all(1)
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    sub = lambda x: None if x is None else t_(np.asarray(x)[hit])
    per_sample = lambda ms: None if ms is None else [sub(m.reshape(n, S, -1)).flatten(0, 1) for m in map(np.asarray, ms)]
    leaf = torch.tensor(np.asarray(rows), dtype=dtype, requires_grad=True)
    assert leaf.shape[0] == -(-n // int(rays_per_param_row)), (leaf.shape, n, rays_per_param_row)
    per_ray = leaf.repeat_interleave(int(rays_per_param_row), 0)[:n]
    w = [t_(a) for a in w_np]
    c = torch.zeros((n, 3), dtype=dtype); a = torch.zeros((n,), dtype=dtype)
    if hit.any():
        idx = torch.as_tensor(np.nonzero(hit)[0])
        args = (w, spec, sub(rays_o), sub(rays_d), sub(z), per_ray[idx], sub(cone_scale), blur_idx, map_exr, composite_bkgd, bkgd, per_sample(masks))
        if has_branches(spec):
            ch, ah = tbo.render(*args, per_sample(branch_masks), sub(sigma_mask), sub(noise))
        else:
            ch, ah = tro.render(*args, sub(sigma_mask), sub(noise))
        c = c.index_put((idx,), ch); a = a.index_put((idx,), ah)
    if composite_bkgd:
        c = c + torch.as_tensor((~hit)[:, None] * np.asarray(bkgd, np.float64)[None, :], dtype=dtype)
    val = tro._loss(loss, t_(color_true), t_(alpha_true), c, a)
    if val.requires_grad:
        val.backward()
    grad = np.zeros(leaf.shape) if leaf.grad is None else leaf.grad.numpy().astype(np.float64)
    return float(val.detach()), np.concatenate([c.detach().numpy(), a.detach().numpy()[:, None]], -1), grad


def column_errors(got, want):
    """rel-Linf per parameter column: the largest error of a column over the rows against that column's largest entry."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max(0) / np.maximum(np.abs(want).max(0), 1e-300)


# ---- the cases of tests/test_gpu_param_gradients.py: (id, n_parameters, arch, freqs, family, knobs, (step seed, batch seed)).  Seeds are chosen on
# the CPU (tests/test_param_gradients.py::test_the_gpu_cases_are_fair: float32 against float64 of this restatement alone, on its own float32 branches)
MODEL_CASES = [
    ("w98_d5_skips13", (1, 6), dict(width=98, depth=5, skips=[1, 3]), None, "carpet", dict(), (11, 3)),
    ("color_depth0", (1, 4), dict(color_depth=0), None, "grass", dict(), (11, 3)),
    ("w128_d4_blur_geo", (2, 3), dict(width=128, depth=4, skips=[]), None, "grass_filtered", dict(blur=0), (11, 3)),
    ("w128_d4_blur_app", (2, 3), dict(width=128, depth=4, skips=[]), None, "grass_filtered", dict(blur=3), (11, 3)),
    ("chain_arch", (1, 6), None, None, "carpet", dict(), (11, 3)),
    ("param_freq0", (1, 6), dict(width=64, depth=3, skips=[1]), (10, 4, 0), "carpet", dict(), (11, 3)),
    ("branches_pd2_pw64", (1, 6), dict(width=128, depth=4, skips=[1], param_depth=2, param_width=64), None, "carpet", dict(), (11, 3)),
    ("branch_geometry_only", (2, 0), dict(width=128, depth=4, skips=[1], param_depth=2, param_width=64), None, "carpet", dict(), (11, 3)),
    ("branch_appearance_only_pw100", (0, 3), dict(width=128, depth=4, skips=[1], param_depth=2, param_width=100), None, "carpet", dict(), (11, 3)),
]
SMALL = ((1, 6), dict(width=64, depth=3, skips=[1]), None, "carpet")          # the network of the cases that are about something else than the architecture
ROW_CASES = [(f"rows_{r}", *SMALL, dict(rpr=r), (11, 3)) for r in (1, 35, 70, 64)]                    # 64: the last row is a short one of 6 rays
OPTION_CASES = [
    ("perturb_noise_alpha_smape", *SMALL, dict(perturb=True, noise_std=0.1, loss_name="alpha_smape"), (11, 3)),
    ("nerf_mse_bkgd", *SMALL, dict(loss_name="nerf_mse", bkgd=True), (11, 3)),
    ("map_exr", *SMALL, dict(map_exr=True), (11, 3)),
]
MISS_RAYS = [0, 5, 33, 34] + list(range(35, 70))                                                        # with 35 rays a row: the whole last row
MISS_CASE = ("rays_that_miss", *SMALL, dict(rpr=35, miss=MISS_RAYS, perturb=True), (11, 3))
DEFAULTS = dict(loss_name="alpha_smape", bkgd=False, map_exr=False, perturb=False, blur=None, noise_std=0.0, rpr=35, miss=(), miss_cone="nan", n=N_RAYS, S=N_SAMPLES,
                z=None, NI=27)

# ---- the edges (profiles/param_gradients/edge_errors.md).  A case's knobs carry its own size (`n` rays x `S` samples) and, with z="merged", its
# own depths.  Every one of these sits 2x inside both guards of `fair` on the CPU (floor <= 2.5e-4, max |grad| >= 2e-6), so that the trainer's own
# ReLU patterns cannot tip a guard on the GPU.
# The fold's trips along a ray: lane l takes the samples l, l + 64, ...: every lane once (64), one lane twice (65), a third trip (129), the configs'
# 256 (9 x 256 = 2304 samples: across one range of the weight gradients), fewer samples than lanes, the step's minimum (batch seed 3 is unfair at
# S = 2: floor 1.3e-3)
SAMPLE_CASES = [(f"samples_{n}x{S}", *SMALL, dict(n=n, S=S, rpr=r), (11, bs)) for n, S, r, bs in ((6, 64, 3, 3), (6, 65, 3, 3), (6, 129, 3, 3), (9, 256, 4, 3), (5, 3, 2, 3),
                                                                                                  (10, 2, 5, 5))]
# The rows' loop over a row's rays is unrolled by 8: rows of 7 / 8 / 9 rays (the last one short: 6, 4, 2), a row longer than the batch, one ray
# in all, a whole row and a row of one
ROW_EDGE_CASES = [(f"rows_{n}_by_{r}", *SMALL, dict(n=n, rpr=r), (11, 3)) for n, r in ((20, 7), (20, 8), (20, 9), (20, 32), (1, 1), (3, 2))]
# The built limits -- n_parameters [4, 8] with 4 bands: 36 and 72 feature columns, P = 12, blur_idx on the first and last column of each group --,
# one-group models without branches (PG[0] or PG[1] is never placed), and branches whose input rows differ from sample to sample (blur_idx)
_TRUNK, _EDGE = dict(width=64, depth=3, skips=[1]), dict(n=20, rpr=10)
LIMIT_CASES = ([(f"limit_4_8_blur_{b}", (4, 8), _TRUNK, None, "carpet", dict(_EDGE, blur=b), (11, 3)) for b in (None, 0, 3, 4, 11)]
               + [(f"one_group_{g}_{a}", (g, a), _TRUNK, None, "carpet", dict(_EDGE), (11, 3)) for g, a in ((0, 3), (2, 0), (1, 0), (0, 1))]
               + [(f"branches_blur_{b}", (2, 3), dict(_TRUNK, param_depth=2, param_width=16), None, "grass_filtered", dict(_EDGE, blur=b), (11, 3)) for b in (0, 3)])
# Missed rays under blur_idx: the fold reads cone_scale, which is NaN for every other missed ray and +inf for the rest
MISS_BLUR_CASES = [(f"miss_blur_{b}", (2, 3), _TRUNK, None, "grass_filtered", dict(rpr=35, miss=MISS_RAYS, miss_cone="nan_inf", perturb=True, blur=b), (11, 3)) for b in (0, 3)]
# Caller's depths (the fine pass of coarse + fine): non-uniform, and a factor of the blurred column
DEPTH_CASES = [(f"depths_blur_{b}", *SMALL, dict(n=10, S=40, NI=27, z="merged", rpr=5, blur=b), (11, 3)) for b in (None, 0, 1, 6)]
# The coarse pass of the coarse + fine test (its fine pass runs on the depths the trainer's sampler merges: no CPU case), and ParameterFitter's options
COARSE_CASE = ("coarse_pass", *SMALL, dict(n=24, S=24, rpr=12, perturb=True), (11, 3))
FITTER_CASE = ("fitter_options", *SMALL, dict(blur=0, perturb=True, noise_std=0.1, map_exr=True), (11, 3))
NEW_CASES = SAMPLE_CASES + ROW_EDGE_CASES + LIMIT_CASES + MISS_BLUR_CASES + DEPTH_CASES + [COARSE_CASE, FITTER_CASE]
ALL_CASES = MODEL_CASES + ROW_CASES + OPTION_CASES + [MISS_CASE] + NEW_CASES
MARGIN = 2.0                                                                     # how far inside `fair`'s guards every case of NEW_CASES sits on the CPU


def case_setup(case, n=None, S=None):
    """(model, spec, weights, (ro, rd, t, cone, rows, color, alpha), knobs with every default, step seed) of a case at its own size (`n`, `S`:
    another one): the batch is `tests.train_flex_common.flex_batch`'s -- a model with more parameters than the family's batch carries draws the
    missing columns --, the parameter rows the first ray's of every `rpr` rays; the rays of `miss` get t = inf and cone_scale = NaN (miss_cone
    "nan_inf": NaN and +inf in turn).  The knobs come back with `n`, `S` = the samples the step runs on, `miss` as a mask and `z` = None (the
    step places its depths) or, for z="merged", z_vals [n, S] on the host: the step's own depths merged and sorted with `NI` float32 draws
    t0 + u (t1 - t0)."""
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    cid, npar, arch, freqs, fam, knobs, (seed, batch_seed) = case
    model, spec, wts = make_model(npar, dense_media=True, arch=arch, freqs=freqs)
    kn = dict(DEFAULTS, **knobs)
    n, S = int(n or kn["n"]), int(S or kn["S"])
    ro, rd, t, cone, params, color, alpha = flex_batch(batch_seed, n, S, spec, fam)
    P = sum(spec.n_parameters)
    if params.shape[1] < P:
        more = np.random.default_rng(batch_seed).uniform(0.2, 1.5, size=(n, P - params.shape[1])).astype(F)
        params = np.ascontiguousarray(np.concatenate([params, more], 1))
    rows = np.ascontiguousarray(params[::kn["rpr"]], F)
    miss = np.zeros(n, bool); miss[list(kn["miss"])] = True
    t = t.copy(); t[miss] = np.inf
    cone = cone.copy(); cone[miss] = np.nan
    if kn["miss_cone"] == "nan_inf":
        cone[np.nonzero(miss)[0][1::2]] = np.inf
    kn["miss"] = miss
    if kn["z"] == "merged":
        assert not miss.any()
        u = np.random.default_rng(batch_seed).uniform(0, 1, size=(n, kn["NI"])).astype(F)
        drawn = t[:, :1] + u * (t[:, 1:] - t[:, :1])
        kn["z"] = np.ascontiguousarray(np.sort(np.concatenate([step_depths(t, S, seed, kn["perturb"]), drawn], 1), 1), F)
        S += kn["NI"]
    else:
        assert kn["z"] is None
    kn["n"], kn["S"] = n, S
    return model, spec, wts, (ro, rd, t, cone, rows, color, alpha), kn, seed


def _depths(t, kn, seed, miss=None):
    """The depths of a case's step: the ones it was given, or the ones it places itself."""
    if kn["z"] is None:
        return step_depths(t, kn["S"], seed, kn["perturb"], miss)
    z = kn["z"].copy()
    if miss is not None:
        z[miss] = np.inf
    return z


def _cone(cone):
    """cone_scale as the restatement takes it: a missed ray's NaN / inf (the ray is filtered out) as 0."""
    return np.where(np.isfinite(cone), cone, 0).astype(F)


def restate(spec, wts, batch, kn, seed, dtype, masks, branch_masks, sigma_mask):
    """`restated_param_gradients` of a case's step on the depths and the noise the step places itself, or on the case's own depths as they are."""
    from tests.train_common import LOSSES
    ro, rd, t, cone, rows, color, alpha = batch
    z, noise = _depths(t, kn, seed, kn["miss"]), step_noise(len(t), kn["S"], seed, kn["noise_std"])
    return restated_param_gradients(wts, spec, ro, rd, z, rows, kn["rpr"], _cone(cone), color, alpha, LOSSES[kn["loss_name"]][0], blur_idx=kn["blur"],
                                    map_exr=kn["map_exr"], composite_bkgd=kn["bkgd"], bkgd=BKGD, dtype=dtype, masks=masks, branch_masks=branch_masks, sigma_mask=sigma_mask,
                                    noise=noise)


def own_patterns(spec, wts, batch, kn, seed):
    """The ReLU patterns of a float32 forward pass of the restatement itself (the hit rays' real, the others' whatever: they are filtered):
    what a float32 step would hand to float64 -- the CPU's stand-in for the patterns a trainer keeps."""
    ro, rd, t, cone, rows, color, alpha = batch
    n = len(t)
    z, noise = _depths(t, kn, seed), step_noise(n, kn["S"], seed, kn["noise_std"])
    per_ray = np.repeat(rows, kn["rpr"], 0)[:n]
    return tbo.own_masks(wts, spec, ro, rd, z, per_ray, _cone(cone), blur_idx=kn["blur"], noise=noise)


def trainer_patterns(tr, spec, n, S, noise):
    """(masks, branch_masks, sigma_mask) of the step a FlexTrainer / BranchTrainer has just taken: the signs of the activations it kept."""
    torch.cuda.synchronize()
    masks = [tr.activation(k, n * S) > 0 for k in range(n_relu(spec))]
    branch_masks = None
    if has_branches(spec):
        slots = ([32 + j for j in range(spec.param_layers)] if spec.n_geo > 0 else []) + ([48 + j for j in range(spec.param_layers)] if spec.n_app > 0 else [])
        branch_masks = [tr.activation(k, n * S) > 0 for k in slots]
    sigma_mask = (tr.activation(64, n * S).reshape(n, S) + (0 if noise is None else noise.astype(F))) > 0
    return masks, branch_masks, sigma_mask


def fair(want_grad, f32_grad, report=print, rows=None, margin=1.0):
    """The guards that keep the floor from hiding a failure, per parameter column (over `rows`, default all): the float32 restatement within 5e-4
    of float64, and a gradient worth the name (max |grad| > 1e-6).  `margin`: how many times inside both guards the case has to sit (the CPU's
    check of the cases in NEW_CASES: MARGIN).  Returns the floors."""
    sel = slice(None) if rows is None else rows
    floors, biggest = column_errors(f32_grad[sel], want_grad[sel]), np.abs(want_grad[sel]).max(0)
    for c in range(len(floors)):
        report(f"  column {c}: floor {floors[c]:.2e} max |grad| {biggest[c]:.3e}")
    assert (biggest > 1e-6).all(), ("a parameter column without a gradient worth the name: change the seed, not the bar", biggest)
    assert (floors <= 5e-4).all(), ("a float32 floor above 5e-4: change the seed, not the bar", floors)
    assert (biggest >= 1e-6 * margin).all() and (floors <= 5e-4 / margin).all(), (f"less than {margin}x inside a guard: change the seed, not the bar", floors, biggest)
    return floors


def check_param_gradients(got, want_grad, f32_grad, report=print, rows=None):
    """The project's standing bar (`check_against_float64`) per parameter column: rel-Linf <= max(1e-4, 4 x floor) under `fair`'s guards.  Every
    figure is printed before it is gated."""
    sel = slice(None) if rows is None else rows
    errs = column_errors(np.asarray(got, np.float64)[sel], want_grad[sel])
    for c, e in enumerate(errs):
        report(f"  column {c}: err {e:.2e}")
    floors = fair(want_grad, f32_grad, report, rows)
    assert np.isfinite(got).all()
    bad = [(c, errs[c], floors[c]) for c in range(len(errs)) if errs[c] > max(1e-4, 4 * floors[c])]
    assert not bad, bad
    return SimpleNamespace(errs=errs, floors=floors)


# ---- fitting end to end: a teacher renders 2 images x 128 rays x 32 samples at known parameters, the fit starts 0.2 off ------------------------
FIT = dict(n_parameters=(1, 4), arch=dict(width=64, depth=3, skips=[1]), fam="grass", images=2, rays=128, S=32, offset=0.2, lrate=1e-2, n_iters=150, seed=0, batch_seed=3,
           loss_name="alpha_mse_soft")


def fit_setup():
    """(model, spec, weights, batch dict [B,R,...] with the teacher's float64 renders as targets, the true parameters [B,P], the start)."""
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    f = FIT
    model, spec, wts = make_model(f["n_parameters"], seed=f["seed"], dense_media=True, arch=f["arch"])
    B, R, S = f["images"], f["rays"], f["S"]
    ro, rd, t, cone, params, _, _ = flex_batch(f["batch_seed"], B * R, S, spec, f["fam"])
    true = np.ascontiguousarray(params[::R], F)
    z = orc.z_values(t, S, F)
    with torch.no_grad():
        t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
        c, a = tro.render([t64(x) for x in wts], spec, t64(ro), t64(rd), t64(z), t64(np.repeat(true, R, 0)), t64(cone))
    batch = dict(rays_o=ro.reshape(B, R, 3), rays_d=rd.reshape(B, R, 3), t=t.reshape(B, R, 2), cone_scale=cone.reshape(B, R, 1),
                 color=c.numpy().astype(F).reshape(B, R, 3), alpha=a.numpy().astype(F).reshape(B, R), parameters=true)
    return model, spec, wts, batch, true, (true + F(f["offset"])).astype(F)


def restated_fit(spec, wts, batch, init, loss, n_iters, lrate):
    """`ParameterFitter.fit` on the CPU: float64 autograd of the restated step (free branches), the same torch Adam.  Returns (parameters, losses)."""
    B, R = batch["rays_o"].shape[:2]
    S = FIT["S"]
    flat = lambda k, *s: np.asarray(batch[k]).reshape(B * R, *s)
    z = orc.z_values(flat("t", 2), S, F)
    p = torch.tensor(np.asarray(init), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lrate)
    losses = []
    for _ in range(n_iters):
        val, _, g = restated_param_gradients(wts, spec, flat("rays_o", 3), flat("rays_d", 3), z, p.detach().numpy(), R, flat("cone_scale"), flat("color", 3), flat("alpha"), loss)
        p.grad = torch.tensor(g)
        opt.step()
        losses.append(val)
    return p.detach().numpy(), losses
