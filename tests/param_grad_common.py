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
ALL_CASES = MODEL_CASES + ROW_CASES + OPTION_CASES + [MISS_CASE]
DEFAULTS = dict(loss_name="alpha_smape", bkgd=False, map_exr=False, perturb=False, blur=None, noise_std=0.0, rpr=35, miss=())


def case_setup(case, n=N_RAYS, S=N_SAMPLES):
    """(model, spec, weights, (ro, rd, t, cone, rows, color, alpha), knobs with every default, step seed) of a case: the batch is
    `tests.train_flex_common.flex_batch`'s, the parameter rows the first ray's of every `rpr` rays; the rays of `miss` get t = inf and
    cone_scale = NaN."""
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    cid, npar, arch, freqs, fam, knobs, (seed, batch_seed) = case
    model, spec, wts = make_model(npar, dense_media=True, arch=arch, freqs=freqs)
    kn = dict(DEFAULTS, **knobs)
    ro, rd, t, cone, params, color, alpha = flex_batch(batch_seed, n, S, spec, fam)
    rows = np.ascontiguousarray(params[::kn["rpr"]], F)
    miss = np.zeros(n, bool); miss[list(kn["miss"])] = True
    t = t.copy(); t[miss] = np.inf
    cone = cone.copy(); cone[miss] = np.nan
    kn["miss"] = miss
    return model, spec, wts, (ro, rd, t, cone, rows, color, alpha), kn, seed


def restate(spec, wts, batch, kn, seed, S, dtype, masks, branch_masks, sigma_mask):
    """`restated_param_gradients` of a case's step on the depths and the noise the step places itself."""
    from tests.train_common import LOSSES
    ro, rd, t, cone, rows, color, alpha = batch
    z, noise = step_depths(t, S, seed, kn["perturb"], kn["miss"]), step_noise(len(t), S, seed, kn["noise_std"])
    return restated_param_gradients(wts, spec, ro, rd, z, rows, kn["rpr"], np.nan_to_num(cone), color, alpha, LOSSES[kn["loss_name"]][0], blur_idx=kn["blur"],
                                    map_exr=kn["map_exr"], composite_bkgd=kn["bkgd"], bkgd=BKGD, dtype=dtype, masks=masks, branch_masks=branch_masks, sigma_mask=sigma_mask,
                                    noise=noise)


def own_patterns(spec, wts, batch, kn, seed, S):
    """The ReLU patterns of a float32 forward pass of the restatement itself (the hit rays' real, the others' whatever: they are filtered):
    what a float32 step would hand to float64 -- the CPU's stand-in for the patterns a trainer keeps."""
    ro, rd, t, cone, rows, color, alpha = batch
    n = len(t)
    z, noise = step_depths(t, S, seed, kn["perturb"]), step_noise(n, S, seed, kn["noise_std"])
    per_ray = np.repeat(rows, kn["rpr"], 0)[:n]
    return tbo.own_masks(wts, spec, ro, rd, z, per_ray, np.nan_to_num(cone), blur_idx=kn["blur"], noise=noise)


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


def fair(want_grad, f32_grad, report=print, rows=None):
    """The guards that keep the floor from hiding a failure, per parameter column (over `rows`, default all): the float32 restatement within 5e-4
    of float64, and a gradient worth the name (max |grad| > 1e-6).  Returns the floors."""
    sel = slice(None) if rows is None else rows
    floors, biggest = column_errors(f32_grad[sel], want_grad[sel]), np.abs(want_grad[sel]).max(0)
    for c in range(len(floors)):
        report(f"  column {c}: floor {floors[c]:.2e} max |grad| {biggest[c]:.3e}")
    assert (biggest > 1e-6).all(), ("a parameter column without a gradient worth the name: change the seed, not the bar", biggest)
    assert (floors <= 5e-4).all(), ("a float32 floor above 5e-4: change the seed, not the bar", floors)
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
