"""What the tests of dL/d parameters and dL/d rays on the FUSED chain share (tests/test_fused_gradients.py on the CPU,
tests/test_gpu_fused_gradients.py on the GPU; `ntx_trainer_enable_gradients`, `Trainer(param_gradients=, input_gradients=)`): the cases, the
step helpers and the product behind the new kernel.

No yardstick of its own: dL/d parameter rows is tests/param_grad_common.py's restatement, dL/d rays tests/input_grad_common.py's, the ReLU
patterns tests/custom_loss_common.chain_patterns' (slots 0-9 and 10 of a chain handle), the bar `pgc.check_param_gradients` per column.  Every
case is 8 x 256 / skips [4] / color_depth 1 (or the width-128 network `_widened` pads into it) with un-normalised rays_d
(`igc.unnormalised`).  Seeds are chosen on the CPU: tests/test_fused_gradients.py::test_the_gpu_cases_are_fair holds every case 2x inside
both guards of `pgc.fair`, for both gradients."""

from unittest import mock

import numpy as np
import torch

from oracle import train_oracle as tro
from tests import custom_loss_common as clc
from tests import input_grad_common as igc
from tests import param_grad_common as pgc
from tests.train_common import BKGD, F, make_loss, step_noise, step_pred

MARGIN = pgc.MARGIN

# (id, n_parameters, arch, freqs, family, knobs, (step seed, batch seed)) as `pgc.case_setup` takes them; arch None: 8 x 256 / [4] / 1.
# 70 rays x 33 samples = 2310 samples = 72 blocks of 32 and a tail of 6
PARITY_CASES = [
    ("carpet_1_6", (1, 6), None, None, "carpet", dict(), (11, 3)),                                                  # Kp 72, Kd 81: three tiles each
    ("grass_1_4", (1, 4), None, None, "grass", dict(), (11, 3)),
    ("grass_filtered_blur_geo", (2, 3), None, None, "grass_filtered", dict(blur=0, perturb=True, noise_std=0.1), (11, 4)),      # Kp 81
    ("blur_app_no_hoist", (2, 3), None, None, "grass_filtered", dict(blur=3), (11, 3)),                             # the forward's per-ray direction hoist is off
    ("narrowest_1_0_0", (1, 6), None, (1, 0, 0), "carpet", dict(model_seed=1), (11, 3)),                            # Kp 10, Kd 9: one partial tile each (seed 0's density is shut everywhere)
    ("widest_3_7", (3, 7), None, (10, 4, 4), "carpet", dict(), (11, 4)),                                            # Kp = Kd = 90: the last tile nearly full
    ("width_128_widened", (1, 6), dict(width=128), None, "carpet", dict(), (11, 3)),
]
# the small carpet batch around a block of 32 samples and around the forward's hoist (S a multiple of 32 or not)
SAMPLE_CASES = [(f"samples_{n}x{S}", (1, 6), None, None, "carpet", dict(n=n, S=S, rpr=r), (11, bs)) for n, S, r, bs in
                ((1, 2, 1, 3), (1, 32, 1, 3), (1, 33, 1, 3), (3, 64, 2, 3), (3, 65, 2, 3))]
ROW_CASES = [(f"rows_{r}", (1, 6), None, None, "carpet", dict(rpr=r), (11, 3)) for r in (1, 35, 70)]
MISS_CASE = ("rays_that_miss", (2, 3), None, None, "grass_filtered", dict(rpr=35, miss=pgc.MISS_RAYS, miss_cone="nan_inf", perturb=True, blur=0), (11, 6))
COARSE_CASE = ("coarse_pass", (1, 6), None, None, "carpet", dict(n=24, S=24, rpr=12, perturb=True), (11, 3))
ALL_CASES = PARITY_CASES + SAMPLE_CASES + ROW_CASES + [MISS_CASE, COARSE_CASE]
CASE = {c[0]: c for c in ALL_CASES}


def case_setup(case):
    """`igc.case_setup` (`pgc.case_setup` with un-normalised rays_d); a knob `model_seed`: the synthetic weights of that seed instead of seed 0's."""
    from tests.common import make_model
    cid, npar, arch, freqs, fam, knobs, seeds = case
    model, spec, wts, batch, kn, seed = igc.case_setup((cid, npar, arch, freqs, fam, {k: v for k, v in knobs.items() if k != "model_seed"}, seeds))
    if "model_seed" in knobs:
        model, spec, wts = make_model(npar, seed=knobs["model_seed"], dense_media=True, arch=arch, freqs=freqs)
    return model, spec, wts, batch, kn, seed


def restate_both(spec, wts, batch, kn, seed, dtype, patterns):
    """(loss, dL/d rows, dL/d rays_o, dL/d rays_d) of a case's step from the two yardsticks, on the same ReLU patterns."""
    p = pgc.restate(spec, wts, batch, kn, seed, dtype, *patterns)
    r = igc.restate(spec, wts, batch, kn, seed, dtype, *patterns)
    return p[0], p[2], r[2], r[3]


def fair_both(want, f32, kn, report=print):
    """Both gradients of a case `MARGIN` times inside `pgc.fair`'s guards, over the parameter rows / the rays that hit."""
    miss = kn["miss"]
    ray_rows = ~miss if miss.any() else None
    row_hit = None
    if miss.any():                                                                # a parameter row without a ray that hits has no gradient
        n_rows = want[1].shape[0]
        row_hit = np.array([(~miss[r * kn["rpr"]:(r + 1) * kn["rpr"]]).any() for r in range(n_rows)])
    pgc.fair(want[1], f32[1], report, rows=row_hit, margin=MARGIN)
    pgc.fair(igc.columns(want[2], want[3]), igc.columns(f32[2], f32[3]), report, rows=ray_rows, margin=MARGIN)
    return row_hit, ray_rows


def feature_gradients(dy0, dy5, dc1o, w_trunk0, w_trunk5, w_c1, Kp, Kd):
    """The product behind the chain's new kernel, on numpy arrays or torch tensors of one dtype: per sample
    G_pos = dy0 . W_trunk0[:Kp]^T + dy5 . W_trunk5[:Kp]^T and G_dir = dc1o . W_c1[:Kd]^T, the dY the gradients at the three layers'
    pre-activations, the W rows the pos_map / dir_map rows of the three kernels."""
    return dy0 @ w_trunk0[:Kp].T + dy5 @ w_trunk5[:Kp].T, dc1o @ w_c1[:Kd].T


def layer_kernels(spec, wts):
    """(W_trunk0 [Kp, 256], W_trunk5 [Kp + w, w], W_c1 [Kd + w, w]) of an 8-deep / skips [4] / color_depth 1 weight list in get_weights() order."""
    w0, w5, wc1 = wts[0], wts[10], wts[18]
    Kp = w0.shape[0]
    assert w5.shape[0] == Kp + spec.width and wc1.shape[0] > spec.width and wc1.shape[1] == spec.width and wts[16].shape == (spec.width, spec.width)
    return w0, w5, wc1


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------------
def chain_trainer(model, kn, pm=True, im=True, max_rays=None, n_samples=None):
    """The fused chain's trainer of a case, made for the case's own size unless another is given."""
    from nerf_tex_amd.train import Trainer
    return Trainer(model, max_rays=max_rays or kn["n"], n_samples=n_samples or kn["S"], perturb=kn["perturb"], blur_idx=kn["blur"], raw_noise_std=kn["noise_std"],
                   map_exr=kn["map_exr"], param_gradients=pm, input_gradients=im)


def results(tr):
    """What the step `tr` has just taken left beside the weight gradient, on the host: (d_rays_o, d_rays_d) or None, dL/d rows or None."""
    rays = tuple(g.cpu().numpy() for g in tr.ray_gradients()) if tr.input_gradients else None
    pg = tr.parameter_gradients().cpu().numpy() if tr.param_gradients else None
    torch.cuda.synchronize()
    return rays, pg


def step(tr, batch, kn, seed):
    """One `gradients_step` of a case; (loss, [color | alpha], (d_rays_o, d_rays_d) or None, dL/d rows or None) on the host."""
    ro, rd, t, cone, rows, color, alpha = batch
    _, loss = make_loss(kn["loss_name"])
    val, cp, ap = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, composite_bkgd=kn["bkgd"], bkgd_color=BKGD, seed=seed, rays_per_param_row=kn["rpr"],
                                    n_samples=kn["S"], z_vals=kn["z"])
    return (float(val.item()), step_pred(cp, ap)) + results(tr)


def held_to_the_bar(tr, spec, wts, batch, kn, seed, val, rays, pg, name=""):
    """Whatever of (d_rays_o, d_rays_d) and dL/d rows the step `tr` has just taken left, against the float64 restatements of that step
    branched by the signs of the activations the chain kept; the missed rays' rows and a row without a hit are exactly 0.  Returns the
    restatement (loss, dL/d rows, dL/d rays_o, dL/d rays_d)."""
    n, S = kn["n"], kn["S"]
    patterns = clc.chain_patterns(tr, n, S, step_noise(n, S, seed, kn["noise_std"]))
    want = restate_both(spec, wts, batch, kn, seed, torch.float64, patterns)
    f32 = restate_both(spec, wts, batch, kn, seed, torch.float32, patterns)
    print(f"{name}: {n} x {S}: loss {val if val is None else format(val, '.9g')} want {want[0]:.9g}")
    if val is not None:
        assert abs(val - want[0]) <= 1e-5 * abs(want[0])
    miss = kn["miss"]
    row_hit = None
    if miss.any():
        row_hit = np.array([(~miss[r * kn["rpr"]:(r + 1) * kn["rpr"]]).any() for r in range(want[1].shape[0])])
    if pg is not None:
        assert pg.shape == want[1].shape and pg.dtype == np.float32 and np.isfinite(pg).all()
        if row_hit is not None:
            assert not pg[~row_hit].any() and not want[1][~row_hit].any()
        res = pgc.check_param_gradients(pg, want[1], f32[1], rows=row_hit)
        print(f"FGERR {name} parameters worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")
    if rays is not None:
        assert rays[0].shape == rays[1].shape == (n, 3) and rays[0].dtype == rays[1].dtype == np.float32
        assert np.isfinite(rays[0]).all() and np.isfinite(rays[1]).all()
        assert not rays[0][miss].any() and not rays[1][miss].any() and not want[2][miss].any() and not want[3][miss].any()
        res = igc.check_input_gradients(rays, want[2:], f32[2:], rows=~miss if miss.any() else None)
        print(f"FGERR {name} rays worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")
    return want


def restate_under(loss_callable, spec, wts, batch, kn, seed, dtype, patterns):
    """`restate_both` under a loss written in torch, `loss(color_true=, alpha_true=, color_pred=, alpha_pred=)`: the same two yardsticks with
    the oracle's loss dispatch (`tro._loss`) handing the predictions to the callable for the length of the call."""
    ro, rd, t, cone, rows, color, alpha = batch
    z, noise = pgc._depths(t, kn, seed, kn["miss"]), step_noise(len(t), kn["S"], seed, kn["noise_std"])
    call = lambda loss, ct, at, c, a: loss(color_true=ct, alpha_true=at, color_pred=c, alpha_pred=a)
    kw = dict(blur_idx=kn["blur"], map_exr=kn["map_exr"], composite_bkgd=kn["bkgd"], bkgd=BKGD, dtype=dtype, masks=patterns[0], branch_masks=patterns[1],
              sigma_mask=patterns[2], noise=noise)
    with mock.patch.object(tro, "_loss", call):
        p = pgc.restated_param_gradients(wts, spec, ro, rd, z, rows, kn["rpr"], pgc._cone(cone), color, alpha, loss_callable, **kw)
        r = igc.restated_ray_gradients(wts, spec, ro, rd, z, rows, kn["rpr"], pgc._cone(cone), color, alpha, loss_callable, **kw)
    return p[0], p[2], r[2], r[3]
