"""What the tests of a `ProposalTrainer` step against float64 share (tests/test_proposal_step.py on the CPU, tests/test_gpu_proposal_step.py on
the GPU; `nerf_tex_amd.train.ProposalTrainer`): the pair of networks, the batch, and the step stated independently of the
product's pieces -- two `wlc.restated_step`s on constant depths.

THE STEP IN FLOAT64.  The depths are constants (no gradient passes through the sampler): z_prop [n, S_p], what the proposal's forward places,
and z_all [n, S], the merged depths of the fine pass.
  1. the fine network at z_all under the caller's loss: the fine loss, its predictions, its gradient, and the fine weights w_f;
  2. the proposal network at z_prop under  (c, a, w) -> interlevel_weight * mean_n ic.dense_torch(w_f.detach(), z_all, w, z_prop):  the dense
     [n, S, S_p] mask statement under autograd, not the kernel's formula; n counts every ray.
The same pair in float32 gives the floors.  TEST INFRASTRUCTURE ONLY, PARITY UNPINNED as the rest of the training oracle.

The bars are the standing ones, imported and not edited: `clc.check_layers` (max(1e-4, 4 float32 floors), floor <= 5e-4, max |grad| > 1e-6) on
the layers, 1e-5 on a loss and 1e-4 on predictions (tests/test_gpu_train_flex.py), `dc.gate` on the kernel.  tests/test_proposal_step.py holds
every compared layer `pgc.MARGIN` times inside `check_layers`' guards on the CPU."""

from types import SimpleNamespace
from unittest import mock

import numpy as np
import torch

from tests import custom_loss_common as clc
from tests import interlevel_common as ic
from tests import param_grad_common as pgc
from tests import weight_loss_common as wlc
from tests.train_common import F, layer_slices, rel_linf, step_depths

N_RAYS, S_PROP, N_IMP, LAMBDA = 24, 40, 30, 0.5          # 70 fine samples: past one chunk of 64, and a multiple of nothing
SMALL = dict(width=64, depth=3, skips=[1])
OTHER = dict(width=128, depth=4, skips=[2])
# the seeds are the ones to change if a layer or a value leaves its guard on the CPU (tests/test_proposal_step.py), never a bar: with model seeds
# (0, 1) and ray seed 1 float32 autograd of the restatement itself is off by 7.6e-6 / 2.2e-5 in the interlevel term -- the term is a sum of
# clipped differences w - bound, and where the proposal bounds the fine weights well it is small against what it is the difference of
MODEL_SEEDS, RAY_SEED, BATCH_SEED, STEP_SEED, U_SEED = (4, 5), 2, 14, 5, 2
# (id, the loss's route, perturb, the fine network's architecture): the two routes obtain the fine weights differently (`_weights_into`, or the
# wrapped callable); with perturb the sampler draws tf.linspace, without it the given u
SETTINGS = [("descriptor-perturb", "descriptor", True, SMALL), ("callable-fixed-other", "callable", False, OTHER)]
SETTING_IDS = [s[0] for s in SETTINGS]


def pair(fine_arch):
    """((proposal model, spec, weights), (fine model, spec, weights)): two `Nerf`s, the proposal always 3 x 64."""
    from tests.common import make_model
    return make_model((0, 0), kind="Nerf", seed=MODEL_SEEDS[0], dense_media=True, arch=SMALL), make_model((0, 0), kind="Nerf", seed=MODEL_SEEDS[1], dense_media=True, arch=fine_arch)


def the_batch(spec):
    """((ro, rd, t, cone, params [n, 0], color, alpha), u [n, N_IMP]): 24 carpet rays, every one a hit (`wlc.restated_step` takes finite depths)."""
    from nerf_tex_amd import synthetic
    from tests.train_common import targets
    f = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(N_RAYS, f["b_0"], f["b_1"], f["cam"], seed=RAY_SEED)
    assert np.isfinite(t).all() and sum(spec.n_parameters) == 0
    color, alpha = targets(N_RAYS, BATCH_SEED)
    return (ro, rd, t, cone, np.zeros((N_RAYS, 0), F), color, alpha), np.random.default_rng(U_SEED).uniform(size=(N_RAYS, N_IMP)).astype(F)


def charbonnier(color_true, alpha_true, color_pred, alpha_pred):
    """A loss the library does not know (any dtype, any device)."""
    return torch.sqrt((color_pred - color_true) ** 2 + 1e-3).mean() + 0.5 * ((alpha_pred - alpha_true) ** 2).mean()


def product_loss(route):
    from nerf_tex_amd.loss import NerfLoss
    return NerfLoss() if route == "descriptor" else charbonnier


def fine_head(route, color, alpha):
    """The caller's loss as the restatement's head(c, a, w): NerfLoss() is mean((c - color)^2) (network/loss.py:6-19), written out here."""
    def head(c, a, w):
        t_ = lambda x: torch.tensor(np.asarray(x), dtype=c.dtype)
        return torch.mean((c - t_(color)) ** 2) if route == "descriptor" else charbonnier(t_(color), t_(alpha), c, a)
    return head


def interlevel_head(w_fine, z_all, z_prop, lam=LAMBDA):
    """(c, a, w) -> lam * mean over ALL rays of the dense statement; the fine weights and both sets of depths are constants."""
    def head(c, a, w):
        t_ = lambda x: torch.tensor(np.asarray(x), dtype=w.dtype)
        return lam * ic.dense_torch(t_(w_fine), t_(z_all), w, t_(z_prop)).mean()
    return head


def restated_pair(prop, fine, batch, z_prop, z_all, route, patterns_prop, patterns_fine, dtype=torch.float64, lam=LAMBDA):
    """(fine step, proposal step) in `dtype`: `wlc.restated_step`'s namespaces; `prop`, `fine` = (spec, weights), `patterns_*` = (masks, sigma_mask)."""
    color, alpha = batch[5], batch[6]
    f = wlc.restated_step(fine[1], fine[0], batch, z_all, 1, fine_head(route, color, alpha), dtype=dtype, masks=patterns_fine[0], sigma_mask=patterns_fine[1])
    p = wlc.restated_step(prop[1], prop[0], batch, z_prop, 1, interlevel_head(f.weights, z_all, z_prop, lam), dtype=dtype, masks=patterns_prop[0],
                          sigma_mask=patterns_prop[1])
    return f, p


def colour_side(name):
    """The layers only the colour depends on ("feature.kernel", "color0.bias", ...): the interlevel term never reaches them."""
    return name.startswith("color") or name.startswith("feature")


def density_slices(spec):
    return [(name, sl) for name, sl in layer_slices(spec) if not colour_side(name)]


def colour_slices(spec):
    return [(name, sl) for name, sl in layer_slices(spec) if colour_side(name)]


def check_density_layers(got, spec, want, f32, report=print):
    """`clc.check_layers`, as it stands, over the proposal network's density-side layers alone (its own `all(max > 0)` is why the colour layers,
    exact zeros on both sides, are held apart)."""
    with mock.patch.object(clc, "layer_slices", density_slices):
        return clc.check_layers(got, spec, want, f32, report)


def fair(spec, want, f32, slices=None, report=print, margin=pgc.MARGIN):
    """Every compared layer `margin` times inside `check_layers`' guards (`wlc.e2e_fair`'s layer part)."""
    rows = [(name, rel_linf(f32.grad[sl], want.grad[sl]), float(np.abs(want.grad[sl]).max())) for name, sl in (slices or layer_slices(spec))]
    for r in rows:
        report(f"  {r[0]:<24} floor {r[1]:.2e} max {r[2]:.3e}")
    assert all(r[2] >= 1e-6 * margin for r in rows), ("a layer without a gradient worth the name: change a seed or interlevel_weight, not the bar", rows)
    assert all(r[1] <= 5e-4 / margin for r in rows), ("a float32 floor less than the margin inside 5e-4: change a seed, not the bar", [r for r in rows if r[1] > 5e-4 / margin])
    return rows


# ---- the CPU's stand-in for the depths and the ReLU patterns a trainer keeps ------------------------------------------------------------------
def own_patterns(spec, wts, batch, z):
    """(masks, sigma_mask) of a float32 forward pass of the restatement itself at depths z."""
    from tests import train_branch_oracle as tbo
    ro, rd, t, cone, params = batch[:5]
    masks, _, sigma_mask = tbo.own_masks(wts, spec, ro, rd, z, params, pgc._cone(cone))
    return masks, sigma_mask


def cpu_depths(prop, batch, perturb, u):
    """(z_prop, z_all) without a device: the step's own depths, and those merged with the reference sampler's draws (renderer.py:125-131) from
    the float32 restatement's proposal weights -- what `ntx_sample_pdf` merges, up to the sampler's conditioning."""
    from oracle import nerftex_oracle as orc
    spec, wts = prop
    z_prop = step_depths(batch[2], S_PROP, STEP_SEED, perturb)
    masks, sigma_mask = own_patterns(spec, wts, batch, z_prop)
    w = wlc.restated_step(wts, spec, batch, z_prop, 1, lambda c, a, w: w.sum(), dtype=torch.float32, masks=masks, sigma_mask=sigma_mask).weights
    mids = (F(0.5) * (z_prop[:, 1:] + z_prop[:, :-1])).astype(F)
    drawn = orc.sample_pdf(mids, w[:, 1:-1].astype(F), N_IMP, det=perturb, u=None if perturb else u, dtype=F)
    return z_prop, np.sort(np.concatenate([z_prop, np.asarray(drawn, F)], 1), 1).astype(F)


# ---- what the product's step hands to its kernel ------------------------------------------------------------------------------------------------
class KernelCall:
    """Stands in `nerf_tex_amd.loss.ray_interlevel` for the length of a block and keeps what the step handed it and what came back."""

    def __init__(self):
        from nerf_tex_amd import loss
        self._loss, self._real, self.calls = loss, loss.ray_interlevel, []

    def __enter__(self):
        def spy(weights, z_vals, weights_prop, z_prop, **kw):
            out = self._real(weights, z_vals, weights_prop, z_prop, **kw)
            self.calls.append(SimpleNamespace(w_fine=weights.detach().clone(), z_all=z_vals.detach().clone(), w_prop=weights_prop.detach().clone(),
                                              z_prop=z_prop.detach().clone(), kw=kw, out=tuple(o.detach().clone() for o in out)))
            return out
        self._patch = mock.patch.object(self._loss, "ray_interlevel", spy)
        self._patch.start()
        return self

    def __exit__(self, *exc):
        self._patch.stop()
        return False
