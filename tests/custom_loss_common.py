"""What the tests of training under any loss share (tests/test_custom_loss.py on the CPU, tests/test_gpu_custom_loss.py on the GPU): a loss the
library does not know, and the float64 restatement of a step under ANY head -- a loss callable, or fixed cotangents through the surrogate
<c, gC> + <a, gA>, whose gradient is the cotangent adjoint `ntx_train_backward` computes -- with the weights AND the parameter rows as leaves.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED as the rest of the training oracle: the forward pass is oracle/train_oracle.py's `render`
(tests/train_branch_oracle.py's for a model with parameter branches), branched by the ReLU patterns a trainer kept; the gradients are what
torch autograd derives from it."""

from types import SimpleNamespace

import numpy as np
import torch

from oracle import train_oracle as tro
from tests import param_grad_common as pgc
from tests import train_branch_oracle as tbo
from tests.train_common import BKGD, F, layer_slices, rel_linf

N_RAYS, N_SAMPLES = 45, 37             # 1665 samples: off the contraction's 128-row tile and off 32 (tests/train_branch_oracle.py)


class CharbonnierAlpha:
    """None of the built-in losses: Charbonnier on the colours, mean(sqrt((c - t)^2 + eps)), plus gamma * mean((a - alpha)^2 (1 + alpha)).
    Called as the reference calls a loss (loss.py:12, 30); a `loss_config` may name it by its module path."""

    def __init__(self, eps: float = 1e-3, gamma: float = 0.1) -> None:
        self.eps, self.gamma = float(eps), float(gamma)

    def __call__(self, color_true, alpha_true, color_pred, alpha_pred):
        return torch.mean(torch.sqrt((color_pred - color_true) ** 2 + self.eps)) + self.gamma * torch.mean((alpha_pred - alpha_true) ** 2 * (1 + alpha_true))


def loss_head(loss, color_true, alpha_true):
    """The head `restated` takes, from a loss callable and the targets."""
    def head(c, a):
        t_ = lambda x: torch.tensor(np.asarray(x), dtype=c.dtype)
        return loss(color_true=t_(color_true), alpha_true=t_(alpha_true), color_pred=c, alpha_pred=a)
    return head


def surrogate_head(d_color, d_alpha=None):
    """<c, gC> + <a, gA>: linear in the predictions, so its gradient with respect to anything is the adjoint applied to the cotangents."""
    def head(c, a):
        val = (c * torch.tensor(np.asarray(d_color), dtype=c.dtype)).sum()
        return val if d_alpha is None else val + (a * torch.tensor(np.asarray(d_alpha), dtype=a.dtype)).sum()
    return head


def restated(w_np, spec, rays_o, rays_d, z, rows, rays_per_param_row, cone_scale, head, blur_idx=None, map_exr=False, composite_bkgd=False, bkgd=BKGD,
             dtype=torch.float64, masks=None, branch_masks=None, sigma_mask=None, noise=None):
    """One step under `head(color_pred, alpha_pred) -> scalar`: rays whose depths are not finite are filtered out, the rest rendered, the
    results scattered back into zeros (plus the background when compositing), the head over ALL rays (renderer.py:58-86) -- as
    `tro.step_gradients` and `pgc.restated_param_gradients` have it, with both the weights and the parameter rows [n_rows, P] as leaves.
    Returns loss, pred = [color | alpha], grad (flat, get_weights() order), param_grad [n_rows, P], and d_color / d_alpha = the head's own
    gradient at the predictions."""
    z = np.asarray(z)
    n, S = z.shape[0], z.shape[1] - (spec.pos_encoding == "ipe")
    hit = np.isfinite(z).all(1)
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    sub = lambda x: None if x is None else t_(np.asarray(x)[hit])
    per_sample = lambda ms: None if ms is None else [sub(m.reshape(n, S, -1)).flatten(0, 1) for m in map(np.asarray, ms)]
    w = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in w_np]
    leaf = torch.tensor(np.asarray(rows, np.float64).reshape(-(-n // int(rays_per_param_row)), -1), dtype=dtype, requires_grad=True)
    per_ray = leaf.repeat_interleave(int(rays_per_param_row), 0)[:n]
    c = torch.zeros((n, 3), dtype=dtype); a = torch.zeros((n,), dtype=dtype)
    if hit.any():
        idx = torch.as_tensor(np.nonzero(hit)[0])
        args = (w, spec, sub(rays_o), sub(rays_d), sub(z), per_ray[idx], sub(cone_scale), blur_idx, map_exr, composite_bkgd, bkgd, per_sample(masks))
        if pgc.has_branches(spec):
            ch, ah = tbo.render(*args, per_sample(branch_masks), sub(sigma_mask), sub(noise))
        else:
            ch, ah = tro.render(*args, sub(sigma_mask), sub(noise))
        c = c.index_put((idx,), ch); a = a.index_put((idx,), ah)
    if composite_bkgd:
        c = c + torch.as_tensor((~hit)[:, None] * np.asarray(bkgd, np.float64)[None, :], dtype=dtype)
    assert hit.any(), "a batch without a hit ray has no gradient to restate"
    c.retain_grad(); a.retain_grad()
    val = head(c, a)
    val.backward()
    grads = [np.zeros(x.shape) if x.grad is None else x.grad.numpy().astype(np.float64) for x in w]
    zero = lambda x: np.zeros(x.shape) if x.grad is None else x.grad.numpy().astype(np.float64)
    return SimpleNamespace(loss=float(val.detach()), pred=np.concatenate([c.detach().numpy(), a.detach().numpy()[:, None]], -1),
                           grad=np.concatenate([g.ravel() for g in grads]), param_grad=zero(leaf), d_color=zero(c), d_alpha=zero(a))


def composite_cotangent_adjoint(raw_rgb, sigma, dists, d_color, d_alpha, map_exr=False, composite_bkgd=False, bkgd=BKGD, noise=None, dtype=torch.float64, z=None,
                                rays_d=None, mip=False):
    """The composite's cotangent adjoint alone: (dL/d raw colour [n, S, 3], dL/d raw density [n, S], color_pred, alpha_pred) = autograd of
    `tro.composite` on GIVEN raw network outputs under the surrogate of the cotangents -- what `composite_adjoint_kernel` is held to, the
    network's rounding left out (tests/train_common.adjoint_errors does the same for the fused kernel).  The sample lengths: `dists` [n, S], or
    (None) formed in `dtype` from the depths `z` and `rays_d` as `tro.composite_gradients` forms them (`mip`: segment edges [n, S + 1])."""
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    rgb = torch.tensor(np.asarray(raw_rgb), dtype=dtype, requires_grad=True); sg = torch.tensor(np.asarray(sigma), dtype=dtype, requires_grad=True)
    lengths = t_(dists) if dists is not None else (tro.mip_dists if mip else tro.fourier_dists)(t_(z), t_(rays_d))
    c, a = tro.composite(rgb, sg, lengths, map_exr, composite_bkgd, bkgd, None, t_(noise))
    surrogate_head(d_color, d_alpha)(c, a).backward()
    return rgb.grad.numpy(), sg.grad.numpy(), c.detach().numpy(), a.detach().numpy()


def chain_patterns(tr, n, S, noise):
    """(masks, None, sigma_mask) of the step a chain `Trainer` has just taken (slots 0-9 and 10, as tests/train_common.restated_step reads them)."""
    torch.cuda.synchronize()
    masks = [tr.activation(k, n * S) > 0 for k in list(range(8)) + [8, 9]]
    return masks, None, (tr.activation(10, n * S).reshape(n, S) + (0 if noise is None else noise.astype(F))) > 0


def check_layers(got, spec, want, f32, report=print):
    """`tests.train_flex_common.check_against_float64`'s convention on a flat gradient: every kernel and bias within max(1e-4, 4 x floor) rel-Linf
    of float64, the floor being float32 autograd of the same restatement on the same branches; every floor <= 5e-4 and a gradient worth the name,
    so that the floor cannot hide a failure.  Every figure is printed before it is gated."""
    rows = []
    for name, sl in layer_slices(spec):
        rows.append((name, rel_linf(got[sl], want.grad[sl]), rel_linf(f32.grad[sl], want.grad[sl]), float(np.abs(want.grad[sl]).max())))
        report(f"  {name:<24} err {rows[-1][1]:.2e} floor {rows[-1][2]:.2e} max {rows[-1][3]:.3e}")
    assert np.isfinite(got).all()
    assert np.abs(want.grad).max() > 1e-6 and all(r[3] > 0 for r in rows), "the batch gives no gradient worth the name: change the seed"
    assert all(r[2] <= 5e-4 for r in rows), ("a float32 floor above 5e-4: change the seed, not the bar", [r for r in rows if r[2] > 5e-4])
    bad = [r for r in rows if r[1] > max(1e-4, 4 * r[2])]
    assert not bad, bad
    return rows


# ---- the three trainers of the end-to-end and special-case tests at 45 x 37: (id, trainer class name, n_parameters, arch, family, knobs) ----------
TRAINER_CASES = [
    ("chain", "Trainer", (1, 6), None, "carpet", dict(perturb=True)),
    ("flex_w98_skips13", "FlexTrainer", (1, 6), dict(width=98, depth=5, skips=[1, 3]), "carpet", dict(perturb=True, rpr=15)),
    ("branches_f", "BranchTrainer", (1, 4), dict(depth=3, width=64, skips=[1], color_depth=1, param_depth=2, param_width=128), "grass", dict(rpr=15)),
]
DEFAULTS = dict(perturb=False, rpr=1, blur=None, map_exr=False, noise_std=0.0, seed=11, batch_seed=3)


def trainer_case(case, n=N_RAYS, S=N_SAMPLES):
    """(model, spec, weights, (ro, rd, t, cone, rows, color, alpha), knobs) of a case: `tests.train_flex_common.flex_batch` (the branch case:
    `tbo.branch_batch`), the parameter rows the first ray's of every `rpr` rays."""
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    cid, cls, npar, arch, fam, knobs = case
    kn = dict(DEFAULTS, **knobs)
    model, spec, wts = make_model(npar, dense_media=True, arch=arch)
    ro, rd, t, cone, params, color, alpha = (tbo.branch_batch(kn["batch_seed"], n, spec, fam) if pgc.has_branches(spec) else flex_batch(kn["batch_seed"], n, S, spec, fam))
    rows = np.ascontiguousarray(params[::kn["rpr"]], F)
    return model, spec, wts, (ro, rd, t, cone, rows, color, alpha), kn
