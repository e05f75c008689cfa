"""What the training tests of both renderers share (tests/test_gpu_train.py, tests/test_gpu_train_mip.py, tests/test_train_mip.py):
the relative error they gate on, the losses by name on the oracle's and the product's side, the layers' places in the flat gradient,
seeded targets and the mip batch, and the step of oracle/train_oracle.py restated beside a `Trainer` that has just taken one."""

from types import SimpleNamespace

import numpy as np
import torch

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro

F = np.float32
BKGD = (1., .5, .25)


def rel_linf(got, want):
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / max(np.max(np.abs(want)), 1e-300))


LOSSES = {"alpha_smape": (dict(kind="alpha", loss_fn="smape", alpha_loss_fn="mse"), dict(loss_fn="network.loss.smape", alpha_loss_fn="network.loss.mse")),
          "alpha_mse_soft": (dict(kind="alpha", loss_fn="mse", gamma=0.5, use_hard_mask=False), dict(loss_fn="network.loss.mse", gamma=0.5, use_hard_mask=False)),
          "nerf_mse": (dict(kind="nerf", loss_fn="mse"), dict(loss_fn="network.loss.mse"))}


def make_loss(name):
    """(the oracle's loss dict, the product's loss object)."""
    from nerf_tex_amd import loss as L
    okw, pkw = LOSSES[name]
    return okw, (L.AlphaLoss(**pkw) if okw["kind"] == "alpha" else L.NerfLoss(**pkw))


def layer_slices(spec):
    out, p = [], 0
    for name, i, o in orc.layer_table(spec):
        out.append((name + ".kernel", slice(p, p + i * o))); p += i * o
        out.append((name + ".bias", slice(p, p + o))); p += o
    return out


def targets(n, seed):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0, 1, size=(n, 3)).astype(F)
    alpha = (rng.uniform(0, 1, size=n) > 0.3).astype(F) * rng.uniform(0.5, 1, size=n).astype(F)
    return color, alpha


def mip_batch(n, P_in, seed=0):
    from nerf_tex_amd import synthetic
    f = synthetic.FAMILIES["grass_filtered"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"], seed=seed + 1)
    rng = np.random.default_rng(seed)
    params = rng.uniform(0.2, 1.5, size=(n, P_in)).astype(F)
    return ro, rd, t, cone, params


def restated_step(tr, spec, wts, ro, rd, t, params, cone, color, alpha, okw, *, seed, perturb, noise_std=0.0, miss=None, blur_idx=None, bkgd=False,
                  bkgd_color=BKGD, chunk_rays=None, workers=1, free=False, dtype=torch.float64):
    """The step `tr.gradients_step(..., seed=seed)` has just taken, restated: the sample depths the kernel placed itself (renderer.py:101-111:
    S of them, or the S + 1 segment edges of an IPE trainer, :374-383; with perturb the product's Philox jitter) and the density
    regulariser's draws (renderer.py:190-192, keyed like the jitter by (seed, ray, sample)), the rays of `miss` at z = inf, through
    `tro.step_gradients`.  Unless `free`, float64 autograd is branched like the float32 forward pass was: by the signs of the activations the
    step kept (a pre-activation within rounding of zero falls on either side of its ReLU depending on summation order -- in TensorFlow's
    float32 as much as here), the density's with the noise added.
    Returns the oracle's `loss`, `pred` = [color | alpha] and flat gradient `grad`, the trainer's `got`, `layers` = rel-Linf of every
    layer's kernel and bias against its own largest entry, and `z`, `noise`, `masks`."""
    n, S = len(t), tr.n_samples
    miss = np.zeros(n, bool) if miss is None else np.asarray(miss, bool)
    edges = S + 1 if spec.pos_encoding == "ipe" else S
    tf = np.where(np.isfinite(t), t, 0).astype(F)
    z = orc.z_values_perturbed(tf, edges, seed, F) if perturb else orc.z_values(tf, edges, F)
    z = z.copy(); z[miss] = np.inf
    noise = noise_std * orc.noise_normals(n, S, seed, dtype=F).astype(np.float64) if noise_std > 0 else None
    torch.cuda.synchronize()
    masks = sigma_mask = None
    if not free:
        masks = [tr.activation(k, n * S) > 0 for k in list(range(8)) + [8, 9]]              # bool: 67 MB each at the configs' batch
        sigma_mask = (tr.activation(10, n * S).reshape(n, S) + (0 if noise is None else noise.astype(F))) > 0
    val, c, a, g = tro.step_gradients(wts, spec, ro, rd, z, params, np.nan_to_num(cone), color, alpha, okw, blur_idx=blur_idx, composite_bkgd=bkgd,
                                      bkgd=bkgd_color, dtype=dtype, masks=masks, sigma_mask=sigma_mask, noise=noise, chunk_rays=chunk_rays, workers=workers)
    got, flat = tr.gradients(), np.concatenate([x.ravel() for x in g])
    assert flat.size == got.size == tr.n_weights
    return SimpleNamespace(loss=val, pred=np.concatenate([c, a[:, None]], -1), grad=flat, got=got, z=z, noise=noise, masks=masks,
                           layers={name: rel_linf(got[sl], flat[sl]) for name, sl in layer_slices(spec)})


def step_pred(color_pred, alpha_pred):
    """[color | alpha] of a `gradients_step`'s GPU tensors."""
    return np.concatenate([color_pred.cpu().numpy(), alpha_pred.cpu().numpy()[:, None]], -1)
