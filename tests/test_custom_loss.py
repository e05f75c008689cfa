"""Training under any loss, on the CPU: the restatement tests/test_gpu_custom_loss.py holds `ntx_train_forward` / `ntx_train_backward` to
(tests/custom_loss_common.py) against itself and against central finite differences, the fairness of the GPU cases -- seeds are judged HERE,
on float32 against float64 of the restatement alone --, and the two entries in the built library and the header.  `-m "not gpu"`."""

import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import train_oracle as tro                                           # noqa: E402
from tests import custom_loss_common as clc                                      # noqa: E402
from tests import param_grad_common as pgc                                       # noqa: E402
from tests import train_branch_oracle as tbo                                     # noqa: E402
from tests.common import make_model                                              # noqa: E402
from tests.train_common import BKGD, layer_slices, rel_linf, step_depths        # noqa: E402
from tests.train_flex_common import flex_batch                                   # noqa: E402

F = np.float32


@pytest.mark.parametrize("branches", [False, True], ids=["features", "branches"])
def test_the_surrogate_of_the_cotangents_has_the_loss_gradient(branches):
    """8 rays x 6 samples, a 3 x 32 network on [2, 3] parameters, two rays a parameter row, one ray missing, free branches, float64: the
    gradient of <c, gC> + <a, gA> with (gC, gA) = the loss's own gradient at the predictions is the loss's gradient -- weights and parameter
    rows -- to 1e-10: every gradient of a step is linear in the two cotangents, which is all `ntx_train_backward` relies on."""
    arch = dict(width=32, depth=3, skips=[1], **(dict(param_depth=2, param_width=16) if branches else {}))
    model, spec, wts = make_model((2, 3), dense_media=True, arch=arch)
    n, S, rpr = 8, 6, 2
    ro, rd, t, cone, params, color, alpha = flex_batch(5, n, S, spec, "grass_filtered")
    miss = np.zeros(n, bool); miss[3] = True
    z = step_depths(t, S, 0, False, miss)
    args = (wts, spec, ro, rd, z, params[::rpr], rpr, cone)
    kw = dict(blur_idx=0, composite_bkgd=True)
    own = clc.restated(*args, clc.loss_head(clc.CharbonnierAlpha(), color, alpha), **kw)
    sur = clc.restated(*args, clc.surrogate_head(own.d_color, own.d_alpha), **kw)
    e_w, e_p = rel_linf(sur.grad, own.grad), rel_linf(sur.param_grad, own.param_grad)
    print("loss", own.loss, "max |grad|", np.abs(own.grad).max(), np.abs(own.param_grad).max(), "surrogate against the loss", e_w, e_p)
    assert np.abs(own.grad).max() > 1e-6 and np.abs(own.param_grad).max() > 1e-6 and np.abs(own.d_alpha).max() > 0
    assert (own.d_color[miss] != 0).all() and (own.param_grad.shape == (4, 5))            # a missed ray HAS a cotangent: its prediction is the background
    assert np.array_equal(sur.pred, own.pred)
    assert e_w <= 1e-10 and e_p <= 1e-10, (e_w, e_p)


@pytest.mark.parametrize("map_exr,bkgd", [(False, False), (True, False), (False, True), (True, True)], ids=lambda v: str(int(v)))
def test_the_composite_cotangent_adjoint_matches_finite_differences(map_exr, bkgd):
    """3 rays x 7 samples of raw colours and densities either side of 0 (no density within 1e-2 of its ReLU's kink), the density regulariser's
    noise on the odd cases, seeded cotangents of both signs: every entry of the adjoint against (f(x + h) - f(x - h)) / 2h, h = 1e-6, of the
    surrogate in float64: 1e-6 rel-Linf, tests/test_param_gradients.py's bar."""
    rng = np.random.default_rng(7 + 2 * map_exr + bkgd)
    n, S = 3, 7
    raw, sigma = rng.normal(size=(n, S, 3)), rng.normal(size=(n, S)) * 3
    noise = rng.normal(size=(n, S)) * 0.1 if map_exr != bkgd else None
    sigma = np.where(np.abs(sigma + (0 if noise is None else noise)) < 1e-2, sigma + 0.05, sigma)
    dists = rng.uniform(0.05, 0.5, size=(n, S))
    gC, gA = rng.normal(size=(n, 3)), rng.normal(size=n)
    d_rgb, d_sg = clc.composite_cotangent_adjoint(raw, sigma, dists, gC, gA, map_exr, bkgd, BKGD, noise)[:2]

    def f(r, s):
        t64 = lambda x: None if x is None else torch.tensor(x, dtype=torch.float64)
        c, a = tro.composite(t64(r), t64(s), t64(dists), map_exr, bkgd, BKGD, None, t64(noise))
        return float(clc.surrogate_head(gC, gA)(c, a))

    h, fd_rgb, fd_sg = 1e-6, np.zeros_like(raw), np.zeros_like(sigma)
    for i in np.ndindex(raw.shape):
        up, dn = raw.copy(), raw.copy(); up[i] += h; dn[i] -= h
        fd_rgb[i] = (f(up, sigma) - f(dn, sigma)) / (2 * h)
    for i in np.ndindex(sigma.shape):
        up, dn = sigma.copy(), sigma.copy(); up[i] += h; dn[i] -= h
        fd_sg[i] = (f(raw, up) - f(raw, dn)) / (2 * h)
    e_rgb, e_sg = rel_linf(d_rgb, fd_rgb), rel_linf(d_sg, fd_sg)
    print("max |d rgb|", np.abs(fd_rgb).max(), "max |d sigma|", np.abs(fd_sg).max(), "against finite differences", e_rgb, e_sg)
    assert np.abs(fd_rgb).max() > 1e-3 and np.abs(fd_sg).max() > 1e-3 and (d_sg[sigma + (0 if noise is None else noise) < 0] == 0).all()
    assert e_rgb <= 1e-6 and e_sg <= 1e-6, (e_rgb, e_sg)


def test_both_entries_are_exported_and_declared():
    """`ntx_train_forward` and `ntx_train_backward`: bound from the built library by `_lib.SYMBOLS`, declared in include/nerftex.h, and the ABI
    version is still 7 (they are appended)."""
    from nerf_tex_amd import _lib
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nerftex.h")) as f:
        header = f.read()
    for name in ("ntx_train_forward", "ntx_train_backward"):
        assert name in _lib.SYMBOLS and callable(getattr(_lib.lib, name))
        assert re.search(r"^int %s\(ntx_trainer \*t," % name, header, re.M), name
    assert _lib.lib.ntx_abi_version() == 7 and re.search(r"#define NTX_ABI_VERSION 7\b", header)


@pytest.mark.parametrize("case", clc.TRAINER_CASES, ids=[c[0] for c in clc.TRAINER_CASES])
def test_the_gpu_cases_are_fair(case):
    """The three end-to-end cases of the GPU file under `CharbonnierAlpha`, BEFORE any GPU run: float32 autograd of the restatement within
    2.5e-4 of float64 in every layer (and every parameter column), on the restatement's own float32 ReLU patterns, and every layer's largest
    gradient above 2e-6 -- twice inside both guards of `check_layers`, so that the trainer's own patterns cannot tip one."""
    model, spec, wts, batch, kn = clc.trainer_case(case)
    ro, rd, t, cone, rows, color, alpha = batch
    n, S = len(t), clc.N_SAMPLES
    z = step_depths(t, S, kn["seed"], kn["perturb"])
    per_ray = np.repeat(rows, kn["rpr"], 0)[:n]
    masks, branch_masks, sigma_mask = tbo.own_masks(wts, spec, ro, rd, z, per_ray, cone)
    head = clc.loss_head(clc.CharbonnierAlpha(), color, alpha)
    run = lambda dtype: clc.restated(wts, spec, ro, rd, z, rows, kn["rpr"], cone, head, dtype=dtype, masks=masks, branch_masks=branch_masks or None, sigma_mask=sigma_mask)
    want, f32 = run(torch.float64), run(torch.float32)
    for name, sl in layer_slices(spec):
        floor, biggest = rel_linf(f32.grad[sl], want.grad[sl]), float(np.abs(want.grad[sl]).max())
        print(f"  {name:<24} floor {floor:.2e} max {biggest:.3e}")
        assert floor <= 2.5e-4 and biggest >= 2e-6, (name, floor, biggest)
    if spec.n_params and case[1] != "Trainer":
        pgc.fair(want.param_grad, f32.param_grad, margin=pgc.MARGIN)
