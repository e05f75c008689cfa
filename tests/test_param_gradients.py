"""The yardstick of dL/d parameters on the CPU (tests/param_grad_common.restated_param_gradients: float64 autograd of the restated step with the
parameter rows as the leaf) against central finite differences of the same loss, the fairness of every case tests/test_gpu_param_gradients.py
runs -- seeds are chosen HERE, on float32 against float64 of the restatement alone --, and the fit's restatement.  `-m "not gpu"`."""

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import param_grad_common as pgc                                      # noqa: E402
from tests.common import make_model                                              # noqa: E402
from tests.train_common import LOSSES, step_depths                               # noqa: E402
from tests.train_flex_common import flex_batch                                   # noqa: E402

F = np.float32


@pytest.mark.parametrize("branches", [False, True], ids=["features", "branches"])
@pytest.mark.parametrize("blur", [0, 3], ids=["blur_geometry", "blur_appearance"])
def test_autograd_of_the_parameter_rows_matches_finite_differences(blur, branches):
    """8 rays x 6 samples, a 3 x 32 network on [2, 3] parameters, free branches, two rays a parameter row, float64: every entry of dL/d rows
    against (L(p + h) - L(p - h)) / 2h at h = 1e-6: 1e-6 rel-Linf over the gradient, and 1e-6 of each COLUMN's own largest entry plus the
    rounding of the difference itself, 4 eps |L| / h (the column of blur_idx is scaled by cone_scale z ~ 1e-3: its entries are ~3e-6, where
    the quotient of two float64 losses 2e-6 apart holds ~7e-12 absolute -- 2.4e-6 of that column, measured -- and no step size does better:
    truncation grows as h^2, rounding as 1 / h)."""
    arch = dict(width=32, depth=3, skips=[1], **(dict(param_depth=2, param_width=16) if branches else {}))
    model, spec, wts = make_model((2, 3), dense_media=True, arch=arch)
    n, S, rpr = 8, 6, 2
    ro, rd, t, cone, params, color, alpha = flex_batch(5, n, S, spec, "grass_filtered")
    rows = params[::rpr].astype(np.float64)
    z = step_depths(t, S, 0, False)
    okw = LOSSES["alpha_mse_soft"][0]
    f = lambda r: pgc.restated_param_gradients(wts, spec, ro, rd, z, r, rpr, cone, color, alpha, okw, blur_idx=blur)
    _, _, grad = f(rows)
    fd, h = np.zeros_like(grad), 1e-6
    for i in range(rows.shape[0]):
        for c in range(rows.shape[1]):
            up, dn = rows.copy(), rows.copy()
            up[i, c] += h; dn[i, c] -= h
            fd[i, c] = (f(up)[0] - f(dn)[0]) / (2 * h)
    val = f(rows)[0]
    errs, top = pgc.column_errors(grad, fd), np.abs(fd).max(0)
    whole = np.abs(grad - fd).max() / np.abs(fd).max()
    print("loss", val, "max |grad| per column", top, "rel err per column", errs, "over the gradient", whole)
    assert grad.shape == (4, 5) and (top > 1e-6).all()
    assert whole <= 1e-6, whole
    assert (np.abs(grad - fd).max(0) <= 1e-6 * top + 4 * np.finfo(np.float64).eps * abs(val) / h).all(), errs


def test_rows_and_rays_that_miss_in_the_restatement():
    """A short last row takes the rays that are left; a row whose rays all miss gets exactly 0, as `step_gradients` filters them."""
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(width=32, depth=2, skips=[]))
    n, S, rpr = 10, 6, 4
    ro, rd, t, cone, params, color, alpha = flex_batch(5, n, S, spec, "carpet")
    miss = np.zeros(n, bool); miss[[1, 8, 9]] = True
    z = step_depths(t, S, 0, False, miss)
    val, pred, grad = pgc.restated_param_gradients(wts, spec, ro, rd, z, params[::rpr], rpr, cone, color, alpha, LOSSES["alpha_smape"][0])
    assert grad.shape == (3, 7) and (grad[2] == 0).all() and np.abs(grad[:2]).max() > 0 and (pred[miss] == 0).all()


@pytest.mark.parametrize("case", pgc.ALL_CASES, ids=[c[0] for c in pgc.ALL_CASES])
def test_the_gpu_cases_are_fair(case):
    """Every case of the GPU file, at its own size and depths, under its guards BEFORE any GPU run: float32 autograd of the restatement within 5e-4
    of float64 in every parameter column, on the restatement's own float32 ReLU patterns, and every column's largest gradient above 1e-6.  The
    cases of `pgc.NEW_CASES` sit twice inside both (floor <= 2.5e-4, max |grad| >= 2e-6): the trainer's own patterns cannot tip a guard."""
    model, spec, wts, batch, kn, seed = pgc.case_setup(case)
    masks, branch_masks, sigma_mask = pgc.own_patterns(spec, wts, batch, kn, seed)
    want = pgc.restate(spec, wts, batch, kn, seed, torch.float64, masks, branch_masks, sigma_mask)
    f32 = pgc.restate(spec, wts, batch, kn, seed, torch.float32, masks, branch_masks, sigma_mask)
    rows = None
    assert want[2].shape == (-(-kn["n"] // kn["rpr"]), spec.n_params) and want[1].shape == (kn["n"], 4)
    if kn["miss"].any():
        live = np.array([not kn["miss"][r * kn["rpr"]:(r + 1) * kn["rpr"]].all() for r in range(want[2].shape[0])])
        assert (want[2][~live] == 0).all() and not live.all()
        rows = live
    pgc.fair(want[2], f32[2], rows=rows, margin=pgc.MARGIN if case in pgc.NEW_CASES else 1.0)


def test_the_fit_restatement_converges():
    """The fit of tests/test_gpu_param_gradients.py on the CPU -- float64 restatement, the same Adam, the same steps: it ends below 0.25 x its
    initial loss, the margin the GPU fit is given twice of."""
    f = pgc.FIT
    model, spec, wts, batch, true, init = pgc.fit_setup()
    params, losses = pgc.restated_fit(spec, wts, batch, init, LOSSES[f["loss_name"]][0], f["n_iters"], f["lrate"])
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e} ({losses[-1] / losses[0]:.3f}); |p - true| {np.abs(init - true).max():.3f} -> {np.abs(params - true).max():.3f}")
    assert f["n_iters"] <= 200 and np.isfinite(losses).all()
    assert losses[-1] < 0.25 * losses[0], (losses[0], losses[-1])
