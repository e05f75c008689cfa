"""The yardsticks of dL/d rays_o, rays_d and dL/d pts, rays_d_map on the CPU (tests/input_grad_common.py: float64 autograd of the restated
steps with the rays / the sample points as leaves) against central finite differences of the same loss, the fairness of every case
tests/test_gpu_input_gradients.py runs -- seeds are chosen HERE, on float32 against float64 of the restatement alone --, and the three
entries of the C ABI.  `-m "not gpu"`."""

import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from tests import input_grad_common as igc                                      # noqa: E402
from tests import instanced_train_common as itc                                  # noqa: E402
from tests import param_grad_common as pgc                                       # noqa: E402
from tests.common import make_model                                              # noqa: E402
from tests.train_common import LOSSES, step_depths, step_noise                   # noqa: E402
from tests.train_flex_common import flex_batch                                   # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def held_to_finite_differences(f, leaves, h=1e-6):
    """`f(*leaves)` -> (loss, gradient per leaf): every entry of every gradient against (L(x + h) - L(x - h)) / 2h -- 1e-6 rel-Linf over each
    gradient, and per COLUMN 1e-6 of its own largest entry plus the rounding of the difference itself, 4 eps |L| / h (the bar and the step of
    tests/test_param_gradients.py)."""
    val, grads = f(*leaves)
    for k, (x, grad) in enumerate(zip(leaves, grads)):
        fd = np.zeros_like(grad)
        for i in np.ndindex(*x.shape):
            up, dn = [a.copy() for a in leaves], [a.copy() for a in leaves]
            up[k][i] += h; dn[k][i] -= h
            fd[i] = (f(*up)[0] - f(*dn)[0]) / (2 * h)
        g2, f2 = grad.reshape(-1, 3), fd.reshape(-1, 3)
        top, whole = np.abs(f2).max(0), np.abs(g2 - f2).max() / np.abs(f2).max()
        print(f"leaf {k}: loss {val:.9g} max |grad| per column {top} over the gradient {whole:.2e} per column {np.abs(g2 - f2).max(0) / top}")
        assert (top > 1e-6).all(), top
        assert whole <= 1e-6, whole
        assert (np.abs(g2 - f2).max(0) <= 1e-6 * top + 4 * np.finfo(np.float64).eps * abs(val) / h).all()


@pytest.mark.parametrize("branches", [False, True], ids=["plain", "branches"])
def test_autograd_of_the_rays_matches_finite_differences(branches):
    """6 rays x 6 samples, a 3 x 32 network on [2, 3] parameters with blur_idx, free branches, float64, rays_d scaled per ray by a factor in
    [0.5, 2] (the normalisation of the direction and the |d| of the distances are exercised) and density noise on: every entry of dL/d rays_o
    and dL/d rays_d against central differences.  The ReLU patterns are the base point's, held over the differences as the GPU's yardstick
    holds the trainer's: behind ten octaves of FourierFeatures a step of 1e-6 in a position moves a pre-activation 500 times as far as one in
    a parameter does, and a difference across a kink is no derivative.  The branch model has six position bands, not ten: its function
    of the rays is steep enough (|dL/d rays_o| up to 418 at a loss of 0.14) for the TRUNCATION of a central difference at h = 1e-6 to reach
    4.4e-5 of the gradient with ten -- 4.4e-3 at h = 1e-5, 4.4e-7 at 1e-7, 1e-8 at 1e-8: h^2, measured -- and the step is the bar's."""
    arch = dict(width=32, depth=3, skips=[1], **(dict(param_depth=2, param_width=16) if branches else {}))
    model, spec, wts = make_model((2, 3), dense_media=True, arch=arch, freqs=(6, 4, 4) if branches else None)
    n, S, rpr = 6, 6, 2
    ro, rd, t, cone, params, color, alpha = flex_batch(5, n, S, spec, "grass_filtered")
    rd = igc.unnormalised(rd, 5)
    lengths = np.linalg.norm(rd, axis=1)
    assert lengths.min() < 0.9 and lengths.max() > 1.1
    z, noise = step_depths(t, S, 0, False), step_noise(n, S, 0, 0.1)
    okw = LOSSES["alpha_mse_soft"][0]
    from tests import train_branch_oracle as tbo
    masks, branch_masks, sigma_mask = tbo.own_masks(wts, spec, ro, rd, z, np.repeat(params[::rpr], rpr, 0), cone, blur_idx=0, noise=noise, dtype=torch.float64)

    def f(o, d):
        val, _, go, gd = igc.restated_ray_gradients(wts, spec, o, d, z, params[::rpr], rpr, cone, color, alpha, okw, blur_idx=0, noise=noise, masks=masks,
                                                    branch_masks=branch_masks if branches else None, sigma_mask=sigma_mask)
        return val, (go, gd)
    held_to_finite_differences(f, [ro.astype(np.float64), rd.astype(np.float64)])


def test_rays_that_miss_in_the_restatement():
    """The rows of a ray whose depths are not finite are exactly 0 in both results."""
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(width=32, depth=2, skips=[]))
    n, S, rpr = 10, 6, 4
    ro, rd, t, cone, params, color, alpha = flex_batch(5, n, S, spec, "carpet")
    miss = np.zeros(n, bool); miss[[1, 8, 9]] = True
    z = step_depths(t, S, 0, False, miss)
    val, pred, go, gd = igc.restated_ray_gradients(wts, spec, ro, igc.unnormalised(rd, 5), z, params[::rpr], rpr, cone, color, alpha, LOSSES["alpha_smape"][0])
    assert go.shape == gd.shape == (n, 3) and not go[miss].any() and not gd[miss].any() and np.abs(go[~miss]).max() > 0 and np.abs(gd[~miss]).max() > 0


@pytest.mark.parametrize("case", [itc.CASES[0], itc.CASES[4]], ids=["plain", "branches"])
def test_autograd_of_the_sample_points_matches_finite_differences(case):
    """The instanced restatement, 4 rays x 5 samples, free branches, float64: every live entry of dL/d pts and dL/d rays_d_map against
    central differences (the base point's ReLU patterns held, as above); exact zeros at samples that are not live."""
    model, spec, wts, bufs, hit, cone, kn, okw = itc.case_setup(case, n=4, S=5, seed=7)
    mask = np.zeros((4, 5), bool); mask[0, 1:4] = True; mask[2, :] = True; mask[3, 2] = True
    bufs, hit = itc.with_live_mask(bufs, hit, mask)
    head = itc.quadratic_head(4)
    live = itc.live_mask(hit, bufs[3])
    clean = lambda a: np.where(live[..., None], np.nan_to_num(np.asarray(a, np.float64)), 0.0)
    base = itc.restated(wts, spec, bufs, hit, cone, None, **okw)
    pat = dict(masks=base.masks, branch_masks=base.branch_masks, sigma_mask=base.sigma_mask)

    def f(pts, dirs):
        val, _, gp, gd = igc.restated_sample_gradients(wts, spec, bufs, hit, cone, head, pts=pts, dirs=dirs, **okw, **pat)
        assert not gp[~live].any() and not gd[~live].any()
        return val, (gp[live], gd[live])

    def shifted(pts_live, dirs_live):                                            # the leaves are the live samples' rows
        p, d = clean(bufs[1]), clean(bufs[0])
        p[live] = pts_live; d[live] = dirs_live
        return f(p, d)
    held_to_finite_differences(shifted, [clean(bufs[1])[live], clean(bufs[0])[live]])


@pytest.mark.parametrize("case", igc.ALL_CASES, ids=[c[0] for c in igc.ALL_CASES])
def test_the_gpu_cases_are_fair(case):
    """Every plain case of the GPU file, at its own size and depths, 2x inside both guards BEFORE any GPU run: float32 autograd of the
    restatement within 2.5e-4 of float64 in every column of dL/d rays_o and dL/d rays_d over the rays that hit, on the restatement's own
    float32 ReLU patterns, and every column's largest gradient above 2e-6."""
    model, spec, wts, batch, kn, seed = igc.case_setup(case)
    patterns = pgc.own_patterns(spec, wts, batch, kn, seed)
    want = igc.restate(spec, wts, batch, kn, seed, torch.float64, *patterns)
    f32 = igc.restate(spec, wts, batch, kn, seed, torch.float32, *patterns)
    lengths = np.linalg.norm(batch[1], axis=1)
    assert want[2].shape == want[3].shape == (kn["n"], 3) and (np.abs(lengths - 1) > 1e-3).any()
    rows = None
    if kn["miss"].any():
        assert not want[2][kn["miss"]].any() and not want[3][kn["miss"]].any()
        rows = ~kn["miss"]
    pgc.fair(igc.columns(*want[2:]), igc.columns(*f32[2:]), rows=rows, margin=igc.MARGIN)


def _instanced_setups():
    return [(c[0], c, None) for c in itc.CASES] + [(e[0], itc.CASES[0], e) for e in igc.INST_EDGES]


@pytest.mark.parametrize("name, case, edge", _instanced_setups(), ids=[s[0] for s in _instanced_setups()])
def test_the_instanced_gpu_cases_are_fair(name, case, edge):
    """The same for the instanced cases and edges, over the live samples (without one, both results are zeros)."""
    model, spec, wts, bufs, hit, cone, kn, okw = itc.case_setup(case) if edge is None else itc.edge_setup(edge)
    head = itc.quadratic_head(bufs[3].shape[0])
    pat = igc.own_instanced_patterns(spec, wts, bufs, hit, cone, okw)
    want = igc.restated_sample_gradients(wts, spec, bufs, hit, cone, head, **okw, **pat)
    f32 = igc.restated_sample_gradients(wts, spec, bufs, hit, cone, head, dtype=torch.float32, **okw, **pat)
    live = itc.live_mask(hit, bufs[3]).reshape(-1)
    assert not want[2].reshape(-1, 3)[~live].any() and not want[3].reshape(-1, 3)[~live].any()
    if live.any():
        pgc.fair(igc.columns(*want[2:]), igc.columns(*f32[2:]), rows=live, margin=igc.MARGIN)


def test_the_three_entries_are_in_the_header_the_loader_and_the_library():
    """ntx_trainer_enable_input_gradients, ntx_trainer_ray_gradients and ntx_trainer_sample_input_gradients: declared in include/nerftex.h,
    listed in `_lib.SYMBOLS` with as many arguments, exported by the built library; the ABI is still version 7."""
    from nerf_tex_amd import _lib
    header = open(os.path.join(ROOT, "include", "nerftex.h")).read()
    assert re.search(r"#define\s+NTX_ABI_VERSION\s+7\b", header) and _lib.ABI_VERSION == 7 and _lib.lib.ntx_abi_version() == 7
    for name, n_args in (("ntx_trainer_enable_input_gradients", 2), ("ntx_trainer_ray_gradients", 4), ("ntx_trainer_sample_input_gradients", 5)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, name
        assert len(m.group(1).split(",")) == n_args == len(_lib.SYMBOLS[name][1]), name
        assert hasattr(_lib.lib, name), name
