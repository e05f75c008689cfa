"""The distortion loss on the compositing weights, without a device (`ntx_ray_distortion`, include/nerftex.h; tests/distortion_common.py has
the restatements, the cases and the gate): the float64 reference is right (its analytic gradient against autograd, the O(S) identity), the
float32 floors leave the gate meaningful, the shift by the first live depth is needed, `as_callable` restates the descriptor losses, and the
entry refuses bad arguments before it touches a device."""

import os
import re

import numpy as np
import pytest
import torch

from tests import distortion_common as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in dc.CASES if c[2] <= 256]


def test_declared_bound_and_the_abi_version_stays():
    from nerf_tex_amd import _lib
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "nerftex.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ntx_ray_distortion\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m, "include/nerftex.h does not declare ntx_ray_distortion"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float *weights", "const float *z_vals", "const float *widths", "const float *live", "const float *ray_scale", "int64_t n_rays", "int n_samples",
                    "float *loss_out", "float *grad_out", "void *stream"]
    assert len(_lib.SYMBOLS["ntx_ray_distortion"][1]) == len(args) and hasattr(_lib.lib, "ntx_ray_distortion")
    assert _lib.lib.ntx_abi_version() == 7


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_analytic_gradient_is_autograd_of_the_pair_sum(case):
    """dL/dw_k = 2 sum_j w_j |z_k - z_j| + (2/3) w_k delta_k, masked by `live`, equals torch float64 autograd of the pair sum to 1e-12."""
    w, z, widths, scale = dc.case_inputs(case)
    live = np.random.default_rng(5).uniform(size=w.shape) < 0.7 if case[6] == "given" else None           # (live needs widths)
    want_loss, want_grad = dc.pairwise64(w, z, widths, None if live is None else live.astype(dc.F), scale)
    wt = torch.tensor(w.astype(np.float64), requires_grad=True)
    zt = torch.tensor(z.astype(np.float64))
    if live is not None:
        zt = torch.where(torch.as_tensor(live), zt, torch.full_like(zt, float("inf")))                      # (pairwise_torch: not finite = not live)
    val = dc.pairwise_torch(wt, zt, None if widths is None else torch.tensor(widths.astype(np.float64)), torch.tensor(scale.astype(np.float64)))
    val.sum().backward()
    assert dc.rel_linf(val.detach().numpy(), want_loss) <= 1e-12 and dc.rel_linf(wt.grad.numpy(), want_grad) <= 1e-12
    if live is not None:
        assert (want_grad[~live] == 0).all() and np.abs(want_grad[live]).max() > 0


@pytest.mark.parametrize("case", dc.CASES, ids=dc.CASE_IDS)
def test_the_linear_form_is_the_pair_sum_and_its_float32_floor_is_small(case):
    """The O(S) identity in float64 (1e-12), and the float32 restatement's floor <= 2.5e-5: four floors never reach the cap of 1e-4."""
    w, z, widths, scale = dc.case_inputs(case)
    want = dc.case_reference(case)
    got = dc.linear_form(w, z, widths, None, scale, dtype=np.float64)
    assert dc.rel_linf(got[0], want[0]) <= 1e-12 and dc.rel_linf(got[1], want[1]) <= 1e-12
    floors = dc.floor(case)
    print(f"| {case[0]} | floor of the loss {floors[0]:.2e} | of the gradient {floors[1]:.2e} |")
    assert max(floors) <= dc.FLOOR_GUARD and dc.gate(max(floors)) < dc.CAP
    assert np.abs(want[0]).max() > 1e-4 and np.abs(want[1]).max() > 1e-3, "a loss worth the name"


@pytest.mark.parametrize("pattern", dc.LIVE_PATTERNS)
def test_liveness_patterns_are_what_they_say(pattern):
    w, z, widths, live, scale, mask = dc.live_case(pattern)
    assert np.isnan(w[~mask]).all() and np.isnan(z[~mask]).all() and np.isnan(widths[~mask]).all() and np.isfinite(w[mask]).all()
    assert np.array_equal(dc.live_mask(z, live), mask)
    if pattern == "all_dead":
        assert not mask.any()
    if pattern == "one_in_last_chunk":
        assert (mask.sum(1) == 1).all() and not mask[:, :192].any()
    if pattern == "first_behind_chunk0":
        assert not mask[:, :64].any() and not mask[0, :128].any() and mask.any(1).all()
    want = dc.pairwise64(w, z, widths, live, scale)
    got = dc.linear_form(w, z, widths, live, scale)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and (want[1][~mask] == 0).all() and (got[1][~mask] == 0).all()
    if mask.any():
        assert max(dc.rel_linf(got[0], want[0]), dc.rel_linf(got[1], want[1])) <= dc.FLOOR_GUARD


def test_the_patch_patterns_have_their_dead_chunks_where_they_say():
    """What an instanced step produces: a whole dead chunk between live ones, whole dead chunks behind the last live sample, patches that
    end on the chunk edges, two short patches -- each with live samples on both sides of what is dead, and a gradient worth the name."""
    m = {p: dc.live_case(p)[5] for p in dc.PATCH_PATTERNS}
    assert dc.LIVE_PATTERNS[:4] == ["all_dead", "one_in_last_chunk", "first_behind_chunk0", "random35"] and dc.LIVE_PATTERNS[4:] == dc.PATCH_PATTERNS
    a = m["dead_chunk_between"]
    assert not a[:, 64:128].any() and a[:, 5].all() and a[:, 190].all() and 0.4 < a[:, :64].mean() < 0.8 and 0.4 < a[:, 128:].mean() < 0.8
    a = m["dead_tail"]
    assert not a[:, 70:].any() and a[:, 3].all() and a[:, 69].all() and 0.5 < a[:, :70].mean() < 0.9
    a = m["patch_ends_on_chunk_edges"]
    assert (a.sum(1) == 27 + 64).all() and a[:, 37:64].all() and a[:, 128:192].all()
    a = m["two_short_patches"]
    assert (a.sum(1) == 7).all() and a[:, 10:14].all() and a[:, 150:153].all()
    for p in dc.PATCH_PATTERNS:
        want, floors = dc.live_figures(p)
        print(f"| {p} | floor of the loss {floors[0]:.2e} | of the gradient {floors[1]:.2e} | max |grad| {np.abs(want[1]).max():.3e} |")
        assert max(floors) <= dc.FLOOR_GUARD and np.abs(want[1]).max() > 1e-3 and (np.abs(want[0]) > 0).all()


def test_the_case_at_the_sample_limit_is_inside_the_guard():
    """S = 4096, live exactly [100, 1000) and [3000, 4090): 31 dead chunks between live ones; NaN where not live; the floors <= FLOOR_GUARD."""
    w, z, widths, live, scale, mask = dc.live_limit_case()
    assert mask.shape == (3, 4096) and (mask.sum(1) == 900 + 1090).all() and mask[:, 100:1000].all() and mask[:, 3000:4090].all()
    assert not mask.reshape(3, 64, 64)[:, 16:46].any() and np.array_equal(dc.live_mask(z, live), mask)
    assert np.isnan(w[~mask]).all() and np.isnan(z[~mask]).all() and np.isnan(widths[~mask]).all() and np.isfinite(w[mask]).all()
    want, floors = dc.live_figures("limit")
    print(f"| S4096 two patches | floor of the loss {floors[0]:.2e} | of the gradient {floors[1]:.2e} | max |grad| {np.abs(want[1]).max():.3e} |")
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and (want[1][~mask] == 0).all()
    assert max(floors) <= dc.FLOOR_GUARD and dc.gate(max(floors)) < dc.CAP and np.abs(want[1]).max() > 1e-3


def test_the_large_batches_cycle_a_base_whose_rows_meet_every_wave():
    """The base of the calls past the capped grid: 257 rows (prime; 8192 mod 257 = 225, so a wave meets another base row in every pass), two
    of them without a live sample and one live in its first 30 samples only; the reference is zeros where it has to be and inside the guard."""
    w, z, dead, (loss, grad), floors = dc.large_base()
    assert len(w) == 257 and dc.GRID_RAYS == 8192 and dc.GRID_RAYS % 257 == 225 and dc.LARGE_N == [8192, 8193, 16389]
    assert np.array_equal(np.nonzero(dead)[0], [dc.MISSED, dc.NAN_W]) and np.isnan(w[dc.NAN_W]).all() and not np.isfinite(z[dc.NAN_W]).any()
    assert np.isfinite(z[dc.PARTIAL, :30]).all() and not np.isfinite(z[dc.PARTIAL, 30:]).any()
    assert np.isfinite(loss).all() and np.isfinite(grad).all() and not loss[dead].any() and not grad[dead].any() and not grad[dc.PARTIAL, 30:].any()
    assert (loss[~dead] > 0).all() and max(floors) <= dc.FLOOR_GUARD
    f32 = dc.linear_form(w, z)
    assert max(dc.rel_linf(f32[0], loss), dc.rel_linf(f32[1], grad)) <= dc.FLOOR_GUARD
    for n in dc.LARGE_N:
        rows = np.arange(n) % 257
        if n > dc.GRID_RAYS:                                                      # the second ray of a wave is another base row; a dead one is followed by a live one
            assert (rows[dc.GRID_RAYS:] != rows[:n - dc.GRID_RAYS]).all() and not dead[rows[dc.GRID_RAYS:][dead[rows[:n - dc.GRID_RAYS]]]].any()
        scale = dc.large_scale(n, dead)
        L, G = dc.large_reference(n, scale)
        assert np.isnan(scale[dead[rows]]).all() and np.isfinite(scale[~dead[rows]]).all() and np.isfinite(L).all() and np.isfinite(G).all()
        k = n - 1                                                                 # the last ray: the base row its index names, times its own scale
        assert not dead[rows[k]] and L[k] == loss[rows[k]] * np.float64(scale[k]) and np.array_equal(G[k], grad[rows[k]] * np.float64(scale[k]))


def test_without_the_shift_float32_loses_its_digits():
    """near = 500, span 0.5, S = 256: the unshifted float32 form is beyond 1e-4, the shifted one inside 2.5e-5 -- why the shift is specified."""
    w, z, widths, scale = dc.case_inputs(dc.NEAR500)
    want = dc.case_reference(dc.NEAR500)
    unshifted = dc.linear_form(w, z, widths, None, scale, shift=False)
    e = max(dc.rel_linf(unshifted[0], want[0]), dc.rel_linf(unshifted[1], want[1]))
    print(f"unshifted {e:.2e}; shifted {max(dc.floor(dc.NEAR500)):.2e}")
    assert e > dc.CAP and max(dc.floor(dc.NEAR500)) <= dc.FLOOR_GUARD


@pytest.mark.parametrize("setting", dc.LOSS_SETTINGS, ids=[s[0] for s in dc.LOSS_SETTINGS])
def test_as_callable_restates_the_descriptor_losses(setting):
    from nerf_tex_amd import loss as L
    _, kind, kw = setting
    rng = np.random.default_rng(3)
    n = 37
    ct, cp = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, (n, 3))
    at, ap = rng.uniform(0, 1, n) * (rng.uniform(size=n) < 0.7), rng.uniform(0, 1, n)
    fn = L.as_callable(getattr(L, kind)(**kw))
    t_ = lambda x: torch.tensor(x, dtype=torch.float64, requires_grad=True)
    c, a = t_(cp), t_(ap)
    val = fn(color_true=torch.tensor(ct), alpha_true=torch.tensor(at), color_pred=c, alpha_pred=a)
    want = dc.descriptor_loss64(kind, kw, ct, at, cp, ap)
    assert abs(float(val.detach()) - want) <= 1e-12 * abs(want)
    val.backward()
    assert c.grad is not None and np.abs(c.grad.numpy()).max() > 0 and ((a.grad is not None) == (kind == "AlphaLoss"))


def test_distortion_wraps_descriptors_configs_and_callables():
    """`Distortion(base)`: a descriptor, a loss_config dict and a callable all become a callable loss that names `weights` and `z_vals` and has
    no `desc()`, so the trainers take the callable route and hand it the weights and the depths."""
    from nerf_tex_amd import loss as L, util
    from nerf_tex_amd.util import loss_keywords as _loss_keywords
    cfg = {"module": "nerf_tex_amd.loss.Distortion", "weight": 0.02,
           "base": {"module": "network.loss.AlphaLoss", "loss_fn": "network.loss.smape", "alpha_loss_fn": "network.loss.mse"}}
    made = [util.instantiate(util.remap_reference_config(cfg)), L.Distortion(L.NerfLoss()), L.Distortion(lambda color_true, alpha_true, color_pred, alpha_pred: color_pred.sum())]
    for d in made:
        assert not hasattr(d, "desc") and {"color_true", "alpha_true", "color_pred", "alpha_pred", "weights", "z_vals"} <= _loss_keywords(d)
    assert made[0].weight == 0.02 and made[0].normalize and made[1].weight == 0.01
    with pytest.raises(TypeError):
        L.Distortion(3.0)
    with pytest.raises(TypeError, match="weights"):                                  # the predictions alone, as `TextureFitter` calls a loss
        made[1](color_true=torch.zeros(2, 3), alpha_true=None, color_pred=torch.zeros(2, 3), alpha_pred=torch.zeros(2))


def entry():
    from nerf_tex_amd import _lib
    return _lib, _lib.lib.ntx_ray_distortion


def test_argument_checks_need_no_device():
    """NULL combinations, S = 0 and 4097, negative and too many rays, `live` without `widths`: NTX_E_INVALID with the message set, before any
    launch -- the buffers here are host memory the call must not touch -- and n_rays = 0 is NTX_OK without one."""
    _lib, fn = entry()
    n, S = 3, 8
    bufs = {k: np.full(n * S, -7.0, dc.F) for k in ("w", "z", "d", "lv", "g")}
    small = {k: np.full(n, -7.0, dc.F) for k in ("rs", "L")}
    p = lambda a: a.ctypes.data
    w, z, d, lv, g, rs, L = tuple(p(bufs[k]) for k in ("w", "z", "d", "lv", "g")) + tuple(p(small[k]) for k in ("rs", "L"))
    bad = {
        "weights NULL": (None, z, d, lv, rs, n, S, L, g),
        "z_vals NULL": (w, None, d, lv, rs, n, S, L, g),
        "both outputs NULL": (w, z, d, lv, rs, n, S, None, None),
        "S = 0": (w, z, d, lv, rs, n, 0, L, g),
        "S = 4097": (w, z, d, lv, rs, n, 4097, L, g),
        "n_rays < 0": (w, z, d, lv, rs, -1, S, L, g),
        "n_rays = 2^31": (w, z, d, lv, rs, 2 ** 31, S, L, g),
        "live without widths": (w, z, None, lv, rs, n, S, L, g),
    }
    for what, args in bad.items():
        assert fn(*args, None) == _lib.NTX_E_INVALID, what
        assert _lib.lib.ntx_last_error(), what
    assert b"live without widths" in _lib.lib.ntx_last_error()
    for args in ((w, z, d, lv, rs, 0, S, L, g), (w, z, None, None, None, 0, 1, L, None), (w, z, None, None, None, 0, 4096, None, g)):
        assert fn(*args, None) == _lib.NTX_OK
    assert all((a == -7.0).all() for a in list(bufs.values()) + list(small.values())), "a refused call has written nothing"
