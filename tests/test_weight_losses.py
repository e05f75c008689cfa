"""Losses on the compositing weights (`ntx_trainer_weight_cotangent`, `Trainer.forward(return_weights=)` / `backward(d_weights=)`; DESIGN
section 10), what can be said without a GPU: the entry exists with its prototype and refuses NULL, the identity the kernels' change rests on --
autograd of the restated composite under dC, dA and g equals `ray_adjoint`'s recurrences with c + g in the place of c, plain and with the
instanced step's appended sample -- in float64, the torch helpers, and every case of tests/test_gpu_weight_losses.py MARGIN times inside the
guards of the bar it is held to, with a weight cotangent that moves the density column by more than ten such bars."""

import os
import re

import numpy as np
import pytest
import torch

from oracle import torch_cpu as tcpu
from tests import param_grad_common as pgc
from tests import weight_loss_common as wlc
from tests.train_common import BKGD, F, step_depths, step_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_declared_exported_and_refuses_null():
    from nerf_tex_amd import _lib
    assert "ntx_trainer_weight_cotangent" in _lib.SYMBOLS
    buf = (_lib.C.c_float * 4)()
    assert _lib.lib.ntx_trainer_weight_cotangent(None, None) == _lib.NTX_E_INVALID
    assert _lib.lib.ntx_trainer_weight_cotangent(None, _lib.C.cast(buf, _lib.C.c_void_p)) == _lib.NTX_E_INVALID      # no device is asked for
    assert _lib.lib.ntx_abi_version() == 7 and _lib.ABI_VERSION == 7
    with open(os.path.join(ROOT, "include", "nerftex.h")) as f:
        header = f.read()
    assert re.search(r"int\s+ntx_trainer_weight_cotangent\(ntx_trainer \*t, const float \*d_weights_dev\);", header)
    assert header.rindex("int ntx_trainer_weight_cotangent(") > header.rindex("int ntx_trainer_enable_instanced(")            # appended
    assert "#define NTX_ABI_VERSION 7" in header


def test_the_restated_composite_is_the_oracles():
    """`wlc.composite` returns the oracle's (c, a) -- every option on -- and the weights those were summed from."""
    rng = np.random.default_rng(0)
    n, S = 4, 9
    raw, sg = torch.tensor(rng.normal(size=(n, S, 3))), torch.tensor(rng.normal(size=(n, S)) * 3)
    dists, noise = torch.tensor(rng.uniform(0.05, 0.4, (n, S))), torch.tensor(rng.normal(size=(n, S)) * 0.1)
    for exr in (False, True):
        for bk in (False, True):
            c, a, w = wlc.composite(raw, sg, dists, exr, bk, BKGD, None, noise)
            c0, a0 = tcpu.composite(raw, sg, dists, exr, bk, BKGD, None, noise)
            assert torch.equal(c, c0) and torch.equal(a, a0) and torch.allclose(w.sum(-1), a, rtol=0, atol=1e-15) and w.shape == (n, S)


@pytest.mark.parametrize("S", [1, 2, 7, 65])
@pytest.mark.parametrize("form", ["plain", "instanced"])
def test_autograd_equals_the_recurrence_with_c_plus_g(form, S):
    """Float64, random raw outputs, every option in turn: d/da of <c, dC> + <a, dA> + <w, g> by autograd of the restated composite equals
    dL/da_i = T_i (dA' Z_i + ((c_i + g_i) - V_i)) with V_{i-1} = (c_i + g_i) a_i + f_i V_i to 1e-12 -- and dL/d rgb does not see g.  The
    instanced form: samples that are not live have a = 0, and the appended sample (no g of its own) starts the carries."""
    rng = np.random.default_rng(S + (100 if form == "instanced" else 0))
    n = 6
    for trial in range(4):
        bkgd = BKGD if trial % 2 else None
        a = torch.tensor(1.0 - np.exp(-np.maximum(rng.normal(size=(n, S)) * 3, 0) * rng.uniform(0.05, 0.6, (n, S))), requires_grad=True)
        if form == "instanced":
            with torch.no_grad():
                a[rng.uniform(size=(n, S)) < 0.4] = 0.0                                # not live
        rgb = torch.tensor(rng.uniform(0, 1.5, (n, S, 3)), requires_grad=True)
        dC, dA, g = rng.normal(size=(n, 3)), rng.normal(size=n), rng.normal(size=(n, S))
        color_last, alpha_last = rng.uniform(0, 1, (n, 3)), rng.uniform(0, 1, n)
        am, rgbm = a, rgb
        if form == "instanced":
            am = torch.cat([a, torch.tensor(alpha_last)[:, None]], 1)
            rgbm = torch.cat([rgb, torch.tensor(color_last)[:, None, :]], 1)
        w = am * wlc.exclusive_cumprod(1.0 - am + 1e-10)
        c, A = (w[..., None] * rgbm).sum(-2), w.sum(-1)
        if bkgd is not None:
            c = c + (1.0 - A[:, None]) * torch.tensor(bkgd, dtype=torch.float64)
        ((c * torch.tensor(dC)).sum() + (A * torch.tensor(dA)).sum() + (w[:, :S] * torch.tensor(g)).sum()).backward()
        d_rgb_plain = (w[:, :S, None] * torch.tensor(dC)[:, None, :]).detach().numpy()
        assert np.abs(rgb.grad.numpy() - d_rgb_plain).max() <= 1e-12 * np.abs(d_rgb_plain).max()           # dL/d rgb = w dC: no g in it
        for r in range(n):
            last = dict(color_last=color_last[r], alpha_last=alpha_last[r]) if form == "instanced" else {}
            got = wlc.recurrence(a.detach().numpy()[r], rgb.detach().numpy()[r], dC[r], dA[r], g[r], bkgd, **last)
            want = a.grad.numpy()[r]
            assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), (form, S, trial, r, got, want)
            without = wlc.recurrence(a.detach().numpy()[r], rgb.detach().numpy()[r], dC[r], dA[r], 0 * g[r], bkgd, **last)
            assert np.abs(without - want).max() > 1e-3                                                       # (and g is seen)


def test_expected_depth_and_the_signature_rule():
    """`expected_depth` is sum_s w_s z_s with a missed ray's infinite depths counted 0; a callable loss gets the weights only if it names them."""
    from nerf_tex_amd.loss import expected_depth
    from nerf_tex_amd.train import _loss_keywords
    from tests.custom_loss_common import CharbonnierAlpha
    w = torch.tensor([[0.25, 0.5, 0.125], [0.0, 0.0, 0.0]], requires_grad=True)
    z = np.array([[1.0, 2.0, 4.0], [np.inf, np.inf, np.inf]], F)
    d = expected_depth(w, z)
    assert d.tolist() == [1.75, 0.0]
    d.sum().backward()
    assert w.grad.tolist() == [[1.0, 2.0, 4.0], [0.0, 0.0, 0.0]]
    assert _loss_keywords(CharbonnierAlpha()) == {"color_true", "alpha_true", "color_pred", "alpha_pred"}
    assert {"weights", "z_vals"} <= _loss_keywords(wlc.depth_loss(None, None))
    assert _loss_keywords(lambda **kw: None) == set()


@pytest.mark.parametrize("case", wlc.ADJ_CASES, ids=wlc.ADJ_IDS)
def test_the_adjoint_cases_are_fair(case):
    """Every case of the adjoint alone, on the oracle's own float32 network outputs: float32 autograd of the restated composite under the three
    cotangents MARGIN times inside 5e-4 of float64, both gradients MARGIN times above 1e-8, and the density column with g more than 10 bars from
    the one without."""
    cid, kind, S, regime, exr, bk, noise_std = case
    _, spec, blob = wlc.kind_model(kind, regime)
    batch, (gC, gA, g) = wlc.adjoint_batch(case)
    z, noise = step_depths(batch[2], S, S, True), step_noise(wlc.ADJ_N, S, S, noise_std)
    raw, sg = wlc.cpu_raw_outputs(spec, blob, batch, z)
    e = wlc.adjoint_figures(None, raw, sg, z, batch[1], gC, gA, g, exr, bk, noise)
    print(f"{cid}: floors {e['f_drgb']:.2e} {e['f_dsigma']:.2e} max {e['max_drgb']:.2e} {e['max_dsigma']:.2e} seen {e['seen']:.2e} alpha {e['pred'][:, 3]}")
    wlc.guards(e, wlc.MARGIN)
    if regime == "saturated":
        assert (e["pred"][:, 3] > 0.99999).sum() >= wlc.ADJ_N / 4, e["pred"][:, 3]


@pytest.mark.parametrize("live", [l for l in wlc.LIVE if l != "none"])
@pytest.mark.parametrize("kind", sorted(wlc.INST_KINDS))
def test_the_instanced_cases_are_fair(kind, live):
    """The same for the instanced composite over the compact rows of every instanced case that has any."""
    model, spec, wts, bufs, hit, cone, kn, okw = wlc.instanced_setup(kind, live)
    n, S = bufs[3].shape
    raw, sg, mask = wlc.cpu_instanced_outputs(spec, wts, bufs, hit, cone, okw)
    gC, gA, g = wlc.cotangents(n, S, 9)
    e = wlc.instanced_figures(None, raw, sg, bufs, hit, okw, gC, gA, g, mask)
    print(f"{kind} {live}: {len(raw)} live; floors {e['f_drgb']:.2e} {e['f_dsigma']:.2e} max {e['max_drgb']:.2e} {e['max_dsigma']:.2e} seen {e['seen']:.2e}")
    assert len(raw) > 0 and (live != "some" or (0 < len(raw) < n * S and not np.asarray(hit, bool).all()))
    wlc.guards(e, wlc.MARGIN)


@pytest.mark.parametrize("case", wlc.E2E_CASES, ids=wlc.E2E_IDS)
def test_the_end_to_end_cases_are_fair(case):
    """The end-to-end cases at their own size, on the restatement's own float32 ReLU patterns: every layer, every parameter column and every
    ray column MARGIN times inside the standing guards, and the depth term a real share of the loss's gradient."""
    model, spec, wts, batch, kn, seed, depth, z = wlc.e2e_setup(case)
    patterns = pgc.own_patterns(spec, wts, batch, kn, seed)
    head = wlc.e2e_head(batch, depth, z)
    kw = dict(masks=patterns[0], branch_masks=patterns[1], sigma_mask=patterns[2])
    want = wlc.restated_step(wts, spec, batch, z, kn["rpr"], head, **kw)
    f32 = wlc.restated_step(wts, spec, batch, z, kn["rpr"], head, dtype=torch.float32, **kw)
    wlc.e2e_fair(spec, want, f32)
    color_only = wlc.restated_step(wts, spec, batch, z, kn["rpr"], wlc.e2e_head(batch, depth, z, lam=0.0), **kw)
    assert np.abs(want.grad - color_only.grad).max() > 0.05 * np.abs(want.grad).max()
