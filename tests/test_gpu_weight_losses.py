"""Losses on the compositing weights on the GPU: `ntx_trainer_weight_cotangent` (`Trainer.forward(return_weights=)` / `backward(d_weights=)`,
`DifferentiableRender(weights=True)`, a callable loss that names `weights`).  `-m gpu`.

1. The adjoint alone: slot 30 after forward + weight cotangent + backward against float64 autograd of the restated composite on the step's own
   raw outputs, depths and noise, at the standing bars (tests/weight_loss_common.py), over the suffix scan's chunk edges on the chain and layer
   by layer, a saturated family, a model with parameter branches; a ray at t = inf with NaN cotangents; the colour columns bit for bit with and
   without g.  2. The weights `ntx_train_forward` hands out.  3. End to end under mse + expected depth, through `gradients_step` with a callable
   that names `weights` and `z_vals`.  4. The registration's rules.  5. Instanced steps.  6. The autograd ops.  7. Streams.
Every case is held MARGIN times inside its guards on the CPU (tests/test_weight_losses.py).  A plain step has at least two samples a ray, so
the sample count 1 is an instanced case."""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import custom_loss_common as clc
from tests import fused_instanced_common as fic
from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests import weight_loss_common as wlc
from tests.train_common import BKGD, raw_outputs, rel_linf, step_depths, step_noise, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
_TRAINERS = {}


def dev():
    return torch.device("cuda", 0)


def kind_trainer(kind):
    """The one trainer of a kind this module's small cases share (8 rays x 130 samples); a case sets its weights, map_exr and noise."""
    from nerf_tex_amd import train
    if kind not in _TRAINERS:
        model, spec, _ = wlc.kind_model(kind)
        _TRAINERS[kind] = (getattr(train, wlc.KINDS[kind][0])(model, max_rays=wlc.CAP_RAYS, n_samples=wlc.CAP_S, perturb=True), spec)
    return _TRAINERS[kind]


def plain_sequence(tr, case, g="case", miss=None, wild=None):
    """forward (with the weights) + weight cotangent + backward of an adjoint case on the shared trainer.  `g`: "case" the case's own, None: no
    registration, or an array.  `miss`: rays set to t = inf; `wild`: the value their three cotangents are set to.  Returns pred [n, 4], the
    weights, slot 30 [n, S, 4], the raw outputs, the trainer's gradient and the cotangents used."""
    cid, kind, S, regime, exr, bk, noise_std = case
    (ro, rd, t, cone, params), (gC, gA, gW) = wlc.adjoint_batch(case)
    n = len(t)
    tr.set_weights(wlc.kind_model(kind, regime)[2])
    tr.map_exr, tr.raw_noise_std = bool(exr), float(noise_std)
    if miss is not None:
        t, cone, gC, gA, gW = t.copy(), cone.copy(), gC.copy(), gA.copy(), gW.copy()
        t[miss], cone[miss] = np.inf, np.nan
        gC[miss], gA[miss], gW[miss] = wild, wild, wild
    g = gW if isinstance(g, str) else g
    cp, ap, w = tr.forward(ro, rd, t, params, cone, composite_bkgd=bk, bkgd_color=BKGD, seed=S, n_samples=S, return_weights=True)
    tr.backward(gC, gA, g)
    torch.cuda.synchronize()
    return SimpleNamespace(pred=step_pred(cp, ap), w=w.cpu().numpy(), adj=tr.activation(30, n * S).reshape(n, S, 4), raw=raw_outputs(tr, n, S), grad=tr.gradients(),
                               cot=(gC, gA, g), rd=rd, t=t)


# ---- 1. the adjoint alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wlc.ADJ_CASES, ids=wlc.ADJ_IDS)
def test_adjoint_alone(case):
    """Slot 30 under the three cotangents at the standing bars; the predictions within 1e-5 and the weights within 1e-5 absolute of float64 on
    the same raw outputs; without g the colour columns are the same BITS and the density column is not."""
    cid, kind, S, regime, exr, bk, noise_std = case
    tr, spec = kind_trainer(kind)
    out = plain_sequence(tr, case)
    gC, gA, g = out.cot
    z, noise = step_depths(out.t, S, S, True), step_noise(wlc.ADJ_N, S, S, noise_std)
    e = wlc.adjoint_figures(out.adj, out.raw[0], out.raw[1], z, out.rd, gC, gA, g, exr, bk, noise)
    e_pred, e_w = rel_linf(out.pred, e["pred"]), float(np.abs(out.w - e["w"]).max())
    print(f"{cid}: pred {e_pred:.2e} weights {e_w:.2e} alpha {out.pred[:, 3].min():.5f} .. {out.pred[:, 3].max():.5f}")
    wlc.held(e, cid)
    assert np.isfinite(out.adj).all() and e_pred <= 1e-5 and e_w <= 1e-5, (e_pred, e_w)
    if regime == "saturated":
        assert (out.pred[:, 3] > 0.99999).sum() >= wlc.ADJ_N / 4, out.pred[:, 3]
    plain = plain_sequence(tr, case, g=None)
    assert np.array_equal(plain.adj[..., :3], out.adj[..., :3]) and not np.array_equal(plain.adj[..., 3], out.adj[..., 3])
    assert np.array_equal(plain.w, out.w) and np.array_equal(plain.pred, out.pred)


@pytest.mark.parametrize("kind", ["chain", "flex"])
def test_a_ray_at_infinity_with_nan_cotangents_takes_exact_zeros(kind):
    """Ray 2 of 5 at t = inf (cone_scale NaN), its rows of d_color, d_alpha and d_weights NaN: its rows of slot 30 are exactly 0, its weights
    are exactly 0, nothing anywhere is non-finite, and every other row -- and the trainer's gradient -- is bit for bit the same batch's with that
    ray's cotangents zeroed."""
    case = [c for c in wlc.ADJ_CASES if c[0] == f"{kind}_S65"][0]
    tr, spec = kind_trainer(kind)
    miss = np.zeros(wlc.ADJ_N, bool); miss[2] = True
    wild, tame = plain_sequence(tr, case, miss=miss, wild=np.nan), plain_sequence(tr, case, miss=miss, wild=0.0)
    assert np.isnan(wild.cot[2][2]).all() and np.isnan(wild.cot[0][2]).all()
    assert (wild.adj[2] == 0).all() and (wild.w[2] == 0).all() and np.isfinite(wild.adj).all() and np.isfinite(wild.grad).all()
    assert np.abs(wild.adj[~miss]).max() > 0 and np.array_equal(wild.adj, tame.adj) and np.array_equal(wild.grad, tame.grad)


# ---- 2. the weights of ntx_train_forward ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chain", "flex"])
def test_the_forward_hands_out_the_fused_steps_weights(kind):
    """`forward(return_weights=True)` leaves the BITS a fused step leaves in a registered buffer (`ntx_trainer_composite_weights`, the coarse
    pass's use), they sum to alpha_pred, and a forward without the keyword writes nothing into a buffer taken back."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.loss import NerfLoss
    case = [c for c in wlc.ADJ_CASES if c[0] == f"{kind}_S129"][0]
    cid, _, S, regime, exr, bk, noise_std = case
    tr, spec = kind_trainer(kind)
    out = plain_sequence(tr, case)
    (ro, rd, t, cone, params), _ = wlc.adjoint_batch(case)
    n = len(t)
    buf = torch.full((n * S + 7,), -7.0, device=dev())
    _lib.check(_lib.lib.ntx_trainer_composite_weights(tr._h, buf.data_ptr()))
    try:
        tr.gradients_step(ro, rd, t, params, cone, np.zeros((n, 3), F), None, NerfLoss(), composite_bkgd=bk, bkgd_color=BKGD, seed=S, n_samples=S)
    finally:
        _lib.check(_lib.lib.ntx_trainer_composite_weights(tr._h, None))
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert (got[n * S:] == -7.0).all() and np.array_equal(got[:n * S].reshape(n, S), out.w) and out.w.sum(1).max() > 0.05
    assert np.abs(out.w.sum(1) - out.pred[:, 3]).max() <= 1e-5
    buf.fill_(-7.0)
    tr.forward(ro, rd, t, params, cone, seed=S, n_samples=S)
    torch.cuda.synchronize()
    assert (buf == -7.0).all()


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", wlc.E2E_CASES, ids=wlc.E2E_IDS)
def test_mse_plus_expected_depth_end_to_end(case):
    """70 rays x 33 samples, loss = mse(color) + 0.5 mean((expected depth - target)^2) as a callable that names `weights` and `z_vals`, through
    `gradients_step`, both gradient modes on: the loss within 1e-5, every layer's weight gradient, dL/d parameters and dL/d rays at the standing
    bars against float64 autograd of the restated step on the trainer's own ReLU patterns."""
    from nerf_tex_amd import train
    model, spec, wts, batch, kn, seed, depth, z = wlc.e2e_setup(case)
    ro, rd, t, cone, rows, color, alpha = batch
    n, S = kn["n"], kn["S"]
    tr = getattr(train, case[1])(model, max_rays=n, n_samples=S, perturb=kn["perturb"], param_gradients=True, input_gradients=True)
    val, cp, ap = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, wlc.depth_loss(color, depth), seed=seed, rays_per_param_row=kn["rpr"])
    got, pg = tr.gradients(), tr.parameter_gradients().cpu().numpy()
    rays = tuple(g.cpu().numpy() for g in tr.ray_gradients())
    torch.cuda.synchronize()
    patterns = clc.chain_patterns(tr, n, S, None) if case[1] == "Trainer" else pgc.trainer_patterns(tr, spec, n, S, None)
    head = wlc.e2e_head(batch, depth, z)
    kw = dict(masks=patterns[0], branch_masks=patterns[1], sigma_mask=patterns[2])
    want = wlc.restated_step(wts, spec, batch, z, kn["rpr"], head, **kw)
    f32 = wlc.restated_step(wts, spec, batch, z, kn["rpr"], head, dtype=torch.float32, **kw)
    val = float(val.item())
    print(f"{case[0]}: loss {val:.9g} want {want.loss:.9g} rel {abs(val - want.loss) / abs(want.loss):.2e}; pred {rel_linf(step_pred(cp, ap), want.pred):.2e}")
    assert abs(val - want.loss) <= 1e-5 * abs(want.loss) and rel_linf(step_pred(cp, ap), want.pred) <= 1e-4
    clc.check_layers(got, spec, want, f32)
    pgc.check_param_gradients(pg, want.param_grad, f32.param_grad)
    igc.check_input_gradients(rays, (want.d_rays_o, want.d_rays_d), (f32.d_rays_o, f32.d_rays_d))
    # the same step by hand -- depths placed first, forward with the weights, the loss in torch, backward with its three cotangents -- is the same bits
    zt = tr._sample_depths(t, seed, S)
    assert np.abs(zt.cpu().numpy() - z).max() <= 1e-6 * np.abs(z).max()
    c, a, w = tr.forward(ro, rd, t, rows, cone, seed=seed, rays_per_param_row=kn["rpr"], z_vals=zt, return_weights=True)
    leaves = [x.detach().requires_grad_(True) for x in (c, a, w)]
    again = wlc.depth_loss(color, depth)(color_pred=leaves[0], alpha_pred=leaves[1], weights=leaves[2], z_vals=zt)
    dc, da, dw = torch.autograd.grad(again, leaves, allow_unused=True)
    tr.backward(dc, da, dw)
    torch.cuda.synchronize()
    assert float(again.item()) == val and np.array_equal(tr.gradients(), got) and np.array_equal(tr.parameter_gradients().cpu().numpy(), pg)


# ---- 4. the registration's rules -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["chain", "flex"])
def test_registration_rules(kind):
    """No registration, a NULL one, and a registration dropped by a new forward or by a fused step all give the plain backward's bits; an
    all-zero g gives equal gradients; g is used once; two identical steps with g give identical bits; nothing pending: NTX_E_INVALID."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.loss import NerfLoss
    case = [c for c in wlc.ADJ_CASES if c[0] == f"{kind}_S65"][0]
    S, bk = case[2], case[5]
    tr, spec = kind_trainer(kind)
    (ro, rd, t, cone, params), (gC, gA, g) = wlc.adjoint_batch(case)
    n = len(t)
    gdev = torch.as_tensor(g, device=dev()).contiguous()
    fwd = lambda: tr.forward(ro, rd, t, params, cone, composite_bkgd=bk, bkgd_color=BKGD, seed=S, n_samples=S)
    register = lambda ptr: _lib.lib.ntx_trainer_weight_cotangent(tr._h, ptr)

    def finish():
        torch.cuda.synchronize()
        return tr.gradients(), tr.activation(30, n * S)

    plain = plain_sequence(tr, case, g=None)
    with_g = plain_sequence(tr, case)
    assert not np.array_equal(plain.grad, with_g.grad) and np.abs(plain.grad).max() > 1e-6
    again = plain_sequence(tr, case)
    assert np.array_equal(again.grad, with_g.grad) and np.array_equal(again.adj, with_g.adj)                  # two identical steps
    after = plain_sequence(tr, case, g=None)                                                                    # used once: the next step is the plain one
    assert np.array_equal(after.grad, plain.grad) and np.array_equal(after.adj, plain.adj)
    zeros = plain_sequence(tr, case, g=np.zeros_like(g))
    assert np.array_equal(zeros.grad, plain.grad) and np.array_equal(zeros.adj, plain.adj)
    # NULL takes a registration back
    fwd(); assert register(gdev.data_ptr()) == _lib.NTX_OK and register(None) == _lib.NTX_OK
    tr.backward(gC, gA)
    assert all(np.array_equal(x, y) for x, y in zip(finish(), (plain.grad, plain.adj.reshape(-1, 4))))
    # a new forward drops it
    fwd(); assert register(gdev.data_ptr()) == _lib.NTX_OK
    fwd(); tr.backward(gC, gA)
    assert all(np.array_equal(x, y) for x, y in zip(finish(), (plain.grad, plain.adj.reshape(-1, 4))))
    # so does a fused step, which also closes the forward
    fwd(); assert register(gdev.data_ptr()) == _lib.NTX_OK
    tr.gradients_step(ro, rd, t, params, cone, np.zeros((n, 3), F), None, NerfLoss(), seed=S, n_samples=S)
    assert register(gdev.data_ptr()) == _lib.NTX_E_INVALID
    fwd(); tr.backward(gC, gA)
    assert all(np.array_equal(x, y) for x, y in zip(finish(), (plain.grad, plain.adj.reshape(-1, 4))))
    # nothing pending
    assert register(gdev.data_ptr()) == _lib.NTX_E_INVALID and register(None) == _lib.NTX_E_INVALID
    with pytest.raises(_lib.NtxError) as err:
        tr.backward(gC, gA, g)
    assert err.value.code == _lib.NTX_E_INVALID
    fwd()
    with pytest.raises(ValueError, match="d_weights"):
        tr.backward(gC, gA, g[:, :-1])
    tr.backward(gC, gA, g)                                                                                      # (a wrong size leaves the forward pending)
    assert all(np.array_equal(x, y) for x, y in zip(finish(), (with_g.grad, with_g.adj.reshape(-1, 4))))


def test_an_ipe_handle_is_refused():
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import Trainer
    from tests.common import make_model
    from tests.train_common import mip_batch
    model, spec, _ = make_model((1, 3), kind="IPE", dense_media=True)
    tr = Trainer(model, max_rays=4, n_samples=8, perturb=False, blur_idx=2)
    ro, rd, t, cone, params = mip_batch(4, 5)
    g = torch.zeros((4, 8), device=dev())
    assert _lib.lib.ntx_trainer_weight_cotangent(tr._h, g.data_ptr()) == _lib.NTX_E_UNSUPPORTED
    tr.forward(ro, rd, t, params, cone)
    assert _lib.lib.ntx_trainer_weight_cotangent(tr._h, g.data_ptr()) == _lib.NTX_E_UNSUPPORTED
    with pytest.raises(_lib.NtxError) as err:
        tr.backward(np.zeros((4, 3), F), None, g)
    assert err.value.code == _lib.NTX_E_UNSUPPORTED
    tr.backward(np.zeros((4, 3), F))                                                                            # the forward was still pending
    with pytest.raises(_lib.NtxError) as err:
        tr.forward(ro, rd, t, params, cone, return_weights=True)
    assert err.value.code == _lib.NTX_E_UNSUPPORTED


# ---- 5. instanced steps ----------------------------------------------------------------------------------------------------------------------
def instanced_trainer(kind, model, n, S):
    case = wlc.INST_KINDS[kind]
    if kind == "chain":
        return fic.chain_trainer(case, model, n, S, pm=True)
    from nerf_tex_amd.train import FlexTrainer
    return FlexTrainer(model, max_rays=n, n_samples=max(S, 2), perturb=False, param_gradients=True)


def instanced_sequence(tr, bufs, hit, cone, kn, cots, g="given"):
    gC, gA, gW = cots
    c, a, w = tr.forward_instanced(bufs, cone, hit=np.asarray(hit).astype(np.uint8), return_weights=True, **fic.fkw(kn))
    tr.backward(gC, gA, gW if g == "given" else None)
    torch.cuda.synchronize()
    return step_pred(c, a), w.cpu().numpy(), tr.gradients(), tr.sample_parameter_gradients().cpu().numpy()


@pytest.mark.parametrize("live", wlc.LIVE)
@pytest.mark.parametrize("kind", sorted(wlc.INST_KINDS))
def test_instanced_steps(kind, live):
    """23 x 70 buffers with some, all and none of the samples live (and 23 x 1): the weights are (1 - el) T at the live samples within 1e-5 of
    float64 and exactly 0 elsewhere, rays with hit == 0 hold NaN in all three cotangents and nothing is non-finite, the compact rows of slot 30
    meet the standing bars, the per-sample parameter gradients are exact zeros off the live samples, and a step without a live sample is
    legal: zero gradients."""
    model, spec, wts, bufs, hit, cone, kn, okw = wlc.instanced_setup(kind, live)
    n, S = bufs[3].shape
    hit = np.asarray(hit, bool)
    mask = itc.live_mask(hit, bufs[3])
    gC, gA, g = (x.copy() for x in wlc.cotangents(n, S, 9))
    clean = (gC.copy(), gA.copy(), g.copy())
    gC[~hit], gA[~hit], g[~hit] = np.nan, np.nan, np.nan
    g[hit[:, None] & ~mask] = np.nan                                                                            # read at live samples only
    tr = instanced_trainer(kind, model, n, S)
    pred, w, grad, spg = instanced_sequence(tr, bufs, hit, cone, kn, (gC, gA, g))
    M = tr.last_live
    assert M == mask.sum() and np.isfinite(pred).all() and np.isfinite(w).all() and np.isfinite(grad).all() and np.isfinite(spg).all()
    assert (w[~mask] == 0).all() and (spg[~mask] == 0).all() and (pred[~hit] == 0).all()
    if live == "some":
        assert (~hit).any() and 0 < M < n * S
    if M == 0:
        assert not grad.any() and not w.any() and not spg.any()
        return
    flex = hasattr(tr, "relu_widths")
    raw, sg = tr.activation(65 if flex else 11, M), tr.activation(64 if flex else 10, M)[:, 0]
    aw = np.asarray(bufs[6]).reshape(-1)[itc.live_order(hit, bufs[3])] if kn["density_reweighting"] else F(1)
    e = wlc.instanced_figures(tr.activation(30, M), raw, sg, bufs, hit, okw, *clean, (sg * aw * F(kn["density_scale"])) > 0)
    e_pred, e_w = rel_linf(pred, e["pred"]), float(np.abs(w - e["w"]).max())
    print(f"{kind} {live}: {M} live; pred {e_pred:.2e} weights {e_w:.2e}")
    wlc.held(e, f"{kind} {live}")
    assert e_pred <= 1e-5 and e_w <= 1e-5 and w.max() > 1e-3, (e_pred, e_w)
    assert np.abs(spg[mask]).max() > 0 and np.abs(grad).max() > 0
    # without g: other gradients, the same weights; and again with g: the same bits
    _, w0, grad0, _ = instanced_sequence(tr, bufs, hit, cone, kn, (gC, gA, g), g=None)
    assert np.array_equal(w0, w) and not np.array_equal(grad0, grad)
    _, _, grad1, spg1 = instanced_sequence(tr, bufs, hit, cone, kn, (gC, gA, g))
    assert np.array_equal(grad1, grad) and np.array_equal(spg1, spg)


# ---- 6. the autograd ops ---------------------------------------------------------------------------------------------------------------------
def test_differentiable_render_with_weights():
    """`DifferentiableRender(trainer, weights=True)`: `total.backward()` of a loss on all three outputs leaves the trainer's gradients bit for
    bit as the explicit forward / weight cotangent / backward sequence does; a loss that leaves the weights out is the plain backward."""
    from nerf_tex_amd.autograd import DifferentiableRender
    from nerf_tex_amd.loss import expected_depth
    case = [c for c in wlc.ADJ_CASES if c[0] == "flex_S65"][0]
    S = case[2]
    tr, spec = kind_trainer("flex")
    (ro, rd, t, cone, params), _ = wlc.adjoint_batch(case)
    tr.set_weights(wlc.kind_model("flex")[2])
    tr.map_exr, tr.raw_noise_std = False, 0.0
    z = tr._sample_depths(t, S, S)
    loss = lambda c, a, w: ((c - 0.5) ** 2).mean() + 0.3 * (a ** 2).mean() + 0.5 * ((expected_depth(w, z) - 1.0) ** 2).mean()
    render = DifferentiableRender(tr, weights=True)
    c, a, w = render(ro, rd, t, params, cone, seed=S, n_samples=S, z_vals=z)
    assert c.requires_grad and a.requires_grad and w.requires_grad and w.shape == (len(t), S)
    loss(c, a, w).backward()
    torch.cuda.synchronize()
    got = tr.gradients()
    c2, a2, w2 = tr.forward(ro, rd, t, params, cone, seed=S, n_samples=S, z_vals=z, return_weights=True)
    assert torch.equal(c2, c) and torch.equal(a2, a) and torch.equal(w2, w)
    leaves = [x.detach().requires_grad_(True) for x in (c2, a2, w2)]
    dc, da, dw = torch.autograd.grad(loss(*leaves), leaves)
    tr.backward(dc, da, dw)
    torch.cuda.synchronize()
    explicit = tr.gradients()
    assert np.abs(got).max() > 1e-6 and np.array_equal(got, explicit)
    tr.forward(ro, rd, t, params, cone, seed=S, n_samples=S, z_vals=z)
    tr.backward(dc, da)
    torch.cuda.synchronize()
    plain = tr.gradients()
    assert not np.array_equal(plain, explicit)
    c, a, w = render(ro, rd, t, params, cone, seed=S, n_samples=S, z_vals=z)
    (((c - 0.5) ** 2).mean() + 0.3 * (a ** 2).mean()).backward()
    torch.cuda.synchronize()
    assert np.array_equal(tr.gradients(), plain)


def test_differentiable_instance_render_with_weights():
    from nerf_tex_amd.autograd import DifferentiableInstanceRender
    model, spec, wts, bufs, hit, cone, kn, okw = wlc.instanced_setup("flex", "some")
    n, S = bufs[3].shape
    tr = instanced_trainer("flex", model, n, S)
    k = fic.fkw(kn)
    render = DifferentiableInstanceRender(tr, k["patch_scale"], k["density_scale"], k["density_reweighting"], weights=True)
    tz = torch.as_tensor(np.nan_to_num(np.asarray(bufs[2], F)), device=dev())
    loss = lambda c, a, w: ((c - 0.5) ** 2).mean() + ((w * tz).sum(-1) ** 2).mean()
    h8 = np.asarray(hit).astype(np.uint8)
    c, a, w = render(bufs, cone, hit=h8, composite_bkgd=k["composite_bkgd"], bkgd_color=BKGD)
    loss(c, a, w).backward()
    torch.cuda.synchronize()
    got = tr.gradients()
    c2, a2, w2 = tr.forward_instanced(bufs, cone, hit=h8, return_weights=True, **k)
    leaves = [x.detach().requires_grad_(True) for x in (c2, a2, w2)]
    dc, da, dw = torch.autograd.grad(loss(*leaves), leaves, allow_unused=True)
    tr.backward(dc, da, dw)
    torch.cuda.synchronize()
    assert torch.equal(w2, w) and np.abs(got).max() > 0 and np.array_equal(tr.gradients(), got)


# ---- 7. streams ----------------------------------------------------------------------------------------------------------------------------------
def test_both_sequences_on_a_side_stream_give_the_null_streams_bits():
    """forward + weight cotangent + backward, plain and instanced, queued on a non-default torch stream: the bits of the null-stream run (the
    registration itself takes no stream and waits for nothing)."""
    case = [c for c in wlc.ADJ_CASES if c[0] == "chain_S129"][0]
    tr, spec = kind_trainer("chain")
    side = torch.cuda.Stream(device=dev())
    ref = plain_sequence(tr, case)
    with torch.cuda.stream(side):
        got = plain_sequence(tr, case)
    assert np.array_equal(got.grad, ref.grad) and np.array_equal(got.adj, ref.adj) and np.array_equal(got.w, ref.w) and np.abs(ref.grad).max() > 0
    model, spec, wts, bufs, hit, cone, kn, okw = wlc.instanced_setup("flex", "some")
    n, S = bufs[3].shape
    itr = instanced_trainer("flex", model, n, S)
    hb = np.asarray(hit, bool)
    cots = wlc.cotangents(n, S, 9)
    ref = instanced_sequence(itr, bufs, hit, cone, kn, cots)
    with torch.cuda.stream(side):
        got = instanced_sequence(itr, bufs, hit, cone, kn, cots)
    assert all(np.array_equal(x, y) for x, y in zip(got, ref)) and np.abs(ref[2]).max() > 0 and hb.any()
