"""Training under any loss on the GPU: `ntx_train_forward` / `ntx_train_backward` (`Trainer.forward` / `backward`,
`nerf_tex_amd.autograd.DifferentiableRender`, `gradients_step` with a loss written in PyTorch).  `-m gpu`.

1. `composite_adjoint_kernel` alone against float64 autograd of the composite on the trainer's own raw outputs, at
   tests/test_gpu_train_composite.py's bars.  2. The fused step is a special case: with NerfLoss(mse)'s cotangents the gradients are the fused
   step's BITS (both kernels share the adjoint's code).  3. A loss the library does not know end to end on the three trainers, against the
   float64 restatement of tests/custom_loss_common.py.  4. Rays that miss the proxy take no gradient whatever their cotangent holds.
   5. Lifecycle: one backward per forward.  6. Reproducibility and capacity.  7. `Train` and `ParameterFitter.fit` with such a loss.
profiles/custom_loss/adjoint_errors.md has the figures test 1 printed on an MI355X."""

from types import SimpleNamespace

import numpy as np
import pytest

from tests import custom_loss_common as clc
from tests import param_grad_common as pgc
from tests.test_gpu_train_composite import CAP_RAYS, CAP_S, chain, mip, ray_batch, regime_blob        # noqa: F401 (chain, mip: fixtures)
from tests.train_common import BKGD, raw_outputs, rel_linf, step_depths, step_noise, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
N, S0 = clc.N_RAYS, clc.N_SAMPLES
GATES = dict(drgb=5e-6, dsigma=5e-5)                                               # tests/test_gpu_train_composite.py's
# case label -> the adjoints held to 4 x the float32 floor measured beside them instead of GATES (profiles/custom_loss/adjoint_errors.md)
FLOOR_GATED = {}
ADJ_S = [2, 3, 64, 65, 129, 257, 1024]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]               # (map_exr, background)


def dev():
    return torch.device("cuda", 0)


def make_trainer(case, mode=False, max_rays=N, n_samples=S0):
    """(trainer, spec, weights, batch, knobs) of a `clc.TRAINER_CASES` entry; `mode`: param_gradients of a layer-by-layer trainer."""
    from nerf_tex_amd import train
    model, spec, wts, batch, kn = clc.trainer_case(case)
    kw = dict(param_gradients=mode) if case[1] != "Trainer" else {}
    tr = getattr(train, case[1])(model, max_rays=max_rays, n_samples=n_samples, perturb=kn["perturb"], **kw)
    return tr, spec, wts, batch, kn


def forward_of(tr, batch, kn, **kw):
    ro, rd, t, cone, rows, _, _ = batch
    return tr.forward(ro, rd, t, rows, cone, seed=kn["seed"], rays_per_param_row=kn["rpr"], n_samples=S0, **kw)


def cotangents(n, seed):
    """Seeded cotangents of both signs, of the size a mean over the rays gives them."""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) / (3 * n)).astype(F), (rng.normal(size=n) / n).astype(F)


# ---- 1. the adjoint alone -----------------------------------------------------------------------------------------------------------
def adjoint_alone(h, S, regime, map_exr, bkgd, noise_std, label):
    """`forward` + `backward` on seeded cotangents; `activation(30)` against float64 autograd of the composite on the step's own raw outputs."""
    n, seed = 5, S
    ro, rd, t, cone, params, _, _ = ray_batch(n, 40 + S, ipe=h.ipe)
    tr = h.tr
    tr.set_weights(regime_blob(h, regime))
    tr.map_exr, tr.raw_noise_std = bool(map_exr), float(noise_std)
    cp, ap = tr.forward(ro, rd, t, params, cone, composite_bkgd=bkgd, bkgd_color=BKGD, seed=seed, n_samples=S)
    gC, gA = cotangents(n, 100 + S)
    tr.backward(gC, gA)
    torch.cuda.synchronize()
    pred = step_pred(cp, ap)
    (raw, sg), adj = raw_outputs(tr, n, S), tr.activation(30, n * S).reshape(n, S, 4)
    z, noise = step_depths(t, S + 1 if h.ipe else S, seed, True), step_noise(n, S, seed, noise_std)
    run = lambda dtype: clc.composite_cotangent_adjoint(raw, sg, None, gC, gA, map_exr, bkgd, BKGD, noise, dtype, z=z, rays_d=rd, mip=h.ipe)
    w_rgb, w_sg, w_c, w_a = run(torch.float64)
    f_rgb, f_sg, _, _ = run(torch.float32)
    e = dict(drgb=rel_linf(adj[..., :3], w_rgb), dsigma=rel_linf(adj[..., 3], w_sg), f_drgb=rel_linf(f_rgb, w_rgb), f_dsigma=rel_linf(f_sg, w_sg))
    e_pred = rel_linf(pred, np.concatenate([w_c, w_a[:, None]], -1))
    floored = FLOOR_GATED.get(label, ())
    print(f"| {label} | {e['drgb']:.2e} | {e['f_drgb']:.2e} | {e['dsigma']:.2e} | {e['f_dsigma']:.2e} | {e_pred:.2e} | alpha {pred[:, 3].min():.5f} .. {pred[:, 3].max():.5f} | "
          f"{' '.join(floored) or '-'} |")
    assert np.isfinite(adj).all() and np.abs(w_rgb).max() > 1e-8 and np.abs(w_sg).max() > 1e-8
    if regime.startswith("saturated"):
        assert (pred[:, 3] > 0.99999).sum() >= n / 4, pred[:, 3]
    assert e_pred <= 1e-5, e_pred
    for key in ("drgb", "dsigma"):
        gate = 4 * e["f_" + key] if key in floored else GATES[key]
        assert e[key] <= gate, (label, key, e[key], gate, e["f_" + key])


@pytest.mark.parametrize("regime", ["mixed", "saturated"])
@pytest.mark.parametrize("S", ADJ_S)
def test_adjoint_alone(chain, S, regime):
    """Sample counts either side of the chunks of 64 both scans work in, up to the 1024 a ray may have; rays of every opacity and rays that end
    opaque; the colour map and the background term in turn over the counts, the density regulariser on once (S = 65, mixed)."""
    map_exr, bkgd = FLAGS[(ADJ_S.index(S) + (regime == "saturated")) % 4]
    label = f"adjoint S{S} {regime} exr{int(map_exr)} bk{int(bkgd)}"
    adjoint_alone(chain, S, regime + "_S2" * (S == 2 and regime == "saturated"), map_exr, bkgd, 0.1 if (S, regime) == (65, "mixed") else 0.0, label)


def test_adjoint_alone_behind_an_ipe_trainer(mip):
    """The same kernel behind an IPE handle: a sample's length is its cone segment's, 65 segments between 66 edges."""
    adjoint_alone(mip, 65, "thin", True, True, 0.1, "adjoint mip S65 thin exr1 bk1")


# ---- 2. the fused step is a special case -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bkgd", [False, True], ids=["no_background", "background"])
@pytest.mark.parametrize("case", clc.TRAINER_CASES, ids=[c[0] for c in clc.TRAINER_CASES])
def test_the_fused_step_is_a_special_case(case, bkgd):
    """`forward`'s predictions are `gradients_step`'s bits, and with NerfLoss(mse)'s cotangents -- formed in float32 as the kernel forms them,
    ((-2) (t - p)) * (1 / (3n)), d_alpha NULL -- `backward` leaves the fused step's gradient vector (and parameter gradients) bit for bit."""
    from nerf_tex_amd.loss import NerfLoss
    tr, spec, wts, batch, kn = make_trainer(case, mode=True)
    ro, rd, t, cone, rows, color, alpha = batch
    n = len(t)
    val, cp, ap = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, NerfLoss("network.loss.mse"), composite_bkgd=bkgd, bkgd_color=BKGD, seed=kn["seed"],
                                    rays_per_param_row=kn["rpr"])
    fused = tr.gradients()
    fused_pg = tr.parameter_gradients().cpu().numpy() if case[1] != "Trainer" else None
    cf, af = forward_of(tr, batch, kn, composite_bkgd=bkgd, bkgd_color=BKGD)
    assert torch.equal(cf, cp) and torch.equal(af, ap)
    p = cp.cpu().numpy()
    d_color = (F(-2) * (color - p)) * (F(1) / F(3 * n))
    assert d_color.dtype == F
    tr.backward(d_color, None)
    torch.cuda.synchronize()
    assert np.abs(fused).max() > 1e-6 and np.array_equal(tr.gradients(), fused)
    if fused_pg is not None:
        assert np.abs(fused_pg).max() > 1e-6 and np.array_equal(tr.parameter_gradients().cpu().numpy(), fused_pg)


# ---- 3. a loss the library does not know, end to end ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", clc.TRAINER_CASES, ids=[c[0] for c in clc.TRAINER_CASES])
def test_a_loss_the_library_does_not_know(case):
    """`DifferentiableRender` + `CharbonnierAlpha` + `total.backward()`: the loss within 1e-5, every layer's gradient within max(1e-4, 4 float32
    floors) of the float64 restatement branched by the trainer's own ReLU patterns; on the layer-by-layer trainers `parameters.grad` per column at
    `check_param_gradients`' bar, and a torch regulariser on the parameters adds its own gradient exactly."""
    from nerf_tex_amd.autograd import DifferentiableRender
    flex = case[1] != "Trainer"
    tr, spec, wts, batch, kn = make_trainer(case, mode=True)
    ro, rd, t, cone, rows, color, alpha = batch
    n = len(t)
    loss, render = clc.CharbonnierAlpha(), DifferentiableRender(tr)
    ct, at = torch.as_tensor(color, device=dev()), torch.as_tensor(alpha, device=dev())
    regulariser = lambda p: 0.01 * (p ** 2).sum() + 0.003 * p.sum()

    def run(with_regulariser):
        params = torch.tensor(rows, device=dev(), requires_grad=flex)
        cp, ap = render(ro, rd, t, params, cone, seed=kn["seed"], rays_per_param_row=kn["rpr"], n_samples=S0)
        assert cp.requires_grad and ap.requires_grad
        val = loss(color_true=ct, alpha_true=at, color_pred=cp, alpha_pred=ap)
        (val + regulariser(params) if with_regulariser else val).backward()
        torch.cuda.synchronize()
        return float(val.item()), params, tr.gradients()

    val, params, got = run(False)
    patterns = pgc.trainer_patterns(tr, spec, n, S0, None) if flex else clc.chain_patterns(tr, n, S0, None)
    z = step_depths(t, S0, kn["seed"], kn["perturb"])
    head = clc.loss_head(loss, color, alpha)
    restate = lambda dtype: clc.restated(wts, spec, ro, rd, z, rows, kn["rpr"], cone, head, dtype=dtype, masks=patterns[0], branch_masks=patterns[1], sigma_mask=patterns[2])
    want, f32 = restate(torch.float64), restate(torch.float32)
    print(f"{case[0]}: loss {val:.9g} want {want.loss:.9g} rel {abs(val - want.loss) / abs(want.loss):.2e}; max |grad| {np.abs(want.grad).max():.3e}")
    assert abs(val - want.loss) <= 1e-5 * abs(want.loss)
    clc.check_layers(got, spec, want, f32)
    if flex:
        pg = params.grad.cpu().numpy()
        assert pg.shape == rows.shape
        pgc.check_param_gradients(pg, want.param_grad, f32.param_grad)
        val2, params2, got2 = run(True)
        leaf = torch.tensor(rows, device=dev(), requires_grad=True)
        own, = torch.autograd.grad(regulariser(leaf), leaf)
        assert val2 == val and np.array_equal(got2, got) and own.abs().min() > 0
        assert torch.equal(params2.grad, params.grad + own)
    else:
        assert params.grad is None


# ---- 4. rays that miss the proxy --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", clc.TRAINER_CASES[:2], ids=[c[0] for c in clc.TRAINER_CASES[:2]])
def test_rays_that_miss_take_no_gradient_whatever_their_cotangent(case):
    """Rays 0, 5, 17 and 44 at t = inf (cone_scale NaN) with cotangents 1e30, NaN, +inf and -inf: every gradient is bit for bit the same batch's
    with those cotangents zeroed, and nothing is non-finite."""
    tr, spec, wts, batch, kn = make_trainer(case, mode=True)
    ro, rd, t, cone, rows, color, alpha = batch
    n = len(t)
    miss = np.zeros(n, bool); miss[[0, 5, 17, 44]] = True
    t, cone = t.copy(), cone.copy()
    t[miss] = np.inf; cone[miss] = np.nan
    batch = (ro, rd, t, cone, rows, color, alpha)
    gC, gA = cotangents(n, 7)
    wild_C, wild_A = gC.copy(), gA.copy()
    wild_C[0], wild_C[5], wild_C[17], wild_C[44] = 1e30, np.nan, np.inf, (-np.inf, 1.0, np.nan)
    wild_A[0], wild_A[5], wild_A[17], wild_A[44] = np.nan, -1e30, np.inf, 0.0
    gC[miss], gA[miss] = 0, 0
    out = []
    for dC, dA in ((wild_C, wild_A), (gC, gA)):
        cp, ap = forward_of(tr, batch, kn, composite_bkgd=True, bkgd_color=BKGD)
        tr.backward(dC, dA)
        torch.cuda.synchronize()
        out.append((tr.gradients(), tr.parameter_gradients().cpu().numpy() if case[1] != "Trainer" else np.zeros(1), step_pred(cp, ap)))
    (g1, p1, pred), (g0, p0, _) = out
    assert (pred[miss, 3] == 0).all() and (pred[miss, :3] == np.asarray(BKGD, F)).all()
    assert np.isfinite(g1).all() and np.isfinite(p1).all() and np.abs(g0).max() > 1e-6
    assert np.array_equal(g1, g0) and np.array_equal(p1, p0)


# ---- 5. lifecycle -------------------------------------------------------------------------------------------------------------------------
def test_one_backward_per_forward():
    """NTX_E_INVALID: backward before any forward, on a NULL d_color (the forward stays pending), twice, and after a fused step in between.
    A parameters-only trainer runs forward and backward, leaves the weight gradient alone and still refuses Adam.  `DifferentiableRender`
    raises on a second backward; a coarse + fine trainer refuses a loss without desc()."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.autograd import DifferentiableRender
    from nerf_tex_amd.loss import NerfLoss
    from nerf_tex_amd.train import CoarseFineTrainer
    from tests.common import make_model
    case = clc.TRAINER_CASES[1]
    tr, spec, wts, batch, kn = make_trainer(case)
    ro, rd, t, cone, rows, color, alpha = batch
    gC, gA = cotangents(len(t), 3)

    def refused(call):
        with pytest.raises(_lib.NtxError) as e:
            call()
        return e.value.code == _lib.NTX_E_INVALID

    assert refused(lambda: tr.backward(gC, gA))
    forward_of(tr, batch, kn)
    assert refused(lambda: tr.backward(None))
    tr.backward(gC)                                                                # d_alpha NULL; the forward was still pending
    first = tr.gradients()
    assert refused(lambda: tr.backward(gC, gA)) and np.abs(first).max() > 0
    forward_of(tr, batch, kn)
    tr.gradients_step(ro, rd, t, rows, cone, color, alpha, NerfLoss(), seed=kn["seed"], rays_per_param_row=kn["rpr"])
    assert refused(lambda: tr.backward(gC, gA))
    with pytest.raises(ValueError):
        forward_of(tr, batch, kn); tr.backward(gC[:-1], gA)
    tr.backward(gC, gA)                                                            # (a wrong size leaves the forward pending too)
    # parameters only
    only, _, _, _, _ = make_trainer(case, mode="only")
    before = only.gradients()
    forward_of(only, batch, kn)
    only.backward(gC, gA)
    pg = only.parameter_gradients()
    torch.cuda.synchronize()
    assert torch.isfinite(pg).all() and float(pg.abs().max()) > 0 and np.array_equal(only.gradients(), before)
    assert refused(only.apply_gradients)
    # the autograd op
    render = DifferentiableRender(tr)
    cp, ap = render(ro, rd, t, rows, cone, seed=kn["seed"], rays_per_param_row=kn["rpr"])
    total = cp.sum() + ap.sum()
    total.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="one backward per forward"):
        total.backward()
    with pytest.raises(ValueError, match="requires_grad"):
        render(ro, rd, t, torch.tensor(rows, device=dev(), requires_grad=True), cone)
    small = lambda seed: make_model((0, 0), kind="Nerf", seed=seed, arch=dict(width=64, depth=3, skips=[1]))[0]
    two = CoarseFineTrainer(small(0), small(1), max_rays=8, n_samples=8, n_importance=8)
    with pytest.raises(TypeError, match="coarse"):
        two.gradients_step(ro[:8], rd[:8], t[:8], None, cone[:8], color[:8], alpha[:8], clc.CharbonnierAlpha())
    with pytest.raises(TypeError):
        DifferentiableRender(two)


# ---- 6. reproducibility and capacity -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", clc.TRAINER_CASES[:2], ids=[c[0] for c in clc.TRAINER_CASES[:2]])
def test_forward_backward_is_reproducible_and_independent_of_capacity(case):
    """The same forward and backward twice, and on a trainer made for 256 rays and more samples a ray whose buffers hold another, bigger batch:
    predictions, weight gradients and parameter gradients bit for bit."""
    from nerf_tex_amd.loss import NerfLoss
    from tests.train_flex_common import flex_batch
    tr, spec, wts, batch, kn = make_trainer(case, mode=True)
    big, _, _, _, _ = make_trainer(case, mode=True, max_rays=256, n_samples=S0 + 7)
    ro, rd, t, cone, params, color, alpha = flex_batch(8, 256, S0 + 7, spec, case[4])
    big.gradients_step(ro, rd, t, params, cone, color, alpha, NerfLoss(), seed=1)
    gC, gA = cotangents(N, 5)
    out = []
    for who in (tr, tr, big):
        cp, ap = forward_of(who, batch, kn)
        who.backward(gC, gA)
        torch.cuda.synchronize()
        out.append((step_pred(cp, ap), who.gradients(), who.parameter_gradients().cpu().numpy() if case[1] != "Trainer" else np.zeros(1)))
    assert np.abs(out[0][1]).max() > 1e-6
    for other in out[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(out[0], other))


# ---- 7. Train and ParameterFitter ------------------------------------------------------------------------------------------------------------
def test_train_with_a_loss_config_naming_a_user_class(tmp_path):
    """`Train` for 3 iterations with `loss_config = {'module': 'tests.custom_loss_common.CharbonnierAlpha', ...}` ends on the weights and Adam
    moments of a hand-written forward / loss / backward / `apply_gradients` loop, bit for bit."""
    from nerf_tex_amd.train import FlexTrainer, Train, Trainer
    from tests.common import make_model
    from tests.test_gpu_train import batch
    from tests.test_gpu_train_flex import carpet_config
    arch = dict(width=64, depth=4)
    seeded, _, _ = make_model((1, 6), dense_media=True, arch=arch)
    B, R, S = 2, 64, 32
    ro, rd, t, cone, params, color, alpha = batch(31, B * R, S, 7, "carpet")
    data = dict(rays_o=ro.reshape(B, R, 3), rays_d=rd.reshape(B, R, 3), t=t.reshape(B, R, 2), cone_scale=cone.reshape(B, R, 1), parameters=params[::R].copy(),
                color=color.reshape(B, R, 3), alpha=alpha.reshape(B, R))

    class Batches:
        composite_bkgd, bkgd_color = False, (1., 1., 1.)
        def __iter__(self):
            while True:
                yield data

    cfg = carpet_config(**arch)
    common = dict(model_config=cfg["model_config"], loss_config={"module": "tests.custom_loss_common.CharbonnierAlpha", "eps": 1e-3, "gamma": 0.1}, lrate=cfg["lrate"],
                  lrate_decay=cfg["lrate_decay"], renderer_config=dict(cfg["renderer_config"], n_samples=S))
    out = Train(str(tmp_path / "a"), Batches(), None, n_iters=3, logger_config=dict(i_print=1, i_img=0, i_checkpoint=0, print_model_summary=False),
                weights=seeded.get_blob(), **common)
    a = out["trainer"]
    assert type(a) is FlexTrainer and a.iterations == 3 and len(out["loss"]) == 3
    b, loss = Trainer.from_config(common, max_rays=B * R, weights=seeded.get_blob())
    assert isinstance(loss, clc.CharbonnierAlpha) and type(b) is FlexTrainer
    ct, at = torch.as_tensor(color, device=dev()), torch.as_tensor(alpha, device=dev())
    values = []
    for _ in range(3):
        cp, ap = b.forward(ro, rd, t, data["parameters"], cone, rays_per_param_row=R)
        c, al = cp.detach().requires_grad_(True), ap.detach().requires_grad_(True)
        val = loss(color_true=ct, alpha_true=at, color_pred=c, alpha_pred=al)
        val.backward()
        b.backward(c.grad, al.grad)
        b.apply_gradients()
        values.append(float(val.item()))
    torch.cuda.synchronize()
    assert values == [v for _, v in out["loss"]] and not np.array_equal(a.weights(), np.asarray(seeded.get_blob(), F).reshape(-1))
    assert np.array_equal(a.weights(), b.weights()) and all(np.array_equal(x, y) for x, y in zip(a.adam_state(), b.adam_state()))


def test_fitting_parameters_under_such_a_loss():
    """`ParameterFitter.fit` with `CharbonnierAlpha` on tests/param_grad_common.py's teacher images: 40 Adam steps from 0.2 off lower the loss."""
    from nerf_tex_amd.fit import ParameterFitter
    f = pgc.FIT
    model, spec, wts, batch, true, init = pgc.fit_setup()
    blob = np.array(model.get_blob(), F, copy=True)
    fitter = ParameterFitter(model, n_samples=f["S"], max_rays=f["images"] * f["rays"], lrate=f["lrate"])
    params, losses = fitter.fit(batch, clc.CharbonnierAlpha(), init, 40)
    params = params.cpu().numpy()
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e}; |p - true| {np.abs(init - true).max():.3f} -> {np.abs(params - true).max():.3f}")
    assert len(losses) == 40 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert not np.array_equal(params, init) and np.array_equal(fitter.weights(), blob)
