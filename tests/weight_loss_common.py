"""What the tests of losses on the compositing weights share (tests/test_weight_losses.py on the CPU, tests/test_gpu_weight_losses.py on the
GPU; `ntx_trainer_weight_cotangent`, `Trainer.forward(return_weights=)` / `backward(d_weights=)`): the composite restated
WITH its weights as a result, the division-free recurrences of `ray_adjoint` with c + g in the place of c written out in float64, the
cases of the GPU file, and a restatement of a whole step whose loss takes the weights.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED as the rest of the training oracle.  The composite is restated here in the issue's words,
    w = a * cumprod(1 - a + 1e-10, exclusive),
because oracle/torch_cpu.composite returns (c, a) alone; tests/test_weight_losses.py holds its c and a to that function's in float64.  The
network is the oracle's (`tro.render`, `tbo.render`): `capture` swaps this composite in for the length of a call and keeps the weights (and the
raw outputs) it saw.

The bars are the standing ones.  The adjoint alone (tests/train_common.adjoint_errors, tests/test_gpu_custom_loss.py): dL/d raw colour within
max(5e-6, 4 float32 floors), dL/d raw density within max(5e-5, 4 floors), rel-Linf over the batch, on the step's own raw outputs.  The guards
that keep a floor from hiding a failure are the project's: floor <= 5e-4 and a gradient worth the name (> 1e-8, test_gpu_custom_loss's).
End to end: `clc.check_layers`, `pgc.check_param_gradients`, `igc.check_input_gradients` (max(1e-4, 4 floors) under floor <= 5e-4, max |grad| >
1e-6).  tests/test_weight_losses.py holds every GPU case MARGIN times inside those guards on the CPU, and the weight cotangent's effect on the
density column more than 10 bars wide."""

from contextlib import contextmanager
from types import SimpleNamespace
from unittest import mock

import numpy as np
import torch

from nerf_tex_amd.loss import expected_depth
from oracle import train_oracle as tro
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests import train_branch_oracle as tbo
from tests.train_common import BKGD, F, layer_slices, rel_linf, step_depths, step_noise

MARGIN = pgc.MARGIN
GATES = dict(drgb=5e-6, dsigma=5e-5)                      # tests/train_common.adjoint_errors' / tests/test_gpu_train_composite.py's
FLOOR_GUARD, GRAD_GUARD = 5e-4, 1e-8
SEEN = 10.0                                               # the cotangent moves the density column by more than this many bars


# ---- the composite, restated with its weights ------------------------------------------------------------------------------------------------
def composite(color, alpha, dists, map_exr=False, composite_bkgd=False, bkgd=BKGD, sigma_mask=None, noise=None):
    """map_model_output (renderer.py:170-213) on raw outputs color [n, S, 3], alpha [n, S] and lengths dists [n, S]: (c, a, w) with
    w = a * cumprod(1 - a + 1e-10, exclusive).  Arguments as oracle/torch_cpu.composite's."""
    if noise is not None:
        alpha = alpha + noise
    rgb = torch.nn.functional.elu(color) + 1 if map_exr else torch.sigmoid(color)
    am = 1.0 - torch.exp(-(torch.relu(alpha) if sigma_mask is None else alpha * sigma_mask) * dists)
    w = am * exclusive_cumprod(1.0 - am + 1e-10)
    c, a = torch.sum(w[..., None] * rgb, -2), torch.sum(w, -1)
    if composite_bkgd:
        c = c + (1.0 - a[..., None]) * torch.as_tensor(bkgd, dtype=c.dtype)
    return c, a, w


def exclusive_cumprod(f):
    trans = torch.cumprod(f, -1)
    return torch.cat([torch.ones_like(trans[..., :1]), trans[..., :-1]], -1)


@contextmanager
def capture():
    """The oracle's renders (`tro.render`, `tbo.render`) on `composite` above for the length of the block; yields a namespace that holds what
    the last call saw: `raw` [n, S, 3], `sigma` [n, S], `dists`, and its weights `w` (torch tensors, in the graph)."""
    seen = SimpleNamespace(raw=None, sigma=None, dists=None, w=None)

    def stand_in(color, alpha, dists, *args):
        c, a, w = composite(color, alpha, dists, *args)
        seen.raw, seen.sigma, seen.dists, seen.w = color, alpha, dists, w
        return c, a
    with mock.patch.object(tro, "composite", stand_in), mock.patch.object(tbo, "composite", stand_in):
        yield seen


def instanced_composite(raw_live, sigma_live, bufs, hit, okw, sigma_mask=None, dtype=torch.float64):
    """The instanced composite (tests/instanced_train_common.restated's lines) on GIVEN network outputs in compact row order, torch tensors
    raw_live [M', 3] and sigma_live [M']: (c [n, 3], a [n], w [n, S]) -- w without the appended sample's weight, 0 at samples that are not
    live and on rays with hit == 0.  `okw`: the restatement's keywords."""
    rays_d_map, pts, tt, dists, color_last, alpha_last, alpha_weight = [np.asarray(b) for b in bufs[:7]]
    n, S = dists.shape
    live = itc.live_order(hit, dists)
    li = torch.as_tensor(live)
    t_ = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=dtype)
    at_live = lambda x: t_(np.nan_to_num(np.asarray(x, np.float64)).reshape(n * S)[live])
    sp = sigma_live * (at_live(alpha_weight) if okw["density_reweighting"] else 1.0) * okw["density_scale"]
    gate = torch.relu(sp) if sigma_mask is None else sp * t_(np.asarray(sigma_mask))
    a_live = 1.0 - torch.exp(-gate * at_live(dists) / itc.PATCH_SCALE)
    rgb_live = torch.nn.functional.elu(raw_live) + 1 if okw["map_exr"] else torch.sigmoid(raw_live)
    am = torch.zeros(n * S, dtype=dtype).index_put((li,), a_live).reshape(n, S)
    rgb = torch.zeros((n * S, 3), dtype=dtype).index_put((li,), rgb_live).reshape(n, S, 3)
    am = torch.cat([am, t_(alpha_last).reshape(n, 1)], 1)
    rgb = torch.cat([rgb, t_(color_last).reshape(n, 1, 3)], 1)
    w = am * exclusive_cumprod(1.0 - am + 1e-10)
    c, a = torch.sum(w[..., None] * rgb, -2), torch.sum(w, -1)
    if okw["composite_bkgd"]:
        c = c + (1.0 - a[..., None]) * torch.as_tensor(BKGD, dtype=dtype)
    h_ = torch.as_tensor(np.asarray(hit, bool))
    zero = torch.zeros((), dtype=dtype)
    return torch.where(h_[:, None], c, zero), torch.where(h_, a, zero), torch.where(h_[:, None], w[:, :S], zero)


# ---- the adjoint under three cotangents: autograd of the restatement, and the kernel's recurrences written out ------------------------------
def surrogate(c, a, w, gC, gA, g):
    """<c, gC> + <a, gA> + <w, g>: linear in the composite's three results, so its gradient is the adjoint applied to the cotangents."""
    t_ = lambda x: torch.tensor(np.asarray(x), dtype=c.dtype)
    val = (c * t_(gC)).sum()
    if gA is not None:
        val = val + (a * t_(gA)).sum()
    return val if g is None else val + (w * t_(g)).sum()


def plain_adjoint(raw, sigma, z, rays_d, gC, gA, g, map_exr=False, bkgd=False, noise=None, dtype=torch.float64, dists=None):
    """(dL/d raw colour [n, S, 3], dL/d raw density [n, S], c, a, w) of the plain composite on GIVEN raw outputs under the surrogate -- what
    slot 30 holds after forward + `weight_cotangent` + backward.  The lengths from the depths `z` and `rays_d` as `tro.fourier_dists` forms them,
    or `dists` as given."""
    t_ = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=dtype)
    rgb, sg = t_(raw).requires_grad_(True), t_(sigma).requires_grad_(True)
    lengths = t_(dists) if dists is not None else tro.fourier_dists(t_(z), t_(rays_d))
    c, a, w = composite(rgb, sg, lengths, map_exr, bkgd, BKGD, None, t_(noise))
    surrogate(c, a, w, gC, gA, g).backward()
    return rgb.grad.numpy(), sg.grad.numpy(), c.detach().numpy(), a.detach().numpy(), w.detach().numpy()


def instanced_adjoint(raw_live, sigma_live, bufs, hit, okw, gC, gA, g, sigma_mask=None, dtype=torch.float64):
    """The same for the instanced composite: ([M', 4] = dL/d raw colour | dL/d raw density in compact row order, c, a, w)."""
    t_ = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=dtype)
    raw, sg = t_(raw_live).requires_grad_(True), t_(sigma_live).requires_grad_(True)
    c, a, w = instanced_composite(raw, sg, bufs, hit, okw, sigma_mask, dtype)
    val = surrogate(c, a, w, gC, gA, g)
    if val.requires_grad:
        val.backward()
    zero = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().astype(np.float64)
    return np.concatenate([zero(raw), zero(sg)[:, None]], -1), c.detach().numpy(), a.detach().numpy(), w.detach().numpy()


def recurrence(a, rgb, dC, dA, g, bkgd=None, color_last=None, alpha_last=None):
    """dL/da [S] of ONE ray by `ray_adjoint`'s recurrences with c + g in the place of c (float64 numpy, back to front, nothing divided):
        dL/da_i = T_i (dA' Z_i + ((c_i + g_i) - V_i)),  V_{i-1} = (c_i + g_i) a_i + f_i V_i,  Z_{i-1} = f_i Z_i - 1e-10,  f_i = (1 - a_i) + 1e-10,
    c_i = dC . rgb_i, dA' = dA - dC . bkgd.  Plain: V_{S-1} = 0, Z_{S-1} = 1.  With an appended sample (`color_last`, `alpha_last`; it has no
    g): V_{S-1} = (dC . color_last) alpha_last, Z_{S-1} = ((1 - alpha_last) + 1e-10) - 1e-10."""
    a, rgb, dC, g = (np.asarray(x, np.float64) for x in (a, rgb, dC, g))
    S = len(a)
    f = (1.0 - a) + 1e-10
    T = np.concatenate([[1.0], np.cumprod(f)[:-1]])
    dAp = float(dA) - (float(dC @ np.asarray(bkgd, np.float64)) if bkgd is not None else 0.0)
    V, Z = 0.0, 1.0
    if alpha_last is not None:
        V, Z = float(dC @ np.asarray(color_last, np.float64)) * float(alpha_last), ((1.0 - float(alpha_last)) + 1e-10) - 1e-10
    out = np.zeros(S)
    for i in range(S - 1, -1, -1):
        cg = float(dC @ rgb[i]) + g[i]
        out[i] = T[i] * (dAp * Z + (cg - V))
        V, Z = cg * a[i] + f[i] * V, f[i] * Z - 1e-10
    return out


def adjoint_figures(got, raw, sigma, z, rays_d, gC, gA, g, map_exr, bkgd, noise, dists=None):
    """Errors and float32 floors of a plain adjoint `got` [n, S, 4] (None: the floors alone) against float64 on the same raw outputs, and how
    far the weight cotangent moves the density column: `seen` = rel-Linf of the float64 column with g against the one without."""
    run = lambda dtype, gg: plain_adjoint(raw, sigma, z, rays_d, gC, gA, gg, map_exr, bkgd, noise, dtype, dists)
    w_rgb, w_sg, c, a, w = run(torch.float64, g)
    f_rgb, f_sg = run(torch.float32, g)[:2]
    _, n_sg = run(torch.float64, None)[:2]
    e = dict(f_drgb=rel_linf(f_rgb, w_rgb), f_dsigma=rel_linf(f_sg, w_sg), seen=rel_linf(n_sg, w_sg), max_drgb=float(np.abs(w_rgb).max()), max_dsigma=float(np.abs(w_sg).max()),
             want=np.concatenate([w_rgb, w_sg[..., None]], -1), pred=np.concatenate([c, a[:, None]], -1), w=w)
    if got is not None:
        e.update(drgb=rel_linf(got[..., :3], w_rgb), dsigma=rel_linf(got[..., 3], w_sg))
    return e


def bars(e):
    return {k: max(GATES[k], 4 * e["f_" + k]) for k in GATES}


def guards(e, margin=1.0):
    """A floor cannot hide a failure, a gradient is worth the name, and a cotangent too small to see would test nothing."""
    for k in GATES:
        assert e["f_" + k] <= FLOOR_GUARD / margin, (k, e["f_" + k], "a float32 floor inside the guard by less than the margin: change the seed, not the bar")
        assert e["max_" + k] >= GRAD_GUARD * margin, (k, e["max_" + k])
    assert e["seen"] > SEEN * bars(e)["dsigma"], ("the weight cotangent moves the density column by", e["seen"], "bars of", bars(e)["dsigma"])


def held(e, label, report=print):
    """The figures, printed; then the guards; then the bars."""
    b = bars(e)
    report(f"| {label} | drgb {e['drgb']:.2e} floor {e['f_drgb']:.2e} bar {b['drgb']:.1e} | dsigma {e['dsigma']:.2e} floor {e['f_dsigma']:.2e} bar {b['dsigma']:.1e} | "
           f"seen {e['seen']:.2e} |")
    guards(e)
    for k in GATES:
        assert e[k] <= b[k], (label, k, e[k], b[k], e["f_" + k])


# ---- the cases of the adjoint alone ------------------------------------------------------------------------------------------------------
# the three trainers: name -> (class, n_parameters, arch, family)
KINDS = {"chain": ("Trainer", (1, 6), None, "carpet"),
         "flex": ("FlexTrainer", (1, 6), dict(width=64, depth=3, skips=[1]), "carpet"),
         "branch": ("BranchTrainer", (1, 4), dict(depth=3, width=64, skips=[1], color_depth=1, param_depth=2, param_width=128), "grass")}
# regime -> (the shift of alpha.bias, of color.bias) on the dense-media weights, as tests/test_gpu_train_composite.py REGIMES: "mixed" rays of
# every opacity; "saturated" tests/test_gpu_train.py test_saturated_rays_keep_their_gradient's family (the density head's bias raised by 10)
REGIMES = dict(mixed=(2.0, 0.45), saturated=(10.0, 0.45))
ADJ_N, ADJ_S = 5, [2, 63, 64, 65, 129]                    # the suffix scan's chunk edges (a plain step has at least 2 samples; S = 1: the instanced cases)
FLAGS = [(False, False), (True, False), (False, True), (True, True)]               # (map_exr, background)
CAP_RAYS, CAP_S = 8, 130


def adjoint_cases():
    """(id, kind, S, regime, map_exr, background, raw_noise_std): every S on the chain and layer by layer with the options in turn and the
    density regulariser on at S = 65; the saturated family on the chain; one case with parameter branches."""
    rows = []
    for kind in ("chain", "flex"):
        for k, S in enumerate(ADJ_S):
            exr, bk = FLAGS[(k + (kind == "flex")) % 4]
            rows.append((f"{kind}_S{S}", kind, S, "mixed", exr, bk, 0.1 if S == 65 else 0.0))
    rows.append(("chain_S65_saturated", "chain", 65, "saturated", True, True, 0.0))
    rows.append(("branch_S65", "branch", 65, "mixed", True, True, 0.1))
    return rows


ADJ_CASES = adjoint_cases()
ADJ_IDS = [c[0] for c in ADJ_CASES]
# case id -> the batch's seed where it is not 40 + S: the first of 40 + S, 140 + S, ... on which the case sits MARGIN times inside the guards on
# the CPU (tests/test_weight_losses.py)
ADJ_SEEDS = {}


def kind_model(kind, regime="mixed"):
    """(model, spec, blob) of a trainer kind with the regime's head biases."""
    from tests.common import make_model
    _, npar, arch, _ = KINDS[kind]
    model, spec, _ = make_model(npar, dense_media=True, arch=arch)
    blob = np.asarray(model.get_blob(), F).reshape(-1).copy()
    sl = dict(layer_slices(spec))
    blob[sl["alpha.bias"]] += F(REGIMES[regime][0]); blob[sl["color.bias"]] += F(REGIMES[regime][1])
    return model, spec, blob


def adjoint_batch(case):
    """(ro, rd, t, cone, params) of an adjoint case -- the family's rays, all hit, per-ray parameters -- and its three cotangents (gC [n, 3], gA
    [n], g [n, S]), seeded, of both signs, of the size a mean over the rays gives them."""
    from nerf_tex_amd import synthetic
    cid, kind, S = case[:3]
    seed = ADJ_SEEDS.get(cid, 40 + S)
    f = synthetic.FAMILIES[KINDS[kind][3]]
    P = sum(KINDS[kind][1])
    rng = np.random.default_rng(1000 + seed)
    ro, rd, t, cone = synthetic.all_hit_rays(ADJ_N, f["b_0"], f["b_1"], f["cam"], seed=seed + 1)
    params = (np.resize(np.asarray(f["params"], F), P)[None, :] * rng.uniform(0.8, 1.2, size=(ADJ_N, P))).astype(F)
    return (ro, rd, t, cone, params), cotangents(ADJ_N, S, 100 + seed)


def cotangents(n, S, seed):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) / (3 * n)).astype(F), (rng.normal(size=n) / n).astype(F), (rng.normal(size=(n, S)) / n).astype(F)


def cpu_raw_outputs(spec, blob, batch, z, dtype=torch.float32):
    """(raw colour [n, S, 3], raw density [n, S]) of the oracle's network in `dtype` on a batch: the CPU's stand-in for what a trainer keeps."""
    from oracle import nerftex_oracle as orc
    ro, rd, t, cone, params = batch[:5]
    t_ = lambda x: torch.tensor(np.asarray(x), dtype=dtype)
    w = [t_(a) for a in orc.split_blob(spec, blob)]
    with capture() as seen, torch.no_grad():
        (tbo.render if pgc.has_branches(spec) else tro.render)(w, spec, t_(ro), t_(rd), t_(z), t_(params), t_(cone))
    return seen.raw.numpy().astype(F), seen.sigma.numpy().astype(F)


# ---- a whole step under a loss that takes the weights --------------------------------------------------------------------------------------
def depth_loss(color_true, depth_true, lam=0.5):
    """mse(color) + lam * mean((`expected_depth` - target)^2), written for torch tensors of any dtype and device: the callable the GPU tests hand
    to the product (it names `weights` and `z_vals`) and, as `head`, to the restatement."""
    targets = (color_true, depth_true)

    def loss(color_true=None, alpha_true=None, color_pred=None, alpha_pred=None, weights=None, z_vals=None):
        t_ = lambda x: torch.as_tensor(x, dtype=color_pred.dtype, device=color_pred.device)
        depth = expected_depth(weights, t_(z_vals))                                     # nerf_tex_amd.loss: sum_s w_s z_s
        return torch.mean((color_pred - t_(targets[0])) ** 2) + lam * torch.mean((depth - t_(targets[1])) ** 2)
    return loss


def restated_step(w_np, spec, batch, z, rpr, head, *, blur_idx=None, map_exr=False, bkgd=False, noise=None, dtype=torch.float64, masks=None, branch_masks=None,
                  sigma_mask=None):
    """One plain step, every ray hit, under `head(c, a, w) -> scalar` with the weights of the network, the parameter rows and rays_o / rays_d as
    leaves (the depths are constants): `tro.render` / `tbo.render` on the composite above.  Returns loss, pred [n, 4], weights [n, S], grad
    (flat, get_weights() order), param_grad [rows, P], d_rays_o, d_rays_d."""
    ro, rd, t, cone, rows = batch[:5]
    z = np.asarray(z)
    n, S = z.shape
    assert np.isfinite(z).all()
    t_ = lambda x: None if x is None else torch.tensor(np.asarray(x), dtype=dtype)
    per_sample = lambda ms: None if ms is None else [t_(np.asarray(m).reshape(n * S, -1)) for m in ms]
    w = [torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in w_np]
    leaf = torch.tensor(np.asarray(rows, np.float64).reshape(-(-n // int(rpr)), -1), dtype=dtype, requires_grad=True)
    lo, ld = (torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True) for x in (ro, rd))
    args = (w, spec, lo, ld, t_(z), leaf.repeat_interleave(int(rpr), 0)[:n], t_(pgc._cone(cone)), blur_idx, map_exr, bkgd, BKGD, per_sample(masks))
    with capture() as seen:
        if pgc.has_branches(spec):
            c, a = tbo.render(*args, per_sample(branch_masks), t_(sigma_mask), t_(noise))
        else:
            c, a = tro.render(*args, t_(sigma_mask), t_(noise))
    val = head(c, a, seen.w)
    val.backward()
    g = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().astype(np.float64)
    return SimpleNamespace(loss=float(val.detach()), pred=np.concatenate([c.detach().numpy(), a.detach().numpy()[:, None]], -1), weights=seen.w.detach().numpy(),
                           grad=np.concatenate([g(x).ravel() for x in w]), param_grad=g(leaf), d_rays_o=g(lo), d_rays_d=g(ld))


# the end-to-end cases at 70 x 33, in `pgc.case_setup`'s form with un-normalised rays_d (`igc.case_setup`): (id, trainer class, case)
E2E_CASES = [
    ("chain", "Trainer", ("carpet_1_6", (1, 6), None, None, "carpet", dict(perturb=True), (11, 3))),
    ("flex", "FlexTrainer", ("w64_d3_skip1", *pgc.SMALL, dict(perturb=True), (11, 3))),
    ("branch", "BranchTrainer", ("branches_pd2_pw64", (1, 6), dict(width=128, depth=4, skips=[1], param_depth=2, param_width=64), None, "carpet", dict(), (11, 3))),
]
E2E_IDS = [c[0] for c in E2E_CASES]


def e2e_setup(case):
    """(model, spec, weights, batch, knobs, step seed, depth target [n], the step's depths z [n, S]) of an end-to-end case: the depth target
    seeded inside the ray's own range of depths."""
    from tests import input_grad_common as igc
    model, spec, wts, batch, kn, seed = igc.case_setup(case[2])
    t = batch[2]
    z = step_depths(t, kn["S"], seed, kn["perturb"])
    u = np.random.default_rng(seed + 5).uniform(0.2, 0.8, size=len(t))
    depth = (t[:, 0] + u * (t[:, 1] - t[:, 0])).astype(F)
    return model, spec, wts, batch, kn, seed, depth, z


def e2e_head(batch, depth, z, lam=0.5):
    """`depth_loss` as the restatement's head(c, a, w)."""
    loss = depth_loss(batch[5], depth, lam)
    return lambda c, a, w: loss(color_pred=c, alpha_pred=a, weights=w, z_vals=z)


def e2e_fair(spec, want, f32, report=print, margin=MARGIN):
    """Every layer, parameter column and ray column of an end-to-end case `margin` times inside the standing guards."""
    from tests import input_grad_common as igc
    rows = [(name, rel_linf(f32.grad[sl], want.grad[sl]), float(np.abs(want.grad[sl]).max())) for name, sl in layer_slices(spec)]
    for r in rows:
        report(f"  {r[0]:<24} floor {r[1]:.2e} max {r[2]:.3e}")
    assert all(r[2] >= 1e-6 * margin for r in rows), "a layer without a gradient worth the name: change the seed"
    assert all(r[1] <= 5e-4 / margin for r in rows), ("a float32 floor less than the margin inside 5e-4: change the seed, not the bar", [r for r in rows if r[1] > 5e-4 / margin])
    pgc.fair(want.param_grad, f32.param_grad, report, margin=margin)
    pgc.fair(igc.columns(want.d_rays_o, want.d_rays_d), igc.columns(f32.d_rays_o, f32.d_rays_d), report, margin=margin)


# ---- the instanced cases: 23 x 70 buffers as tests/fused_instanced_common.py's, live fractions all, some and none -----------------------------
INST_KINDS = {"chain": ("carpet_1_6", "Trainer", (1, 6), None, None, dict()), "flex": itc.CASES[0]}
LIVE = ["some", "all", "none", "S1"]


def instanced_setup(kind, live):
    """(model, spec, weights, bufs, hit, cone, knobs, restatement keywords) of an instanced case.  "some": the instancer's buffers as they
    come (rays with hit == 0 among them); "all": every sample of every ray live, in a medium ten times thinner (as `itc.edge_setup` has it for
    such masks); "none": no live sample, n_live = 0; "S1": one sample a ray."""
    case = INST_KINDS[kind]
    model, spec, wts, bufs, hit, cone, kn, okw = itc.case_setup(case, **(dict(n=23, S=1, seed=42) if live == "S1" else {}))
    n, S = bufs[3].shape
    if live in ("all", "none"):
        bufs, hit = itc.with_live_mask(bufs, hit, np.full((n, S), live == "all"))
    if live == "all":
        okw = dict(okw, density_scale=okw["density_scale"] / 10)
        kn = dict(kn, density_scale=okw["density_scale"])
    return model, spec, wts, bufs, hit, cone, kn, okw


def cpu_instanced_outputs(spec, wts, bufs, hit, cone, okw):
    """(raw colour [M', 3], raw density [M'], the density's sign pattern) of the restatement's float32 network on the live samples."""
    out = itc.restated(wts, spec, bufs, hit, cone, None, dtype=torch.float32, **okw)
    live = out.live
    if len(live) == 0:
        return np.zeros((0, 3), F), np.zeros(0, F), np.zeros(0, bool)
    n, S = bufs[3].shape
    from oracle import torch_cpu as tcpu
    t_ = lambda x: torch.tensor(np.asarray(x, np.float64), dtype=torch.float32)
    at_live = lambda x, k: t_(np.asarray(x).reshape(n * S, *([k] if k else []))[live])
    par = at_live(bufs[9], np.asarray(bufs[9]).shape[-1])
    assert okw["blur_idx"] is None
    with torch.no_grad():
        raw, sg = tcpu.mlp([t_(x) for x in wts], spec, tcpu.fourier_features(at_live(bufs[1], 3), spec.pos_freq), at_live(bufs[0], 3), par, None)
    return raw.numpy().astype(F), sg[:, 0].numpy().astype(F), out.sigma_mask


def instanced_figures(got, raw, sigma, bufs, hit, okw, gC, gA, g, sigma_mask):
    """`adjoint_figures` for the instanced composite: compact rows [M', 4]."""
    run = lambda dtype, gg: instanced_adjoint(raw, sigma, bufs, hit, okw, gC, gA, gg, sigma_mask, dtype)
    want, c, a, w = run(torch.float64, g)
    f32 = run(torch.float32, g)[0]
    none = run(torch.float64, None)[0]
    e = dict(f_drgb=rel_linf(f32[:, :3], want[:, :3]), f_dsigma=rel_linf(f32[:, 3], want[:, 3]), seen=rel_linf(none[:, 3], want[:, 3]),
             max_drgb=float(np.abs(want[:, :3]).max()), max_dsigma=float(np.abs(want[:, 3]).max()), want=want, pred=np.concatenate([c, a[:, None]], -1), w=w)
    if got is not None:
        e.update(drgb=rel_linf(got[:, :3], want[:, :3]), dsigma=rel_linf(got[:, 3], want[:, 3]))
    return e
