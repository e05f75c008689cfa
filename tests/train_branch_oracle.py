"""The training step of oracle/train_oracle.py for a ParamNerf WITH parameter branches (model.py:88-101, `param_depth` > 0), in torch, and the
bars of tests/train_flex_common.check_against_float64 restated for a `BranchTrainer` that has just taken a step.

`oracle/torch_cpu.mlp` walks the weight list trunk first, which is where the layers of a model without branches sit; with branches the geometry
branch comes before the trunk and the appearance branch lies among the trunk layers (orc.layer_table), so `mlp` here picks every layer's
weights by NAME.  The Fourier features, the composite, the distances and the losses are the oracle's own, imported, not restated.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED as the rest of the training oracle: the forward pass is checked against
nerftex_oracle.model_forward (tests/test_train_branches.py), the gradients are what autograd derives from it."""

from types import SimpleNamespace

import numpy as np
import torch

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro
from oracle.torch_cpu import composite, fourier_features
from oracle.train_oracle import fourier_dists
from tests.train_common import BKGD, F, layer_slices, rel_linf
from tests.train_flex_common import n_relu


def n_branch_relu(spec):
    """ReLU layers of the branches: `param_depth` per branch the model has (model.py:88, 96)."""
    return spec.param_layers * ((spec.n_geo > 0) + (spec.n_app > 0))


def _activation(masks, kept):
    """relu, or `x * mask` on GIVEN patterns taken in order; `kept`: a list that takes the sign pattern of every pre-activation it meets."""
    mk = None if masks is None else iter(masks)

    def act(x):
        if kept is not None:
            kept.append((x.detach() > 0).numpy())
        return torch.relu(x) if mk is None else x * next(mk)
    return act


def mlp(w, spec, pos_map, dirs, params, masks=None, branch_masks=None, kept=None, branch_kept=None):
    """ParamNerf (model.py:58-125) behind FourierFeatures(pos), parameter branches included; `w` in get_weights() order (orc.layer_table),
    every layer found by its name.  `masks`: torch_cpu.mlp's (trunk 0..depth-1, colour layers, colour half); `branch_masks`: the same for the
    branch ReLUs, geometry layers 0..param_depth-1, then appearance layers.  `kept` / `branch_kept`: lists that take the ReLU patterns of
    this pass in those orders."""
    names = [n for n, _, _ in orc.layer_table(spec)]
    assert len(w) == 2 * len(names), (len(w), len(names))
    W = {n: (w[2 * j], w[2 * j + 1]) for j, n in enumerate(names)}
    dense = lambda h, name: torch.addmm(W[name][1], h, W[name][0])
    act, bact = _activation(masks, kept), _activation(branch_masks, branch_kept)
    g, a, pd = spec.n_geo, spec.n_app, spec.param_layers

    def branch(p, name):                                                              # model.py:89-92 / 97-100
        h = fourier_features(p, spec.param_freq)
        for i in range(pd):
            h = bact(dense(h, f"{name}{i}"))
        return h

    dir_map = fourier_features(dirs, spec.dir_freq)                                   # :78
    if g > 0:
        pos_map = torch.cat([pos_map, branch(params[:, :g], "param_geo")], -1)        # :93
    if a > 0:
        dir_map = torch.cat([dir_map, branch(params[:, g:g + a], "param_app")], -1)   # :101
    h = pos_map
    for i in range(spec.depth):                                                       # :104-108
        h = act(dense(h, f"trunk{i}"))
        if i in spec.skips:
            h = torch.cat([pos_map, h], -1)
    alpha = dense(h, "alpha")                                                         # :111
    h = torch.cat([dir_map, dense(h, "feature")], -1)                                 # :114-115
    if spec.kind == "ParamNerf":
        for i in range(spec.color_depth):                                             # :118-119
            h = act(dense(h, f"color_hidden{i}"))
    h = act(dense(h, "color_half"))                                                   # :122
    return dense(h, "color"), alpha                                                   # :123


def model_forward(w, spec, pos, dirs, params, masks=None, branch_masks=None, kept=None, branch_kept=None):
    """The network on sample positions: FourierFeatures(pos) (model.py:77) into `mlp`."""
    return mlp(w, spec, fourier_features(pos, spec.pos_freq), dirs, params, masks, branch_masks, kept, branch_kept)


def _samples(spec, rays_o, rays_d, z, parameters, cone_scale, blur_idx):
    """renderer.py:98, 114, 151-158: the network's inputs (pos, dirs, params) of every sample, rows [ray][sample]."""
    n, S = z.shape
    rays_d_n = rays_d / torch.linalg.norm(rays_d, dim=-1, keepdim=True)
    pts = rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]
    params = parameters.repeat_interleave(S, 0)
    if blur_idx is not None:                                                          # :155-158
        scale = (cone_scale.reshape(n, 1, 1) * z[:, :, None]).reshape(-1, 1)
        params = torch.cat([params[:, :blur_idx], params[:, blur_idx, None] * scale, params[:, blur_idx + 1:]], -1)
    return pts.reshape(-1, 3), rays_d_n.repeat_interleave(S, 0), params


def render(w, spec, rays_o, rays_d, z, parameters, cone_scale, blur_idx=None, map_exr=False, composite_bkgd=False, bkgd=(1., 1., 1.), masks=None,
           branch_masks=None, sigma_mask=None, noise=None):
    """tro.render's Renderer half (renderer.py:114-213 on GIVEN depths z [n, S]) with this file's `mlp`."""
    if spec.pos_encoding != "fourier":
        raise ValueError("parameter branches train under the Renderer (FourierFeatures) only")
    n, S = z.shape
    color, alpha = model_forward(w, spec, *_samples(spec, rays_o, rays_d, z, parameters, cone_scale, blur_idx), masks, branch_masks)
    return composite(color.reshape(n, S, 3), alpha.reshape(n, S), fourier_dists(z, rays_d), map_exr, composite_bkgd, bkgd, sigma_mask, noise)


def step_gradients(w_np, spec, rays_o, rays_d, z, parameters, cone_scale, color_true, alpha_true, loss, blur_idx=None, map_exr=False, composite_bkgd=False,
                   bkgd=(1., 1., 1.), dtype=torch.float64, masks=None, branch_masks=None, sigma_mask=None, noise=None):
    """tro.step_gradients (one autograd pass, no chunks) with the branches: (loss, color_pred, alpha_pred, gradients in get_weights() order).
    Rays whose depths are not finite are filtered out, the rest rendered, the results scattered back into zeros -- plus the background for
    the filtered ones when compositing -- and the loss runs over ALL rays (renderer.py:58-86).  `masks` [M, width] / `branch_masks`
    [M, param_width] per ReLU layer, `sigma_mask` [n, S], `noise` [n, S] as tro.step_gradients takes them."""
    z = np.asarray(z)
    n, S = z.shape
    hit = np.isfinite(z).all(1)
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    sub = lambda x: None if x is None else t_(np.asarray(x)[hit])
    per_sample = lambda ms: None if ms is None else [sub(m.reshape(n, S, -1)).flatten(0, 1) for m in map(np.asarray, ms)]
    w = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in w_np]
    c = torch.zeros((n, 3), dtype=dtype); a = torch.zeros((n,), dtype=dtype)
    if hit.any():
        ch, ah = render(w, spec, sub(rays_o), sub(rays_d), sub(z), sub(parameters), sub(cone_scale), blur_idx, map_exr, composite_bkgd, bkgd, per_sample(masks),
                        per_sample(branch_masks), sub(sigma_mask), sub(noise))
        idx = torch.as_tensor(np.nonzero(hit)[0])
        c = c.index_put((idx,), ch); a = a.index_put((idx,), ah)
    if composite_bkgd:
        c = c + torch.as_tensor((~hit)[:, None] * np.asarray(bkgd, np.float64)[None, :], dtype=dtype)
    val = tro._loss(loss, t_(color_true), t_(alpha_true), c, a)
    if val.requires_grad:
        val.backward()
    return float(val.detach()), c.detach().numpy(), a.detach().numpy(), [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in w]


def own_masks(w_np, spec, rays_o, rays_d, z, parameters, cone_scale, blur_idx=None, noise=None, dtype=torch.float32):
    """The ReLU patterns of a forward pass of this oracle itself in `dtype`, every ray a hit: (masks, branch_masks, sigma_mask) as bool
    arrays -- what a float32 step would hand to float64."""
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    kept, branch_kept = [], []
    with torch.no_grad():
        z_t = t_(z)
        _, alpha = model_forward([t_(x) for x in w_np], spec, *_samples(spec, t_(rays_o), t_(rays_d), z_t, t_(parameters), t_(cone_scale), blur_idx),
                                 kept=kept, branch_kept=branch_kept)
        alpha = alpha.reshape(z_t.shape)
        sigma_mask = (alpha if noise is None else alpha + t_(noise)).numpy() > 0
    return kept, branch_kept, sigma_mask


def restated_branch_step(tr, spec, wts, ro, rd, t, params, cone, color, alpha, okw, *, seed, perturb, S=None, z=None, noise_std=0.0, miss=None, blur_idx=None,
                         bkgd=False, bkgd_color=BKGD, map_exr=False, dtype=torch.float64, masks=None, branch_masks=None, sigma_mask=None):
    """tests.train_flex_common.restated_flex_step beside a `BranchTrainer`: the step `tr.gradients_step(..., seed=seed)` has just taken through
    `step_gradients`, float64 autograd branched by the signs of the activations the trainer kept -- slots 0 .. n_relu - 1, 32 + j (geometry
    branch), 48 + j (appearance branch), and 64 = the raw density with the noise added."""
    n = len(t)
    S = S or tr.n_samples
    miss = np.zeros(n, bool) if miss is None else np.asarray(miss, bool)
    if z is None:
        tf = np.where(np.isfinite(t), t, 0).astype(F)
        z = orc.z_values_perturbed(tf, S, seed, F) if perturb else orc.z_values(tf, S, F)
        z = z.copy(); z[miss] = np.inf
    noise = noise_std * orc.noise_normals(n, S, seed, dtype=F).astype(np.float64) if noise_std > 0 else None
    torch.cuda.synchronize()
    if masks is None:
        masks = [tr.activation(k, n * S) > 0 for k in range(n_relu(spec))]
        assert [m.shape[1] for m in masks] == tr.relu_widths()
        slots = ([32 + j for j in range(spec.param_layers)] if spec.n_geo > 0 else []) + ([48 + j for j in range(spec.param_layers)] if spec.n_app > 0 else [])
        branch_masks = [tr.activation(k, n * S) > 0 for k in slots]
        assert [m.shape[1] for m in branch_masks] == tr.branch_widths() and len(branch_masks) == n_branch_relu(spec)
        sigma_mask = (tr.activation(64, n * S).reshape(n, S) + (0 if noise is None else noise.astype(F))) > 0
    val, c, a, g = step_gradients(wts, spec, ro, rd, z, params, np.nan_to_num(cone), color, alpha, okw, blur_idx=blur_idx, map_exr=map_exr, composite_bkgd=bkgd,
                                  bkgd=bkgd_color, dtype=dtype, masks=masks, branch_masks=branch_masks, sigma_mask=sigma_mask, noise=noise)
    got, flat = tr.gradients(), np.concatenate([np.asarray(x, np.float64).ravel() for x in g])
    assert flat.size == got.size == tr.n_weights
    return SimpleNamespace(loss=val, pred=np.concatenate([c, a[:, None]], -1), grad=flat, got=got, z=z, noise=noise, masks=masks, branch_masks=branch_masks,
                           sigma_mask=sigma_mask, layers={name: rel_linf(got[sl], flat[sl]) for name, sl in layer_slices(spec)})


def floors(spec, want_grad, f32_grad):
    """(name, float32-vs-float64 floor, max |grad|) per kernel and bias."""
    return [(name, rel_linf(f32_grad[sl], want_grad[sl]), float(np.abs(want_grad[sl]).max())) for name, sl in layer_slices(spec)]


def check_against_float64(tr, spec, val, pred, step_args, kw, report=print):
    """The bars of tests/train_flex_common.check_against_float64 on a step a `BranchTrainer` has just taken, restated, not re-chosen: the loss
    within 1e-5 relative of float64 autograd branched like the float32 pass; the predictions and every layer's gradient -- branch layers
    included -- within max(1e-4, 4 x floor) rel-Linf, the floor being what float32 torch autograd of the same restatement with the same
    branches is off by from float64; every floor <= 5e-4, max |grad| > 1e-6, no layer's gradient all zero.  Every figure is printed before
    it is gated."""
    want = restated_branch_step(tr, spec, *step_args, **kw)
    f32 = restated_branch_step(tr, spec, *step_args, dtype=torch.float32, masks=want.masks, branch_masks=want.branch_masks, sigma_mask=want.sigma_mask, **kw)
    e_loss = abs(val - want.loss) / abs(want.loss)
    e_pred, floor_pred = rel_linf(pred, want.pred), rel_linf(f32.pred, want.pred)
    report(f"loss {val:.9g} want {want.loss:.9g} rel {e_loss:.2e} | pred {e_pred:.2e} floor {floor_pred:.2e} | max|grad| {np.abs(want.grad).max():.3e}")
    rows = []
    for name, floor, biggest in floors(spec, want.grad, f32.grad):
        rows.append((name, want.layers[name], floor, biggest))
        report(f"  {name:<24} err {want.layers[name]:.2e} floor {floor:.2e} max {biggest:.3e}")
    assert np.isfinite(want.got).all()
    assert np.abs(want.grad).max() > 1e-6 and all(r[3] > 0 for r in rows), "the batch gives no gradient worth the name: change the seed"
    assert all(r[2] <= 5e-4 for r in rows), ("a float32 floor above 5e-4: change the seed, not the bar", [r for r in rows if r[2] > 5e-4])
    assert e_loss <= 1e-5, e_loss
    assert e_pred <= max(1e-4, 4 * floor_pred), (e_pred, floor_pred)
    bad = [r for r in rows if r[1] > max(1e-4, 4 * r[2])]
    assert not bad, bad
    return want


# ---- the cases tests/test_gpu_train_branches.py trains and tests/test_train_branches.py shows to be fair: (id, n_parameters, arch, the family
# whose rays and parameters the batch takes, the step's knobs).  45 rays x 37 samples = 1665 samples: off the contraction's 128-row tile and off 32.
N_RAYS, N_SAMPLES = 45, 37
GPU_CASES = [
    ("a_reference_pd1", (1, 6), dict(depth=8, width=256, skips=[4], color_depth=1, param_depth=1), "carpet", dict(loss_name="alpha_smape", perturb=True)),
    ("b_blur_cd0_pd3", (2, 3), dict(depth=4, width=128, skips=[1, 2], color_depth=0, param_depth=3, param_width=64), "grass_filtered",
     dict(loss_name="alpha_smape", blur=0, noise_std=0.1, perturb=True)),                       # the branch input varies per sample; the appearance branch feeds the colour half layer
    ("c_three_readers_pd4", (4, 8), dict(depth=6, width=200, skips=[0, 4], color_depth=2, param_depth=4, param_width=100), "carpet",
     dict(loss_name="alpha_mse_soft", bkgd=True)),                                              # trunk 0, 1 and 5 read the geometry branch
    ("d_appearance_only", (0, 5), dict(depth=5, width=256, skips=[2], color_depth=1, param_depth=2), "carpet", dict(loss_name="nerf_mse")),
    ("e_geometry_only", (3, 0), dict(depth=5, width=256, skips=[2], color_depth=1, param_depth=2), "carpet", dict(loss_name="alpha_smape", map_exr=True)),
    ("f_branch_wider_than_trunk", (1, 4), dict(depth=3, width=64, skips=[1], color_depth=1, param_depth=2, param_width=128), "grass", dict(loss_name="alpha_smape")),
    ("g_depth1_pw2", (1, 6), dict(depth=1, width=96, skips=[], color_depth=3, param_depth=1, param_width=2), "carpet", dict(loss_name="alpha_smape", perturb=True)),
    ("h_pw37", (1, 6), dict(depth=4, width=128, skips=[], color_depth=1, param_depth=2, param_width=37), "carpet", dict(loss_name="alpha_smape", perturb=True)),
]
# id -> (step seed, batch seed) where the defaults (11, 3) leave a float32 floor above the cap (tests/test_train_branches.py: case b's density bias
# sits at 5.5e-4 of float64 under them with the oracle's own float32 masks, at 1.0e-4 under these)
CASE_SEEDS = {"b_blur_cd0_pd3": (13, 5)}


def branch_batch(seed, n, spec, fam):
    """tests.test_gpu_train.batch for a model with any parameter counts: the family's rays (all hit), its parameter row repeated to the
    model's P columns and scaled per ray, seeded targets."""
    from nerf_tex_amd import synthetic
    rng = np.random.default_rng(seed)
    f = synthetic.FAMILIES[fam]
    P = spec.n_params
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"])
    params = np.resize(np.asarray(f["params"], F), P)[None, :] * rng.uniform(0.8, 1.2, size=(n, P)).astype(F)
    color = rng.uniform(0, 1, size=(n, 3)).astype(F)
    alpha = (rng.uniform(0, 1, size=n) > 0.3).astype(F) * rng.uniform(0.5, 1, size=n).astype(F)
    return ro, rd, t, cone, np.ascontiguousarray(params, F), color, alpha


def case_setup(case, n=N_RAYS, S=N_SAMPLES):
    """(model, spec, weights, batch, knobs with every default filled in, (step seed, batch seed)) of a GPU case."""
    from tests.common import make_model
    cid, npar, arch, fam, knobs = case
    model, spec, wts = make_model(npar, dense_media=True, arch=arch)
    seed, batch_seed = CASE_SEEDS.get(cid, (11, 3))
    kn = dict(dict(bkgd=False, map_exr=False, perturb=False, blur=None, noise_std=0.0), **knobs)
    return model, spec, wts, branch_batch(batch_seed, n, spec, fam), kn, seed
