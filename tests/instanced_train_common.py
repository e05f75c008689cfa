"""What the tests of the differentiable InstanceRenderer tail share (tests/test_train_instanced.py on the CPU, tests/test_gpu_train_instanced.py
on the GPU): the cases, their synthetic instancer buffers, and a float64 torch restatement of `ntx_train_forward_instanced` +
`ntx_train_backward` -- InstanceRenderer.evaluate_model + map_model_output (renderer.py:247-354) with the network on the live samples alone
and the weights AND params_map as leaves.

TEST INFRASTRUCTURE ONLY, PARITY UNPINNED as the rest of the training oracle: the network is `oracle.torch_cpu.mlp` (tests/train_branch_oracle's
for a model with parameter branches) with its `masks`, the composite the few lines below; its forward is held to
`oracle.nerftex_oracle.instance_evaluate_model` in float64 (tests/test_train_instanced.py), the gradients are what autograd derives from it."""

from types import SimpleNamespace

import numpy as np
import torch

from oracle import torch_cpu as tcpu
from tests import param_grad_common as pgc
from tests import train_branch_oracle as tbo
from tests.train_common import BKGD, F

PATCH_SCALE, STEP = 0.09, 0.002

# (id, trainer class name, n_parameters, arch, blur_idx, knobs).  Widths <= 128, N x S <= about 3000.  density_scale is chosen so that the float32
# floor of every layer's gradient stays <= 5e-4 (tests/test_train_instanced.py checks that on the CPU with the restatement's own masks): the
# instanced path multiplies the raw density by alpha_weight x density_scale before the exponential, which amplifies the density's rounding.
CASES = [
    ("w64_d3_skip1", "FlexTrainer", (1, 6), dict(width=64, depth=3, skips=[1]), None, dict()),
    ("w128_d4_blur_geo", "FlexTrainer", (2, 3), dict(width=128, depth=4, skips=[]), 0, dict()),
    ("cd0_blur_app_exr_bkgd", "FlexTrainer", (1, 4), dict(width=64, depth=3, skips=[1], color_depth=0), 2, dict(map_exr=True, composite_bkgd=True)),
    ("no_reweighting", "FlexTrainer", (1, 6), dict(width=64, depth=2, skips=[]), None, dict(density_reweighting=False)),
    ("branches_pd2", "BranchTrainer", (1, 4), dict(depth=3, width=64, skips=[1], color_depth=1, param_depth=2, param_width=128), None, dict()),
]
DEFAULTS = dict(n=23, S=70, density_scale=20.0, density_reweighting=True, map_exr=False, composite_bkgd=False, seed=5, weight_seed=0, run_len=None)
CASE_IDS = [c[0] for c in CASES]


def knobs_of(case):
    return dict(DEFAULTS, **case[5])


def instancer_buffers(npar, seed, n, S, run_len=None, p_in=0.35):
    """`tests.test_gpu_instance.FakeInstancer`'s ten buffers for n rays x S samples (the rays and parameters it is asked with are seeded too),
    the hit mask [n] bool and a cone_scale [n]."""
    from tests.test_gpu_instance import FakeInstancer
    P = sum(npar)
    rng = np.random.default_rng(seed + 1000)
    inst = FakeInstancer(P, seed=seed, run_len=run_len, n_geo=npar[0], p_in=p_in)
    ro, rd = rng.normal(size=(n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    params = np.repeat(rng.uniform(0.2, 1, size=(1, P)), n, 0).astype(F)
    bufs = inst.get_model_input(ro, rd, params, S, STEP)
    cone = rng.uniform(1e-3, 5e-3, size=n).astype(F)
    return bufs, np.asarray(inst.last[-1], bool), cone


def live_mask(hit, dists):
    return np.asarray(hit, bool)[:, None] & (np.asarray(dists) > 0)


def live_order(hit, dists):
    """The compact rows on the host: the flat indices ray * S + s of the live samples, ascending."""
    return np.nonzero(live_mask(hit, dists).reshape(-1))[0]


def with_live_mask(bufs, hit, mask):
    """The buffers with an EXPLICIT live mask [n, S]: dists > 0 exactly there (what it held where it was positive, else one step), 0 elsewhere,
    and every ray hit."""
    bufs = list(bufs)
    d = np.where(bufs[3] > 0, bufs[3], F(STEP)).astype(F)
    bufs[3] = np.where(mask, d, F(0)).astype(F)
    return tuple(bufs), np.ones(mask.shape[0], bool)


def quadratic_head(n, seed=2):
    """A fixed quadratic of the predictions in torch, any dtype, any device: mean((c - tc)^2 wc) + 0.5 mean((a - ta)^2)."""
    rng = np.random.default_rng(seed)
    tc, wc, ta = rng.uniform(0, 1, (n, 3)), rng.uniform(0.5, 1.5, (n, 3)), rng.uniform(0, 1, n)

    def head(c, a):
        t_ = lambda x: torch.as_tensor(x, dtype=c.dtype, device=c.device)
        return torch.mean((c - t_(tc)) ** 2 * t_(wc)) + 0.5 * torch.mean((a - t_(ta)) ** 2)
    return head


def restated(w_np, spec, bufs, hit, cone, head=None, *, blur_idx=None, patch_scale=PATCH_SCALE, density_scale=1.0, density_reweighting=True, map_exr=False,
             composite_bkgd=False, bkgd=BKGD, dtype=torch.float64, masks=None, branch_masks=None, sigma_mask=None):
    """One instanced step.  The network (positions pts, directions rays_d_map as given, parameters params_map with column blur_idx times
    cone_scale t / patch_scale) on the live samples in ascending (ray, sample) order; sigma' = sigma alpha_weight density_scale; a = 1 -
    exp(-relu(sigma') dists / patch_scale), 0 at a sample that is not live; the appended sample (color_last, alpha_last); the composite of
    map_model_output; rays with hit == 0 predict 0.  Nothing is read at a sample that is not live.  `masks` / `branch_masks` [M', width] and
    `sigma_mask` [M']: GIVEN ReLU patterns in compact row order (None: the pass's own, which are returned).  `head(color_pred, alpha_pred)`:
    the loss; None: forward only.  Returns pred [n, 4], loss, grad (flat, get_weights() order), param_grad [n, S, P], d_color, d_alpha, live,
    masks, branch_masks, sigma_mask, sigma (the raw density [M'])."""
    rays_d_map, pts, tt, dists, color_last, alpha_last, alpha_weight, _, _, params_map = [np.asarray(b) for b in bufs]
    n, S = dists.shape
    P = params_map.shape[-1]
    hit = np.asarray(hit, bool)
    live = live_order(hit, dists)
    li = torch.as_tensor(live)
    t_ = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    at_live = lambda a, w: t_(np.asarray(a).reshape(n * S, *([w] if w else []))[live])
    w = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in w_np]
    leaf = torch.tensor(np.nan_to_num(np.asarray(params_map, np.float64)), dtype=dtype, requires_grad=True)      # (what is not live never reaches the graph)
    par = leaf.reshape(n * S, P)[li]
    if blur_idx is not None:                                                                                     # renderer.py:259-263
        scale = (t_(np.repeat(np.asarray(cone).reshape(n, 1), S, 1).reshape(-1)[live]) * at_live(tt, 0) / patch_scale)[:, None]
        par = torch.cat([par[:, :blur_idx], par[:, blur_idx, None] * scale, par[:, blur_idx + 1:]], -1)
    kept, bkept = [], []
    m_ = lambda ms: None if ms is None else [t_(np.asarray(m)) for m in ms]
    pos_map = tcpu.fourier_features(at_live(pts, 3), spec.pos_freq)
    if len(live) == 0:
        raw, sg = torch.zeros((0, 3), dtype=dtype), torch.zeros((0, 1), dtype=dtype)
    elif pgc.has_branches(spec):
        raw, sg = tbo.mlp(w, spec, pos_map, at_live(rays_d_map, 3), par, m_(masks), m_(branch_masks), kept, bkept)
    else:
        if masks is None:                                                                                        # the pass's own patterns, for the caller
            tbo.mlp([x.detach() for x in w], spec, pos_map, at_live(rays_d_map, 3), par.detach(), None, None, kept, bkept)
        raw, sg = tcpu.mlp(w, spec, pos_map, at_live(rays_d_map, 3), par, m_(masks))
    sg = sg[:, 0]
    sp = sg * (at_live(alpha_weight, 0) if density_reweighting else 1.0) * density_scale                         # :300
    own_sigma = (sp.detach() > 0).numpy()
    gate = torch.relu(sp) if sigma_mask is None else sp * t_(np.asarray(sigma_mask))
    a_live = 1.0 - torch.exp(-gate * at_live(dists, 0) / patch_scale)                                            # :339
    rgb_live = torch.nn.functional.elu(raw) + 1 if map_exr else torch.sigmoid(raw)                               # :325-330
    am = torch.zeros(n * S, dtype=dtype).index_put((li,), a_live).reshape(n, S)
    rgb = torch.zeros((n * S, 3), dtype=dtype).index_put((li,), rgb_live).reshape(n, S, 3)
    am = torch.cat([am, t_(alpha_last).reshape(n, 1)], 1)                                                        # :331, :339
    rgb = torch.cat([rgb, t_(color_last).reshape(n, 1, 3)], 1)
    trans = torch.cumprod(1.0 - am + 1e-10, -1)
    wts = am * torch.cat([torch.ones_like(trans[:, :1]), trans[:, :-1]], -1)                                     # :342
    c = torch.sum(wts[..., None] * rgb, -2); a = torch.sum(wts, -1)
    if composite_bkgd:                                                                                           # :351-352
        c = c + (1.0 - a[..., None]) * torch.as_tensor(bkgd, dtype=dtype)
    h_ = torch.as_tensor(hit)
    c = torch.where(h_[:, None], c, torch.zeros_like(c)); a = torch.where(h_, a, torch.zeros_like(a))             # :313-314
    out = SimpleNamespace(pred=np.concatenate([c.detach().numpy(), a.detach().numpy()[:, None]], -1), live=live, sigma=sg.detach().numpy(),
                          masks=masks if masks is not None else kept, branch_masks=branch_masks if branch_masks is not None else (bkept or None),
                          sigma_mask=sigma_mask if sigma_mask is not None else own_sigma)
    if head is None:
        return out
    val = head(c, a)
    if c.requires_grad:                                                                                          # (without a live sample nothing depends on a leaf)
        c.retain_grad(); a.retain_grad()
        val.backward()
    zero = lambda x: np.zeros(tuple(x.shape)) if x.grad is None else x.grad.numpy().astype(np.float64)
    out.loss, out.grad = float(val.detach()), np.concatenate([zero(x).ravel() for x in w])
    out.param_grad, out.d_color, out.d_alpha = zero(leaf), zero(c), zero(a)
    return out


# The edges, each on the first case's model: sample counts around the composite's chunk of 64, and live counts M' around a wave's 32 rows and
# the weight gradients' range of 2048 rows (30 x 70 = 2100 samples, an explicit live mask over every ray).  (id, kind, value)
EDGES = [(f"S{S}", "S", S) for S in (1, 64, 65, 130)] + [(f"live{K}", "live", K) for K in (0, 1, 31, 32, 33, 2047, 2048, 2049)]
EDGE_IDS = [e[0] for e in EDGES]
LIVE_N, LIVE_S = 30, 70
LIVE_MASK_SEEDS = {1: 601}                 # the mask's seed, where it is not the count: the ONE live sample has to lie inside the medium (most positions have density 0 and no gradient)


def edge_setup(edge):
    """`case_setup` of the first case at an edge: (model, spec, weights, bufs, hit, cone, knobs, restatement keywords)."""
    _, kind, value = edge
    if kind == "S":
        return case_setup(CASES[0], n=23, S=value, seed=40 + value)
    model, spec, wts, bufs, hit, cone, kn, okw = case_setup(CASES[0], n=LIVE_N, S=LIVE_S, seed=11)
    mask = np.zeros(LIVE_N * LIVE_S, bool)
    mask[np.random.default_rng(LIVE_MASK_SEEDS.get(value, value)).choice(mask.size, value, replace=False)] = True
    bufs, hit = with_live_mask(bufs, hit, mask.reshape(LIVE_N, LIVE_S))
    if value > 2000:                       # nearly every sample of every ray in a patch: a thinner medium, or the rays saturate within a few samples
        okw = dict(okw, density_scale=okw["density_scale"] / 10)
        kn = dict(kn, density_scale=okw["density_scale"])
    return model, spec, wts, bufs, hit, cone, kn, okw


def case_setup(case, n=None, S=None, seed=None):
    """(model, spec, weights, bufs, hit, cone, knobs, the restatement's keyword arguments) of a case."""
    from tests.common import make_model
    cid, cls, npar, arch, blur, _ = case
    kn = knobs_of(case)
    n, S = n or kn["n"], S or kn["S"]
    model, spec, wts = make_model(npar, seed=kn["weight_seed"], dense_media=True, arch=arch)
    bufs, hit, cone = instancer_buffers(npar, kn["seed"] if seed is None else seed, n, S, kn["run_len"])
    okw = dict(blur_idx=blur, density_scale=kn["density_scale"], density_reweighting=kn["density_reweighting"], map_exr=kn["map_exr"], composite_bkgd=kn["composite_bkgd"])
    return model, spec, wts, bufs, hit, cone, kn, okw
