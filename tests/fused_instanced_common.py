"""What the tests of the instanced step on the FUSED chain share (tests/test_fused_instanced.py on the CPU, tests/test_gpu_fused_instanced.py on the
GPU; `ntx_trainer_enable_instanced`, `Trainer(instanced=True)`): the cases, the step helpers, and a numpy restatement of the chain's encoder
for compact rows.

No yardstick of its own: the step is tests/instanced_train_common.py's float64 restatement (`itc.restated`), the per-sample input gradients
tests/input_grad_common.restated_sample_gradients', the ReLU patterns the chain's own slots 0-9 and 10 over the compact rows
(`clc.chain_patterns`), the bars `clc.check_layers` (`check_against_float64`'s convention on a flat gradient), `pgc.check_param_gradients` and
`igc.check_input_gradients`.  Every model is 8 x 256 / skips [4] / color_depth 1 with `dense_media=True` (or the width-128 network `_widened`
pads into it).  Seeds are chosen on the CPU: tests/test_fused_instanced.py holds every case 2x inside the guards."""

import numpy as np
import torch

from tests import custom_loss_common as clc
from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests.common import make_model
from tests.train_common import BKGD, F, layer_slices, rel_linf

MARGIN = pgc.MARGIN

# `itc.CASES`' form: (id, trainer class name, n_parameters, arch, blur_idx, knobs); arch None: 8 x 256 / [4] / 1.  23 rays x 70 samples.
CASES = [
    ("carpet_1_6", "Trainer", (1, 6), None, None, dict()),
    ("grass_filtered_blur_geo", "Trainer", (2, 3), None, 0, dict()),
    ("grass_filtered_blur_app", "Trainer", (2, 3), None, 3, dict()),
    ("map_exr", "Trainer", (1, 6), None, None, dict(map_exr=True)),
    ("background", "Trainer", (1, 6), None, None, dict(composite_bkgd=True)),
    ("no_reweighting", "Trainer", (1, 6), None, None, dict(density_reweighting=False)),
]
WIDE_CASE = ("width_128_widened", "Trainer", (1, 6), dict(width=128), None, dict())
CASE = {c[0]: c for c in CASES + [WIDE_CASE]}
CASE_IDS = [c[0] for c in CASES]
MODE_CASES = [CASE["carpet_1_6"], CASE["grass_filtered_blur_app"]]
MODES = [(1, 1), (2, 0), (0, 2)]
# the edges' seeds where they are not `itc.edge_setup`'s, (buffer seed, mask seed): with `itc`'s, the one sample a ray has (S = 1) / the ONE live
# sample lies where the 8 x 256 model's density is 0, and the step has no gradient at all (`itc.LIVE_MASK_SEEDS` says the same of its model)
EDGE_SEEDS = {"S1": (42, None), "live1": (11, 615)}


def edge_setup(edge):
    """`itc.edge_setup` with the chain's model in the place of its 64-wide one: the same buffers, live masks and thinner medium."""
    _, kind, value = edge
    model, spec, wts = make_model((1, 6), seed=0, dense_media=True)
    if edge[0] in EDGE_SEEDS:
        bseed, mseed = EDGE_SEEDS[edge[0]]
        if kind == "S":
            return (model, spec, wts) + itc.case_setup(itc.CASES[0], n=23, S=value, seed=bseed)[3:]
        _, _, _, bufs, hit, cone, kn, okw = itc.case_setup(itc.CASES[0], n=itc.LIVE_N, S=itc.LIVE_S, seed=bseed)
        mask = np.zeros(itc.LIVE_N * itc.LIVE_S, bool)
        mask[np.random.default_rng(mseed).choice(mask.size, value, replace=False)] = True
        bufs, hit = itc.with_live_mask(bufs, hit, mask.reshape(itc.LIVE_N, itc.LIVE_S))
        if value > 2000:
            okw = dict(okw, density_scale=okw["density_scale"] / 10)
            kn = dict(kn, density_scale=okw["density_scale"])
        return model, spec, wts, bufs, hit, cone, kn, okw
    return (model, spec, wts) + itc.edge_setup(edge)[3:]


# ---- the CPU side: a case's fairness --------------------------------------------------------------------------------------------------------
def restate_all(spec, w, bufs, hit, cone, okw, head, pat, dtype):
    """(`itc.restated`'s result, (dL/d pts, dL/d rays_d_map)) of a step on given patterns."""
    out = itc.restated(w, spec, bufs, hit, cone, head, dtype=dtype, **okw, **pat)
    smp = igc.restated_sample_gradients(w, spec, bufs, hit, cone, head, dtype=dtype, **okw, **pat)
    return out, (smp[2], smp[3])


def fair_all(spec, want, f32, want_in, f32_in, hit, bufs, report=print, margin=MARGIN, samples=True):
    """Every layer's float32 floor, and -- `samples` -- the per-sample parameter and input gradients' columns, `margin` times inside the guards
    (floor <= 5e-4, max |grad| > 1e-6), over the live samples."""
    rows = [(name, rel_linf(f32.grad[sl], want.grad[sl]), float(np.abs(want.grad[sl]).max())) for name, sl in layer_slices(spec)]
    for r in rows:
        report(f"  {r[0]:<24} floor {r[1]:.2e} max {r[2]:.3e}")
    assert all(r[2] >= 1e-6 * margin for r in rows), "a layer without a gradient worth the name: change the seed"
    assert all(r[1] <= 5e-4 / margin for r in rows), ("a float32 floor less than the margin inside 5e-4: change the seed, not the bar", [r for r in rows if r[1] > 5e-4 / margin])
    assert rel_linf(f32.pred, want.pred) <= 1e-4 / margin
    if samples:
        live = itc.live_mask(hit, bufs[3]).reshape(-1)
        P = want.param_grad.shape[-1]
        pgc.fair(want.param_grad.reshape(-1, P), f32.param_grad.reshape(-1, P), report, rows=live, margin=margin)
        pgc.fair(igc.columns(*want_in), igc.columns(*f32_in), report, rows=live, margin=margin)


# ---- the encoder's contract, in numpy ----------------------------------------------------------------------------------------------------
def o_index(blk, tiles, row, p):
    """The chain's O layout (ntx_encode.h `o_index`): a block of 32 samples x `tiles` tiles of 32 rows, element (row, sample p of the block)."""
    return ((blk * tiles + (row >> 5)) * 4 + (p >> 3)) * 256 + ((row & 31) + 32 * ((p >> 2) & 1)) * 4 + (p & 3)


def fourier_row_of(D, band, h, c):
    return D + 2 * D * band + h * D + c


def blur_factor(cone, t_map, patch_scale, m, S):
    """What column blur_idx of live sample m is multiplied by: cone_scale[ray] * t[ray, s] / patch_scale (renderer.py:259-263), in float32 and
    in the kernel's order of operations."""
    return F(F(np.asarray(cone, F).reshape(-1)[m // S]) * F(np.asarray(t_map, F).reshape(-1)[m])) / F(patch_scale)


def emulate_encoder(bufs, hit, cone, part, n_geo, n_app, freqs, blur_idx, patch_scale=itc.PATCH_SCALE, fill=np.nan):
    """encode_samples_kernel lane by lane, on float64 sines: one wave per block of 32 compact rows, lane (n, h) writes x itself (h = 0) and
    sin (h = 0) / cos (h = 1) of every band of compact row blk * 32 + n = live sample m = live[row] into the O layout; the tail rows of the last
    block as zeros; nothing else is written (`fill`).  `part` 0: pts | geometry parameters, 1: rays_d_map | appearance parameters.  Returns
    (O [blocks * tiles * 1024], tiles, K)."""
    rays_d_map, pts, tt, dists = [np.asarray(b) for b in bufs[:4]]
    params_map = np.asarray(bufs[9])
    S, P = dists.shape[1], n_geo + n_app
    live = itc.live_order(hit, dists)
    pos_freq, dir_freq, param_freq = freqs
    L3, D, c0 = (pos_freq, n_geo, 0) if part == 0 else (dir_freq, n_app, n_geo)
    K = 3 * (1 + 2 * L3) + D * (1 + 2 * param_freq)
    tiles, blocks = (K + 31) // 32, (len(live) + 31) // 32
    O = np.full(blocks * tiles * 1024, fill, np.float64)
    xyz = (pts if part == 0 else rays_d_map).reshape(-1, 3)
    for blk in range(blocks):
        for lane in range(64):
            n, h = lane & 31, lane >> 5
            row = blk * 32 + n
            valid = row < len(live)
            m = int(live[row]) if valid else 0

            def param(col):
                p = float(params_map.reshape(-1, P)[m, col])
                return p * float(blur_factor(cone, tt, patch_scale, m, S)) if col == blur_idx else p

            def fourier(r0, width, L, x):
                def put(r, v):
                    O[o_index(blk, tiles, r, n)] = v if valid else 0.0
                if h == 0:
                    for c in range(width):
                        put(r0 + c, x(c) if valid else 0.0)
                for f in range(L):
                    for c in range(width):
                        v = x(c) if valid else 0.0
                        put(r0 + fourier_row_of(width, f, h, c), np.cos(2.0 ** f * v) if h else np.sin(2.0 ** f * v))
            fourier(0, 3, L3, lambda c: float(xyz[m, c]))
            if D > 0:
                fourier(3 * (1 + 2 * L3), D, param_freq, lambda c: param(c0 + c))
    return O, tiles, K


def expected_rows(bufs, hit, cone, part, n_geo, n_app, freqs, blur_idx, patch_scale=itc.PATCH_SCALE):
    """The same map row by row as the restatements state it: FourierFeatures(pts | rays_d_map of the live samples) | FourierFeatures(their
    geometry | appearance parameters, column blur_idx scaled), [n_live, K] float64."""
    rays_d_map, pts, tt, dists = [np.asarray(b) for b in bufs[:4]]
    S, P = dists.shape[1], n_geo + n_app
    live = itc.live_order(hit, dists)
    par = np.asarray(bufs[9], np.float64).reshape(-1, P)[live].copy()
    if blur_idx is not None and blur_idx >= 0:
        par[:, blur_idx] *= [float(blur_factor(cone, tt, patch_scale, int(m), S)) for m in live]
    pos_freq, dir_freq, param_freq = freqs
    ff = lambda x, L: np.concatenate([x] + [fn(2.0 ** k * x) for k in range(L) for fn in (np.sin, np.cos)], -1)      # layer.py:18-23, as oracle.torch_cpu.fourier_features
    x = np.asarray(pts if part == 0 else rays_d_map, np.float64).reshape(-1, 3)[live]
    q = par[:, :n_geo] if part == 0 else par[:, n_geo:]
    return np.concatenate([ff(x, pos_freq if part == 0 else dir_freq)] + ([ff(q, param_freq)] if q.shape[1] else []), -1)


# ---- the GPU side ----------------------------------------------------------------------------------------------------------------------------
def dev():
    return torch.device("cuda", 0)


def chain_trainer(case, model, n, S, pm=False, im=False, max_rays=None, instanced=True):
    from nerf_tex_amd.train import Trainer
    kn = itc.knobs_of(case)
    return Trainer(model, max_rays=max_rays or n, n_samples=max(S, 2), perturb=False, blur_idx=case[4], map_exr=kn["map_exr"], param_gradients=pm, input_gradients=im,
                   instanced=instanced)


def flex_trainer(case, model, n, S):
    from nerf_tex_amd.train import FlexTrainer
    kn = itc.knobs_of(case)
    return FlexTrainer(model, max_rays=n, n_samples=max(S, 2), perturb=False, blur_idx=case[4], map_exr=kn["map_exr"])


def fkw(kn):
    return dict(patch_scale=itc.PATCH_SCALE, density_scale=kn["density_scale"], density_reweighting=kn["density_reweighting"], composite_bkgd=kn["composite_bkgd"], bkgd_color=BKGD)


def step(tr, bufs, hit, cone, kn, head, spoil=None):
    """forward_instanced, the head and its cotangents in torch on the device, backward.  `spoil`: (rays, value) -- their cotangents are set to
    the value.  Returns pred [n, 4], the weight gradient, the head's value."""
    c, a = tr.forward_instanced(bufs, cone, hit=np.asarray(hit).astype(np.uint8), **fkw(kn))
    cd, ad = c.detach().requires_grad_(True), a.detach().requires_grad_(True)
    val = head(cd, ad)
    dc, da = torch.autograd.grad(val, (cd, ad))
    if spoil is not None:
        dc, da = dc.clone(), da.clone()
        dc[spoil[0]] = spoil[1]; da[spoil[0]] = spoil[1]
    tr.backward(dc, da)
    torch.cuda.synchronize()
    return np.concatenate([c.cpu().numpy(), a.cpu().numpy()[:, None]], -1), tr.gradients(), float(val.item())


def sample_results(tr):
    """(dL/d params_map [n, S, P] or None, (dL/d pts, dL/d rays_d_map) or None) of the instanced step `tr` has just taken, on the host."""
    pg = tr.sample_parameter_gradients().cpu().numpy() if tr.param_gradients else None
    ig = tuple(g.cpu().numpy() for g in tr.sample_input_gradients()) if tr.input_gradients else None
    torch.cuda.synchronize()
    return pg, ig


def patterns(tr, bufs, hit, kn):
    """The ReLU patterns of the instanced step the chain has just taken, in compact row order (`clc.chain_patterns` over the n_live rows), and
    the sign of the scaled density."""
    live = itc.live_order(hit, bufs[3])
    M = len(live)
    assert tr.last_live == M
    if M == 0:
        return dict(masks=[], branch_masks=None, sigma_mask=np.zeros(0, bool))
    masks, _, _ = clc.chain_patterns(tr, M, 1, None)
    sg = tr.activation(10, M)[:, 0]
    aw = np.asarray(bufs[6]).reshape(-1)[live] if kn["density_reweighting"] else F(1)
    return dict(masks=masks, branch_masks=None, sigma_mask=(sg * aw * F(kn["density_scale"])) > 0)


def restated_adjoint(raw, sg, bufs, hit, head, okw, sigma_mask, dtype=torch.float64):
    """dL/d raw colour [M', 3] and dL/d raw density [M'] of the instanced composite (`itc.restated`'s lines) at GIVEN network outputs in compact
    row order, under `head`: what slot 30 of an instanced step holds."""
    rays_d_map, pts, tt, dists, color_last, alpha_last, alpha_weight = [np.asarray(b) for b in bufs[:7]]
    n, S = dists.shape
    live = itc.live_order(hit, dists)
    li = torch.as_tensor(live)
    t_ = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype)
    at_live = lambda a: t_(np.nan_to_num(np.asarray(a, np.float64)).reshape(n * S)[live])
    raw, sg = t_(raw).requires_grad_(True), t_(sg).requires_grad_(True)
    sp = sg * (at_live(alpha_weight) if okw["density_reweighting"] else 1.0) * okw["density_scale"]
    a_live = 1.0 - torch.exp(-(sp * t_(np.asarray(sigma_mask))) * at_live(dists) / itc.PATCH_SCALE)
    rgb_live = torch.nn.functional.elu(raw) + 1 if okw["map_exr"] else torch.sigmoid(raw)
    am = torch.zeros(n * S, dtype=dtype).index_put((li,), a_live).reshape(n, S)
    rgb = torch.zeros((n * S, 3), dtype=dtype).index_put((li,), rgb_live).reshape(n, S, 3)
    am = torch.cat([am, t_(alpha_last).reshape(n, 1)], 1)
    rgb = torch.cat([rgb, t_(color_last).reshape(n, 1, 3)], 1)
    trans = torch.cumprod(1.0 - am + 1e-10, -1)
    wts = am * torch.cat([torch.ones_like(trans[:, :1]), trans[:, :-1]], -1)
    c = torch.sum(wts[..., None] * rgb, -2); a = torch.sum(wts, -1)
    if okw["composite_bkgd"]:
        c = c + (1.0 - a[..., None]) * torch.as_tensor(BKGD, dtype=dtype)
    h_ = torch.as_tensor(np.asarray(hit, bool))
    c = torch.where(h_[:, None], c, torch.zeros_like(c)); a = torch.where(h_, a, torch.zeros_like(a))
    head(c, a).backward()
    return np.concatenate([raw.grad.numpy().astype(np.float64), sg.grad.numpy().astype(np.float64)[:, None]], -1)


def checked_step(setup, case, pm=False, im=False, tr=None, report=print):
    """An instanced step on a (fresh) enabled chain trainer, held to the float64 restatement branched by the chain's kept signs: predictions
    within 1e-4, every layer's kernel and bias gradient by `clc.check_layers`, slot 30 (the composite's adjoint over the compact rows) by the
    same bar.  Returns (trainer, pred, gradient, want, f32, head, patterns)."""
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    tr = tr or chain_trainer(case, model, n, S, pm, im)
    head = itc.quadratic_head(n)
    pred, got, val = step(tr, bufs, hit, cone, kn, head)
    pat = patterns(tr, bufs, hit, kn)
    want = itc.restated(w, spec, bufs, hit, cone, head, **okw, **pat)
    f32 = itc.restated(w, spec, bufs, hit, cone, head, dtype=torch.float32, **okw, **pat)
    err = rel_linf(pred, want.pred)
    report(f"{case[0]}: {n} x {S}, {tr.last_live} live: loss {val:.9g} want {want.loss:.9g}; pred err {err:.2e} floor {rel_linf(f32.pred, want.pred):.2e}")
    assert err <= 1e-4, err
    assert np.all(pred[~np.asarray(hit, bool)] == 0)
    M = tr.last_live
    if M > 0 and tr.param_gradients != "only" and tr.input_gradients != "only":
        clc.check_layers(got, spec, want, f32, report)
    if M > 0:
        adj = tr.activation(30, M)
        raw, sg = tr.activation(11, M), tr.activation(10, M)[:, 0]
        a64 = restated_adjoint(raw, sg, bufs, hit, head, okw, pat["sigma_mask"])
        a32 = restated_adjoint(raw, sg, bufs, hit, head, okw, pat["sigma_mask"], torch.float32)
        e, fl = rel_linf(adj, a64), rel_linf(a32, a64)
        report(f"  slot 30 (adjoint, compact rows) err {e:.2e} floor {fl:.2e}")
        assert fl <= 5e-4 and e <= max(1e-4, 4 * fl), (e, fl)
    return tr, pred, got, want, f32, head, pat
