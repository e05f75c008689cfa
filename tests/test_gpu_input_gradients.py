"""dL/d rays_o, rays_d and dL/d pts, rays_d_map of the layer-by-layer training step (`ntx_trainer_enable_input_gradients`,
`FlexTrainer(input_gradients=...)`, the autograd ops) on the GPU against float64 autograd of the restated steps with the
rays / the sample points as leaves (tests/input_grad_common.py), branched by the signs of the activations the trainer kept.  The bar is the
project's standing one per output column (x, y, z of each of the two results, over the rays that hit or the live samples): rel-Linf <=
max(1e-4, 4 x floor), the floor what float32 autograd of the same restatement is off by, under the guards floor <= 5e-4 and max |grad| > 1e-6;
tests/test_input_gradients.py shows every case here to sit 2x inside the guards on the CPU.  Every case has un-normalised rays_d.  The
measured figures: profiles/input_gradients/errors.md.  `-m gpu`."""

import numpy as np
import pytest

from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests.train_common import BKGD, F, make_loss, step_noise, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def trainer_of(model, spec, kn, mode=True, pmode=False, max_rays=None, n_samples=None):
    """The layer-by-layer trainer of a case, made for the case's own size unless another is given."""
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer
    cls = BranchTrainer if pgc.has_branches(spec) else FlexTrainer
    return cls(model, max_rays=max_rays or kn["n"], n_samples=n_samples or kn["S"], perturb=kn["perturb"], blur_idx=kn["blur"], raw_noise_std=kn["noise_std"],
               map_exr=kn["map_exr"], param_gradients=pmode, input_gradients=mode)


def results(tr):
    """What the step `tr` has just taken left beside the weight gradient, on the host: (d_rays_o, d_rays_d) or None, dL/d rows or None."""
    rays = tuple(g.cpu().numpy() for g in tr.ray_gradients()) if tr.input_gradients else None
    pg = tr.parameter_gradients().cpu().numpy() if tr.param_gradients else None
    torch.cuda.synchronize()
    return rays, pg


def step(tr, batch, kn, seed):
    """One `gradients_step` of a case; (loss, [color | alpha], (d_rays_o, d_rays_d) or None, dL/d rows or None) on the host."""
    ro, rd, t, cone, rows, color, alpha = batch
    _, loss = make_loss(kn["loss_name"])
    val, cp, ap = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, composite_bkgd=kn["bkgd"], bkgd_color=BKGD, seed=seed, rays_per_param_row=kn["rpr"],
                                    n_samples=kn["S"], z_vals=kn["z"])
    return (float(val.item()), step_pred(cp, ap)) + results(tr)


def held_to_the_bar(tr, spec, wts, batch, kn, seed, val, got, name=""):
    """The ray gradients `got` and the loss `val` of the step `tr` has just taken against the float64 restatement of that step, branched by the
    signs of the activations the trainer kept, over the rays that hit; the missed rays' rows are exactly 0.  Returns the restatement."""
    n, S = kn["n"], kn["S"]
    patterns = pgc.trainer_patterns(tr, spec, n, S, step_noise(n, S, seed, kn["noise_std"]))
    want = igc.restate(spec, wts, batch, kn, seed, torch.float64, *patterns)
    f32 = igc.restate(spec, wts, batch, kn, seed, torch.float32, *patterns)
    print(f"{name}: {n} x {S}: loss {val if val is None else format(val, '.9g')} want {want[0]:.9g}")
    assert got[0].shape == got[1].shape == (n, 3) and got[0].dtype == got[1].dtype == np.float32
    if val is not None:
        assert abs(val - want[0]) <= 1e-5 * abs(want[0])
    miss = kn["miss"]
    assert not got[0][miss].any() and not got[1][miss].any() and not want[2][miss].any() and not want[3][miss].any()
    res = igc.check_input_gradients(got, want[2:], f32[2:], rows=~miss if miss.any() else None)
    print(f"IGERR {name} worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")
    return want


def run_case(case):
    """A case's step at its own size, its ray gradients held to the bar; returns (trainer, batch, knobs, seed, got)."""
    model, spec, wts, batch, kn, seed = igc.case_setup(case)
    lengths = np.linalg.norm(batch[1], axis=1)
    assert (np.abs(lengths - 1) > 1e-3).any()
    tr = trainer_of(model, spec, kn)
    val, pred, got, _ = step(tr, batch, kn, seed)
    held_to_the_bar(tr, spec, wts, batch, kn, seed, val, got, case[0])
    return tr, batch, kn, seed, got


# ---- 1 - 3. architectures, options, the fold's trips --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", igc.ARCH_CASES, ids=[c[0] for c in igc.ARCH_CASES])
def test_ray_gradients_match_float64_autograd(case):
    """70 rays x 33 samples per architecture: one, two and three readers of FF(xyz), the colour half layer as the reader of FF(dir), the chain's
    shape, FF(xyz) beside a branch's output, a Nerf, identity rows only, blur_idx on a geometry and on an appearance column."""
    run_case(case)


@pytest.mark.parametrize("case", igc.OPTION_CASES, ids=[c[0] for c in igc.OPTION_CASES])
def test_the_steps_options(case):
    """perturb + raw_noise_std 0.1 under AlphaLoss (the noise enters the |d| term); map_exr; NerfLoss(mse) over a background; caller's merged,
    non-uniform depths; a parameter row per ray beside the default two rows of 35."""
    run_case(case)


@pytest.mark.parametrize("case", igc.SAMPLE_CASES, ids=[c[0] for c in igc.SAMPLE_CASES])
def test_the_folds_trips_along_a_ray(case):
    """flex_ray_fold_kernel gives lane l the samples l, l + 64, ...: S = 2, 3 (62 / 61 idle lanes), 64, 65, 129, 256 (9 rays: 2304 samples),
    and one ray in all."""
    run_case(case)


# ---- 4. rays that miss -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", igc.MISS_CASES, ids=[c[0] for c in igc.MISS_CASES])
def test_rays_that_miss_get_exact_zeros(case):
    """`MISS_RAYS` at t = inf with cone_scale NaN (under blur_idx: NaN and +inf in turn): their rows are exactly 0 (`held_to_the_bar`), nothing
    is non-finite, the others meet the bar.  Then through forward + backward with NaN cotangents on the missed rays: every row is, bit for
    bit, the one of the same cotangents with zeros there."""
    tr, batch, kn, seed, got = run_case(case)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(tr.gradients()).all()
    ro, rd, t, cone, rows, color, alpha = batch
    miss, outs = kn["miss"], []
    rng = np.random.default_rng(1)
    dc, da = (rng.normal(size=(kn["n"], 3)) / kn["n"]).astype(F), (rng.normal(size=kn["n"]) / kn["n"]).astype(F)
    for spoil in (0.0, np.nan):
        dcs, das = dc.copy(), da.copy()
        dcs[miss] = spoil; das[miss] = spoil
        tr.forward(ro, rd, t, rows, cone, seed=seed, rays_per_param_row=kn["rpr"], n_samples=kn["S"])
        tr.backward(dcs, das)
        outs.append(results(tr)[0])
    for a, b in zip(*outs):
        assert np.array_equal(a, b) and np.isfinite(b).all() and not b[miss].any() and np.abs(b[~miss]).max() > 1e-6


# ---- 5. nothing else moves ----------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    """One batch on a trainer with parameter gradients on that has already stepped, input-gradient modes 0 -> 1 -> 2 -> 1 -> 0: loss,
    predictions, weight gradients and parameter gradients are the same bits in modes 0 and 1; mode 2 leaves the pre-filled gradient buffer
    untouched, gives mode 1's ray gradients and makes Adam and the stash refuse.  Then every pair of the two modes: the weight gradient is
    taken unless either is "only"."""
    from nerf_tex_amd import _lib
    model, spec, wts, batch, kn, seed = igc.case_setup(igc.ARCH_CASES[1])              # three readers of FF(xyz)
    other = tuple(np.ascontiguousarray(a[::-1]) if i in (5, 6) else a for i, a in enumerate(batch))
    tr = trainer_of(model, spec, kn, mode=False, pmode=True)
    step(tr, other, kn, seed + 1)
    fill = np.full(tr.n_weights, 7, F)
    prefill = lambda: tr._set(_lib.TRAINER_GRADIENTS, fill)
    v0, p0, none, pg0 = step(tr, batch, kn, seed)
    w0 = tr.gradients()
    assert none is None and np.abs(w0).max() > 1e-6 and np.abs(pg0).max() > 1e-6
    g1 = None
    for mode in (True, "only", True, False):
        tr.set_input_gradients(mode)
        prefill()
        v, p, g, pg = step(tr, batch, kn, seed)
        assert v == v0 and np.array_equal(p, p0) and np.array_equal(pg, pg0), mode
        assert np.array_equal(tr.gradients(), fill if mode == "only" else w0), mode
        if mode is False:
            assert g is None
            with pytest.raises(_lib.NtxError) as e:
                tr.ray_gradients()
            assert e.value.code == _lib.NTX_E_INVALID
            continue
        g1 = g if g1 is None else g1
        assert np.array_equal(g[0], g1[0]) and np.array_equal(g[1], g1[1]) and np.abs(g[0]).max() > 1e-6 and np.abs(g[1]).max() > 1e-6
        if mode == "only":
            with pytest.raises(_lib.NtxError) as e:
                tr.apply_gradients()
            assert e.value.code == _lib.NTX_E_INVALID
            assert _lib.lib.ntx_trainer_stash_gradients(tr._h, 0, None) == _lib.NTX_E_INVALID
    for pm in (False, True, "only"):
        for im in (False, True, "only"):
            tr.set_param_gradients(pm); tr.set_input_gradients(im)
            prefill()
            v, p, g, pg = step(tr, batch, kn, seed)
            assert v == v0 and np.array_equal(p, p0), (pm, im)
            assert np.array_equal(tr.gradients(), fill if "only" in (pm, im) else w0), (pm, im)
            assert (pg is None) if pm is False else np.array_equal(pg, pg0), (pm, im)
            assert (g is None) if im is False else (np.array_equal(g[0], g1[0]) and np.array_equal(g[1], g1[1])), (pm, im)
            refuses = _lib.lib.ntx_trainer_stash_gradients(tr._h, 0, None) == _lib.NTX_E_INVALID
            assert refuses == ("only" in (pm, im)), (pm, im)


# ---- 6. reproducible ---------------------------------------------------------------------------------------------------------------------
def test_ray_gradients_are_reproducible_and_independent_of_capacity():
    """The same step twice, and on a trainer made for 200 rays whose buffers hold another batch: the same bits.  forward + backward with
    NerfLoss(mse)'s cotangents, formed in float32 as the fused kernel forms them: the fused step's bits."""
    case = ("reproducible", *pgc.SMALL, dict(loss_name="nerf_mse"), (11, 3))
    model, spec, wts, batch, kn, seed = igc.case_setup(case)
    ro, rd, t, cone, rows, color, alpha = batch
    tr = trainer_of(model, spec, kn)
    first, again = step(tr, batch, kn, seed), step(tr, batch, kn, seed)
    big = trainer_of(model, spec, kn, max_rays=200, n_samples=kn["S"] + 7)
    _, _, _, other, okn, _ = igc.case_setup(("other", *pgc.SMALL, dict(n=200, S=kn["S"] + 7), (11, 4)))
    step(big, other, okn, 1)
    third = step(big, batch, kn, seed)
    assert np.abs(first[2][0]).max() > 1e-6 and np.abs(first[2][1]).max() > 1e-6
    for o in (again, third):
        assert o[0] == first[0] and np.array_equal(o[1], first[1]) and np.array_equal(o[2][0], first[2][0]) and np.array_equal(o[2][1], first[2][1])
    cf, af = tr.forward(ro, rd, t, rows, cone, seed=seed, rays_per_param_row=kn["rpr"], n_samples=kn["S"])
    p = cf.cpu().numpy()
    assert np.array_equal(p, first[1][:, :3])
    tr.backward((F(-2) * (color - p)) * (F(1) / F(3 * kn["n"])), None)
    split = results(tr)[0]
    assert np.array_equal(split[0], first[2][0]) and np.array_equal(split[1], first[2][1])


# ---- 7. the instanced step ----------------------------------------------------------------------------------------------------------------
def inst_trainer(case, model, n, S, mode=True, pmode=False, max_rays=None):
    from nerf_tex_amd import train
    kn = itc.knobs_of(case)
    return getattr(train, case[1])(model, max_rays=max_rays or n, n_samples=max(S, 2), perturb=False, blur_idx=case[4], map_exr=kn["map_exr"], param_gradients=pmode,
                                   input_gradients=mode)


def inst_step(tr, bufs, hit, cone, kn, head):
    """forward_instanced, the head and its cotangents in torch on the device, backward; (pred [n, 4], (d_pts, d_rays_d_map) on the host)."""
    from tests.test_gpu_train_instanced import step as plain_inst_step
    pred, _, _ = plain_inst_step(tr, bufs, hit, cone, kn, head)
    got = tuple(g.cpu().numpy() for g in tr.sample_input_gradients()) if tr.input_gradients else None
    torch.cuda.synchronize()
    return pred, got


def inst_checked(setup, case=itc.CASES[0], name="", poison=False):
    """An instanced step on a fresh trainer, its sample gradients held to the restatement over the live samples; exact zeros elsewhere."""
    from tests.test_gpu_train_instanced import patterns
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    live = itc.live_mask(hit, bufs[3])
    if poison:                                                                     # nothing of pts / rays_d_map is read at a sample that is not live
        bufs = list(bufs)
        for k in (0, 1):
            b = np.array(bufs[k], F, copy=True); b[~live] = np.nan; bufs[k] = b
        bufs = tuple(bufs)
    tr = inst_trainer(case, model, n, S)
    head = itc.quadratic_head(n)
    pred, got = inst_step(tr, bufs, hit, cone, kn, head)
    assert got[0].shape == got[1].shape == (n, S, 3) and np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(pred).all()
    assert not got[0][~live].any() and not got[1][~live].any()
    if not live.any():
        assert tr.last_live == 0
        return tr, got
    pat = patterns(tr, spec, bufs, hit, kn)
    want = igc.restated_sample_gradients(w, spec, bufs, hit, cone, head, **okw, **pat)
    f32 = igc.restated_sample_gradients(w, spec, bufs, hit, cone, head, dtype=torch.float32, **okw, **pat)
    print(f"{name}: {n} x {S}, {tr.last_live} live")
    res = igc.check_input_gradients(got, want[2:], f32[2:], rows=live.reshape(-1))
    print(f"IGERR instanced_{name} worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")
    return tr, got


@pytest.mark.parametrize("case", itc.CASES, ids=itc.CASE_IDS)
def test_sample_gradients_match_float64_autograd(case):
    """The cases of the instanced step (alpha_weight NULL, map_exr + background, blur_idx on a geometry and on an appearance parameter,
    parameter branches) with pts / rays_d_map NaN at every sample that is not live: finite results, exact zeros there."""
    inst_checked(itc.case_setup(case), case, case[0], poison=True)


@pytest.mark.parametrize("edge", igc.INST_EDGES, ids=igc.INST_EDGE_IDS)
def test_sample_and_live_count_edges(edge):
    """S = 1, 64, 65 and live counts 0, 1, 32, 33, 2047, 2049 by an explicit live mask; without a live sample both results are zeros."""
    tr, got = inst_checked(itc.edge_setup(edge), name=edge[0], poison=True)
    if edge[1] == "live":
        assert tr.last_live == edge[2]


def test_the_instanced_step_moves_nothing_else_and_the_getters_refuse_each_others_steps():
    """The per-sample parameter gradients, the predictions and the weight gradient of an instanced step are the same bits with input gradients
    off, on and "only" (no weight gradient then); `ray_gradients` refuses after an instanced step, `sample_input_gradients` after a plain one."""
    from nerf_tex_amd import _lib
    from tests.test_gpu_train_instanced import step as plain_inst_step
    case = itc.CASES[1]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    head = itc.quadratic_head(n)
    tr = inst_trainer(case, model, n, S, mode=False, pmode=True)
    p0, w0, _ = plain_inst_step(tr, bufs, hit, cone, kn, head)
    spg0 = tr.sample_parameter_gradients().cpu().numpy()
    with pytest.raises(_lib.NtxError):
        tr.sample_input_gradients()
    tr.set_input_gradients(True)
    p1, w1, _ = plain_inst_step(tr, bufs, hit, cone, kn, head)
    g1 = [g.cpu().numpy() for g in tr.sample_input_gradients()]
    assert np.array_equal(p1, p0) and np.array_equal(w1, w0) and np.array_equal(tr.sample_parameter_gradients().cpu().numpy(), spg0) and np.abs(spg0).max() > 1e-6
    with pytest.raises(_lib.NtxError) as e:
        tr.ray_gradients()
    assert e.value.code == _lib.NTX_E_INVALID
    tr.set_input_gradients("only")
    fill = np.full(tr.n_weights, 7, F)
    tr._set(_lib.TRAINER_GRADIENTS, fill)
    p2, w2, _ = plain_inst_step(tr, bufs, hit, cone, kn, head)
    g2 = [g.cpu().numpy() for g in tr.sample_input_gradients()]
    assert np.array_equal(p2, p0) and np.array_equal(w2, fill) and np.array_equal(tr.sample_parameter_gradients().cpu().numpy(), spg0)
    assert all(np.array_equal(a, b) and np.abs(a).max() > 1e-6 for a, b in zip(g1, g2))
    # a plain step on the same handle: the getters change places
    rng = np.random.default_rng(0)
    ro, rd = rng.normal(size=(n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    t = np.tile(np.array([[0.5, 1.5]], F), (n, 1))
    color, alpha = rng.uniform(0, 1, (n, 3)).astype(F), rng.uniform(0, 1, n).astype(F)
    params = rng.uniform(0.2, 1, (n, spec.n_params)).astype(F)
    tr.gradients_step(ro, rd, t, params, cone, color, alpha, make_loss("alpha_smape")[1], seed=0, n_samples=S)
    assert tr.ray_gradients()[0].shape == (n, 3)
    with pytest.raises(_lib.NtxError) as e:
        tr.sample_input_gradients()
    assert e.value.code == _lib.NTX_E_INVALID


# ---- 8. the autograd ops ------------------------------------------------------------------------------------------------------------------
def test_the_autograd_ops_hand_the_input_gradients_on():
    """`DifferentiableRender`: rays_o.grad / rays_d.grad are `ray_gradients()` plus a second torch term on the same leaves; a second backward
    raises; with input gradients off the leaves get no gradient from the render, as before.  `DifferentiableInstanceRender`: the same for pts
    and rays_d_map."""
    from nerf_tex_amd.autograd import DifferentiableInstanceRender, DifferentiableRender
    dev = torch.device("cuda", 0)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).float()
    model, spec, wts, batch, kn, seed = igc.case_setup(igc.ARCH_CASES[0])
    ro, rd, t, cone, rows, color, alpha = batch
    head = itc.quadratic_head(kn["n"])
    for mode in (True, False):
        tr = trainer_of(model, spec, kn, mode=mode)
        o, dd = d(ro).requires_grad_(True), d(rd).requires_grad_(True)
        c, a = DifferentiableRender(tr)(o, dd, t, rows, cone, seed=seed, rays_per_param_row=kn["rpr"], n_samples=kn["S"])
        extra = 3.0 * o.sum() - 2.0 * dd.sum() if mode else 0.0
        (head(c, a) + extra).backward(retain_graph=True)
        if not mode:
            assert o.grad is None and dd.grad is None and np.abs(tr.gradients()).max() > 1e-6
            continue
        go, gd = tr.ray_gradients()
        assert go.abs().max() > 1e-6 and gd.abs().max() > 1e-6
        assert torch.equal(o.grad, go + 3.0) and torch.equal(dd.grad, gd - 2.0)
        with pytest.raises(RuntimeError, match="one backward per forward"):
            head(c, a).backward()
    case = itc.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    live = itc.live_mask(hit, bufs[3])
    head = itc.quadratic_head(n)
    for mode in (True, False):
        tr = inst_trainer(case, model, n, S, mode=mode)
        dirs, pts = d(np.nan_to_num(bufs[0])).requires_grad_(True), d(np.nan_to_num(bufs[1])).requires_grad_(True)
        tb = (dirs, pts) + tuple(bufs[2:])
        render = DifferentiableInstanceRender(tr, patch_scale=itc.PATCH_SCALE, density_scale=kn["density_scale"], density_reweighting=kn["density_reweighting"])
        c, a = render(tb, cone, hit=hit.astype(np.uint8))
        extra = 3.0 * pts.sum() - 2.0 * dirs.sum() if mode else 0.0
        (head(c, a) + extra).backward()
        if not mode:
            assert pts.grad is None and dirs.grad is None
            continue
        gp, gdm = tr.sample_input_gradients()
        assert gp.abs().max() > 1e-6 and gdm.abs().max() > 1e-6 and not gp.cpu().numpy()[~live].any()
        assert torch.equal(pts.grad, gp + 3.0) and torch.equal(dirs.grad, gdm - 2.0)


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """The chain's handle: NTX_E_UNSUPPORTED (`trainer_for(model, input_gradients=...)` names the layer-by-layer class for its shape).  Mode 3:
    NTX_E_INVALID.  Either getter in mode 0 and before any step: NTX_E_INVALID."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import FlexTrainer, Trainer, trainer_class_for, trainer_for
    from tests.common import make_model
    chain_model, _, _ = make_model((1, 6), dense_media=True)
    chain = Trainer(chain_model, max_rays=8, n_samples=8)
    assert _lib.lib.ntx_trainer_enable_input_gradients(chain._h, 1) == _lib.NTX_E_UNSUPPORTED and b"ntx_trainer_create_flex" in _lib.lib.ntx_last_error()
    assert trainer_class_for(chain_model) is Trainer and trainer_class_for(chain_model, input_gradients=True) is FlexTrainer
    assert type(trainer_for(chain_model, max_rays=8, n_samples=8)) is Trainer
    assert type(trainer_for(chain_model, max_rays=8, n_samples=8, input_gradients="only")) is FlexTrainer
    model, spec, wts, batch, kn, seed = igc.case_setup(igc.ARCH_CASES[0])
    tr = trainer_of(model, spec, kn, mode=False)
    for enable in (False, True):                                                   # the mode off; on, but no step yet
        if enable:
            tr.set_input_gradients(True)
        for getter in (tr.ray_gradients, tr.sample_input_gradients):
            with pytest.raises(_lib.NtxError) as e:
                getter()
            assert e.value.code == _lib.NTX_E_INVALID
    with pytest.raises(ValueError):
        tr.set_input_gradients(2)
    assert _lib.lib.ntx_trainer_enable_input_gradients(tr._h, 3) == _lib.NTX_E_INVALID
    step(tr, batch, kn, seed)
    assert tr.ray_gradients()[1].shape == (kn["n"], 3)
