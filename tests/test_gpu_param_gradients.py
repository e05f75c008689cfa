"""dL/d material parameters of the layer-by-layer training step (`ntx_trainer_enable_param_gradients`, `FlexTrainer(param_gradients=...)`,
`nerf_tex_amd.fit.ParameterFitter`) on the GPU against float64 autograd of the restated step with the parameter rows as the
leaf (tests/param_grad_common.py), branched by the signs of the activations the trainer kept.  The bar is the project's standing one per
parameter column -- rel-Linf <= max(1e-4, 4 x floor), the floor what float32 autograd of the same restatement is off by, under the guards
floor <= 5e-4 and max |grad| > 1e-6; tests/test_param_gradients.py shows every case here to meet the guards on the CPU.  Every case runs at its
own size and depths; the second half of the file is the edges (sample counts, rows, limits, missed rays under blur_idx, caller's depths, enabling
late, coarse + fine, the fitter's options, parameters too small), measured in profiles/param_gradients/edge_errors.md.  `-m gpu`."""

import numpy as np
import pytest

from tests import param_grad_common as pgc
from tests.train_common import BKGD, make_loss, step_noise, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
S = pgc.N_SAMPLES


def trainer_of(model, spec, kn, mode=True, max_rays=None, n_samples=None):
    """The layer-by-layer trainer of a case, made for the case's own size unless another is given."""
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer
    cls = BranchTrainer if pgc.has_branches(spec) else FlexTrainer
    return cls(model, max_rays=max_rays or kn["n"], n_samples=n_samples or kn["S"], perturb=kn["perturb"], blur_idx=kn["blur"], raw_noise_std=kn["noise_std"],
               map_exr=kn["map_exr"], param_gradients=mode)


def step(tr, batch, kn, seed):
    """One `gradients_step` of a case, on the case's own depths where it has them; (loss, [color | alpha], dL/d rows) on the host."""
    ro, rd, t, cone, rows, color, alpha = batch
    _, loss = make_loss(kn["loss_name"])
    val, cp, ap = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, composite_bkgd=kn["bkgd"], bkgd_color=BKGD, seed=seed, rays_per_param_row=kn["rpr"],
                                    n_samples=kn["S"], z_vals=kn["z"])
    pg = tr.parameter_gradients() if tr.param_gradients else None
    torch.cuda.synchronize()
    return float(val.item()), step_pred(cp, ap), None if pg is None else pg.cpu().numpy()


def held_to_the_bar(tr, spec, wts, batch, kn, seed, val, got, rows=None, name=""):
    """The parameter gradients `got` and the loss `val` of the step `tr` has just taken against the float64 restatement of that step, branched by
    the signs of the activations the trainer kept; returns the restatement."""
    n, S = kn["n"], kn["S"]
    patterns = pgc.trainer_patterns(tr, spec, n, S, step_noise(n, S, seed, kn["noise_std"]))
    want = pgc.restate(spec, wts, batch, kn, seed, torch.float64, *patterns)
    f32 = pgc.restate(spec, wts, batch, kn, seed, torch.float32, *patterns)
    print(f"{name}: {n} x {S}, {kn['rpr']} rays a row: loss {val if val is None else format(val, '.9g')} want {want[0]:.9g}; rows {got.shape}")
    assert got.shape == want[2].shape == (-(-n // kn["rpr"]), spec.n_params)
    if val is not None:
        assert abs(val - want[0]) <= 1e-5 * abs(want[0])
    pgc.check_param_gradients(got, want[2], f32[2], rows=rows)
    return want


def run_case(case, rows=None):
    """A case's step at its own size, its parameter gradients held to the bar; returns (trainer, got, the float64 restatement, knobs)."""
    model, spec, wts, batch, kn, seed = pgc.case_setup(case)
    tr = trainer_of(model, spec, kn)
    val, pred, got = step(tr, batch, kn, seed)
    want = held_to_the_bar(tr, spec, wts, batch, kn, seed, val, got, rows, case[0])
    return tr, got, want, kn


@pytest.mark.parametrize("case", pgc.MODEL_CASES, ids=[c[0] for c in pgc.MODEL_CASES])
def test_parameter_gradients_match_float64_autograd(case):
    """70 rays x 33 samples, two parameter rows, per architecture: every reader of the parameter features (or the first layer of every branch),
    the fold through FourierFeatures and the per-sample scale of blur_idx."""
    run_case(case)


@pytest.mark.parametrize("case", pgc.ROW_CASES, ids=[c[0] for c in pgc.ROW_CASES])
def test_rays_per_parameter_row(case):
    """A row per ray, two rows of 35, one row of 70, and 64 rays a row, where the last row is a short one of 6 rays."""
    _, got, _, kn = run_case(case)
    assert got.shape[0] == {1: 70, 35: 2, 70: 1, 64: 2}[kn["rpr"]]


@pytest.mark.parametrize("case", pgc.OPTION_CASES, ids=[c[0] for c in pgc.OPTION_CASES])
def test_the_steps_options(case):
    """perturb + raw_noise_std 0.1 under AlphaLoss(smape, mse); NerfLoss(mse) over a background; map_exr."""
    run_case(case)


def test_rays_that_miss_contribute_exactly_zero():
    """Rays 0, 5, 33, 34 and the whole last parameter row at t = inf with cone_scale = NaN: that row's gradient is exactly 0, nothing is NaN, and
    the other row still meets the bar."""
    case = pgc.MISS_CASE
    live = np.array([True, False])
    tr, got, want, kn = run_case(case, rows=live)
    assert kn["miss"][35:].all() and (got[1] == 0).all() and (want[2][1] == 0).all() and np.isfinite(got).all()
    assert np.isfinite(tr.gradients()).all()


def test_nothing_else_moves():
    """Mode 1 beside a twin that never enabled it: loss, predictions and weight gradients bit for bit.  Mode 2: loss, predictions and parameter
    gradients are mode 1's bits, the weight gradient buffer keeps what the last mode-1 step left, and Adam refuses."""
    from nerf_tex_amd import _lib
    for case in (pgc.MODEL_CASES[0], pgc.MODEL_CASES[6]):                          # parameter features read by three layers; branches on both groups
        model, spec, wts, batch, kn, seed = pgc.case_setup(case)
        twin, tr = trainer_of(model, spec, kn, mode=False), trainer_of(model, spec, kn, mode=True)
        v0, p0, none = step(twin, batch, kn, seed)
        v1, p1, g1 = step(tr, batch, kn, seed)
        w1 = tr.gradients()
        assert none is None and v0 == v1 and np.array_equal(p0, p1) and np.array_equal(twin.gradients(), w1) and np.abs(w1).max() > 1e-6
        tr.set_param_gradients("only")
        other = tuple(np.ascontiguousarray(a[::-1]) if i in (5, 6) else a for i, a in enumerate(batch))       # other targets: another weight gradient, were one taken
        step(tr, other, kn, seed)
        assert np.array_equal(tr.gradients(), w1)
        v2, p2, g2 = step(tr, batch, kn, seed)
        assert v2 == v1 and np.array_equal(p2, p1) and np.array_equal(g2, g1) and np.array_equal(tr.gradients(), w1)
        with pytest.raises(_lib.NtxError) as e:
            tr.apply_gradients()
        assert e.value.code == _lib.NTX_E_INVALID
        tr.set_param_gradients(True)
        tr.apply_gradients()                                                       # ... and takes it again on the gradient it still holds
        assert tr.iterations == 1


def test_parameter_gradients_are_reproducible_and_independent_of_capacity():
    """The same step twice, and on a trainer made for 256 rays and more samples whose buffers hold another batch: the same bits."""
    case = pgc.ROW_CASES[3]                                                        # 64 rays a row: a short last row
    model, spec, wts, batch, kn, seed = pgc.case_setup(case)
    tr = trainer_of(model, spec, kn, mode="only")
    first, again = step(tr, batch, kn, seed), step(tr, batch, kn, seed)
    big = trainer_of(model, spec, kn, mode="only", max_rays=256, n_samples=S + 7)
    _, _, _, other, okn, _ = pgc.case_setup(pgc.ROW_CASES[1], n=256, S=S + 7)
    ro, rd, t, cone, rows, color, alpha = other
    big.gradients_step(ro, rd, t, rows, cone, color, alpha, make_loss(okn["loss_name"])[1], seed=1, rays_per_param_row=okn["rpr"])
    third = step(big, batch, kn, seed)
    assert np.abs(first[2]).max() > 1e-6
    for o in (again, third):
        assert o[0] == first[0] and np.array_equal(o[1], first[1]) and np.array_equal(o[2], first[2])


def test_refusals():
    """The chain's handle: NTX_E_UNSUPPORTED.  A Nerf: NTX_E_INVALID.  Reading with the mode off, or before a step: NTX_E_INVALID."""
    import ctypes as C
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import FlexTrainer, Trainer, trainer_class_for, trainer_for
    from tests.common import make_model
    chain_model, _, _ = make_model((1, 6), dense_media=True)
    chain = Trainer(chain_model, max_rays=8, n_samples=8)
    rc = _lib.lib.ntx_trainer_enable_param_gradients(chain._h, 1)
    assert rc == _lib.NTX_E_UNSUPPORTED and b"ntx_trainer_create_flex" in _lib.lib.ntx_last_error()
    assert trainer_class_for(chain_model) is Trainer and trainer_class_for(chain_model, param_gradients=True) is FlexTrainer
    assert type(trainer_for(chain_model, max_rays=8, n_samples=8)) is Trainer
    assert type(trainer_for(chain_model, max_rays=8, n_samples=8, param_gradients="only")) is FlexTrainer
    nerf, _, _ = make_model((0, 0), kind="Nerf", dense_media=True, arch=dict(width=64, depth=3, skips=[1]))
    with pytest.raises(_lib.NtxError) as e:
        FlexTrainer(nerf, max_rays=8, n_samples=8, param_gradients=True)
    assert e.value.code == _lib.NTX_E_INVALID and "ParamNerf" in str(e.value)
    model, spec, wts, batch, kn, seed = pgc.case_setup(pgc.ROW_CASES[1])
    tr = trainer_of(model, spec, kn, mode=False)
    for enable in (False, True):                                                   # the mode off; on, but no step yet
        if enable:
            tr.set_param_gradients(True)
        with pytest.raises(_lib.NtxError) as e:
            tr.parameter_gradients()
        assert e.value.code == _lib.NTX_E_INVALID
    with pytest.raises(ValueError):
        tr.set_param_gradients(2)
    assert _lib.lib.ntx_trainer_enable_param_gradients(tr._h, 3) == _lib.NTX_E_INVALID
    step(tr, batch, kn, seed)
    assert tr.parameter_gradients().shape == (2, 7)


def test_fitting_parameters_end_to_end():
    """A teacher ParamNerf [1, 4] renders 2 images x 128 rays x 32 samples at known parameters; `ParameterFitter.fit` starts 0.2 off.  The float64
    restatement of the same fit (tests/test_param_gradients.py) ends below 0.25 x its initial loss; float32 and another order of the sums move an
    Adam trajectory, so the GPU fit is given twice that margin: below 0.5 x.  Every loss is finite and the weights do not change by a bit."""
    from nerf_tex_amd.fit import ParameterFitter
    f = pgc.FIT
    model, spec, wts, batch, true, init = pgc.fit_setup()
    blob = np.array(model.get_blob(), np.float32, copy=True)
    fitter = ParameterFitter(model, n_samples=f["S"], max_rays=f["images"] * f["rays"], lrate=f["lrate"])
    val, grad = fitter.step(batch, make_loss(f["loss_name"])[1], init)
    assert grad.shape == init.shape and torch.isfinite(grad).all() and grad.abs().max() > 0
    params, losses = fitter.fit(batch, make_loss(f["loss_name"])[1], init, f["n_iters"])
    params = params.cpu().numpy()
    print(f"loss {losses[0]:.4e} -> {losses[-1]:.4e} ({losses[-1] / losses[0]:.3f}); |p - true| {np.abs(init - true).max():.3f} -> {np.abs(params - true).max():.3f}")
    assert len(losses) == f["n_iters"] and np.isfinite(losses).all() and abs(losses[0] - float(val.item())) <= 1e-6 * abs(losses[0])
    assert losses[-1] < 0.5 * losses[0], (losses[0], losses[-1])
    assert np.array_equal(fitter.weights(), blob) and np.array_equal(np.asarray(model.get_blob(), np.float32), blob)
    bounded = ParameterFitter(model, n_samples=f["S"], max_rays=f["images"] * f["rays"], lrate=f["lrate"], bounds=(init.min() - 0.01, init.max() + 0.01))
    p2, _ = bounded.fit(batch, make_loss(f["loss_name"])[1], init, 5)
    assert float(p2.min()) >= init.min() - 0.01 and float(p2.max()) <= init.max() + 0.01


# ---- the edges: sample counts, rows, limits, missed rays under blur_idx, caller's depths (profiles/param_gradients/edge_errors.md) -------------
@pytest.mark.parametrize("case", pgc.SAMPLE_CASES, ids=[c[0] for c in pgc.SAMPLE_CASES])
def test_the_folds_trips_along_a_ray(case):
    """flex_param_fold_kernel gives lane l the samples l, l + 64, ...: S = 64 (every lane once), 65 (one lane twice), 129 (a third trip), 256
    (9 rays: 2304 samples), 3 and the step's minimum 2 (61 / 62 lanes carry nothing)."""
    run_case(case)


@pytest.mark.parametrize("case", pgc.ROW_EDGE_CASES, ids=[c[0] for c in pgc.ROW_EDGE_CASES])
def test_rows_around_the_unrolled_loop(case):
    """flex_param_rows_kernel's loop over a row's rays is unrolled by 8: 20 rays in rows of 7, 8, 9 (short last rows of 6, 4, 2) and of 32 (a row
    longer than the batch), one ray in all, three rays in rows of 2."""
    _, got, _, kn = run_case(case)
    assert got.shape[0] == {(20, 7): 3, (20, 8): 3, (20, 9): 3, (20, 32): 1, (1, 1): 1, (3, 2): 2}[kn["n"], kn["rpr"]]


@pytest.mark.parametrize("case", pgc.LIMIT_CASES, ids=[c[0] for c in pgc.LIMIT_CASES])
def test_the_built_limits_and_one_group_models(case):
    """n_parameters [4, 8] (36 and 72 feature columns, P = 12) with blur_idx on the first and last column of each group; [0, a] and [g, 0]
    without branches, where one of the two feature gradients is never placed; branches whose input rows differ from sample to sample."""
    run_case(case)


@pytest.mark.parametrize("case", pgc.MISS_BLUR_CASES, ids=[c[0] for c in pgc.MISS_BLUR_CASES])
def test_rays_that_miss_under_blur_idx(case):
    """The missed rays of `MISS_CASE` where the fold reads cone_scale (blur_idx on a geometry and on an appearance column), NaN for every other
    missed ray and +inf for the rest: a missed sample is selected to 0, so the missed row is exactly 0 and nothing is NaN or inf."""
    live = np.array([True, False])
    tr, got, want, kn = run_case(case, rows=live)
    _, _, _, batch, _, _ = pgc.case_setup(case)
    cone = batch[3][kn["miss"]]
    assert np.isnan(cone).any() and np.isposinf(cone).any() and not np.isfinite(cone).any()
    assert kn["miss"][35:].all() and (got[1] == 0).all() and (want[2][1] == 0).all() and np.isfinite(got).all()
    assert np.isfinite(tr.gradients()).all()


@pytest.mark.parametrize("case", pgc.DEPTH_CASES, ids=[c[0] for c in pgc.DEPTH_CASES])
def test_callers_depths(case):
    """`z_vals` as the fine pass of coarse + fine hands them over: 40 + 27 merged, non-uniform depths a ray, which enter the blurred column's
    cone_scale * z factor (blur_idx None, the geometry column, the first and the last appearance column)."""
    _, _, _, kn = run_case(case)
    gaps = np.diff(kn["z"], axis=1)
    assert kn["z"].shape == (10, 67) and (gaps >= 0).all() and (gaps.max(1) > 2 * gaps.min(1)).all()          # sorted, and no even spacing


def test_rows_are_the_ascending_sum_of_their_rays():
    """20 rays x 33 samples, once with a row per ray (every ray given its row's parameters) and once in rows of 7, 8, 9 and 32 rays: the same
    loss and predictions, and each row of the grouped result is, bit for bit, the float32 running sum of its rays' gradients in ascending ray
    order -- flex_param_rows_kernel's loop is sequential (the build has no fast-math), whatever its unrolling."""
    model, spec, wts, batch, kn, seed = pgc.case_setup(("per_ray", *pgc.SMALL, dict(n=20, rpr=1), (11, 3)))
    tr = trainer_of(model, spec, kn, mode="only")
    ro, rd, t, cone, per_ray, color, alpha = batch
    for r in (7, 8, 9, 32):
        rows = np.ascontiguousarray(per_ray[::r])
        spread = np.ascontiguousarray(np.repeat(rows, r, 0)[:20])
        v1, p1, g1 = step(tr, (ro, rd, t, cone, spread, color, alpha), kn, seed)
        vr, pr, gr = step(tr, (ro, rd, t, cone, rows, color, alpha), dict(kn, rpr=r), seed)
        assert g1.shape == (20, 7) and gr.shape == (len(rows), 7) and g1.dtype == gr.dtype == np.float32 and np.abs(g1).max() > 1e-6
        assert vr == v1 and np.array_equal(pr, p1)
        want = np.zeros_like(gr)
        for row in range(len(rows)):
            for c in range(7):
                acc = np.float32(0)
                for ray in range(row * r, min((row + 1) * r, 20)):
                    acc = np.float32(acc + g1[ray, c])
                want[row, c] = acc
        assert np.array_equal(gr, want), (r, np.abs(gr - want).max())


@pytest.mark.parametrize("case", [pgc.MODEL_CASES[0], pgc.MODEL_CASES[6]], ids=["features", "branches"])
def test_enabling_late_and_switching_modes(case):
    """`set_param_gradients(True)` on a trainer that has stepped twice places the feature gradients and re-places the transposed weights and their
    segment table: the third step is, bit for bit, the one of a trainer created with the mode on and taken through the same two steps.  Then
    True -> False (reading raises NTX_E_INVALID) -> "only" -> True: the parameter gradients of the same batch are the same bits each time."""
    from nerf_tex_amd import _lib
    model, spec, wts, batch, kn, seed = pgc.case_setup(case)
    other = tuple(np.ascontiguousarray(a[::-1]) if i in (5, 6) else a for i, a in enumerate(batch))
    late, early = trainer_of(model, spec, kn, mode=False), trainer_of(model, spec, kn, mode=True)
    for tr in (late, early):
        for b, s in ((batch, seed), (other, seed + 1)):
            step(tr, b, kn, s)
            tr.apply_gradients()
    late.set_param_gradients(True)
    v0, p0, g0 = step(late, batch, kn, seed + 2)
    v1, p1, g1 = step(early, batch, kn, seed + 2)
    assert late.iterations == early.iterations == 2 and np.array_equal(late.weights(), early.weights()) and not np.array_equal(late.weights(), np.asarray(model.get_blob(), np.float32))
    assert v0 == v1 and np.array_equal(p0, p1) and np.array_equal(late.gradients(), early.gradients()) and np.array_equal(g0, g1)
    assert np.isfinite(g0).all() and np.abs(g0).max() > 1e-6 and np.abs(late.gradients()).max() > 1e-6
    for mode in (False, "only", True):
        late.set_param_gradients(mode)
        v, p, g = step(late, batch, kn, seed + 2)
        assert v == v0 and np.array_equal(p, p0)
        if mode is False:
            assert g is None
            with pytest.raises(_lib.NtxError) as e:
                late.parameter_gradients()
            assert e.value.code == _lib.NTX_E_INVALID
        else:
            assert np.array_equal(g, g0), mode
    assert np.array_equal(late.gradients(), early.gradients())


def test_coarse_and_fine_passes_leave_their_own_parameter_gradients():
    """CoarseFineTrainer on one network, 24 + 16 samples, perturb, 24 rays in rows of 12: between the passes `parameter_gradients()` is the coarse
    pass's (on the depths the step places), after the step the fine pass's (on the merged depths the sampler left, `last_z`); both are held to
    the bar, and the weight gradients are a twin's without parameter gradients bit for bit.  The coarse pass is a case of the CPU's fairness
    test; the fine pass's depths come from the trainer's own float32 sampler, so `check_param_gradients`' guards decide here."""
    from nerf_tex_amd.train import CoarseFineTrainer, FlexTrainer
    model, spec, wts, batch, kn, seed = pgc.case_setup(pgc.COARSE_CASE)
    ro, rd, t, cone, rows, color, alpha = batch
    n, S, NI = kn["n"], kn["S"], 16
    _, loss = make_loss(kn["loss_name"])
    tr = CoarseFineTrainer(model, None, max_rays=n, n_samples=S, n_importance=NI, perturb=True, param_gradients=True)
    twin = CoarseFineTrainer(model, None, max_rays=n, n_samples=S, n_importance=NI, perturb=True)
    assert type(tr.fine) is FlexTrainer and tr.coarse is tr.fine and type(twin.fine) is FlexTrainer
    seen = {}

    def on_coarse():
        seen["got"] = tr.coarse.parameter_gradients().cpu().numpy()
        seen["want"] = held_to_the_bar(tr.coarse, spec, wts, batch, kn, seed, None, seen["got"], name="coarse pass")

    out = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, seed=seed, rays_per_param_row=kn["rpr"], on_coarse=on_coarse)
    got_fine = tr.fine.parameter_gradients().cpu().numpy()
    z = tr.last_z.cpu().numpy()
    assert z.shape == (n, S + NI) and (np.diff(z, axis=1) >= 0).all()
    fine_kn = dict(kn, S=S + NI, z=z)
    want_fine = held_to_the_bar(tr.fine, spec, wts, batch, fine_kn, seed, None, got_fine, name="fine pass")
    val, want_val = float(out[0].item()), seen["want"][0] + want_fine[0]
    assert abs(val - want_val) <= 1e-5 * abs(want_val)
    assert not np.array_equal(seen["got"], got_fine)
    out2 = twin.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, seed=seed, rays_per_param_row=kn["rpr"])
    assert float(out2[0].item()) == val and np.array_equal(twin.last_z.cpu().numpy(), z)
    assert np.array_equal(twin.fine.gradients(), tr.fine.gradients()) and np.abs(tr.fine.gradients()).max() > 1e-6


def test_fitter_options():
    """`ParameterFitter` beyond its defaults: a branch model gets a BranchTrainer; blur_idx / perturb / raw_noise_std / map_exr reach the step (its
    gradient within the bar of the restatement of that same step); per-parameter bounds; an iterable of batches is taken in turn as `step` by
    hand under the same Adam; n_iters = 0 returns the start.  The weights do not change by a bit in any of these."""
    from nerf_tex_amd.fit import ParameterFitter
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer
    unchanged = lambda fitter, model, blob: np.array_equal(fitter.weights(), blob) and np.array_equal(np.asarray(model.get_blob(), np.float32), blob)
    # a branch model
    model, spec, wts, batch, kn, seed = pgc.case_setup(pgc.MODEL_CASES[6])
    assert type(ParameterFitter(model, n_samples=8, max_rays=8).trainer) is BranchTrainer
    # the renderer's options: the step is the restatement's
    model, spec, wts, batch, kn, seed = pgc.case_setup(pgc.FITTER_CASE)
    blob = np.array(model.get_blob(), np.float32, copy=True)
    ro, rd, t, cone, rows, color, alpha = batch
    B, R = len(rows), kn["rpr"]
    images = dict(rays_o=ro.reshape(B, R, 3), rays_d=rd.reshape(B, R, 3), t=t.reshape(B, R, 2), cone_scale=cone.reshape(B, R, 1), color=color.reshape(B, R, 3),
                  alpha=alpha.reshape(B, R))
    fitter = ParameterFitter(model, n_samples=kn["S"], max_rays=kn["n"], blur_idx=kn["blur"], perturb=kn["perturb"], raw_noise_std=kn["noise_std"], map_exr=kn["map_exr"])
    assert type(fitter.trainer) is FlexTrainer and fitter.trainer.param_gradients == "only"
    val, grad = fitter.step(images, make_loss(kn["loss_name"])[1], rows, seed=seed)
    held_to_the_bar(fitter.trainer, spec, wts, batch, kn, seed, float(val.item()), grad.cpu().numpy(), name=pgc.FITTER_CASE[0])
    assert unchanged(fitter, model, blob)
    # bounds per parameter, batches in turn, no iteration at all
    f = pgc.FIT
    model, spec, wts, batch, true, init = pgc.fit_setup()
    blob = np.array(model.get_blob(), np.float32, copy=True)
    loss = make_loss(f["loss_name"])[1]
    P = init.shape[1]
    low, high = init.min(0) - 0.002 * (1 + np.arange(P, dtype=np.float32)), init.max(0) + 0.002 * (1 + np.arange(P, dtype=np.float32))
    make = lambda **kw: ParameterFitter(model, n_samples=f["S"], max_rays=f["images"] * f["rays"], lrate=f["lrate"], **kw)
    free, bounded = make(), make(bounds=(low, high))
    pf, _ = free.fit(batch, loss, init, 5)
    pb, _ = bounded.fit(batch, loss, init, 5)
    pf, pb = pf.cpu().numpy(), pb.cpu().numpy()
    assert ((pf < low) | (pf > high)).any(), "the free fit stays inside the bounds: they bind nothing"
    assert (pb >= low).all() and (pb <= high).all() and not np.array_equal(pb, init)
    second = dict(batch, **{k: np.ascontiguousarray(np.asarray(batch[k])[:, ::-1]) for k in ("rays_o", "rays_d", "t", "cone_scale", "color", "alpha")})
    p3, history = free.fit([batch, second], loss, init, 3)
    params = torch.as_tensor(init, dtype=torch.float32).to(p3.device).clone().requires_grad_(True)
    opt, by_hand = torch.optim.Adam([params], lr=f["lrate"]), []
    for b in (batch, second, batch):
        v, g = free.step(b, loss, params.detach())
        params.grad = g.clone()
        opt.step()
        by_hand.append(float(v.item()))
    assert np.array_equal(p3.cpu().numpy(), params.detach().cpu().numpy()) and history == by_hand and history[0] != history[1]
    p0, h0 = free.fit(batch, loss, init, 0)
    assert h0 == [] and np.array_equal(p0.cpu().numpy(), init) and p0.dtype == torch.float32
    assert unchanged(free, model, blob) and unchanged(bounded, model, blob)


def test_parameters_too_small_are_refused():
    """`gradients_step` counts the floats of `parameters` before any pointer is taken: one row or one column short of
    ceil(n / rays_per_param_row) x P raises ValueError, as does `ParameterFitter.fit` from a start with a column missing -- the encoder and the fold
    would read past the tensor.  What the step before left stays as it was."""
    from nerf_tex_amd.fit import ParameterFitter
    model, spec, wts, batch, kn, seed = pgc.case_setup(pgc.ROW_EDGE_CASES[0])                  # 20 rays in rows of 7: 3 rows of 7 parameters
    ro, rd, t, cone, rows, color, alpha = batch
    assert rows.shape == (3, 7)
    tr = trainer_of(model, spec, kn)
    before = step(tr, batch, kn, seed)
    for short in (rows[:-1], rows[:, :-1]):
        with pytest.raises(ValueError, match="floats"):
            step(tr, (ro, rd, t, cone, np.ascontiguousarray(short), color, alpha), kn, seed)
        assert np.array_equal(tr.parameter_gradients().cpu().numpy(), before[2])
    step(tr, (ro, rd, t, cone, np.concatenate([rows, rows]), color, alpha), kn, seed)           # more rows than the step reads: taken as before
    assert np.array_equal(tr.parameter_gradients().cpu().numpy(), before[2])
    f = pgc.FIT
    model, spec, wts, images, true, init = pgc.fit_setup()
    fitter = ParameterFitter(model, n_samples=f["S"], max_rays=f["images"] * f["rays"])
    for bad in (init[:, :-1], np.concatenate([init, init[:, :1]], 1)):
        with pytest.raises(ValueError, match="columns"):
            fitter.fit(images, make_loss(f["loss_name"])[1], np.ascontiguousarray(bad), 1)
