"""dL/d material parameters of the layer-by-layer training step (`ntx_trainer_enable_param_gradients`, `FlexTrainer(param_gradients=...)`,
`nerf_tex_amd.fit.ParameterFitter`) on the GPU against float64 autograd of the restated step with the parameter rows as the
leaf (tests/param_grad_common.py), branched by the signs of the activations the trainer kept.  The bar is the project's standing one per
parameter column -- rel-Linf <= max(1e-4, 4 x floor), the floor what float32 autograd of the same restatement is off by, under the guards
floor <= 5e-4 and max |grad| > 1e-6; tests/test_param_gradients.py shows every case here to meet the guards on the CPU.  `-m gpu`."""

import numpy as np
import pytest

from tests import param_grad_common as pgc
from tests.train_common import BKGD, make_loss, step_noise, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
N, S = pgc.N_RAYS, pgc.N_SAMPLES


def trainer_of(model, spec, kn, mode=True, max_rays=N, n_samples=S):
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer
    cls = BranchTrainer if pgc.has_branches(spec) else FlexTrainer
    return cls(model, max_rays=max_rays, n_samples=n_samples, perturb=kn["perturb"], blur_idx=kn["blur"], raw_noise_std=kn["noise_std"], map_exr=kn["map_exr"],
               param_gradients=mode)


def step(tr, batch, kn, seed):
    """One `gradients_step` of a case; (loss, [color | alpha], dL/d rows) on the host."""
    ro, rd, t, cone, rows, color, alpha = batch
    _, loss = make_loss(kn["loss_name"])
    val, cp, ap = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, composite_bkgd=kn["bkgd"], bkgd_color=BKGD, seed=seed, rays_per_param_row=kn["rpr"], n_samples=S)
    pg = tr.parameter_gradients() if tr.param_gradients else None
    torch.cuda.synchronize()
    return float(val.item()), step_pred(cp, ap), None if pg is None else pg.cpu().numpy()


def run_case(case, rows=None):
    """A case's step, its parameter gradients held to the bar; returns (trainer, got, the float64 restatement)."""
    model, spec, wts, batch, kn, seed = pgc.case_setup(case)
    tr = trainer_of(model, spec, kn)
    val, pred, got = step(tr, batch, kn, seed)
    patterns = pgc.trainer_patterns(tr, spec, N, S, step_noise(N, S, seed, kn["noise_std"]))
    want = pgc.restate(spec, wts, batch, kn, seed, S, torch.float64, *patterns)
    f32 = pgc.restate(spec, wts, batch, kn, seed, S, torch.float32, *patterns)
    print(f"{case[0]}: loss {val:.9g} want {want[0]:.9g}; rows {got.shape}")
    assert got.shape == want[2].shape == (-(-N // kn["rpr"]), spec.n_params)
    assert abs(val - want[0]) <= 1e-5 * abs(want[0])
    pgc.check_param_gradients(got, want[2], f32[2], rows=rows)
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
