"""dL/d parameters and dL/d rays_o, rays_d on the fused 8 x 256 chain (`ntx_trainer_enable_gradients`, `Trainer(param_gradients=,
input_gradients=)`, `trainer_for(..., fused=True)`, `ParameterFitter(fused=True)`) on the GPU, against the float64
restatements of tests/param_grad_common.py and tests/input_grad_common.py branched by the signs of the activations the chain kept
(tests/custom_loss_common.chain_patterns).  The bar is the project's standing one per parameter column and per ray-gradient column:
rel-Linf <= max(1e-4, 4 x floor), the floor what float32 autograd of the same restatement is off by, under the guards floor <= 5e-4 and
max |grad| > 1e-6; tests/test_fused_gradients.py shows every case here to sit 2x inside the guards on the CPU.  Every case has un-normalised
rays_d.  The measured figures: profiles/fused_gradients/errors.md.  `-m gpu`."""

from unittest import mock

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro
from tests import custom_loss_common as clc
from tests import fused_grad_common as fgc
from tests import input_grad_common as igc
from tests import param_grad_common as pgc
from tests.train_common import F, make_loss, rel_linf, step_noise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def run_case(case, pm=True, im=True):
    """A case's step at its own size with both gradients in one step, held to the bar; returns (trainer, spec, wts, batch, knobs, seed, rays, pg)."""
    model, spec, wts, batch, kn, seed = fgc.case_setup(case)
    assert (np.abs(np.linalg.norm(batch[1], axis=1) - 1) > 1e-3).any()
    tr = fgc.chain_trainer(model, kn, pm, im)
    val, pred, rays, pg = fgc.step(tr, batch, kn, seed)
    fgc.held_to_the_bar(tr, spec, wts, batch, kn, seed, val, rays, pg, case[0])
    return tr, spec, wts, batch, kn, seed, rays, pg


# ---- 1. parity at 70 x 33 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fgc.PARITY_CASES, ids=[c[0] for c in fgc.PARITY_CASES])
def test_both_gradients_match_float64_autograd(case):
    """70 rays x 33 samples = 72 blocks of 32 and a tail of 6, modes (1, 1): carpet (Kp 72, Kd 81), grass, grass_filtered with blur_idx 0 under
    perturb and noise (Kp 81), blur_idx on an appearance parameter (no per-ray direction hoist), the narrowest encodings (one partial tile
    each), Kp = Kd = 90, and a width-128 network padded into the chain."""
    tr = run_case(case)[0]
    assert type(tr).__name__ == "Trainer" and np.abs(tr.gradients()).max() > 1e-6


# ---- 2. sample counts around a block ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fgc.SAMPLE_CASES, ids=[c[0] for c in fgc.SAMPLE_CASES])
def test_sample_counts_around_a_block(case):
    """The step's minimum (1 ray x 2 samples: 30 rows of the block are not written), exactly one block, one block and one sample, S = 64 (the
    forward's hoist on) and S = 65 (blocks that straddle rays, hoist off)."""
    run_case(case)


# ---- 3. more blocks than one pass of the kernel's grid ---------------------------------------------------------------------------------------
def test_a_batch_that_wraps_the_grid_is_its_two_halves():
    """feat_grad_kernel's grid is at most 2 workgroups x 4 waves per CU, a wave a block of 32 samples at a time: R = 256 rays x 256 samples are
    2048 blocks, one pass of 256 CUs; 2 R rays wrap it.  forward / backward with fixed random cotangents, a parameter row per ray: the batch
    of 2 R rays gives, bit for bit, the ray and parameter gradients of its two halves run as two batches -- on a trainer made for 2 R rays and
    on one made for 4 R."""
    from tests.train_flex_common import flex_batch
    R, S = 256, 256
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * R * S // 32 > 8 * cus, "the large batch has to wrap the grid"
    case = fgc.CASE["carpet_1_6"]
    model, spec, wts, _, kn, seed = fgc.case_setup(case)
    ro, rd, t, cone, rows, _, _ = flex_batch(3, 2 * R, S, spec, "carpet")
    rd = igc.unnormalised(rd, 3)
    rng = np.random.default_rng(2)
    dc, da = (rng.normal(size=(2 * R, 3)) / R).astype(F), (rng.normal(size=2 * R) / R).astype(F)

    def run(tr, sl):
        tr.forward(ro[sl], rd[sl], t[sl], rows[sl], cone[sl], seed=seed, rays_per_param_row=1, n_samples=S)
        tr.backward(dc[sl], da[sl])
        rays, pg = fgc.results(tr)
        return np.concatenate([rays[0], rays[1], pg], 1)

    first = None
    for cap in (2 * R, 4 * R):
        tr = fgc.chain_trainer(model, dict(kn, perturb=False), max_rays=cap, n_samples=S)
        whole = run(tr, slice(None))
        halves = np.concatenate([run(tr, slice(0, R)), run(tr, slice(R, 2 * R))], 0)
        assert whole.shape == (2 * R, 6 + 7) and np.isfinite(whole).all() and (np.abs(whole).max(0) > 1e-7).all()
        assert np.array_equal(whole, halves), cap
        first = whole if first is None else first
        assert np.array_equal(whole, first), cap
        del tr


# ---- 4. rows and misses ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fgc.ROW_CASES, ids=[c[0] for c in fgc.ROW_CASES])
def test_parameter_rows(case):
    """A parameter row per ray, two rows of 35 rays, one row of all 70."""
    pg = run_case(case)[7]
    assert pg.shape == (-(-70 // case[5]["rpr"]), 7)


def test_rays_that_miss_get_exact_zeros():
    """`pgc.MISS_RAYS` at t = inf with cone_scale NaN and +inf in turn, under blur_idx (the fold reads cone_scale): their rows of both ray
    gradients and the all-missed parameter row are exactly 0 (`held_to_the_bar`), and nothing anywhere is non-finite."""
    tr, spec, wts, batch, kn, seed, rays, pg = run_case(fgc.MISS_CASE)
    cone = batch[3][kn["miss"]]
    assert np.isnan(cone).any() and np.isposinf(cone).any() and not np.isfinite(cone).any()
    assert kn["miss"][35:].all() and not pg[1].any() and np.abs(pg[0]).max() > 1e-6
    assert np.isfinite(pg).all() and np.isfinite(rays[0]).all() and np.isfinite(rays[1]).all() and np.isfinite(tr.gradients()).all()


# ---- 5. modes ------------------------------------------------------------------------------------------------------------------------------------
def test_modes():
    """One batch on one trainer that has already stepped, (0,0) -> (1,0) -> (2,0) -> (0,1) -> (1,1) -> (0,0): loss and predictions are the same
    bits in every state, the weight gradient is a twin's (both modes off from its creation) bit for bit unless a mode is 2 -- then the
    pre-filled gradient buffer is untouched and the three entries that use a weight gradient return NTX_E_INVALID --, whatever gradient a state
    takes meets the bar and is the same bits whenever it is taken again, and the getter of a gradient that is off refuses."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import Trainer
    model, spec, wts, batch, kn, seed = fgc.case_setup(fgc.CASE["carpet_1_6"])
    other = tuple(np.ascontiguousarray(a[::-1]) if i in (5, 6) else a for i, a in enumerate(batch))
    twin = Trainer(model, max_rays=kn["n"], n_samples=kn["S"], perturb=False)
    v0, p0, none_r, none_p = fgc.step(twin, batch, kn, seed)
    w0 = twin.gradients()
    assert none_r is None and none_p is None and np.abs(w0).max() > 1e-6
    tr = fgc.chain_trainer(model, kn, False, False)
    fgc.step(tr, other, kn, seed + 1)
    fill = np.full(tr.n_weights, 7, F)
    seen = {}
    for pm, im in ((False, False), (True, False), ("only", False), (False, True), (True, True), (False, False)):
        tr.set_gradients(pm, im)
        assert (tr.param_gradients, tr.input_gradients) == (pm, im)
        tr._set(_lib.TRAINER_GRADIENTS, fill)
        v, p, rays, pg = fgc.step(tr, batch, kn, seed)
        only = "only" in (pm, im)
        assert v == v0 and np.array_equal(p, p0), (pm, im)
        assert np.array_equal(tr.gradients(), fill if only else w0), (pm, im)
        assert (rays is None) == (im is False) and (pg is None) == (pm is False)
        if pm or im:
            fgc.held_to_the_bar(tr, spec, wts, batch, kn, seed, v, rays, pg, f"modes {pm} {im}")
        for key, got in (("pg", pg), ("rays", rays)):
            if got is not None:
                got = np.concatenate(got, 1) if key == "rays" else got
                assert np.array_equal(got, seen.setdefault(key, got)), (key, pm, im)
        for off, getter in ((pm is False, tr.parameter_gradients), (im is False, tr.ray_gradients)):
            if off:
                with pytest.raises(_lib.NtxError) as e:
                    getter()
                assert e.value.code == _lib.NTX_E_INVALID
        with torch.cuda.device(0):
            rc_all = _lib.lib.ntx_trainer_allreduce_gradients(tr._h, None, None)     # (no communicator: NTX_E_INVALID either way)
            rc_stash = _lib.lib.ntx_trainer_stash_gradients(tr._h, 0, None)
        assert rc_all == _lib.NTX_E_INVALID and (rc_stash == _lib.NTX_E_INVALID) == only, (pm, im)
        if only:
            assert b"only" in _lib.lib.ntx_last_error()
            with pytest.raises(_lib.NtxError) as e:
                tr.apply_gradients()
            assert e.value.code == _lib.NTX_E_INVALID and tr.iterations == 0
    assert set(seen) == {"pg", "rays"}
    # mode 2 of the inputs, and of both
    for pm, im in ((False, "only"), ("only", "only")):
        tr.set_gradients(pm, im)
        tr._set(_lib.TRAINER_GRADIENTS, fill)
        v, p, rays, pg = fgc.step(tr, batch, kn, seed)
        assert v == v0 and np.array_equal(p, p0) and np.array_equal(tr.gradients(), fill)
        assert np.array_equal(np.concatenate(rays, 1), seen["rays"]) and (pg is None or np.array_equal(pg, seen["pg"]))
    tr.set_gradients(True, True)                                                       # the same step twice: the same bits
    a, b = fgc.step(tr, batch, kn, seed), fgc.step(tr, batch, kn, seed)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[2], b[2])) and np.array_equal(a[3], b[3]) and np.array_equal(a[3], seen["pg"])
    tr.apply_gradients()
    assert tr.iterations == 1


def test_a_mode_change_drops_the_pending_forward():
    """forward, a change of either mode, backward: NTX_E_INVALID.  The same modes set again keep it."""
    from nerf_tex_amd import _lib
    model, spec, wts, batch, kn, seed = fgc.case_setup(fgc.CASE["samples_1x33"])
    ro, rd, t, cone, rows, color, alpha = batch
    tr = fgc.chain_trainer(model, kn, True, False)
    dc, da = np.ones((kn["n"], 3), F), np.ones(kn["n"], F)
    fwd = lambda: tr.forward(ro, rd, t, rows, cone, seed=seed, rays_per_param_row=kn["rpr"], n_samples=kn["S"])
    fwd(); tr.set_gradients(True, False); tr.backward(dc, da)
    assert tr.parameter_gradients().abs().max() > 0
    for change in ((True, True), (False, True), (False, False), ("only", False)):
        fwd(); tr.set_gradients(*change)
        with pytest.raises(_lib.NtxError) as e:
            tr.backward(dc, da)
        assert e.value.code == _lib.NTX_E_INVALID, change
        tr.set_gradients(True, False)


# ---- 6. the kernel alone ---------------------------------------------------------------------------------------------------------------------
def test_the_kernel_alone():
    """After a (1, 1) step at 70 x 33: slots 40 / 41 (G_pos [n, Kp], G_dir [n, Kd]) against the float64 product of the trainer's OWN kept
    gradients (slots 20, 25, 28) and weights -- rel-Linf <= 2e-6 sqrt(K), K = 512 for G_pos and 256 for G_dir: tests/test_gpu_gemm.py's bar
    for an f32 contraction.  Before any step under a mode, and with both modes off again, the slots refuse."""
    from nerf_tex_amd import _lib
    model, spec, wts, batch, kn, seed = fgc.case_setup(fgc.CASE["carpet_1_6"])
    M = kn["n"] * kn["S"]
    tr = fgc.chain_trainer(model, kn, False, False)
    fgc.step(tr, batch, kn, seed)
    for state in ((False, False), (True, True)):                                       # off; on, but no step yet
        tr.set_gradients(*state)
        with pytest.raises(_lib.NtxError) as e:
            tr.activation(40, M)
        assert e.value.code == _lib.NTX_E_INVALID
    fgc.step(tr, batch, kn, seed)
    torch.cuda.synchronize()
    w0, w5, wc1 = (np.asarray(w, np.float64) for w in fgc.layer_kernels(spec, wts))
    Kp, Kd = model.pos_map_dim, model.dir_map_dim
    dy0, dy5, dc1o = (tr.activation(k, M).astype(np.float64) for k in (20, 25, 28))
    want_pos, want_dir = fgc.feature_gradients(dy0, dy5, dc1o, w0, w5, wc1, Kp, Kd)
    got_pos, got_dir = tr.activation(40, M), tr.activation(41, M)
    assert got_pos.shape == (M, Kp) and got_dir.shape == (M, Kd) and (Kp, Kd) == (72, 81)
    e_pos, e_dir = rel_linf(got_pos, want_pos), rel_linf(got_dir, want_dir)
    print(f"FGERR kernel alone: G_pos rel-Linf {e_pos:.3e} (bar {2e-6 * np.sqrt(512):.3e}), G_dir {e_dir:.3e} (bar {2e-6 * np.sqrt(256):.3e})")
    assert (np.abs(want_pos).max(0) > 0).all() and (np.abs(want_dir).max(0) > 0).all()
    assert e_pos <= 2e-6 * np.sqrt(512) and e_dir <= 2e-6 * np.sqrt(256)
    # per column as well: a wrong row of W or a dropped term in one tile cannot hide behind the largest column
    col = lambda g, w: (np.abs(g - w).max(0) / np.abs(w).max(0)).max()
    assert col(got_pos, want_pos) <= 2e-6 * np.sqrt(512) and col(got_dir, want_dir) <= 2e-6 * np.sqrt(256)


# ---- 7. through the ops -----------------------------------------------------------------------------------------------------------------------
def test_through_the_autograd_op():
    """`DifferentiableRender(chain trainer)` under `CharbonnierAlpha`: parameters.grad, rays_o.grad and rays_d.grad at the bar against the two
    yardsticks under that loss; another torch term on the parameters adds its own gradient exactly."""
    from nerf_tex_amd.autograd import DifferentiableRender
    dev = torch.device("cuda", 0)
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev).float()
    model, spec, wts, batch, kn, seed = fgc.case_setup(fgc.CASE["carpet_1_6"])
    ro, rd, t, cone, rows, color, alpha = batch
    n, S = kn["n"], kn["S"]
    loss = clc.CharbonnierAlpha()
    tr = fgc.chain_trainer(model, kn)
    o, dd, p = d(ro).requires_grad_(True), d(rd).requires_grad_(True), d(rows).requires_grad_(True)
    c, a = DifferentiableRender(tr)(o, dd, t, p, cone, seed=seed, rays_per_param_row=kn["rpr"], n_samples=S)
    val = loss(color_true=d(color), alpha_true=d(alpha), color_pred=c, alpha_pred=a)
    (val + 0.01 * (p ** 2).sum() + 0.003 * p.sum()).backward()
    pg = tr.parameter_gradients()
    assert pg.abs().max() > 1e-6 and torch.allclose(p.grad, pg + (0.02 * p.detach() + 0.003), rtol=1e-6, atol=1e-8)
    go, gd = tr.ray_gradients()
    assert torch.equal(o.grad, go) and torch.equal(dd.grad, gd)
    patterns = clc.chain_patterns(tr, n, S, None)
    want = fgc.restate_under(loss, spec, wts, batch, kn, seed, torch.float64, patterns)
    f32 = fgc.restate_under(loss, spec, wts, batch, kn, seed, torch.float32, patterns)
    assert abs(float(val.item()) - want[0]) <= 1e-5 * abs(want[0])
    res = pgc.check_param_gradients(pg.cpu().numpy(), want[1], f32[1])
    print(f"FGERR op parameters worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")
    res = igc.check_input_gradients((o.grad.cpu().numpy(), dd.grad.cpu().numpy()), want[2:], f32[2:])
    print(f"FGERR op rays worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """Checked before anything is placed, and a refused call leaves both modes as they were: a mode outside 0..2 (NTX_E_INVALID), parameter
    gradients of a model without parameters (NTX_E_INVALID; its input gradients are taken), an IPE chain handle (NTX_E_UNSUPPORTED), an
    instanced step on a chain handle (NTX_E_UNSUPPORTED, as before).  The two old entries refuse a chain handle before and after the new one
    has enabled it, and the class pickers answer as before without `fused`."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import FlexTrainer, Trainer, trainer_class_for, trainer_for
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    lib = _lib.lib
    model, spec, wts, batch, kn, seed = fgc.case_setup(fgc.CASE["samples_1x33"])
    tr = fgc.chain_trainer(model, kn, False, False)
    old = lambda: (lib.ntx_trainer_enable_param_gradients(tr._h, 1), lib.ntx_trainer_enable_input_gradients(tr._h, 2))
    assert old() == (_lib.NTX_E_UNSUPPORTED, _lib.NTX_E_UNSUPPORTED) and b"ntx_trainer_create_flex" in lib.ntx_last_error()
    with pytest.raises(ValueError):
        tr.set_gradients(2, False)
    tr.set_gradients(True, True)
    assert old() == (_lib.NTX_E_UNSUPPORTED, _lib.NTX_E_UNSUPPORTED)
    for pm, im in ((3, 0), (0, 3), (-1, 1), (1, -1)):
        assert lib.ntx_trainer_enable_gradients(tr._h, pm, im) == _lib.NTX_E_INVALID
    v, p, rays, pg = fgc.step(tr, batch, kn, seed)                                      # both modes are what they were
    assert rays is not None and pg is not None and np.abs(pg).max() > 0
    inst = lib.ntx_train_forward_instanced(tr._h, *[None] * 10, 1, 2, -1, 1.0, 1.0, 0, None, None, None, None, None)
    assert inst == _lib.NTX_E_UNSUPPORTED and b"instanced" in lib.ntx_last_error()
    # a model without parameters
    bare, bspec, _ = make_model((0, 0), dense_media=True)
    assert trainer_class_for(bare) is Trainer
    nb = Trainer(bare, max_rays=8, n_samples=33, perturb=False)
    assert lib.ntx_trainer_enable_gradients(nb._h, 1, 1) == _lib.NTX_E_INVALID and b"no parameters" in lib.ntx_last_error()
    with pytest.raises(_lib.NtxError) as e:
        nb.ray_gradients()                                                             # the refused call enabled nothing
    assert e.value.code == _lib.NTX_E_INVALID
    nb.set_gradients(False, True)
    ro, rd, t, cone, _, color, alpha = flex_batch(3, 8, 33, bspec, "carpet")
    nb.gradients_step(ro, igc.unnormalised(rd, 3), t, None, cone, color, alpha, make_loss("nerf_mse")[1], seed=seed)
    go, gd = nb.ray_gradients()
    assert go.shape == (8, 3) and torch.isfinite(go).all() and torch.isfinite(gd).all() and go.abs().max() > 0
    # an IPE chain handle
    ipe, _, _ = make_model((1, 6), kind="IPE")
    mip = Trainer(ipe, max_rays=8, n_samples=8, blur_idx=0)
    for pm, im in ((1, 0), (0, 2), (2, 2)):
        assert lib.ntx_trainer_enable_gradients(mip._h, pm, im) == _lib.NTX_E_UNSUPPORTED and b"IPE" in lib.ntx_last_error()
    assert lib.ntx_trainer_enable_gradients(mip._h, 0, 0) == _lib.NTX_OK
    with pytest.raises(_lib.NtxError) as e:
        Trainer(ipe, max_rays=8, n_samples=8, blur_idx=0, input_gradients=True)
    assert e.value.code == _lib.NTX_E_UNSUPPORTED
    # the pickers
    assert trainer_class_for(model, param_gradients=True) is FlexTrainer and trainer_class_for(model, param_gradients=True, fused=True) is Trainer
    assert type(trainer_for(model, max_rays=8, n_samples=8, param_gradients="only")) is FlexTrainer
    fused = trainer_for(model, max_rays=8, n_samples=8, param_gradients="only", fused=True)
    assert type(fused) is Trainer and fused.param_gradients == "only" and fused.input_gradients is False
    plain = trainer_for(model, max_rays=8, n_samples=8, fused=True)
    assert type(plain) is Trainer and plain.param_gradients is False


def test_the_entry_on_a_layer_by_layer_handle():
    """On a `FlexTrainer`, `set_gradients(pm, im)` (the new entry) is `set_param_gradients(pm)` then `set_input_gradients(im)` (the two old
    ones): the same bits in every gradient, for every pair of modes, and a Nerf's parameter gradients are refused as there."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import FlexTrainer
    from tests.common import make_model
    model, spec, wts, batch, kn, seed = igc.case_setup(igc.ARCH_CASES[0])
    make = lambda: FlexTrainer(model, max_rays=kn["n"], n_samples=kn["S"], perturb=kn["perturb"])
    new, old = make(), make()
    for pm in (False, True, "only"):
        for im in (False, True, "only"):
            new.set_gradients(pm, im)
            old.set_param_gradients(pm); old.set_input_gradients(im)
            assert (new.param_gradients, new.input_gradients) == (old.param_gradients, old.input_gradients) == (pm, im)
            a, b = fgc.step(new, batch, kn, seed), fgc.step(old, batch, kn, seed)
            assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(new.gradients(), old.gradients()), (pm, im)
            assert (a[2] is None) == (im is False) and (a[3] is None) == (pm is False)
            assert a[2] is None or all(np.array_equal(x, y) and np.abs(x).max() > 1e-6 for x, y in zip(a[2], b[2])), (pm, im)
            assert a[3] is None or (np.array_equal(a[3], b[3]) and np.abs(a[3]).max() > 1e-6), (pm, im)
    nerf, _, _ = make_model((0, 0), kind="Nerf", arch=dict(width=64, depth=3, skips=[1]))
    bare = FlexTrainer(nerf, max_rays=8, n_samples=8)
    assert _lib.lib.ntx_trainer_enable_gradients(bare._h, 1, 0) == _lib.NTX_E_INVALID
    bare.set_gradients(False, "only")
    assert bare.input_gradients == "only" and _lib.lib.ntx_trainer_stash_gradients(bare._h, 0, None) == _lib.NTX_E_INVALID


# ---- 9. ParameterFitter(fused=True) --------------------------------------------------------------------------------------------------------------
def test_fitting_parameters_on_the_chain():
    """A [1, 4] 8 x 256 teacher renders 2 images x 128 rays x 32 samples at known parameters; `ParameterFitter(fused=True)` and
    `ParameterFitter(fused=False)` start 0.2 off.  The first step's loss agrees to 1e-5, its gradient per column within the sum of the two
    trainers' bars (2 x max(1e-4, 4 floors) of the restatement on the chain's patterns), and after 150 Adam steps the chain's loss is at most
    2 x the layer-by-layer fitter's: 150 Adam steps amplify gradient differences of 1e-4."""
    from nerf_tex_amd.fit import ParameterFitter
    from nerf_tex_amd.train import FlexTrainer, Trainer
    f = pgc.FIT
    with mock.patch.dict(pgc.FIT, arch=None):
        model, spec, wts, batch, true, init = pgc.fit_setup()
    assert (spec.depth, spec.width, tuple(spec.skips)) == (8, 256, (4,))
    B, R, S = pgc.FIT["images"], pgc.FIT["rays"], pgc.FIT["S"]
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    rd = igc.unnormalised(batch["rays_d"].reshape(B * R, 3), 3)                         # the teacher again, on un-normalised directions
    with torch.no_grad():
        c, a = tro.render([t64(x) for x in wts], spec, t64(batch["rays_o"].reshape(B * R, 3)), t64(rd), t64(orc.z_values(batch["t"].reshape(B * R, 2), S, F)),
                          t64(np.repeat(true, R, 0)), t64(batch["cone_scale"].reshape(B * R)))
    batch = dict(batch, rays_d=rd.reshape(B, R, 3), color=c.numpy().astype(F).reshape(B, R, 3), alpha=a.numpy().astype(F).reshape(B, R))
    B, R, S = f["images"], f["rays"], f["S"]
    okw, loss = make_loss(f["loss_name"])
    make = lambda fused: ParameterFitter(model, n_samples=S, max_rays=B * R, lrate=f["lrate"], fused=fused)
    chain, flex = make(True), make(False)
    assert type(chain.trainer) is Trainer and type(flex.trainer) is FlexTrainer and chain.trainer.param_gradients == "only"
    blob = np.array(model.get_blob(), np.float32, copy=True)
    (v_c, g_c), (v_f, g_f) = chain.step(batch, loss, init), flex.step(batch, loss, init)
    v_c, v_f, g_c, g_f = float(v_c.item()), float(v_f.item()), g_c.cpu().numpy(), g_f.cpu().numpy()
    assert abs(v_c - v_f) <= 1e-5 * abs(v_f)
    flat = lambda k, *s: np.asarray(batch[k]).reshape(B * R, *s)
    patterns = clc.chain_patterns(chain.trainer, B * R, S, None)
    args = (wts, spec, flat("rays_o", 3), flat("rays_d", 3), orc.z_values(flat("t", 2), S, F), init, R, flat("cone_scale"), flat("color", 3), flat("alpha"), okw)
    kw = dict(masks=patterns[0], sigma_mask=patterns[2])
    want = pgc.restated_param_gradients(*args, dtype=torch.float64, **kw)
    f32 = pgc.restated_param_gradients(*args, dtype=torch.float32, **kw)
    res = pgc.check_param_gradients(g_c, want[2], f32[2])
    between = np.abs(g_c.astype(np.float64) - g_f).max(0) / np.abs(want[2]).max(0)
    print(f"FGERR fitter first gradient: chain vs float64 {res.errs.max():.2e}, chain vs layer by layer {between.max():.2e}")
    assert (between <= 2 * np.maximum(1e-4, 4 * res.floors)).all(), (between, res.floors)
    (p_c, l_c), (p_f, l_f) = chain.fit(batch, loss, init, f["n_iters"]), flex.fit(batch, loss, init, f["n_iters"])
    ratio = l_c[-1] / l_f[-1]
    print(f"FGERR fitter: chain {l_c[0]:.4e} -> {l_c[-1]:.4e}, layer by layer {l_f[0]:.4e} -> {l_f[-1]:.4e}, final ratio {ratio:.4f}; "
          f"|p - true| {np.abs(init - true).max():.3f} -> {np.abs(p_c.cpu().numpy() - true).max():.3f}")
    assert len(l_c) == f["n_iters"] and np.isfinite(l_c).all() and l_c[-1] < l_c[0]
    assert l_c[-1] <= 2 * l_f[-1], (l_c[-1], l_f[-1])
    assert np.array_equal(chain.weights(), blob)


# ---- 10. coarse + fine ---------------------------------------------------------------------------------------------------------------------------
def test_coarse_and_fine_passes_on_one_chain():
    """`CoarseFineTrainer(..., fused=True, param_gradients=True)` on one shared chain-shaped network, 24 + 16 samples, perturb, 24 rays in rows of
    12: between the passes `parameter_gradients()` is the coarse pass's, after the step the fine pass's (on the merged depths the sampler
    left); both at the bar, and the weight gradients are a twin's without parameter gradients bit for bit."""
    from nerf_tex_amd.train import CoarseFineTrainer, Trainer
    model, spec, wts, batch, kn, seed = fgc.case_setup(fgc.COARSE_CASE)
    ro, rd, t, cone, rows, color, alpha = batch
    n, S, NI = kn["n"], kn["S"], 16
    _, loss = make_loss(kn["loss_name"])
    tr = CoarseFineTrainer(model, None, max_rays=n, n_samples=S, n_importance=NI, perturb=True, param_gradients=True, fused=True)
    twin = CoarseFineTrainer(model, None, max_rays=n, n_samples=S, n_importance=NI, perturb=True)
    assert type(tr.fine) is Trainer and tr.coarse is tr.fine and type(twin.fine) is Trainer and tr.fine.param_gradients is True
    seen = {}

    def on_coarse():
        seen["got"] = tr.coarse.parameter_gradients().cpu().numpy()
        seen["want"] = fgc.held_to_the_bar(tr.coarse, spec, wts, batch, kn, seed, None, None, seen["got"], name="coarse pass")

    out = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, seed=seed, rays_per_param_row=kn["rpr"], on_coarse=on_coarse)
    got_fine = tr.fine.parameter_gradients().cpu().numpy()
    z = tr.last_z.cpu().numpy()
    assert z.shape == (n, S + NI) and (np.diff(z, axis=1) >= 0).all()
    want_fine = fgc.held_to_the_bar(tr.fine, spec, wts, batch, dict(kn, S=S + NI, z=z), seed, None, None, got_fine, name="fine pass")
    val, want_val = float(out[0].item()), seen["want"][0] + want_fine[0]
    assert abs(val - want_val) <= 1e-5 * abs(want_val)
    assert not np.array_equal(seen["got"], got_fine)
    out2 = twin.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, seed=seed, rays_per_param_row=kn["rpr"])
    assert float(out2[0].item()) == val and np.array_equal(twin.last_z.cpu().numpy(), z)
    assert np.array_equal(twin.fine.gradients(), tr.fine.gradients()) and np.abs(tr.fine.gradients()).max() > 1e-6
