"""Opt-in bf16x6 training on the GPU (`ntx_trainer_set_precision`, `FlexTrainer(..., precision="bf16x6")`): the layer-by-layer step with every
contraction on the 16-bit matrix cores, held to the SAME gates as the float32 step -- tests/train_flex_common.check_against_float64 (loss 1e-5,
predictions and every layer's gradient max(1e-4, 4 float32 floors) of float64 autograd), its twin for parameter branches, and the standing
checkers of the parameter, input and instanced gradients.  Then what a precision switch must not disturb: reproducibility, the float32 step
bit for bit after a switch back, and the refusals.  `-m gpu`.  Durations: profiles/bf16x6/notes.md."""

import numpy as np
import pytest

from tests import custom_loss_common as clc
from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests import train_branch_oracle as bro
from tests.common import make_model
from tests.train_common import make_loss, step_pred
from tests.train_flex_common import ARCHS, check_against_float64, flex_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
BK = (1., .5, .25)
X6 = "bf16x6"


def one_step(model, spec, wts, fam, n, S, loss_name, *, bkgd=False, map_exr=False, perturb=False, blur=None, noise_std=0.0, seed=11, batch_seed=3):
    """tests/test_gpu_train_flex.one_step with the trainer in bf16x6: a `gradients_step` on a seeded batch, checked by `check_against_float64`"""
    from nerf_tex_amd.train import FlexTrainer
    ro, rd, t, cone, params, color, alpha = flex_batch(batch_seed, n, S, spec, fam)
    okw, loss = make_loss(loss_name)
    tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=perturb, blur_idx=blur, raw_noise_std=noise_std, map_exr=map_exr, precision=X6)
    assert tr.precision == X6
    val, cp, ap = tr.gradients_step(ro, rd, t, params if params.shape[1] else None, cone, color, alpha, loss, composite_bkgd=bkgd, bkgd_color=BK, seed=seed)
    torch.cuda.synchronize()
    check_against_float64(tr, spec, float(val.item()), step_pred(cp, ap), (wts, ro, rd, t, params, cone, color, alpha, okw),
                          dict(seed=seed, perturb=perturb, noise_std=noise_std, miss=np.zeros(n, bool), blur_idx=blur, bkgd=bkgd, bkgd_color=BK, map_exr=map_exr))
    return tr


PLAIN = ["chain_arch", "w98_d5_skips13", "nerf_w64_d3_skip1", "color_depth0"]


@pytest.mark.parametrize("arch_id", PLAIN)
def test_gradients_of_every_layer_match_float64_autograd(arch_id):
    """One step at 45 rays x 37 samples (1665 samples: off the 128-row tile and off 32): the chain's own shape, width 98 (odd leading dimensions:
    the unaligned path), a Nerf of width 64, a model without colour layers -- with the knobs the float32 test gives them."""
    from tests.test_gpu_train_flex import KNOBS
    _, npar, kind, arch, fam = [a for a in ARCHS if a[0] == arch_id][0]
    model, spec, wts = make_model(npar, kind=kind, dense_media=True, arch=arch)
    one_step(model, spec, wts, fam, 45, 37, **KNOBS[arch_id])


def test_parameter_branches():
    """A BranchTrainer with param_depth 2 (the branch wider than the trunk), against the branch oracle's twin of the gate."""
    from nerf_tex_amd.train import BranchTrainer
    case = [c for c in bro.GPU_CASES if c[0] == "f_branch_wider_than_trunk"][0]
    model, spec, wts, batch, kn, seed = bro.case_setup(case)
    assert spec.param_layers == 2
    ro, rd, t, cone, params, color, alpha = batch
    n, S = bro.N_RAYS, bro.N_SAMPLES
    okw, loss = make_loss(kn["loss_name"])
    tr = BranchTrainer(model, max_rays=n, n_samples=S, perturb=kn["perturb"], blur_idx=kn["blur"], raw_noise_std=kn["noise_std"], map_exr=kn["map_exr"], precision=X6)
    val, cp, ap = tr.gradients_step(ro, rd, t, params, cone, color, alpha, loss, composite_bkgd=kn["bkgd"], bkgd_color=BK, seed=seed)
    torch.cuda.synchronize()
    bro.check_against_float64(tr, spec, float(val.item()), step_pred(cp, ap), (wts, ro, rd, t, params, cone, color, alpha, okw),
                              dict(seed=seed, perturb=kn["perturb"], noise_std=kn["noise_std"], miss=np.zeros(n, bool), blur_idx=kn["blur"], bkgd=kn["bkgd"], bkgd_color=BK,
                                   map_exr=kn["map_exr"]))


@pytest.mark.parametrize("n,S", [(41, 70), (239, 64)])
def test_the_weight_gradients_split(n, S):
    """2870 samples: two ranges of the weight gradients (2048 + 822); 15 296: eight (the last of 960), which take the XCD-major tile numbering."""
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(width=64, depth=3))
    assert -(-n * S // 2048) in (2, 8)
    one_step(model, spec, wts, "carpet", n, S, "alpha_smape", perturb=True)


def test_parameter_and_input_gradients_together():
    """The 64 x 3 model with `param_gradients=True` and `input_gradients=True`: dL/d parameter rows and dL/d rays against the float64
    restatements of tests/param_grad_common.py and tests/input_grad_common.py, at their standing bars."""
    from nerf_tex_amd.train import FlexTrainer
    from tests.test_gpu_input_gradients import held_to_the_bar as rays_held, step
    model, spec, wts, batch, kn, seed = igc.case_setup(("x6_both", *pgc.SMALL, dict(), (11, 3)))
    tr = FlexTrainer(model, max_rays=kn["n"], n_samples=kn["S"], perturb=kn["perturb"], blur_idx=kn["blur"], raw_noise_std=kn["noise_std"], map_exr=kn["map_exr"],
                     param_gradients=True, input_gradients=True, precision=X6)
    val, pred, rays, pg = step(tr, batch, kn, seed)
    rays_held(tr, spec, wts, batch, kn, seed, val, rays, "x6_both")
    n, S = kn["n"], kn["S"]
    from tests.train_common import step_noise
    patterns = pgc.trainer_patterns(tr, spec, n, S, step_noise(n, S, seed, kn["noise_std"]))
    want = pgc.restate(spec, wts, batch, kn, seed, torch.float64, *patterns)
    f32 = pgc.restate(spec, wts, batch, kn, seed, torch.float32, *patterns)
    assert pg.shape == want[2].shape and np.abs(pg).max() > 1e-6
    pgc.check_param_gradients(pg, want[2], f32[2])


def test_an_instanced_step():
    """One instanced step on tests/instanced_train_common.py's buffers, about a third of the samples live: predictions and every layer's
    gradient at the instanced float32 test's bars."""
    from nerf_tex_amd import train
    from tests.test_gpu_train_instanced import check_pred, patterns, restate_both, step
    case = itc.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    live = itc.live_mask(hit, bufs[3]).sum()
    assert 0.15 * n * S < live < 0.5 * n * S
    tr = getattr(train, case[1])(model, max_rays=n, n_samples=S, perturb=False, blur_idx=case[4], map_exr=kn["map_exr"], precision=X6)
    head = itc.quadratic_head(n)
    pred, got, val = step(tr, bufs, hit, cone, kn, head)
    assert tr.last_live == live
    want, f32 = restate_both(spec, w, bufs, hit, cone, okw, head, patterns(tr, spec, bufs, hit, kn))
    check_pred(pred, want, f32, "bf16x6 instanced")
    clc.check_layers(got, spec, want, f32)


def small_step(tr, batch, seed=11):
    ro, rd, t, cone, params, color, alpha = batch
    val, cp, ap = tr.gradients_step(ro, rd, t, params, cone, color, alpha, make_loss("alpha_smape")[1], seed=seed)
    torch.cuda.synchronize()
    return np.float32(val.item()), cp.cpu().numpy(), ap.cpu().numpy(), tr.gradients()


def test_reproducible_and_the_round_trip_to_float32():
    """The same bf16x6 step twice: the same bits (and other bits than float32's: the switch does something).  `set_precision("float32")`
    behind it: bit for bit the step of a trainer that never left float32."""
    from nerf_tex_amd.train import FlexTrainer
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(width=64, depth=3))
    n, S = 75, 41                                                                # 3075 samples: ragged, two ranges of the weight gradients
    batch = flex_batch(7, n, S, spec, "carpet")
    fresh = small_step(FlexTrainer(model, max_rays=n, n_samples=S, perturb=True), batch)
    tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=True, precision=X6)
    first, again = small_step(tr, batch), small_step(tr, batch)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert np.abs(first[3]).max() > 1e-6 and not np.array_equal(first[3], fresh[3])
    assert np.abs(first[3] - fresh[3]).max() <= 2e-4 * np.abs(fresh[3]).max()         # both lie within 1e-4 of float64
    tr.set_precision("float32")
    assert tr.precision == "float32"
    back = small_step(tr, batch)
    assert all(np.array_equal(a, b) for a, b in zip(back, fresh))
    tr.set_precision(X6)
    assert all(np.array_equal(a, b) for a, b in zip(small_step(tr, batch), first))


def test_refusals():
    """A chain handle refuses (NTX_E_UNSUPPORTED) and then steps as before; fp16x3 is unsupported, another value invalid; between `forward` and
    `backward` the precision stays (NTX_E_INVALID) and the pending backward still works."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import FlexTrainer, Trainer
    model, spec, wts = make_model((1, 6), dense_media=True)
    n, S = 24, 16
    batch = flex_batch(3, n, S, spec, "carpet")
    ro, rd, t, cone, params, color, alpha = batch
    with pytest.raises(_lib.NtxError) as e:
        Trainer(model, max_rays=n, n_samples=S, perturb=False, precision=X6)
    assert e.value.code == _lib.NTX_E_UNSUPPORTED
    chain = Trainer(model, max_rays=n, n_samples=S, perturb=False)
    before = small_step(chain, batch)
    with pytest.raises(_lib.NtxError) as e:
        chain.set_precision(X6)
    assert e.value.code == _lib.NTX_E_UNSUPPORTED and chain.precision == "float32" and _lib.lib.ntx_trainer_precision(chain._h) == 0
    assert all(np.array_equal(a, b) for a, b in zip(small_step(chain, batch), before))

    small, sspec, _ = make_model((1, 6), dense_media=True, arch=dict(width=64, depth=3))
    tr = FlexTrainer(small, max_rays=n, n_samples=S, perturb=False)
    assert _lib.lib.ntx_trainer_precision(tr._h) == 0
    assert _lib.lib.ntx_trainer_set_precision(tr._h, 1) == _lib.NTX_E_UNSUPPORTED
    for bad in (3, -1, 7):
        assert _lib.lib.ntx_trainer_set_precision(tr._h, bad) == _lib.NTX_E_INVALID
    assert _lib.lib.ntx_trainer_precision(tr._h) == 0
    tr.set_precision(X6)
    assert _lib.lib.ntx_trainer_precision(tr._h) == 2
    whole = small_step(tr, batch)
    cf, af = tr.forward(ro, rd, t, params, cone, seed=11)
    with pytest.raises(_lib.NtxError) as e:
        tr.set_precision("float32")
    assert e.value.code == _lib.NTX_E_INVALID and tr.precision == X6 and _lib.lib.ntx_trainer_precision(tr._h) == 2
    dc, da = torch.full_like(cf, 1e-3), torch.full_like(af, -2e-3)
    tr.backward(dc, da)
    torch.cuda.synchronize()
    pending = tr.gradients()
    tr.forward(ro, rd, t, params, cone, seed=11)                                   # the same forward and backward, nothing between them
    tr.backward(dc, da)
    torch.cuda.synchronize()
    assert np.array_equal(pending, tr.gradients()) and np.abs(pending).max() > 1e-9 and np.array_equal(cf.cpu().numpy(), whole[1])
    tr.set_precision("float32")                                                    # between steps it is taken
    assert _lib.lib.ntx_trainer_precision(tr._h) == 0


def test_the_keyword_reaches_the_trainer_from_configs_pairs_and_fitters():
    """A config's top-level `precision` key: the carpet block as written gets a FlexTrainer in bf16x6 (the chain's own shape), and without the
    key the chain's `Trainer` as before; `CoarseFineTrainer(**kw)` and `ParameterFitter(..., precision=...)` pass the keyword on; `trainer_for`
    with `fused=True` raises."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.fit import ParameterFitter
    from nerf_tex_amd.train import CoarseFineTrainer, FlexTrainer, Trainer, trainer_for
    from tests.test_gpu_train_flex import carpet_config
    tr, _ = Trainer.from_config(dict(carpet_config(), precision=X6), max_rays=8)
    assert type(tr) is FlexTrainer and tr.precision == X6 and _lib.lib.ntx_trainer_precision(tr._h) == 2
    tr, _ = Trainer.from_config(dict(carpet_config(), precision="float32"), max_rays=8)
    assert type(tr) is Trainer and tr.precision == "float32"
    model = make_model((1, 6), dense_media=True, arch=dict(width=64, depth=3))[0]
    pair = CoarseFineTrainer(model, max_rays=8, n_samples=8, n_importance=4, precision=X6)
    assert [t.precision for t in pair.trainers] == [X6]
    fit = ParameterFitter(make_model((1, 6), dense_media=True)[0], n_samples=8, max_rays=8, precision=X6)
    assert type(fit.trainer) is FlexTrainer and fit.trainer.precision == X6 and fit.trainer.param_gradients == "only"
    with pytest.raises(_lib.NtxError) as e:
        trainer_for(make_model((1, 6), dense_media=True)[0], max_rays=8, n_samples=8, precision=X6, fused=True)
    assert e.value.code == _lib.NTX_E_UNSUPPORTED
