"""Training steps of more than 1024 rays on the GPU against float64: the instanced step's live compaction beyond one ray per scan thread
(`live_scan_kernel`: `per = ceil(n_rays / 1024)` rays a thread) on both instanced back ends, and whole-ray steps of the three trainers where
`loss_sum_kernel` adds a second ray per thread and every grid sized by the ray count (dirrow_kernel, the composites, the parameter and ray folds,
the jitter's and the noise's keys) passes 1024.  Many SHORT rays: a step has a few thousand samples.  The fixtures, and why each size is
there: tests/many_rays_common.py; tests/test_train_many_rays.py holds every one of them inside the guards of its bars on the CPU.  The bars are
the project's own: `clc.check_layers`, `pgc.check_param_gradients`, `igc.check_input_gradients`, 1e-5 on a loss, 1e-4 on predictions, and
`np.array_equal` where bits are compared.  `-m gpu`."""

import numpy as np
import pytest

from tests import custom_loss_common as clc
from tests import fused_grad_common as fgc
from tests import fused_instanced_common as fic
from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import many_rays_common as mrc
from tests import param_grad_common as pgc
from tests.train_common import make_loss, rel_linf, restated_step, step_noise, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


# ---- 1. instanced steps ----------------------------------------------------------------------------------------------------------------------
def inst_trainer(backend, model, n, S, pm=False, im=False, max_rays=None):
    if backend == "chain":
        return fic.chain_trainer(fic.CASES[0], model, n, S, pm, im, max_rays=max_rays)
    from nerf_tex_amd.train import FlexTrainer
    return FlexTrainer(model, max_rays=max_rays or n, n_samples=max(S, 2), perturb=False, param_gradients=pm, input_gradients=im)


def checked_step(backend, setup, pm=False, im=False):
    """An instanced step on a fresh trainer of the back end, held to the float64 restatement branched by the trainer's kept signs -- the chain's
    by `fic.checked_step`, the layer-by-layer trainer's as tests/test_gpu_train_instanced.checked_step holds it -- and `last_live` to the host's
    live order.  Returns (trainer, pred, gradient, want, f32, head, patterns)."""
    from tests import test_gpu_train_instanced as gti
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    if backend == "chain":
        out = fic.checked_step(setup, fic.CASES[0], pm, im)
    else:
        tr = inst_trainer(backend, model, n, S, pm, im)
        head = itc.quadratic_head(n)
        pred, got, val = fic.step(tr, bufs, hit, cone, kn, head)
        pat = gti.patterns(tr, spec, bufs, hit, kn)
        want, f32 = gti.restate_both(spec, w, bufs, hit, cone, okw, head, pat)
        print(f"flex: {n} x {S}, {tr.last_live} live: loss {val:.9g} want {want.loss:.9g}")
        gti.check_pred(pred, want, f32)
        assert np.all(pred[~hit] == 0)
        clc.check_layers(got, spec, want, f32)
        out = (tr, pred, got, want, f32, head, pat)
    assert out[0].last_live == len(itc.live_order(hit, bufs[3])) == len(out[3].live)
    return out


def check_samples(tr, setup, want, f32, head, pat):
    """The per-sample parameter and input gradients of the step `tr` has just taken, as tests/test_gpu_fused_instanced.py::test_gradient_modes
    holds them, and exactly 0 at every sample that is not live."""
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    P = want.param_grad.shape[-1]
    live = itc.live_mask(hit, bufs[3])
    pg, ig = fic.sample_results(tr)
    assert pg.shape == (n, S, P) and np.all(pg[~live] == 0) and np.all(want.param_grad[~live] == 0)
    pgc.check_param_gradients(pg.reshape(-1, P), want.param_grad.reshape(-1, P), f32.param_grad.reshape(-1, P), rows=live.reshape(-1))
    assert ig[0].shape == ig[1].shape == (n, S, 3) and np.all(ig[0][~live] == 0) and np.all(ig[1][~live] == 0)
    w64 = igc.restated_sample_gradients(w, spec, bufs, hit, cone, head, **okw, **pat)
    w32 = igc.restated_sample_gradients(w, spec, bufs, hit, cone, head, dtype=torch.float32, **okw, **pat)
    igc.check_input_gradients(ig, w64[2:], w32[2:], rows=live.reshape(-1))


@pytest.mark.parametrize("n", mrc.INST_SIZES)
@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_random_buffers_beyond_one_ray_per_scan_thread(backend, n):
    """n x 3 random instancer buffers at 1023 (the last scan thread's range empty), 1024 (the largest per = 1), 1025 (per = 2: a one-ray last
    range, 511 threads beyond the end), 2049 (per = 3, a thread whose first ray is n_rays) and 3000 (a ragged per = 3): predictions, every
    layer's kernel and bias gradient and `last_live` against float64."""
    setup = mrc.inst_setup(backend, n)
    live = mrc.check_random_buffers(setup)
    tr = checked_step(backend, setup)[0]
    assert tr.last_live == live > 64


@pytest.mark.parametrize("n", mrc.MODE_SIZES)
@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_per_sample_gradients_follow_row_of(backend, n):
    """dL/d params_map [n, 3, P] and dL/d pts, rays_d_map [n, 3, 3] at 1024 (per = 1) and 2049 (per = 3) rays: a wrong first row of a ray puts a
    sample's gradient on another sample, which nothing else shows as plainly."""
    setup = mrc.inst_setup(backend, n)
    tr, pred, got, want, f32, head, pat = checked_step(backend, setup, pm=True, im=True)
    check_samples(tr, setup, want, f32, head, pat)


@pytest.mark.parametrize("name", mrc.MASKS)
@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_explicit_live_masks_at_three_rays_a_scan_thread(backend, name):
    """2049 x 3, 683 non-empty scan ranges: the live samples in ray 0 alone, in the last ray alone (the third ray of thread 682's range), every
    sample of every ray, every other scan range fully live, exactly one live sample in the first ray of every range."""
    setup, mask = mrc.mask_setup(backend, name)
    live = mrc.check_mask(setup, mask, name)
    tr = checked_step(backend, setup)[0]
    assert tr.last_live == live
    if name == "every_sample":
        assert tr.last_live == mrc.MASK_N * mrc.INST_S


def bits(tr, setup, head):
    model, spec, w, bufs, hit, cone, kn, okw = setup
    pred, got, _ = fic.step(tr, bufs, hit, cone, kn, head)
    pg, ig = fic.sample_results(tr)
    return [pred, got, pg] + list(ig)


@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_a_step_depends_on_neither_the_capacity_nor_the_batch(backend):
    """2049 rays on a trainer made for 2049 and on one made for 4100: the same bits in the predictions, the weight gradients and the
    per-sample gradients.  Rays 0 .. 1023 of that step predict the bits of a 1024-ray step on the first 1024 rays' buffers."""
    setup = mrc.inst_setup(backend, 2049)
    model, S = setup[0], mrc.INST_S
    head = itc.quadratic_head(2049)
    exact, roomy = (inst_trainer(backend, model, 2049, S, True, True, max_rays=cap) for cap in (2049, 4100))
    first = bits(exact, setup, head)
    assert len(first) == 5 and all(np.abs(x).max() > 0 for x in first)
    for a, b in zip(first, bits(roomy, setup, head)):
        assert np.array_equal(a, b)
    front = mrc.first_rays(setup, 1024)
    small = inst_trainer(backend, model, 1024, S)
    pred, _, _ = fic.step(small, front[3], front[4], front[5], front[6], itc.quadratic_head(1024))
    assert small.last_live > 64 and np.abs(pred).max() > 0 and np.array_equal(first[0][:1024], pred)


# ---- 2. whole-ray steps ----------------------------------------------------------------------------------------------------------------------
def whole_trainer(fx):
    from nerf_tex_amd import train
    return getattr(train, fx.cls)(fx.model, max_rays=fx.n, n_samples=fx.S, perturb=fx.perturb, blur_idx=fx.blur, raw_noise_std=fx.noise_std)


def whole_step(fx, tr):
    """(loss, [color | alpha]) of one `gradients_step` of a fixture."""
    ro, rd, t, cone, params, color, alpha = fx.batch
    val, cp, ap = tr.gradients_step(ro, rd, t, params, cone, color, alpha, make_loss(fx.loss_name)[1], seed=fx.seed)
    torch.cuda.synchronize()
    return float(val.item()), step_pred(cp, ap)


def whole_restated(fx, tr, dtype, like=None):
    """The step `tr` has just taken, restated on the signs it kept: `restated_step` beside a chain (or IPE) trainer, its layer-by-layer and
    branch counterparts beside the others (`like`: the float64 restatement whose patterns the float32 one takes)."""
    from tests.train_flex_common import restated_flex_step
    from tests.train_branch_oracle import restated_branch_step
    ro, rd, t, cone, params, color, alpha = fx.batch
    args = (tr, fx.spec, fx.wts, ro, rd, t, params, cone, color, alpha, fx.okw)
    kw = dict(seed=fx.seed, perturb=fx.perturb, noise_std=fx.noise_std, miss=fx.miss, blur_idx=fx.blur, dtype=dtype)
    if fx.cls == "Trainer":
        return restated_step(*args, **kw)
    if like is not None:
        kw.update(masks=like.masks, sigma_mask=like.sigma_mask)
    if fx.cls == "FlexTrainer":
        return restated_flex_step(*args, **kw)
    return restated_branch_step(*args, branch_masks=None if like is None else like.branch_masks, **kw)


def check_whole_step(fx, tr=None):
    """A fixture's step against float64 as tests/test_gpu_train.py::test_gradients_at_the_configs_batch holds one -- the loss within 1e-5, the
    predictions within 1e-4 -- and every layer's gradient by `clc.check_layers`; missed rays predict exactly 0.  Returns (trainer, loss, want)."""
    tr = tr or whole_trainer(fx)
    val, pred = whole_step(fx, tr)
    want = whole_restated(fx, tr, torch.float64)
    f32 = whole_restated(fx, tr, torch.float32, want)
    e_loss, e_pred = abs(val - want.loss) / abs(want.loss), rel_linf(pred, want.pred)
    print(f"{fx.trainer} {fx.id}: loss {val:.9g} want {want.loss:.9g} rel {e_loss:.2e} (float32 {abs(f32.loss - want.loss) / abs(want.loss):.2e}) | "
          f"pred {e_pred:.2e} (float32 {rel_linf(f32.pred, want.pred):.2e})")
    assert e_loss <= 1e-5, e_loss
    assert e_pred <= 1e-4, e_pred
    clc.check_layers(want.got, fx.spec, want, f32)
    assert np.all(pred[fx.miss] == 0) and np.all(want.pred[fx.miss] == 0)
    return tr, val, want


@pytest.mark.parametrize("trainer,case", mrc.WHOLE_RUNS, ids=mrc.WHOLE_RUN_IDS)
def test_whole_ray_steps(trainer, case):
    """The chain, the layer-by-layer trainer (width 98, skips [1, 3]) and the branch trainer at 1025 x 2 (jittered depths), 2500 x 3 (30 missed
    rays: the front, either side of ray 1024, the back) and 1025 x 32 (raw_noise_std 0.1; the chain's hoisted build), under AlphaLoss(smape, mse)
    and NerfLoss(mse); the IPE chain at 1025 x 2 with blur_idx 0.  At 2500 rays `loss_sum_kernel`'s threads add up to three rays each: the loss
    is the float64 mean of the rays' terms to 1e-5, and a second step gives its bits again."""
    fx = mrc.whole_setup(trainer, case)
    tr, val, _ = check_whole_step(fx)
    if fx.n == 2500:
        assert fx.miss.sum() == len(mrc.MISS_2500)
        again, _ = whole_step(fx, tr)
        assert again == val


def test_the_direction_rows_of_1025_rays_per_ray_and_per_sample(monkeypatch):
    """1025 x 32 on the chain with the per-ray direction segment (dirrow_kernel on 1025 rays, its n_rays x 1024-byte buffer in the forward chain)
    and with the per-sample path forced by the environment: both against float64, and the same gradients bit for bit, as
    tests/test_gpu_train.py::test_direction_segment_per_ray_and_per_sample_agree has it at 48 rays."""
    fx = mrc.whole_setup("chain", mrc.NO_HOIST_CASE)
    assert fx.S % 32 == 0 and fx.blur is None
    _, _, per_ray = check_whole_step(fx)
    monkeypatch.setenv("NERFTEX_TRAIN_NO_DIR_HOIST", "1")
    _, _, per_sample = check_whole_step(fx)
    monkeypatch.delenv("NERFTEX_TRAIN_NO_DIR_HOIST")
    assert np.array_equal(per_ray.got, per_sample.got)


# ---- parameter and ray gradients ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", mrc.GRAD_IDS)
@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_parameter_and_ray_gradients(backend, cid):
    """dL/d parameter rows at 1025 rays in rows of 256 (five rows, the last of one ray) and at 2500 rays with a row per ray, and dL/d rays_o,
    rays_d [n, 3], on the chain and on the layer-by-layer trainer: per column at `pgc.check_param_gradients`' bar; the 30 missed rays' rows
    of all three are exactly 0."""
    model, spec, wts, batch, kn, seed = mrc.grad_setup(backend, cid)
    n, S = kn["n"], kn["S"]
    if backend == "chain":
        tr = fgc.chain_trainer(model, kn)
    else:
        from nerf_tex_amd.train import FlexTrainer
        tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=kn["perturb"], blur_idx=kn["blur"], raw_noise_std=kn["noise_std"], map_exr=kn["map_exr"],
                         param_gradients=True, input_gradients=True)
    val, pred, rays, pg = fgc.step(tr, batch, kn, seed)
    noise = step_noise(n, S, seed, kn["noise_std"])
    patterns = clc.chain_patterns(tr, n, S, noise) if backend == "chain" else pgc.trainer_patterns(tr, spec, n, S, noise)
    want = mrc.grad_restate(spec, wts, batch, kn, seed, torch.float64, patterns)
    f32 = mrc.grad_restate(spec, wts, batch, kn, seed, torch.float32, patterns)
    print(f"{backend} {cid}: {n} x {S}, {kn['rpr']} rays a row: loss {val:.9g} want {want[0]:.9g}")
    assert abs(val - want[0]) <= 1e-5 * abs(want[0])
    n_rows = -(-n // kn["rpr"])
    row_hit, ray_hit = mrc.grad_rows(kn, n_rows)
    assert pg.shape == want[1].shape == (n_rows, spec.n_params) and pg.dtype == np.float32 and np.isfinite(pg).all()
    assert rays[0].shape == rays[1].shape == (n, 3) and np.isfinite(rays[0]).all() and np.isfinite(rays[1]).all()
    if row_hit is not None:
        assert (~ray_hit).sum() == len(mrc.MISS_2500) and not pg[~row_hit].any() and not rays[0][~ray_hit].any() and not rays[1][~ray_hit].any()
        assert not want[1][~row_hit].any() and not want[2][~ray_hit].any() and not want[3][~ray_hit].any()
    pgc.check_param_gradients(pg, want[1], f32[1], rows=row_hit)
    igc.check_input_gradients(rays, want[2:], f32[2:], rows=ray_hit)
