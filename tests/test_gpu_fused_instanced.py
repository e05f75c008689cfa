"""The instanced step on the fused 8 x 256 chain on the GPU (`ntx_trainer_enable_instanced`, `Trainer(instanced=True)`,
`DifferentiableInstanceRender` over a chain trainer) against the float64 restatement of tests/instanced_train_common.py branched by the
chain's kept signs.  tests/test_fused_instanced.py holds every case 2x inside the guards on the CPU.  `-m gpu`."""

import numpy as np
import pytest

from tests import fused_instanced_common as fic
from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests.common import make_model
from tests.train_common import BKGD, F, rel_linf

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def bits(tr, bufs, hit, cone, kn, head, **kw):
    """(pred, gradient, per-sample parameter gradients, per-sample input gradients) of one instanced step, for bit comparisons."""
    pred, got, _ = fic.step(tr, bufs, hit, cone, kn, head, **kw)
    pg, ig = fic.sample_results(tr)
    return [pred, got] + ([pg] if pg is not None else []) + (list(ig) if ig is not None else [])


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fic.CASES, ids=fic.CASE_IDS)
def test_parity_with_the_float64_restatement(case):
    """Predictions, every layer's kernel and bias gradient and slot 30 (the adjoint over the compact rows) against float64 branched by the
    chain's kept signs; the direct difference to a `FlexTrainer` instanced step on the same buffers is printed, not gated."""
    setup = itc.case_setup(case)
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    assert (~hit).any() and (~itc.live_mask(hit, bufs[3])[hit]).all(1).any()
    tr, pred, got, want, f32, head, _ = fic.checked_step(setup, case)
    assert tr.last_live > 64
    flex = fic.flex_trainer(case, model, n, S)
    fpred, fgot, _ = fic.step(flex, bufs, hit, cone, kn, head)
    assert flex.last_live == tr.last_live
    print(f"against FlexTrainer on the same buffers: pred {rel_linf(pred, fpred):.2e} gradient {rel_linf(got, fgot):.2e}")


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", itc.EDGES, ids=itc.EDGE_IDS)
def test_sample_and_live_count_edges(edge):
    """n_live 0, 1, 31, 32, 33 (a block of 32 rows) and 2047, 2048, 2049 by an explicit live mask; S = 1, 64, 65, 130 (the composite's chunk
    of 64).  n_live = 0: the predictions are the appended sample's alone and every weight gradient is exactly 0."""
    setup = fic.edge_setup(edge)
    tr, pred, got, want, f32, _, _ = fic.checked_step(setup, fic.CASES[0])
    if edge[1] == "live":
        assert tr.last_live == edge[2]
    if tr.last_live == 0:
        assert not got.any() and np.abs(want.grad).max() == 0 and np.abs(pred).max() > 0


# ---- 3. nothing is read where nothing is live ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [fic.CASE["grass_filtered_blur_geo"], fic.CASE["grass_filtered_blur_app"]], ids=["blur_geo", "blur_app"])
def test_nothing_is_read_at_a_sample_that_is_not_live(case):
    """NaN in pts / rays_d_map / t / alpha_weight / params_map at every sample that is not live, NaN / inf in cone_scale and in the cotangents
    of the rays that are not hit: every result -- predictions, weight gradients, per-sample parameter and input gradients -- is bit for bit
    the clean run's; rays that are not hit predict 0 / 0."""
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    live = itc.live_mask(hit, bufs[3])
    dead = np.nonzero(~hit)[0]
    assert len(dead) and (bufs[3][dead] > 0).any()
    spoiled = list(bufs)
    for k in (0, 1, 2, 6, 9):
        b = np.array(spoiled[k], copy=True)
        b[~live] = np.nan
        spoiled[k] = b
    cone2 = cone.copy()
    cone2[dead[::2]] = np.nan; cone2[dead[1::2]] = np.inf
    tr = fic.chain_trainer(case, model, n, S, pm=True, im=True)
    head = itc.quadratic_head(n)
    clean = bits(tr, bufs, hit, cone, kn, head)
    for value in (float("nan"), float("inf")):
        dirty = bits(tr, tuple(spoiled), hit, cone2, kn, head, spoil=(torch.as_tensor(dead, device=fic.dev()), value))
        assert all(np.isfinite(x).all() for x in dirty) and same_bits(clean, dirty)
    assert np.all(clean[0][dead] == 0) and np.abs(clean[1]).max() > 0 and len(clean) == 5


# ---- 4. no residue, nothing else changes ------------------------------------------------------------------------------------------------------
def test_no_residue_and_plain_steps_are_unchanged():
    """On one enabled handle: plain step, instanced step with many live rows, instanced step with few, plain step.  Each is bit for bit
    (loss, predictions, gradients) the same step on a fresh handle, and the plain steps are bit for bit a never-enabled twin's."""
    from tests import fused_grad_common as fgc
    case = fic.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    few_mask = np.zeros(n * S, bool)
    few_mask[np.random.default_rng(9).choice(n * S, 45, replace=False)] = True
    few_bufs, few_hit = itc.with_live_mask(bufs, hit, few_mask.reshape(n, S))
    pcase = ("plain", (1, 6), None, None, "carpet", dict(n=n, S=S, rpr=1), (11, 3))
    _, _, _, batch, pkn, seed = fgc.case_setup(pcase)
    head = itc.quadratic_head(n)
    make = lambda enabled: fic.chain_trainer(case, model, n, S, instanced=enabled)

    def plain(tr):
        val, pred, _, _ = fgc.step(tr, batch, pkn, seed)
        return [np.float32(val), pred, tr.gradients()]
    runs = [plain, lambda tr: bits(tr, bufs, hit, cone, kn, head), lambda tr: bits(tr, few_bufs, few_hit, cone, kn, head), plain]
    one = make(True)
    seq = [run(one) for run in runs]
    assert one.last_live == 45
    for i, run in enumerate(runs):
        assert same_bits(seq[i], run(make(True))), i
    twin = make(False)
    assert same_bits(seq[0], plain(twin)) and same_bits(seq[3], plain(twin))
    assert np.abs(seq[1][1]).max() > 0 and np.abs(seq[2][1]).max() > 0 and not same_bits(seq[1], seq[2])


# ---- 5. gradient modes -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("modes", fic.MODES, ids=[f"param{p}_input{i}" for p, i in fic.MODES])
@pytest.mark.parametrize("case", fic.MODE_CASES, ids=[c[0] for c in fic.MODE_CASES])
def test_gradient_modes(case, modes):
    """`sample_parameter_gradients()` [N, S, P] and `sample_input_gradients()` ([N, S, 3] twice) at the existing bars against
    `itc.restated` / `igc.restated_sample_gradients`, exact zeros where the sample is not live; mode 1's weight gradients are bit for bit mode
    0's; under a mode 2 the gradient buffer is untouched and `apply_gradients` raises; the plain getters refuse after an instanced step."""
    from nerf_tex_amd import _lib
    setup = itc.case_setup(case)
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    P = sum(case[2])
    name = {0: False, 1: True, 2: "only"}
    pm, im = name[modes[0]], name[modes[1]]
    tr = fic.chain_trainer(case, model, n, S, pm, im)
    marker = np.arange(tr.n_weights, dtype=F)
    tr._set(_lib.TRAINER_GRADIENTS, marker)
    tr, pred, got, want, f32, head, pat = fic.checked_step(setup, case, tr=tr)
    live = itc.live_mask(hit, bufs[3])
    pg, ig = fic.sample_results(tr)
    if pm:
        assert pg.shape == (n, S, P) and np.all(pg[~live] == 0) and np.all(want.param_grad[~live] == 0)
        pgc.check_param_gradients(pg.reshape(-1, P), want.param_grad.reshape(-1, P), f32.param_grad.reshape(-1, P), rows=live.reshape(-1))
        with pytest.raises(_lib.NtxError) as e:
            tr.parameter_gradients()
        assert e.value.code == _lib.NTX_E_INVALID
    if im:
        assert ig[0].shape == ig[1].shape == (n, S, 3) and np.all(ig[0][~live] == 0) and np.all(ig[1][~live] == 0)
        w64 = igc.restated_sample_gradients(w, spec, bufs, hit, cone, head, **okw, **pat)
        w32 = igc.restated_sample_gradients(w, spec, bufs, hit, cone, head, dtype=torch.float32, **okw, **pat)
        igc.check_input_gradients(ig, w64[2:], w32[2:], rows=live.reshape(-1))
        with pytest.raises(_lib.NtxError) as e:
            tr.ray_gradients()
        assert e.value.code == _lib.NTX_E_INVALID
    # the feature gradients' slots over the compact rows
    assert tr.activation(40, tr.last_live).shape == (tr.last_live, model.pos_map_dim) and tr.activation(41, tr.last_live).shape == (tr.last_live, model.dir_map_dim)
    if 2 in modes:
        assert np.array_equal(got, marker)
        with pytest.raises(_lib.NtxError) as e:
            tr.apply_gradients()
        assert e.value.code == _lib.NTX_E_INVALID
    else:
        plain = fic.chain_trainer(case, model, n, S)
        pred0, got0, _ = fic.step(plain, bufs, hit, cone, kn, head)
        assert np.array_equal(got0, got) and np.array_equal(pred0, pred) and np.abs(got).max() > 0


# ---- 6. reproducibility -----------------------------------------------------------------------------------------------------------------------------
def test_a_step_is_reproducible_and_does_not_depend_on_the_capacity():
    case = fic.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    head = itc.quadratic_head(n)
    small, large = (fic.chain_trainer(case, model, n, S, pm=True, im=True, max_rays=cap) for cap in (23, 64))
    first = bits(small, bufs, hit, cone, kn, head)
    assert len(first) == 5 and all(np.abs(x).max() > 0 for x in first)
    assert same_bits(first, bits(small, bufs, hit, cone, kn, head))
    assert same_bits(first, bits(large, bufs, hit, cone, kn, head))


# ---- 7. refusals and state ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_state():
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import FlexTrainer, Trainer
    from tests.test_gpu_train_instanced import raw_args
    lib, INV, UNS = _lib.lib, _lib.NTX_E_INVALID, _lib.NTX_E_UNSUPPORTED
    case = fic.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case, n=9, S=12)
    n, S = bufs[3].shape
    stream = torch.cuda.current_stream(fic.dev()).cuda_stream
    ones = torch.ones((n, 3), device=fic.dev())
    alive = []

    def fwd(tr, **over):
        kept, args = raw_args(bufs, hit, cone, **over)
        alive.append(kept)
        return lib.ntx_train_forward_instanced(tr._h, *args)
    back = lambda tr: lib.ntx_train_backward(tr._h, ones.data_ptr(), None, stream)
    # an IPE chain handle: refused, and it stays refused
    ipe_model, _, _ = make_model((1, 6), kind="IPE")
    ipe = Trainer(ipe_model, max_rays=n, n_samples=S, perturb=False, blur_idx=0)
    assert lib.ntx_trainer_enable_instanced(ipe._h) == UNS
    with pytest.raises(_lib.NtxError) as e:
        Trainer(ipe_model, max_rays=n, n_samples=S, perturb=False, blur_idx=0, instanced=True)
    assert e.value.code == UNS
    # a chain handle that never asked: the refusal of before, with the message that names the layer-by-layer entries
    plain = Trainer(model, max_rays=n, n_samples=S, perturb=False)
    assert fwd(plain) == UNS and b"ntx_trainer_create_flex" in lib.ntx_last_error()
    # a layer-by-layer handle: NTX_OK, nothing changes
    flex = FlexTrainer(model, max_rays=n, n_samples=S, perturb=False, instanced=True)
    assert lib.ntx_trainer_enable_instanced(flex._h) == 0 and fwd(flex) == 0 and back(flex) == 0
    # enabled, twice
    tr = Trainer(model, max_rays=n, n_samples=S, perturb=False, instanced=True)
    tr.enable_instanced()
    assert lib.ntx_trainer_enable_instanced(tr._h) == 0
    assert back(tr) == INV
    assert fwd(tr) == 0
    assert lib.ntx_train_backward(tr._h, None, None, stream) == INV and back(tr) == 0 and back(tr) == INV      # NULL d_color leaves it pending; one backward per forward
    for over in (dict(S=0), dict(S=1025), dict(n=n + 1), dict(n=0), dict(patch_scale=0.0), dict(patch_scale=-1.0), dict(blur=0, cone=None), dict(blur=0, t=None),
                 dict(blur=sum(case[2])), dict(flags=_lib.FLAG_PERTURB), dict(flags=_lib.FLAG_RAW_NOISE), dict(rd=None), dict(pts=None), dict(dists=None), dict(cl=None),
                 dict(al=None), dict(hit=None), dict(pm=None)):
        assert fwd(tr, **over) == INV, over
        assert back(tr) == INV, over
    assert fwd(tr, aw=None) == 0 and fwd(tr, t=None, cone=None) == 0 and back(tr) == 0
    big = itc.case_setup(case, n=9, S=13)
    keep2, args2 = raw_args(big[3], big[4], big[5])
    assert lib.ntx_train_forward_instanced(tr._h, *args2) == INV                                               # n x S beyond the capacity although either fits
    torch.cuda.synchronize()


# ---- 8. the Python surface -------------------------------------------------------------------------------------------------------------------------
def test_differentiable_instance_render_over_the_chain():
    """`params_map.grad` is `sample_parameter_gradients()` (plus the caller's own term), `pts.grad` / `rays_d_map.grad` are
    `sample_input_gradients()`; the weight gradient is the plain pair's."""
    from nerf_tex_amd.autograd import DifferentiableInstanceRender
    case = fic.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    tr = fic.chain_trainer(case, model, n, S, pm=True, im=True)
    head = itc.quadratic_head(n)
    pred, got, _ = fic.step(tr, bufs, hit, cone, kn, head)
    native_pg = tr.sample_parameter_gradients()
    native_pts, native_dirs = tr.sample_input_gradients()
    render = DifferentiableInstanceRender(tr, itc.PATCH_SCALE, density_scale=kn["density_scale"], density_reweighting=kn["density_reweighting"])
    regulariser = lambda p: 0.01 * (p ** 2).sum() + 0.003 * p.sum()
    leaf = lambda a: torch.tensor(np.nan_to_num(a), device=fic.dev(), requires_grad=True)
    field, pts, dirs = leaf(bufs[9]), leaf(bufs[1]), leaf(bufs[0])
    tensors = (dirs, pts) + tuple(bufs[2:9]) + (field,)
    c, a = render(tensors, cone, params_map=field, hit=hit, composite_bkgd=kn["composite_bkgd"], bkgd_color=BKGD)
    (head(c, a) + regulariser(field)).backward()
    torch.cuda.synchronize()
    own, = torch.autograd.grad(regulariser(f2 := leaf(bufs[9])), f2)
    assert native_pg.abs().max() > 0 and native_pts.abs().max() > 0 and native_dirs.abs().max() > 0
    assert torch.equal(field.grad, native_pg + own) and torch.equal(pts.grad, native_pts) and torch.equal(dirs.grad, native_dirs)
    assert np.array_equal(tr.gradients(), got)
    assert np.array_equal(np.concatenate([c.detach().cpu().numpy(), a.detach().cpu().numpy()[:, None]], -1), pred)


def test_twenty_adam_steps_against_a_teacher_lower_the_loss():
    """128 rays x 32 samples: a teacher's instanced predictions as targets, a student of other weights on the chain, Adam."""
    from nerf_tex_amd.train import trainer_for
    npar = (1, 6)
    teacher_model, _, _ = make_model(npar, seed=0, dense_media=True)
    student_model, _, _ = make_model(npar, seed=1, dense_media=True)
    n, S = 128, 32
    bufs, hit, cone = itc.instancer_buffers(npar, 21, n, S)
    kn = itc.knobs_of(fic.CASES[0])
    teacher = fic.chain_trainer(fic.CASES[0], teacher_model, n, S)
    tc, ta = teacher.forward_instanced(bufs, cone, hit=hit.astype(np.uint8), **fic.fkw(kn))
    tc, ta = tc.clone(), ta.clone()
    student = trainer_for(student_model, fused=True, instanced=True, max_rays=n, n_samples=S, perturb=False, lrate=5e-4)
    assert type(student).__name__ == "Trainer"
    dbufs = tuple(torch.as_tensor(np.ascontiguousarray(np.nan_to_num(b)), device=fic.dev()) if i not in (7, 8) else b for i, b in enumerate(bufs))
    losses = []
    for _ in range(20):
        c, a = student.forward_instanced(dbufs, cone, hit=hit.astype(np.uint8), **fic.fkw(kn))
        cd, ad = c.detach().requires_grad_(True), a.detach().requires_grad_(True)
        val = torch.mean((cd - tc) ** 2) + torch.mean((ad - ta) ** 2)
        dc, da = torch.autograd.grad(val, (cd, ad))
        student.backward(dc, da)
        student.apply_gradients()
        losses.append(float(val.item()))
    print("losses", " ".join(f"{v:.4e}" for v in losses))
    assert student.last_live > 0 and losses[0] > 0 and losses[-1] < losses[0] and np.isfinite(losses).all()


def test_the_widened_width_128_model_takes_an_instanced_step():
    """A width-128 Fourier network that `_widened` pads into the chain, at case 1's bars (the kept activations are the narrow network's own
    columns)."""
    setup = itc.case_setup(fic.WIDE_CASE)
    tr, pred, got, want, f32, _, _ = fic.checked_step(setup, fic.WIDE_CASE)
    assert tr._pad is not None and got.size == want.grad.size and tr.last_live > 64
