"""Training a ParamNerf with parameter branches (`ntx_trainer_create_flex_ex`, `nerf_tex_amd.train.BranchTrainer`) on the
GPU: the layer-by-layer step with the branch layers in it against the reference's step restated with float64 autograd
(tests/train_branch_oracle.py), at the bars the other trainers are held to.  `-m gpu`."""

import json
import os

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from tests import train_branch_oracle as bro
from tests.common import make_model
from tests.train_common import layer_slices, make_loss, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
BK = (1., .5, .25)


def dev():
    return torch.device("cuda", 0)


def one_step(model, spec, wts, batch, n, S, loss_name, *, bkgd=False, map_exr=False, perturb=False, blur=None, noise_std=0.0, seed=11, miss=None, cap=None):
    """A BranchTrainer's `gradients_step` on a batch, checked by `bro.check_against_float64`; returns (trainer, the oracle's, (color, alpha))."""
    from nerf_tex_amd.train import BranchTrainer
    ro, rd, t, cone, params, color, alpha = batch
    miss = np.zeros(n, bool) if miss is None else miss
    t = t.copy(); t[miss] = np.inf
    cone = cone.copy(); cone[miss] = np.nan                                       # whatever a ray sampler leaves there
    okw, loss = make_loss(loss_name)
    tr = BranchTrainer(model, max_rays=cap or n, n_samples=S, perturb=perturb, blur_idx=blur, raw_noise_std=noise_std, map_exr=map_exr)
    val, cp, ap = tr.gradients_step(ro, rd, t, params, cone, color, alpha, loss, composite_bkgd=bkgd, bkgd_color=BK, seed=seed)
    torch.cuda.synchronize()
    want = bro.check_against_float64(tr, spec, float(val.item()), step_pred(cp, ap), (wts, ro, rd, t, params, cone, color, alpha, okw),
                                     dict(seed=seed, perturb=perturb, noise_std=noise_std, miss=miss, blur_idx=blur, bkgd=bkgd, bkgd_color=BK, map_exr=map_exr))
    return tr, want, (cp.cpu().numpy(), ap.cpu().numpy())


@pytest.mark.parametrize("case", bro.GPU_CASES, ids=[c[0] for c in bro.GPU_CASES])
def test_gradients_of_every_layer_match_float64_autograd(case):
    """One step at 45 rays x 37 samples per architecture: the loss, [color | alpha] and every kernel's and bias's gradient, the branch layers'
    included, against float64 autograd branched by the trainer's own stored ReLU patterns (trunk, colour, both branches) and density sign."""
    from nerf_tex_amd import _lib
    model, spec, wts, batch, kn, seed = bro.case_setup(case)
    tr, _, _ = one_step(model, spec, wts, batch, bro.N_RAYS, bro.N_SAMPLES, seed=seed, **kn)
    for slot in ([32] if spec.n_geo == 0 else []) + ([48] if spec.n_app == 0 else []) + [32 + spec.param_layers, 48 + spec.param_layers]:
        with pytest.raises(_lib.NtxError) as e:                                   # a branch, or a layer of one, that the model does not have
            tr.activation(slot, bro.N_RAYS * bro.N_SAMPLES)
        assert e.value.code == _lib.NTX_E_INVALID


def test_the_weight_gradients_split():
    """Case h's model (param_width 37: an odd leading dimension) at 41 x 70 = 2870 samples: the weight gradients, the branch layers' too, are
    one whole range of 2048 samples and one of 822, added in ascending order."""
    case = [c for c in bro.GPU_CASES if c[0] == "h_pw37"][0]
    n, S = 41, 70
    model, spec, wts, batch, kn, seed = bro.case_setup(case, n, S)
    assert n * S == 2048 + 822
    one_step(model, spec, wts, batch, n, S, seed=seed, **kn)


@pytest.mark.parametrize("bkgd", [False, True])
def test_rays_that_miss_the_proxy(bkgd):
    """Eight of 96 rays with t = inf and cone_scale = NaN stay in the batch: they predict exactly 0 / the background, and loss, predictions
    and gradients are the oracle's filter-and-scatter (renderer.py:58-86)."""
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(depth=4, width=128, skips=[1], param_depth=2, param_width=64))
    n, S = 96, 48
    miss = np.zeros(n, bool); miss[[0, 5, 17, 31, 32, 33, 64, 95]] = True
    tr, want, (cp, ap) = one_step(model, spec, wts, bro.branch_batch(6, n, spec, "carpet"), n, S, "alpha_smape", bkgd=bkgd, perturb=True, miss=miss)
    assert (ap[miss] == 0).all() and (cp[miss] == (np.asarray(BK, np.float32) if bkgd else 0)).all()


def test_steps_are_reproducible_and_independent_of_capacity():
    """Two BranchTrainers on the same weights take three steps bit for bit; so does one made for twice the rays and more samples a ray whose
    buffers still hold a bigger, different batch."""
    from nerf_tex_amd.train import BranchTrainer
    model, spec, wts = make_model((2, 3), dense_media=True, arch=dict(depth=4, width=128, skips=[1, 2], color_depth=0, param_depth=3, param_width=64))
    n, S = 75, 41                                                                # 3075 samples: ragged, two ranges of the weight gradients
    ro, rd, t, cone, params, color, alpha = bro.branch_batch(7, n, spec, "grass_filtered")
    big = bro.branch_batch(8, 2 * n, spec, "grass_filtered")
    okw, loss = make_loss("alpha_smape")
    ends = []
    for cap, cap_S, history in ((n, S, False), (n, S, False), (2 * n, S + 9, True)):
        tr = BranchTrainer(model, max_rays=cap, n_samples=cap_S, lrate=5e-4, lrate_decay=0.002, perturb=True, blur_idx=0, raw_noise_std=0.1)
        if history:
            tr.gradients_step(*big[:3], big[4], big[3], big[5], big[6], loss, seed=1)
        for it in range(3):
            tr.gradients_step(ro, rd, t, params, cone, color, alpha, loss, seed=it, n_samples=S)
            first = tr.gradients() if it == 0 else first
            tr.apply_gradients()
        assert tr.iterations == 3
        ends.append((tr.weights(), *tr.adam_state(), first))
    g = ends[0][3]
    assert all(np.abs(g[sl]).max() > 0 for name, sl in layer_slices(spec) if name.startswith("param_"))
    for other in ends[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(ends[0], other))


def test_param_depth_0_is_the_flex_step_bit_for_bit():
    """param_depth 0 through `BranchTrainer` (the extended descriptor, the new entry): the gradients after one step, and the weights and Adam's
    moments after two, are FlexTrainer's on the same model."""
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer
    model, spec, wts = make_model((2, 3), dense_media=True, arch=dict(depth=4, width=128, skips=[1, 2], color_depth=0))
    n, S = 75, 41
    ro, rd, t, cone, params, color, alpha = bro.branch_batch(7, n, spec, "grass_filtered")
    okw, loss = make_loss("alpha_smape")
    ends = []
    for cls in (FlexTrainer, BranchTrainer):
        tr = cls(model, max_rays=n, n_samples=S, lrate=5e-4, perturb=True, blur_idx=0, raw_noise_std=0.1)
        assert tr.n_weights == model.n_weight_floats()
        for it in range(2):
            tr.gradients_step(ro, rd, t, params, cone, color, alpha, loss, seed=it)
            first = tr.gradients() if it == 0 else first
            tr.apply_gradients()
        ends.append((first, tr.weights(), *tr.adam_state()))
    assert np.abs(ends[0][0]).max() > 1e-6 and all(np.array_equal(a, b) for a, b in zip(*ends))
    assert tr.branch_widths() == []
    from nerf_tex_amd import _lib
    for slot in (32, 48, 63):                                                     # a branch the model does not have
        with pytest.raises(_lib.NtxError) as e:
            tr.activation(slot, n * S)
        assert e.value.code == _lib.NTX_E_INVALID


def carpet_config(**model_kw):
    cfg = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "train_configs.json")))["carpet"]
    return dict(cfg, model_config=dict(cfg["model_config"], **model_kw))


def test_configs_with_branches_reach_the_branch_trainer():
    """`Trainer.from_config` on the carpet block with param_depth 2 and depth 6 gives a `BranchTrainer`; `CoarseFine` + n_importance a
    `CoarseFineTrainer` of two, one step of which has a finite loss and a gradient in every branch layer of both networks."""
    from nerf_tex_amd.train import BranchTrainer, CoarseFineTrainer, Trainer
    tr, _ = Trainer.from_config(carpet_config(param_depth=2, depth=6), max_rays=8)
    assert type(tr) is BranchTrainer and tr.n_samples == 256 and tr.branch_widths() == [128] * 4
    cfg = carpet_config(param_depth=2, depth=6)
    cfg = dict(cfg, model_config={"module": "network.model.CoarseFine", "model_config": dict(cfg["model_config"])}, renderer_config=dict(cfg["renderer_config"], n_samples=32, n_importance=16))
    n = 64
    tr, loss = Trainer.from_config(cfg, max_rays=n)
    assert isinstance(tr, CoarseFineTrainer) and not tr.shared and [type(x) for x in tr.trainers] == [BranchTrainer, BranchTrainer]
    _, spec, _ = make_model((1, 6), arch=dict(depth=6, param_depth=2))
    ro, rd, t, cone, params, color, alpha = bro.branch_batch(5, n, spec, "carpet")
    val = tr.gradients_step(ro, rd, t, params, cone, color, alpha, loss, seed=2)[0]
    torch.cuda.synchronize()
    assert np.isfinite(float(val.item()))
    for x in tr.trainers:
        g = x.gradients()
        assert x.model.layer_table() == orc.layer_table(spec)
        branch = [(name, sl) for name, sl in layer_slices(spec) if name.startswith("param_")]
        assert len(branch) == 8 and np.isfinite(g).all() and all(np.abs(g[sl]).max() > 0 for _, sl in branch), [(nm, float(np.abs(g[sl]).max())) for nm, sl in branch]


def test_the_training_loop_with_branches(tmp_path):
    """`Train` on an iterable of batch dicts with a 4 x 64 ParamNerf of param_depth 2, param_width 32: 40 steps, every loss finite and the
    mean of the last five below the mean of the first five; a run checkpointed at step 20 and resumed from other initial weights ends bit
    for bit where the uninterrupted one does; and the 32 x 32 validation view rendered through `Renderer` with the weights handed over on
    the device equals the render after `model.set_blob(trainer.weights())` -- trainer and renderer agree on the blob order of a branch model."""
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.render import render_image
    from nerf_tex_amd.train import BranchTrainer, Train
    arch = dict(width=64, depth=4, param_depth=2, param_width=32)
    seeded, spec, _ = make_model((1, 6), dense_media=True, arch=arch)
    B, R, S = 2, 128, 32
    ro, rd, t, cone, params, color, alpha = bro.branch_batch(31, B * R, spec, "carpet")
    data = dict(rays_o=ro.reshape(B, R, 3), rays_d=rd.reshape(B, R, 3), t=t.reshape(B, R, 2), cone_scale=cone.reshape(B, R, 1), parameters=params[::R].copy(),
                color=color.reshape(B, R, 3), alpha=alpha.reshape(B, R))

    class Batches:
        composite_bkgd, bkgd_color = False, (1., 1., 1.)
        def __iter__(self):
            while True:
                yield data

    class Views:
        height, width, composite_bkgd, bkgd_color = 32, 32, False, (1., 1., 1.)
        def __iter__(self):
            f = synthetic.FAMILIES["carpet"]
            vo, vd, vt, vc = synthetic.all_hit_rays(32 * 32, f["b_0"], f["b_1"], f["cam"], seed=3)
            d = lambda x: torch.as_tensor(x, device=dev())
            yield dict(rays_o=d(vo)[None], rays_d=d(vd)[None], t=d(vt)[None], cone_scale=d(vc).reshape(1, -1, 1), parameters=d(params[:1]), seed=77)

    cfg = carpet_config(**arch)
    common = dict(model_config=cfg["model_config"], loss_config=cfg["loss_config"], lrate=cfg["lrate"], lrate_decay=cfg["lrate_decay"],
                  renderer_config=dict(cfg["renderer_config"], n_samples=S), weights=seeded.get_blob())
    whole = Train(str(tmp_path / "a"), Batches(), Views(), n_iters=40, logger_config=dict(i_print=1, i_img=40, i_checkpoint=0, print_model_summary=False), **common)
    assert type(whole["trainer"]) is BranchTrainer and whole["step"] == 40
    losses = [v for _, v in whole["loss"]]
    print("losses", [f"{v:.4g}" for v in losses[::5]], f"first five {np.mean(losses[:5]):.5g} last five {np.mean(losses[-5:]):.5g}")
    assert len(losses) == 40 and np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses[::5]
    first = Train(str(tmp_path / "b"), Batches(), None, n_iters=20, logger_config=dict(i_print=0, i_img=0, i_checkpoint=20, print_model_summary=False), **common)
    assert first["step"] == 20 and os.path.exists(str(tmp_path / "b" / "checkpoints" / "ckpt-20.index"))
    other, _, _ = make_model((1, 6), seed=5, arch=arch)                           # other initial weights: everything comes from the checkpoint
    rest = Train(str(tmp_path / "b"), Batches(), None, n_iters=40, logger_config=dict(i_print=0, i_img=0, i_checkpoint=0, print_model_summary=False),
                 **dict(common, weights=other.get_blob()))
    a, b = whole["trainer"], rest["trainer"]
    assert rest["step"] == 40 and a.iterations == b.iterations == 40 and np.array_equal(a.weights(), b.weights())
    assert all(np.array_equal(x, y) for x, y in zip(a.adam_state(), b.adam_state()))
    image = whole["images"][40][0]
    assert image.shape == (32, 32, 4) and float(image.abs().max()) > 0
    a.model.set_blob(a.weights())                                                 # the same weights through the host: the same image
    again = render_image(whole["renderer"], Views(), next(iter(Views())))[0]
    assert torch.equal(again, image)
