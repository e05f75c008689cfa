"""The layer-by-layer training step (`ntx_trainer_create_flex`, `nerf_tex_amd.train.FlexTrainer`) on the GPU: any Nerf /
ParamNerf of the renderer's flex family against the reference's step restated with float64 autograd (oracle/train_oracle.py), at the bars
the chain trainer is held to (tests/test_gpu_train.py).  `-m gpu`."""

import json
import os

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro
from tests.common import make_model
from tests.train_common import layer_slices, make_loss, rel_linf, step_pred
from tests.train_flex_common import ARCHS, check_against_float64, flex_batch, n_relu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
BK = (1., .5, .25)


def dev():
    return torch.device("cuda", 0)


def one_step(model, spec, wts, fam, n, S, loss_name, *, bkgd=False, map_exr=False, perturb=False, blur=None, noise_std=0.0, seed=11, batch_seed=3, miss=None, cap=None):
    """A FlexTrainer's `gradients_step` on a seeded batch, checked by `check_against_float64`; returns (trainer, what the oracle gave)."""
    from nerf_tex_amd.train import FlexTrainer
    ro, rd, t, cone, params, color, alpha = flex_batch(batch_seed, n, S, spec, fam)
    miss = np.zeros(n, bool) if miss is None else miss
    t = t.copy(); t[miss] = np.inf
    cone = cone.copy(); cone[miss] = np.nan                                       # whatever a ray sampler leaves there
    okw, loss = make_loss(loss_name)
    tr = FlexTrainer(model, max_rays=cap or n, n_samples=S, perturb=perturb, blur_idx=blur, raw_noise_std=noise_std, map_exr=map_exr)
    val, cp, ap = tr.gradients_step(ro, rd, t, params if params.shape[1] else None, cone, color, alpha, loss, composite_bkgd=bkgd, bkgd_color=BK, seed=seed)
    torch.cuda.synchronize()
    want = check_against_float64(tr, spec, float(val.item()), step_pred(cp, ap), (wts, ro, rd, t, params, cone, color, alpha, okw),
                                 dict(seed=seed, perturb=perturb, noise_std=noise_std, miss=miss, blur_idx=blur, bkgd=bkgd, bkgd_color=BK, map_exr=map_exr))
    return tr, want, (cp.cpu().numpy(), ap.cpu().numpy())


# loss, background and map_exr vary over the architectures; the [2, 3] family runs as its config does (blur_idx 0, raw_noise_std 0.1, perturb)
KNOBS = {"nerf_8x256": dict(loss_name="nerf_mse", bkgd=True), "depth6": dict(loss_name="alpha_smape"), "skip2": dict(loss_name="alpha_mse_soft", bkgd=True),
         "color_depth2": dict(loss_name="alpha_smape", map_exr=True), "color_depth0": dict(loss_name="nerf_mse", bkgd=True, perturb=True),
         "w128_d4": dict(loss_name="alpha_smape", blur=0, noise_std=0.1, perturb=True), "w98_d5_skips13": dict(loss_name="alpha_mse_soft"),
         "depth1": dict(loss_name="alpha_smape", perturb=True), "nerf_w64_d3_skip1": dict(loss_name="alpha_smape", bkgd=True), "chain_arch": dict(loss_name="alpha_smape", perturb=True)}


@pytest.mark.parametrize("arch_id,npar,kind,arch,fam", ARCHS, ids=[a[0] for a in ARCHS])
def test_gradients_of_every_layer_match_float64_autograd(arch_id, npar, kind, arch, fam):
    """One step at 45 rays x 37 samples (1665 samples: off the contraction's 128-row tile and off 32) per architecture: the loss, [color | alpha] and
    every kernel's and bias's gradient against float64 autograd branched by the trainer's own stored ReLU patterns and density sign."""
    model, spec, wts = make_model(npar, kind=kind, dense_media=True, arch=arch)
    one_step(model, spec, wts, fam, 45, 37, **KNOBS[arch_id])


@pytest.mark.parametrize("n,S", [(300, 70), (41, 70), (239, 64), (500, 64)])
def test_the_weight_gradients_split(n, S):
    """dW = X^T . dY is summed over ranges of 2048 samples (FLEX_SPLIT in csrc/ntx_backend_flex.hip), the ranges added in ascending order: 21 000 samples
    are ten whole ranges and one of 520, 2870 samples one whole range and one of 822.  70 samples a ray also cross the composite's 64-sample chunk.
    15 296 samples are 8 ranges (the last of 960) and 32 000 are 16 (the last of 1280): a multiple of 8 ranges, as every real batch has, takes the
    contraction's XCD-major tile numbering (gemm_place in csrc/ntx_gemm.hip)."""
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(width=64, depth=3))
    assert (n * S) % 2048 not in (0, 1024) and n * S > 2048
    one_step(model, spec, wts, "carpet", n, S, "alpha_smape", perturb=True)


@pytest.mark.parametrize("bkgd", [False, True])
def test_rays_that_miss_the_proxy(bkgd):
    """Eight of 96 rays with t = inf stay in the batch: they predict exactly 0 / the background, and loss, predictions and gradients are the
    oracle's filter-and-scatter (renderer.py:58-86), as tests/test_gpu_train.py has it for the chain."""
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(color_depth=2))
    n, S = 96, 48
    miss = np.zeros(n, bool); miss[[0, 5, 17, 31, 32, 33, 64, 95]] = True
    tr, want, (cp, ap) = one_step(model, spec, wts, "carpet", n, S, "alpha_smape", bkgd=bkgd, perturb=True, seed=11, batch_seed=6, miss=miss)
    assert (ap[miss] == 0).all() and (cp[miss] == (np.asarray(BK, np.float32) if bkgd else 0)).all()


def test_steps_are_reproducible_and_independent_of_capacity():
    """Two FlexTrainers on the same weights take three steps bit for bit; so does one made for twice the rays and more samples a ray whose buffers
    still hold a bigger, different batch.  One Adam step against its float64 restatement, as the chain's test has it."""
    from nerf_tex_amd.train import FlexTrainer
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(depth=6))
    n, S = 75, 41                                                                # 3075 samples: ragged, two ranges of the weight gradients
    ro, rd, t, cone, params, color, alpha = flex_batch(7, n, S, spec, "carpet")
    big = flex_batch(8, 2 * n, S + 9, spec, "carpet")
    okw, loss = make_loss("alpha_smape")
    ends = []
    for cap, cap_S, history in ((n, S, False), (n, S, False), (2 * n, S + 9, True)):
        tr = FlexTrainer(model, max_rays=cap, n_samples=cap_S, lrate=5e-4, lrate_decay=0.002, perturb=True)
        if history:
            tr.gradients_step(*big[:3], big[4], big[3], big[5], big[6], loss, seed=1)
        first = None
        for it in range(3):
            tr.gradients_step(ro, rd, t, params, cone, color, alpha, loss, seed=it, n_samples=S)
            if it == 0:
                first = (tr.gradients(), tr.weights(), *tr.adam_state())
            tr.apply_gradients()
            if it == 0:
                first += (tr.weights(), *tr.adam_state())
        assert tr.iterations == 3
        ends.append((tr.weights(), *tr.adam_state(), first))
    assert np.abs(ends[0][3][0]).max() > 1e-6
    for other in ends[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(ends[0][:3], other[:3]))
        assert np.array_equal(ends[0][3][0], other[3][0])
    g, wb, mb, vb, wa, ma, va = ends[0][3]
    ww, mm, vv = tro.adam_step(wb, g, mb, vb, 0, 5e-4, decay_steps=2.0, decay_rate=0.1)
    g64, mb64, vb64 = g.astype(np.float64), mb.astype(np.float64), vb.astype(np.float64)
    assert (np.abs(ma - mm) <= 4e-7 * (np.abs(g64) + np.abs(mb64)) + 1e-30).all()
    assert (np.abs(va - vv) <= 4e-7 * (g64 * g64 + vb64) + 1e-38).all()
    step = ww - wb.astype(np.float64)
    assert (np.abs(wa.astype(np.float64) - ww) <= 1.01 * np.spacing(np.abs(wa)) + 1e-6 * np.abs(step)).all() and np.abs(step).max() > 1e-5


@pytest.mark.parametrize("pair", ["two_nerfs", "shared_w128_d4"])
def test_coarse_and_fine_training(pair):
    """n_importance > 0 for the classic pair -- `CoarseFine` of two plain Nerf 8 x 256 networks -- and for one shared 4 x 128 ParamNerf: both passes
    and every layer's gradient of both networks against `tro.step_gradients_coarse_fine` on the depths the step placed, with the bars of
    tests/test_gpu_train.py::test_coarse_and_fine_training."""
    from nerf_tex_amd.train import CoarseFineTrainer, FlexTrainer
    shared = pair != "two_nerfs"
    kind, npar, arch = ("ParamNerf", (1, 6), dict(width=128, depth=4)) if shared else ("Nerf", (0, 0), None)
    model, spec, wts = make_model(npar, kind=kind, dense_media=True, arch=arch)
    fine, _, wts_f = make_model(npar, kind=kind, seed=3, dense_media=True, arch=arch)
    n, S, NI = 72, 24, 16
    ro, rd, t, cone, params, color, alpha = flex_batch(14, n, S, spec, "carpet")
    okw, loss = make_loss("alpha_smape")
    tr = CoarseFineTrainer(model, None if shared else fine, max_rays=n, n_samples=S, n_importance=NI, perturb=True)
    assert all(type(x) is FlexTrainer for x in tr.trainers) and len(tr.trainers) == (1 if shared else 2)
    kept, M, MF, R = {}, n * S, n * (S + NI), n_relu(spec)

    def on_coarse():
        torch.cuda.synchronize()
        kept["masks"] = [(tr.coarse.activation(k, M) > 0).astype(np.float64) for k in range(R)]
        kept["sigma"] = (tr.coarse.activation(64, M).reshape(n, S) > 0).astype(np.float64)
        kept["grad"] = tr.coarse.gradients()
    val, cf, af, cc, ac = tr.gradients_step(ro, rd, t, params if params.shape[1] else None, cone, color, alpha, loss, seed=6, on_coarse=on_coarse)
    torch.cuda.synchronize()
    z_c, z_f = orc.z_values_perturbed(t, S, 6, np.float32), tr.last_z.cpu().numpy()
    assert z_f.shape == (n, S + NI) and (np.diff(z_f, axis=-1) >= 0).all() and all(np.isin(z_c[r], z_f[r]).all() for r in range(n))
    masks_f = [(tr.fine.activation(k, MF) > 0).astype(np.float64) for k in range(R)]
    sigma_f = (tr.fine.activation(64, MF).reshape(n, S + NI) > 0).astype(np.float64)
    args = (wts, None if shared else wts_f, spec, ro, rd, z_c, z_f, params, cone, color, alpha, okw)
    mk = dict(masks_coarse=kept["masks"], sigma_mask_coarse=kept["sigma"], masks_fine=masks_f, sigma_mask_fine=sigma_f)
    want, (wc2, wa2), (wc1, wa1), g_c, g_f = tro.step_gradients_coarse_fine(*args, **mk)
    _, _, _, f_c, f_f = tro.step_gradients_coarse_fine(*args, dtype=torch.float32, **mk)
    print(f"loss {float(val.item()):.9g} want {want:.9g}")
    assert abs(float(val.item()) - want) <= 1e-5 * abs(want)
    pred = lambda c, a: np.concatenate([c.cpu().numpy(), a.cpu().numpy()[:, None]], -1)
    assert orc.rel_linf(pred(cf, af), np.concatenate([wc2, wa2[:, None]], -1)) <= 1e-4 and orc.rel_linf(pred(cc, ac), np.concatenate([wc1, wa1[:, None]], -1)) <= 1e-4
    flat = lambda g: np.concatenate([np.asarray(x, np.float64).ravel() for x in g])
    checks = [(tr.fine.gradients(), flat(g_c), flat(f_c))] if shared else [(tr.coarse.gradients(), flat(g_c), flat(f_c)), (tr.fine.gradients(), flat(g_f), flat(f_f))]
    for got, wantg, f32 in checks:
        assert np.abs(wantg).max() > 1e-6
        for name, sl in layer_slices(spec):
            floor, err = rel_linf(f32[sl], wantg[sl]), rel_linf(got[sl], wantg[sl])
            print(f"  {name:<24} err {err:.2e} floor {floor:.2e}")
            assert err <= max(1e-4, 4 * floor), (name, err, floor)
    if shared:
        assert not np.array_equal(kept["grad"], tr.fine.gradients())             # the coarse pass's gradient alone is not the step's
    w0 = [x.weights() for x in tr.trainers]
    tr.apply_gradients()
    assert all(x.iterations == 1 for x in tr.trainers) and all(not np.array_equal(a, x.weights()) for a, x in zip(w0, tr.trainers))


def carpet_config(**model_kw):
    cfg = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "train_configs.json")))["carpet"]
    return dict(cfg, model_config=dict(cfg["model_config"], **model_kw))


def test_configs_reach_the_trainer_that_takes_their_model():
    """`Trainer.from_config`: the carpet block as written still gets the chain's `Trainer`; the same block with depth 6, and one whose model is
    network.model.Nerf, get a `FlexTrainer`; `CoarseFine` + n_importance a `CoarseFineTrainer` of two FlexTrainers."""
    from nerf_tex_amd.train import CoarseFineTrainer, FlexTrainer, Trainer
    tr, _ = Trainer.from_config(carpet_config(), max_rays=8)
    assert type(tr) is Trainer
    tr, _ = Trainer.from_config(carpet_config(depth=6), max_rays=8)
    assert type(tr) is FlexTrainer and tr.n_samples == 256
    tr, _ = Trainer.from_config(carpet_config(module="network.model.Nerf"), max_rays=8)
    assert type(tr) is FlexTrainer and tr.model.n_params == 0
    cfg = carpet_config(depth=6)
    cfg = dict(cfg, model_config={"module": "network.model.CoarseFine", "model_config": dict(cfg["model_config"])}, renderer_config=dict(cfg["renderer_config"], n_samples=32, n_importance=16))
    tr, _ = Trainer.from_config(cfg, max_rays=64)
    assert isinstance(tr, CoarseFineTrainer) and not tr.shared and [type(x) for x in tr.trainers] == [FlexTrainer, FlexTrainer]


def test_the_training_loop_on_another_architecture(tmp_path):
    """`Train` on an iterable of batch dicts with a 4 x 64 ParamNerf: 40 steps, the loss falls (the rule of test_a_few_steps_fit_a_target), a run
    checkpointed at step 20 and resumed ends bit for bit where the uninterrupted one does, and the 32 x 32 validation view rendered through
    `Renderer` with the weights handed over on the device equals the render after `model.set_blob(trainer.weights())`."""
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.render import render_image
    from nerf_tex_amd.train import FlexTrainer, Train
    from tests.test_gpu_train import batch
    arch = dict(width=64, depth=4)
    seeded, _, _ = make_model((1, 6), dense_media=True, arch=arch)
    B, R, S = 2, 128, 32
    ro, rd, t, cone, params, color, alpha = batch(31, B * R, S, 7, "carpet")
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
    assert type(whole["trainer"]) is FlexTrainer and whole["step"] == 40
    losses = [v for _, v in whole["loss"]]
    assert len(losses) == 40 and np.isfinite(losses).all()
    assert losses[-1] < 0.9 * losses[0] and np.mean(losses[-5:]) < np.mean(losses[5:10]) < np.mean(losses[:5]), losses[::5]
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


def test_gradient_allreduce_on_a_one_rank_communicator():
    """ntx_trainer_allreduce_gradients on a flex trainer's handle, one-rank RCCL: the gradient stays bit for bit, the step after it is the step without it."""
    from nerf_tex_amd.dist import Comm
    from nerf_tex_amd.train import FlexTrainer
    model, spec, wts = make_model((1, 6), dense_media=True, arch=dict(width=128, depth=4))
    n, S = 64, 32
    ro, rd, t, cone, params, color, alpha = flex_batch(4, n, S, spec, "carpet")
    okw, loss = make_loss("alpha_smape")
    comm = Comm(0)
    assert comm.world == 1
    a = FlexTrainer(model, max_rays=n, n_samples=S, perturb=False); b = FlexTrainer(model, max_rays=n, n_samples=S, perturb=False)
    a.gradients_step(ro, rd, t, params, cone, color, alpha, loss); g = a.gradients()
    a.sync_gradients(comm)
    torch.cuda.synchronize()
    assert np.array_equal(a.gradients(), g) and np.abs(g).max() > 1e-6
    a.apply_gradients()
    b.step(ro, rd, t, params, cone, color, alpha, loss, comm=comm)
    assert np.array_equal(a.weights(), b.weights())
    comm.close()
