"""The training-step restatement (oracle/train_oracle.py <- network/train.py:49-70, network/loss.py) against hand-computed cases and against
finite differences: it is what the GPU trainer's gradients are compared with (tests/test_gpu_train.py), so it gets its own checks.  CPU only."""

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro
from tests.train_common import LOSSES, make_loss

torch = pytest.importorskip("torch")
F = np.float32


def test_losses_known_answers():
    t = torch.tensor([[0.5, 0.0, 1.0]], dtype=torch.float64); p = torch.tensor([[0.25, 0.5, 1.0]], dtype=torch.float64)
    assert float(tro.mse(t, p)) == pytest.approx((0.0625 + 0.25 + 0) / 3)                                   # loss.py:51-54
    assert float(tro.smape(t, p)) == pytest.approx((0.25 / 0.76 + 0.5 / 0.51 + 0) / 3)                       # loss.py:56-59, eps 1e-2
    at = torch.tensor([0.0], dtype=torch.float64); ap = torch.tensor([0.3], dtype=torch.float64)
    # AlphaLoss (loss.py:21-49): a pixel with alpha_true = 0 is masked out of the colour term (hard mask), the alpha term stays
    assert float(tro.alpha_loss(t, at, p, ap)) == pytest.approx(0.0 + 0.09)
    assert float(tro.alpha_loss(t, at + 0.5, p, ap, gamma=2.0, use_hard_mask=False)) == pytest.approx(float(tro.mse(0.5 * t, 0.5 * p)) + 2.0 * 0.04)
    assert float(tro.nerf_loss(t, p, "smape")) == pytest.approx(float(tro.smape(t, p)))


def test_adam_first_step_known_answer():
    # t = 1: m = (1 - b1) g, v = (1 - b2) g^2, lr_t = lr sqrt(1 - b2) / (1 - b1)  ->  w -= lr g / (|g| + eps / sqrt(1 - b2)): a step of lr against the sign
    w = np.asarray([1.0, -2.0, 0.5]); g = np.asarray([0.3, -4.0, 1e-3])
    w1, m1, v1 = tro.adam_step(w, g, np.zeros(3), np.zeros(3), 0, 5e-4)
    omb1, omb2 = float(F(1) - F(0.9)), float(F(1) - F(0.999))                  # Keras forms 1 - beta in float32
    assert np.allclose(m1, omb1 * g) and np.allclose(v1, omb2 * g * g)
    assert np.allclose(w1, w - 5e-4 * np.sign(g), rtol=0, atol=5e-4 * 5e-3)      # (eps / sqrt(1 - b2) = 3.2e-6 against |g| >= 1e-3)
    # ExponentialDecay(lrate, decay_steps, 0.1) without staircase: the rate at iteration 5e5 of config_carpet_train.py (lrate_decay 500) is a tenth
    wa, _, _ = tro.adam_step(w, g, m1, v1, 500000, 5e-4, decay_steps=5e5)
    wb, _, _ = tro.adam_step(w, g, m1, v1, 500000, 5e-5)
    assert np.allclose(wa, wb, rtol=0, atol=1e-12)


def tiny_batch(seed=0, n=6, S=5):
    rng = np.random.default_rng(seed)
    ro = rng.normal(size=(n, 3)); rd = rng.normal(size=(n, 3)); rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    t = np.stack([np.full(n, 0.5), np.full(n, 1.5)], -1)
    z = orc.z_values(t.astype(F), S, F).astype(np.float64)
    return ro, rd, z, rng.uniform(0.2, 1, size=(n, 3)), rng.uniform(1e-3, 5e-3, size=(n, 1)), rng.uniform(0, 1, size=(n, 3)), (rng.uniform(0, 1, size=n) > 0.3) * 0.8


@pytest.mark.parametrize("loss", [dict(kind="alpha", loss_fn="smape", alpha_loss_fn="mse"), dict(kind="nerf", loss_fn="mse")])
def test_autograd_matches_finite_differences(loss):
    """The float64 gradients the GPU trainer is held to, against central differences of the same restated step on a small network."""
    spec = orc.ModelSpec(kind="ParamNerf", n_parameters=(1, 2), depth=3, width=8, skips=(1,), pos_freq=2, dir_freq=1, param_freq=1)
    rng = np.random.default_rng(1)
    w = [rng.normal(size=(i, o)) * 0.5 if b == 0 else rng.normal(size=o) * 0.1 for _, i, o in orc.layer_table(spec) for b in (0, 1)]
    ro, rd, z, par, cone, ct, at = tiny_batch()
    noise = 0.1 * rng.normal(size=z.shape)                                       # the density regulariser (renderer.py:190-192) rides along
    val, c, a, g = tro.step_gradients(w, spec, ro, rd, z, par, cone, ct, at, loss, blur_idx=0, composite_bkgd=True, bkgd=(1., .5, .2), noise=noise)
    assert abs(val - tro.step_gradients(w, spec, ro, rd, z, par, cone, ct, at, loss, blur_idx=0, composite_bkgd=True, bkgd=(1., .5, .2))[0]) > 1e-6
    f = lambda ws: tro.step_gradients(ws, spec, ro, rd, z, par, cone, ct, at, loss, blur_idx=0, composite_bkgd=True, bkgd=(1., .5, .2), noise=noise)[0]
    for k in range(len(w)):
        idx = tuple(rng.integers(0, s_) for s_ in w[k].shape)
        h = 1e-6
        wp = [x.copy() for x in w]; wp[k][idx] += h
        wm = [x.copy() for x in w]; wm[k][idx] -= h
        fd = (f(wp) - f(wm)) / (2 * h)
        assert fd == pytest.approx(g[k][idx], rel=2e-5, abs=1e-9), (k, idx)
    # handing the restatement its own ReLU pattern changes nothing
    n, S = z.shape
    wt = [torch.tensor(x) for x in w]
    pos = torch.tensor(ro)[:, None, :] + torch.tensor(rd)[:, None, :] * torch.tensor(z)[:, :, None]
    assert val == pytest.approx(float(tro.step_gradients(w, spec, ro, rd, z, par, cone, ct, at, loss, blur_idx=0, composite_bkgd=True, bkgd=(1., .5, .2), noise=noise)[0]))


@pytest.mark.parametrize("name", sorted(LOSSES))
def test_loss_descriptor_carries_what_the_oracle_dict_says(name):
    """Both sides of a `LOSSES` entry describe ONE loss: the `ntx_loss_desc` of the product's object holds the kind, the functions, gamma and
    the two mask switches of the oracle's dict, with the reference's defaults where the dict is silent (loss.py:25: gamma 1, filter_color_loss,
    use_hard_mask, and no alpha_loss_fn means loss_fn)."""
    import ctypes, inspect
    from nerf_tex_amd import _lib
    okw, loss = make_loss(name)
    d, fn = loss.desc(), {"mse": _lib.LOSS_MSE, "smape": _lib.LOSS_SMAPE}
    assert d.size == ctypes.sizeof(_lib.LossDesc) and d.kind == {"nerf": _lib.LOSS_NERF, "alpha": _lib.LOSS_ALPHA}[okw["kind"]]
    assert d.loss_fn == fn[okw["loss_fn"]]
    if okw["kind"] == "nerf":
        assert set(okw) == {"kind", "loss_fn"}
        return
    full = {k: p.default for k, p in inspect.signature(tro.alpha_loss).parameters.items() if p.default is not inspect.Parameter.empty}
    assert set(okw) - {"kind"} <= set(full)
    full.update({k: v for k, v in okw.items() if k != "kind"})
    assert d.alpha_loss_fn == fn[full["alpha_loss_fn"] or full["loss_fn"]]
    assert d.gamma == np.float32(full["gamma"]) and d.filter_color_loss == int(full["filter_color_loss"]) and d.use_hard_mask == int(full["use_hard_mask"])


def test_loss_names_keep_their_meaning():
    """tools/dev/soak_train.py and tests/_dp_train_worker.py read the first three by name; the rest are the settings the GPU tests add."""
    assert LOSSES["alpha_smape"][0] == dict(kind="alpha", loss_fn="smape", alpha_loss_fn="mse")
    assert LOSSES["alpha_mse_soft"][0] == dict(kind="alpha", loss_fn="mse", gamma=0.5, use_hard_mask=False) and LOSSES["nerf_mse"][0] == dict(kind="nerf", loss_fn="mse")
    assert {"alpha_smape_smape", "alpha_mse_unfiltered", "alpha_smape_soft_g2", "alpha_mse_hard_g3", "nerf_smape"} <= set(LOSSES)
    assert "alpha_loss_fn" not in LOSSES["alpha_smape_smape"][0] and "alpha_loss_fn" not in LOSSES["alpha_smape_smape"][1]      # the default is the case
    u = LOSSES["alpha_mse_unfiltered"][0]
    assert (u["loss_fn"], u["alpha_loss_fn"], u["gamma"], u["filter_color_loss"]) == ("mse", "smape", 0.25, False)


@pytest.mark.parametrize("map_exr,bkgd", [(False, False), (True, True)])
@pytest.mark.parametrize("name", sorted(LOSSES))
def test_composite_gradients_match_finite_differences(name, map_exr, bkgd):
    """`tro.composite_gradients` -- what the GPU composite's hand-written adjoint is held to (tests/test_gpu_train_composite.py) -- against central
    differences in float64 at 3 rays x 5 samples, for every loss setting, with the sigmoid and with elu + 1 on raw colours either side of 0,
    with and without the background term, under the density regulariser, through the Renderer's sample distances and through the
    MipRenderer's segment lengths.  One alpha target is 0 (the masks), densities lie either side of the ReLU."""
    okw = LOSSES[name][0]
    n, S = 3, 5
    rng = np.random.default_rng(7)
    raw = rng.normal(size=(n, S, 3)) * 1.5
    sg = rng.normal(size=(n, S)) * 4 + 2
    noise = 0.1 * rng.normal(size=(n, S))
    sg[np.abs(sg + noise) < 1e-2] = 0.5                                           # off the ReLU's kink by more than the step
    rd = rng.normal(size=(n, 3))
    ct, at = rng.uniform(0, 1, size=(n, 3)), np.asarray([0.7, 0.0, 0.4])
    assert (raw > 0).any() and (raw < 0).any() and (sg + noise > 0).any() and (sg + noise < 0).any()
    for mip in (False, True):
        z = np.sort(rng.uniform(0.5, 1.5, size=(n, S + mip)), -1)
        kw = dict(map_exr=map_exr, composite_bkgd=bkgd, bkgd=(1., .5, .2), noise=noise, mip=mip)
        val, c, a, d_rgb, d_sg = tro.composite_gradients(raw, sg, z, rd, ct, at, okw, **kw)
        assert 0.05 < a.max() < 0.999999 and np.abs(d_rgb).max() > 1e-4 and np.abs(d_sg).max() > 1e-4
        other = tro.composite_gradients(raw, sg, z[:, :S] if mip else np.concatenate([z, z[:, -1:] + 0.3], -1), rd, ct, at, okw, **dict(kw, mip=not mip))[0]
        assert abs(val - other) > 1e-6                                            # the two renderers' lengths are not the same composite
        f = lambda r, s: tro.composite_gradients(r, s, z, rd, ct, at, okw, **kw)[0]
        h = 1e-6
        for idx in np.ndindex(n, S, 3):
            rp, rm = raw.copy(), raw.copy(); rp[idx] += h; rm[idx] -= h
            assert (f(rp, sg) - f(rm, sg)) / (2 * h) == pytest.approx(d_rgb[idx], rel=2e-5, abs=1e-9), (mip, idx)
        for idx in np.ndindex(n, S):
            sp, sm = sg.copy(), sg.copy(); sp[idx] += h; sm[idx] -= h
            assert (f(raw, sp) - f(raw, sm)) / (2 * h) == pytest.approx(d_sg[idx], rel=2e-5, abs=1e-9), (mip, idx)
    with pytest.raises(ValueError):
        tro.composite_gradients(raw, sg, z, rd, ct, at, okw, mip=False)           # S + 1 depths are a mip step's


def _dp_worker(rank, world, port, q):
    """Rank `rank` of a data-parallel step on CPU: the restated step on ITS half of the rays, the product's host-side mean over ranks."""
    import os
    import torch.distributed as dist
    from nerf_tex_amd.train import allreduce_mean_host
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    spec = orc.ModelSpec(kind="ParamNerf", n_parameters=(1, 2), depth=3, width=8, skips=(1,), pos_freq=2, dir_freq=1, param_freq=1)
    rng = np.random.default_rng(1)
    w = [rng.normal(size=(i, o)) * 0.5 if b == 0 else rng.normal(size=o) * 0.1 for _, i, o in orc.layer_table(spec) for b in (0, 1)]
    ro, rd, z, par, cone, ct, at = tiny_batch(seed=3, n=8, S=5)
    ok = True
    for loss in (dict(kind="alpha", loss_fn="smape", alpha_loss_fn="mse"), dict(kind="nerf", loss_fn="mse")):
        whole = np.concatenate([g.ravel() for g in tro.step_gradients(w, spec, ro, rd, z, par, cone, ct, at, loss, blur_idx=0)[3]])
        lo, hi = rank * 8 // world, (rank + 1) * 8 // world
        mine = np.concatenate([g.ravel() for g in tro.step_gradients(w, spec, ro[lo:hi], rd[lo:hi], z[lo:hi], par[lo:hi], cone[lo:hi], ct[lo:hi], at[lo:hi], loss, blur_idx=0)[3]])
        mean = allreduce_mean_host(mine)
        ok = ok and mean.dtype == np.float32 and bool(np.allclose(mean, whole, rtol=2e-6, atol=1e-7 * np.abs(whole).max())) and not np.allclose(mine, whole, rtol=1e-3)
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


def test_data_parallel_step_world2_gloo():
    """N > 1 training on CPU: the losses of loss.py are means over rays, so the mean over ranks of the gradients of equal shards is the whole
    batch's gradient -- the one collective of data-parallel training (`Trainer.sync_gradients`: ncclAllReduce behind the C ABI on GPUs, this
    host-side mean otherwise), executed by two gloo ranks on the restated step."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted(q.get(timeout=180) for _ in procs)
    [p.join(60) for p in procs]
    assert res == [(0, True), (1, True)]


def test_train_config_fixture_is_what_the_trainer_is_built_from():
    """tests/golden/train_configs.json (oracle/gen_golden.py train_configs, from the reference's config modules): the five shipped training
    configs' blocks -- what `Trainer.from_config` reads on the GPU box (tests/test_gpu_train.py) -- and the reference paths they name remap
    to this package's classes."""
    import json, os
    from nerf_tex_amd import util
    cfgs = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "train_configs.json")))
    assert sorted(cfgs) == ["carpet", "fur", "grass", "grass_filtered", "plush"]
    for fam, c in cfgs.items():
        assert c["source"] == f"configs/config_{fam}_train.py" and c["batchsize"] * c["rays_per_image"] == 1024 and c["renderer_config"]["n_samples"] == 256
        r = util.remap_reference_config(c)
        assert r["model_config"]["module"] == "nerf_tex_amd.model.ParamNerf" and r["loss_config"]["module"] == "nerf_tex_amd.loss.AlphaLoss"
        loss = util.instantiate(dict(r["loss_config"]))
        d = loss.desc()
        assert d.size > 0                                                        # (the descriptor is built without a device)
    assert cfgs["grass_filtered"]["renderer_config"]["raw_noise_std"] == 0.1 and cfgs["grass_filtered"]["renderer_config"]["blur_idx"] == 0
    assert all("raw_noise_std" not in cfgs[f]["renderer_config"] for f in ("carpet", "fur", "grass", "plush"))


def test_from_config_refuses_what_a_step_does_not_do():
    """`Trainer.from_config` on a config's blocks: a renderer key without a meaning in a training step is an error, and so is the `Train` loop
    on a coarse + fine configuration (n_importance > 0 is a `CoarseFineTrainer`'s: tests/test_gpu_train.py) -- before any device is touched."""
    import copy, json, os
    from nerf_tex_amd.train import Trainer
    cfg = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "train_configs.json")))["carpet"]
    c = copy.deepcopy(cfg); c["renderer_config"]["no_such_key"] = 1
    with pytest.raises(TypeError):
        Trainer.from_config(c)
