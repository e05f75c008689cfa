"""Training an IPE model as the MipRenderer renders it (renderer.py:356-473): the parts that need no GPU.  The float64 restatement of a mip
step (oracle/train_oracle.py on an IPE spec) is anchored to the oracle's MipRenderer, and the trainer's dispatch on the renderer_config's module and
the C ABI's acceptance of the IPE descriptor are checked before any device is asked for."""

import ctypes as C

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from tests.common import make_model
from tests.train_common import mip_batch

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("blur_idx", [0, 2, 4])
def test_restated_mip_forward_matches_the_oracle(blur_idx):
    """The restatement's forward in float64 (cone-segment gaussians, IPE, the MLP, the composite with the mip dists) against
    nerftex_oracle.mip_render_rays on the same rays and depths, perturb off."""
    from oracle import train_oracle as tro
    model, spec, wts = make_model((1, 3), kind="IPE", dense_media=True)
    n, S = 24, 20
    ro, rd, t, cone, params = mip_batch(n, 5)
    want = orc.mip_render_rays(wts, spec, ro, rd, t, params, cone, S, blur_idx, True, (1., .5, .25), dtype=np.float64)
    z = orc.z_values(np.asarray(t, np.float64), S + 1, np.float64)
    assert np.array_equal(z, want["z_vals"])
    t_ = lambda a: torch.tensor(np.asarray(a, np.float64))
    c, a = tro.render([t_(w) for w in wts], spec, t_(ro), t_(rd), t_(z), t_(params), t_(cone), blur_idx, composite_bkgd=True, bkgd=(1., .5, .25))
    got = np.concatenate([c.numpy(), a.numpy()[:, None]], -1)
    ref = np.concatenate([want["color_pred"], want["alpha_pred"][:, None]], -1)
    assert np.abs(ref[:, 3]).max() > 0.05                                        # media that the rays see
    assert orc.rel_linf(got, ref) <= 1e-9


def _cfg(module, ipe, n_importance=0, blur_idx=0):
    pos = {"module": "network.layer.IntegratedPositionalEncoding", "n_freq_bands": 10} if ipe else {"module": "network.model.FourierFeatures", "n_freq_bands": 10}
    emb = lambda k: {"module": "network.model.FourierFeatures", "n_freq_bands": k}
    model = {"module": "network.model.ParamNerf", "pos_embedding": pos, "dir_embedding": emb(4), "param_embedding": emb(4), "n_parameters": [1, 3]}
    if ipe:
        model["n_pos"] = 6
    r = {"module": module, "n_samples": 64, "perturb": True}
    if blur_idx is not None:
        r["blur_idx"] = blur_idx
    if n_importance:
        r["n_importance"] = n_importance
    return {"model_config": model, "loss_config": {"module": "network.loss.AlphaLoss", "loss_fn": "network.loss.smape", "alpha_loss_fn": "network.loss.mse"},
            "renderer_config": r, "lrate": 5e-4, "lrate_decay": 500}


def test_from_config_refuses_mismatched_renderers_and_importance():
    """Trainer.from_config dispatches on renderer_config['module'] as the render side pairs them (renderer.py:71, :338): an IPE model under
    Renderer and a FourierFeatures model under MipRenderer are NTX_E_UNSUPPORTED; MipRenderer with n_importance > 0 is NotImplementedError
    (renderer.py:403-404); MipRenderer without blur_idx is ValueError.  All of it before a device is asked for."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import Trainer
    for module, ipe in (("network.renderer.Renderer", True), ("network.renderer.MipRenderer", False), ("nerf_tex_amd.renderer.MipRenderer", False)):
        with pytest.raises(_lib.NtxError) as e:
            Trainer.from_config(_cfg(module, ipe), max_rays=8)
        assert e.value.code == _lib.NTX_E_UNSUPPORTED, (module, ipe)
    with pytest.raises(NotImplementedError):
        Trainer.from_config(_cfg("network.renderer.MipRenderer", True, n_importance=64), max_rays=8)
    with pytest.raises(ValueError):
        Trainer.from_config(_cfg("network.renderer.MipRenderer", True, blur_idx=None), max_rays=8)
    model, _, _ = make_model((1, 3), kind="IPE")
    with pytest.raises(ValueError):
        Trainer(model, max_rays=8, n_samples=8)


def test_the_abi_accepts_the_ipe_descriptor():
    """ntx_trainer_create takes NTX_POS_IPE on n_pos 6 past its architecture check (here stopped by max_rays = 0, NTX_E_INVALID, before any
    device is asked for); IPE on n_pos 3 and Fourier features on n_pos 6 stay NTX_E_UNSUPPORTED, and so does a narrower IPE network."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.model import ParamNerf
    model, _, _ = make_model((1, 3), kind="IPE")
    blob = np.zeros(model.n_weight_floats(), np.float32)
    assert model.n_weight_floats() == _lib.lib.ntx_weight_count(C.byref(model.desc()))

    def create(desc, max_rays):
        h = C.c_void_p()
        return _lib.lib.ntx_trainer_create(C.byref(desc), blob.ctypes.data_as(C.POINTER(C.c_float)), blob.size, 0, max_rays, 64, C.byref(h))

    assert create(model.desc(), 0) == _lib.NTX_E_INVALID
    d = model.desc(); d.n_pos = 3
    assert create(d, 0) == _lib.NTX_E_UNSUPPORTED
    f, _, _ = make_model((1, 3))
    d = f.desc(); d.n_pos = 6
    assert create(d, 0) == _lib.NTX_E_UNSUPPORTED
    ipe = {"module": "network.layer.IntegratedPositionalEncoding", "n_freq_bands": 10}
    emb = {"module": "network.model.FourierFeatures", "n_freq_bands": 4}
    narrow = ParamNerf(ipe, emb, emb, [1, 3], n_pos=6, width=128)["model"]
    assert create(narrow.desc(), 0) == _lib.NTX_E_UNSUPPORTED
