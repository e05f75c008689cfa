"""Host side of the layer-by-layer trainer (no GPU): what `ntx_trainer_create_flex` accepts and refuses before it asks for a device, and which
trainer class `nerf_tex_amd.train.trainer_class_for` picks -- a decision taken without creating anything."""

import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.common import EMB, make_model
from tests.train_flex_common import ARCHS


def create_flex(desc, n_floats, max_rays=0, samples=64):
    from nerf_tex_amd import _lib
    blob, h = np.zeros(max(1, n_floats), np.float32), C.c_void_p()
    rc = _lib.lib.ntx_trainer_create_flex(C.byref(desc), blob.ctypes.data_as(C.POINTER(C.c_float)), n_floats, 0, max_rays, samples, C.byref(h))
    assert rc != _lib.NTX_OK and not h.value
    return rc


@pytest.mark.parametrize("arch_id,npar,kind,arch,fam", ARCHS, ids=[a[0] for a in ARCHS])
def test_the_architecture_check_comes_first_and_accepts(arch_id, npar, kind, arch, fam):
    """Every architecture the GPU tests train passes the architecture check: max_rays = 0 is then NTX_E_INVALID, before any device is asked for;
    so are samples per ray outside 2..1024 and a wrong weight count."""
    from nerf_tex_amd import _lib
    model, _, _ = make_model(npar, kind=kind, arch=arch)
    n = model.n_weight_floats()
    assert n == _lib.lib.ntx_weight_count(C.byref(model.desc()))
    assert create_flex(model.desc(), n) == _lib.NTX_E_INVALID
    assert create_flex(model.desc(), n, max_rays=4, samples=1) == _lib.NTX_E_INVALID and create_flex(model.desc(), n, max_rays=4, samples=1025) == _lib.NTX_E_INVALID
    assert create_flex(model.desc(), n - 1, max_rays=4) == _lib.NTX_E_INVALID and b"floats" in _lib.lib.ntx_last_error()


def test_what_the_entry_refuses():
    """NTX_E_UNSUPPORTED -- although max_rays = 0 would be NTX_E_INVALID: the architecture is looked at first -- for an IPE model, parameter
    branches, a skip at depth - 1, a width above 256."""
    from nerf_tex_amd import _lib
    ipe, _, _ = make_model((1, 3), kind="IPE")
    branches, _, _ = make_model((1, 6), arch=dict(param_depth=1))
    flex, _, _ = make_model((1, 6), arch=dict(depth=6))
    last = flex.desc(); last.skip = 5
    masked = flex.desc(); masked.skip = _lib.SKIP_MASK | 0b100010
    wide = flex.desc(); wide.width = 258
    deep = flex.desc(); deep.depth = 25
    for name, desc in (("ipe", ipe.desc()), ("param_depth", branches.desc()), ("skip at depth-1", last), ("skip mask with depth-1", masked), ("width 258", wide), ("depth 25", deep)):
        assert create_flex(desc, 1000) == _lib.NTX_E_UNSUPPORTED, name
    inside = flex.desc(); inside.skip = _lib.SKIP_MASK | 0b10010                    # skips [1, 4] of six layers
    assert create_flex(inside, 1000) == _lib.NTX_E_INVALID


def test_the_chooser_decides_without_creating_anything():
    """`trainer_class_for`: the chain's `Trainer` for what it takes today (8 x 256 / [4] / 1 with Fourier features or IPE, a narrower network padded
    into it), `FlexTrainer` for every other model of the flex domain, the library's NTX_E_UNSUPPORTED for the rest."""
    from nerf_tex_amd import _lib, util
    from nerf_tex_amd.model import ParamNerf
    from nerf_tex_amd.train import FlexTrainer, Trainer, trainer_class_for
    pick = lambda *a, **k: trainer_class_for(make_model(*a, **k)[0])
    assert pick((1, 6)) is Trainer and pick((2, 3)) is Trainer and pick((1, 3), kind="IPE") is Trainer
    assert pick((1, 6), arch=dict(width=128)) is Trainer and pick((1, 6), arch=dict(width=30)) is Trainer
    for arch_id, npar, kind, arch, _ in ARCHS:
        assert pick(npar, kind=kind, arch=arch) is (Trainer if arch_id == "chain_arch" else FlexTrainer), arch_id
    assert pick((1, 6), arch=dict(width=128, depth=4)) is FlexTrainer and pick((1, 6), arch=dict(width=97)) is FlexTrainer      # (an odd width does not pad into the chain)
    assert pick((4, 8)) is FlexTrainer                                                # pos_map / dir_map of 99 features: wider than the chain holds
    narrow_ipe = ParamNerf({"module": "network.layer.IntegratedPositionalEncoding", "n_freq_bands": 10}, EMB(4), EMB(4), [1, 3], n_pos=6, width=128)["model"]
    for bad in (narrow_ipe, make_model((1, 6), arch=dict(param_depth=1))[0], make_model((1, 6), arch=dict(depth=6, skips=[5]))[0]):
        with pytest.raises(_lib.NtxError) as e:
            trainer_class_for(bad)
        assert e.value.code == _lib.NTX_E_UNSUPPORTED
    # the configs of tests/test_gpu_train_flex.py::test_configs_reach_the_trainer_that_takes_their_model, as far as the decision goes
    cfg = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "train_configs.json")))["carpet"]
    model_of = lambda **kw: util.instantiate(dict(util.remap_reference_config(dict(cfg, model_config=dict(cfg["model_config"], **kw)))["model_config"]))["model"]
    assert trainer_class_for(model_of()) is Trainer
    assert trainer_class_for(model_of(depth=6)) is FlexTrainer and trainer_class_for(model_of(module="network.model.Nerf")) is FlexTrainer
    both = util.instantiate(dict(util.remap_reference_config(dict(cfg, model_config={"module": "network.model.CoarseFine", "model_config": dict(cfg["model_config"], depth=6)}))["model_config"]))
    assert sorted(both) == ["model", "model_fine"] and all(trainer_class_for(m) is FlexTrainer for m in both.values())
