"""dL/d parameters and dL/d rays on the fused chain (`ntx_trainer_enable_gradients`, `Trainer(param_gradients=, input_gradients=)`,
`trainer_for(..., fused=True)`), what can be said without a GPU: the entry exists and refuses NULL, the class pickers answer
as before without `fused` and with the chain class with it, the fused + IPE refusal, the identity behind the chain's new kernel in float64
torch, and every case of tests/test_gpu_fused_gradients.py 2x inside the guards of `pgc.fair` for both gradients."""

import os
import re

import numpy as np
import pytest
import torch

from oracle import torch_cpu as tcpu
from tests import fused_grad_common as fgc
from tests import param_grad_common as pgc
from tests.common import make_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_exported_declared_and_refuses_null():
    from nerf_tex_amd import _lib
    assert "ntx_trainer_enable_gradients" in _lib.SYMBOLS
    for pm, im in ((0, 0), (1, 1), (3, 0)):
        assert _lib.lib.ntx_trainer_enable_gradients(None, pm, im) == _lib.NTX_E_INVALID
    assert _lib.lib.ntx_abi_version() == 7
    with open(os.path.join(ROOT, "include", "nerftex.h")) as f:
        header = f.read()
    assert re.search(r"int\s+ntx_trainer_enable_gradients\(ntx_trainer \*t, int param_mode, int input_mode\);", header)


def test_the_class_pickers_keep_the_chain_only_when_asked():
    from nerf_tex_amd.train import FlexTrainer, Trainer, trainer_class_for
    chain_model, _, _ = make_model((1, 6))
    narrow, _, _ = make_model((1, 6), arch=dict(width=128))
    other, _, _ = make_model((1, 6), arch=dict(width=64, depth=3, skips=[1]))
    for kw in (dict(param_gradients=True), dict(input_gradients="only"), dict(param_gradients="only", input_gradients=True)):
        assert trainer_class_for(chain_model, **kw) is FlexTrainer
        assert trainer_class_for(chain_model, fused=True, **kw) is Trainer
        assert trainer_class_for(narrow, fused=True, **kw) is Trainer and trainer_class_for(narrow, **kw) is FlexTrainer
        assert trainer_class_for(other, fused=True, **kw) is FlexTrainer            # a model the chain does not take: as without `fused`
    assert trainer_class_for(chain_model) is Trainer and trainer_class_for(chain_model, fused=True) is Trainer
    assert trainer_class_for(other, fused=True) is FlexTrainer


def test_fused_gradients_of_an_ipe_model_are_refused():
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import Trainer, trainer_class_for, trainer_for
    ipe, _, _ = make_model((1, 6), kind="IPE")
    assert trainer_class_for(ipe) is Trainer and trainer_class_for(ipe, fused=True) is Trainer
    for kw in (dict(param_gradients=True), dict(input_gradients="only")):
        with pytest.raises(_lib.NtxError) as e:
            trainer_class_for(ipe, fused=True, **kw)
        assert e.value.code == _lib.NTX_E_UNSUPPORTED
        with pytest.raises(_lib.NtxError) as e:
            trainer_for(ipe, fused=True, max_rays=8, n_samples=8, blur_idx=0, **kw)
        assert e.value.code == _lib.NTX_E_UNSUPPORTED
        with pytest.raises(_lib.NtxError) as e:                                        # without `fused`: the layer-by-layer entry's own refusal, as before
            trainer_class_for(ipe, **kw)
        assert e.value.code == _lib.NTX_E_UNSUPPORTED


def test_the_identity_behind_the_kernel():
    """A dozen samples through `torch_cpu.mlp` (8 x 256, [1, 6]) in float64 under a random linear head: with dy0, dy5, dc1o = autograd's
    gradients at the pre-activations of trunk layers 0 and 5 and of the first colour layer (the gradient of a per-sample bias), dL/d pos_map =
    dy0 . W0[:Kp]^T + dy5 . W5[:Kp]^T and dL/d dir_map = dc1o . Wc1[:Kd]^T to 1e-12 -- in every column: the FF(xyz) / FF(dir) columns directly,
    the parameter-feature columns through the encoder to the parameters."""
    _, spec, wts = make_model((1, 6), dense_media=True)
    rng = np.random.default_rng(5)
    n, g = 12, spec.n_geo
    t64 = lambda a: torch.tensor(np.asarray(a, np.float64))
    w = [t64(a) for a in wts]
    w0, w5, wc1 = fgc.layer_kernels(spec, w)
    Kp, Kd = w0.shape[0], wc1.shape[0] - spec.width
    assert (Kp, Kd) == (72, 81)
    for j in (1, 11, 19):                                                              # the three biases per sample: their gradient is the pre-activation's
        w[j] = w[j].expand(n, -1).clone().requires_grad_(True)
    pos_ff = tcpu.fourier_features(t64(rng.uniform(-1, 1, (n, 3))), spec.pos_freq).requires_grad_(True)
    dirs = t64(rng.normal(size=(n, 3))).requires_grad_(True)
    params = t64(rng.uniform(0.2, 1.5, (n, 7))).requires_grad_(True)
    raw, sigma = tcpu.mlp(w, spec, pos_ff, dirs, params)
    head = (raw * t64(rng.normal(size=(n, 3)))).sum() + (sigma * t64(rng.normal(size=(n, 1)))).sum()
    head.backward()
    G_pos, G_dir = fgc.feature_gradients(w[1].grad, w[11].grad, w[19].grad, w0.detach(), w5.detach(), wc1.detach(), Kp, Kd)
    assert G_pos.shape == (n, Kp) and G_dir.shape == (n, Kd)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()) and float(b.abs().max()) > 1e-6
    K3 = pos_ff.shape[1]
    assert close(G_pos[:, :K3], pos_ff.grad)
    leaves = [t64(params.detach().numpy()).requires_grad_(True), t64(dirs.detach().numpy()).requires_grad_(True)]
    p2, d2 = leaves
    geo = tcpu.fourier_features(p2[:, :g], spec.param_freq)
    dir_map = torch.cat([tcpu.fourier_features(d2, spec.dir_freq), tcpu.fourier_features(p2[:, g:], spec.param_freq)], -1)
    assert geo.shape[1] == Kp - K3 and dir_map.shape[1] == Kd
    gp, gd = torch.autograd.grad([geo, dir_map], leaves, grad_outputs=[G_pos[:, K3:], G_dir])
    assert close(gp, params.grad) and close(gd, dirs.grad)
    # and the mutations the GPU tests are held to catch do break it
    G_no_skip, _ = fgc.feature_gradients(w[1].grad, 0 * w[11].grad, w[19].grad, w0.detach(), w5.detach(), wc1.detach(), Kp, Kd)
    assert not close(G_no_skip[:, :K3], pos_ff.grad)


@pytest.mark.parametrize("case", fgc.ALL_CASES, ids=[c[0] for c in fgc.ALL_CASES])
def test_the_gpu_cases_are_fair(case):
    """Every case of the GPU file, at its own size, 2x inside both guards BEFORE any GPU run, for dL/d parameter rows and for dL/d rays_o, rays_d:
    float32 autograd of the restatements within 2.5e-4 of float64 in every column, on the restatement's own float32 ReLU patterns, and every
    column's largest gradient above 2e-6."""
    model, spec, wts, batch, kn, seed = fgc.case_setup(case)
    lengths = np.linalg.norm(batch[1], axis=1)
    assert (np.abs(lengths - 1) > 1e-3).any()
    patterns = pgc.own_patterns(spec, wts, batch, kn, seed)
    want = fgc.restate_both(spec, wts, batch, kn, seed, torch.float64, patterns)
    f32 = fgc.restate_both(spec, wts, batch, kn, seed, torch.float32, patterns)
    fgc.fair_both(want, f32, kn)
