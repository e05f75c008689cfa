"""The differentiable InstanceRenderer tail on the host: the float64 restatement the GPU tests are held to (tests/instanced_train_common.py)
against the oracle's InstanceRenderer, the two entries in the ABI, and the GPU cases' float32 floors.  No GPU."""

import re

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from tests import instanced_train_common as itc
from tests.common import make_model
from tests.train_common import BKGD, layer_slices, rel_linf

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("npar", [(1, 6), (2, 3)])
@pytest.mark.parametrize("blur", [None, "geometry", "appearance"])
@pytest.mark.parametrize("opts", [dict(), dict(density_reweighting=False), dict(map_exr=True, composite_bkgd=True)], ids=["plain", "no_reweighting", "exr_bkgd"])
def test_restatement_is_the_oracles_instance_renderer(npar, blur, opts):
    """Float64 forward of the restatement == `instance_evaluate_model(dtype=float64)` to 1e-12 on the same buffers (un-hit rays, a hit ray
    without a live sample and negative dists among them)."""
    _, spec, w = make_model(npar, dense_media=True, arch=dict(width=64, depth=3, skips=[1]))
    blur_idx = {None: None, "geometry": 0, "appearance": npar[0]}[blur]
    bufs, hit, cone = itc.instancer_buffers(npar, seed=7, n=19, S=45)
    kw = dict(dict(density_reweighting=True, map_exr=False, composite_bkgd=False), **opts)
    got = itc.restated(w, spec, bufs, hit, cone, blur_idx=blur_idx, density_scale=400.0, bkgd=BKGD, **kw).pred
    rays_d_map, pts, tt, dists, color_last, alpha_last, alpha_weight, instance_id, _, params_map = bufs
    c, a = orc.instance_evaluate_model(w, spec, rays_d_map, pts, tt, dists, color_last, alpha_last, alpha_weight, instance_id, hit, params_map, cone, blur_idx, itc.PATCH_SCALE,
                                       400.0, kw["density_reweighting"], kw["map_exr"], kw["composite_bkgd"], BKGD, dtype=np.float64)
    want = np.concatenate([c, a[:, None]], -1)
    assert (~hit).any() and (dists[hit] < 0).any() and float(want[:, 3].max()) > 0.3
    assert np.all(got[~hit] == 0)
    assert np.abs(got - want).max() <= 1e-12, np.abs(got - want).max()


def test_abi_has_the_two_entries():
    """Declared in the header, bound with argtypes, exported and callable (a NULL trainer is NTX_E_INVALID without a device); the ABI is still 7."""
    import os
    from nerf_tex_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nerftex.h")).read()
    for name, n_args in (("ntx_train_forward_instanced", 22), ("ntx_trainer_sample_param_gradients", 5)):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n_args
        fn = getattr(_lib.lib, name)
        assert fn(*([None] * 11 + [1, 1, -1, 1.0, 1.0, 0] + [None] * 5 if n_args == 22 else [None] * 5)) == _lib.NTX_E_INVALID
        assert b"NULL" in _lib.lib.ntx_last_error()
    assert _lib.ABI_VERSION == 7 and _lib.lib.ntx_abi_version() == 7 and "#define NTX_ABI_VERSION 7" in header


@pytest.mark.parametrize("case", itc.CASES, ids=itc.CASE_IDS)
def test_the_gpu_cases_keep_their_float32_floors(case):
    """Before any GPU run: with the float32 restatement's OWN ReLU patterns, float32 autograd sits within 5e-4 of float64 autograd on the same
    patterns in every layer (and per parameter column), and every layer has a gradient worth the name -- so the GPU tests' bar max(1e-4, 4 x
    floor) with the floor capped at 5e-4 can hold.  density_scale was lowered until it did; the cap was not raised."""
    _floors(itc.case_setup(case), 100)


@pytest.mark.parametrize("edge", [e for e in itc.EDGES if e[2] > 0], ids=[e[0] for e in itc.EDGES if e[2] > 0])
def test_the_gpu_edges_keep_their_float32_floors(edge):
    """The same for the edges (sample counts 1 / 64 / 65 / 130, live counts 1 .. 2049): each has at least one live sample and a gradient."""
    _floors(itc.edge_setup(edge), 1)


def _floors(setup, least_live):
    _, spec, w, bufs, hit, cone, kn, okw = setup
    head = itc.quadratic_head(len(hit))
    own = itc.restated(w, spec, bufs, hit, cone, head, dtype=torch.float32, **okw)
    pat = dict(masks=own.masks, branch_masks=own.branch_masks, sigma_mask=own.sigma_mask)
    f32 = itc.restated(w, spec, bufs, hit, cone, head, dtype=torch.float32, **okw, **pat)
    want = itc.restated(w, spec, bufs, hit, cone, head, **okw, **pat)
    assert len(want.live) >= least_live and np.array_equal(f32.grad, own.grad)
    rows = [(name, rel_linf(f32.grad[sl], want.grad[sl]), float(np.abs(want.grad[sl]).max())) for name, sl in layer_slices(spec)]
    for r in rows:
        print(f"  {r[0]:<24} floor {r[1]:.2e} max {r[2]:.3e}")
    assert np.abs(want.grad).max() > 1e-6 and all(r[2] > 0 for r in rows)
    assert all(r[1] <= 5e-4 for r in rows), [r for r in rows if r[1] > 5e-4]
    P = want.param_grad.shape[-1]
    from tests import param_grad_common as pgc
    if least_live >= 100:                                      # (the parameter gradients are tested on the cases, not on the edges)
        pgc.fair(want.param_grad.reshape(-1, P), f32.param_grad.reshape(-1, P))
    live = itc.live_mask(hit, bufs[3])
    assert np.all(want.param_grad[~live] == 0) and rel_linf(f32.pred, want.pred) <= 1e-4
