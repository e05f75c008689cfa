"""Training a ParamNerf with parameter branches (param_depth > 0, model.py:88-101), the part that needs no GPU: the float64 restatement of
the step the GPU tests compare with (tests/train_branch_oracle.py) against the oracle's own forward pass, against `tro.step_gradients` where
there are no branches and against finite differences; that the cases of tests/test_gpu_train_branches.py are fair ones; and what
`ntx_trainer_create_flex_ex` accepts and refuses before it asks for a device."""

import ctypes as C

import numpy as np
import pytest
import torch

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro
from tests import train_branch_oracle as bro
from tests.common import make_model, random_samples
from tests.train_common import BKGD, F, LOSSES, layer_slices, targets

# the architectures of the issue: (n_parameters, arch)
ARCHS = [((1, 6), dict(depth=8, width=256, skips=[4], color_depth=1, param_depth=1)),
         ((1, 4), dict(depth=4, width=128, skips=[1, 2], color_depth=0, param_depth=3, param_width=64)),
         ((4, 8), dict(depth=6, width=200, skips=[0, 4], color_depth=2, param_depth=4, param_width=100)),
         ((0, 5), dict(depth=5, width=256, skips=[2], color_depth=1, param_depth=2)),
         ((3, 0), dict(depth=5, width=256, skips=[2], color_depth=1, param_depth=2)),
         ((1, 6), dict(depth=1, width=96, skips=[], color_depth=3, param_depth=1, param_width=2))]
ARCH_IDS = ["reference_pd1", "cd0_pd3_pw64", "all_slots_pd4_pw100", "appearance_only", "geometry_only", "depth1_pw2"]


@pytest.mark.parametrize("npar,arch", ARCHS, ids=ARCH_IDS)
def test_forward_is_the_oracles(npar, arch):
    """The new restatement's float64 forward pass equals orc.model_forward in float64 on 64 random samples: 1e-12, the figure
    tests/test_oracle_train.py uses between two float64 evaluations."""
    _, spec, wts = make_model(npar, arch=arch)
    pos, dirs, params = random_samples(64, sum(npar), seed=5)
    t64 = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    with torch.no_grad():
        color, alpha = bro.model_forward([t64(x) for x in wts], spec, t64(pos), t64(dirs), t64(params))
    rc, ra = orc.model_forward(wts, spec, pos, dirs, params, dtype=np.float64)
    np.testing.assert_allclose(color.numpy(), rc, rtol=0, atol=1e-12)
    np.testing.assert_allclose(alpha.numpy(), ra, rtol=0, atol=1e-12)


def small_batch(spec, n=12, S=9, seed=2, fam="carpet"):
    ro, rd, t, cone, params, color, alpha = bro.branch_batch(seed, n, spec, fam)
    z = orc.z_values_perturbed(t, S, seed, F)
    return ro, rd, z, params, cone, color, alpha


@pytest.mark.parametrize("npar,arch", [((1, 6), dict(depth=3, width=32, skips=[1], param_depth=0)), ((0, 0), dict(depth=5, width=32, skips=[2], param_depth=2))],
                         ids=["param_depth0", "no_parameters_pd2"])
def test_without_branches_it_is_the_oracles_step(npar, arch):
    """param_depth 0, and param_depth 2 on a model without parameters (model.py:88, 96: no branch then): loss and every gradient are
    tro.step_gradients', 1e-12."""
    _, spec, wts = make_model(npar, arch=arch)
    assert not any(n.startswith("param_") for n, _, _ in orc.layer_table(spec))
    ro, rd, z, params, cone, color, alpha = small_batch(spec)
    kw = dict(blur_idx=0 if npar[0] else None, composite_bkgd=True, bkgd=BKGD, noise=0.1 * orc.noise_normals(len(z), z.shape[1], 4).astype(np.float64))
    okw = LOSSES["alpha_smape"][0]
    v0, c0, a0, g0 = tro.step_gradients(wts, spec, ro, rd, z, params, cone, color, alpha, okw, **kw)
    v1, c1, a1, g1 = bro.step_gradients(wts, spec, ro, rd, z, params, cone, color, alpha, okw, **kw)
    assert abs(v0 - v1) <= 1e-12 and len(g0) == len(g1)
    np.testing.assert_allclose(c1, c0, rtol=0, atol=1e-12); np.testing.assert_allclose(a1, a0, rtol=0, atol=1e-12)
    for x, y in zip(g0, g1):
        np.testing.assert_allclose(y, x, rtol=0, atol=1e-12)
    assert max(np.abs(x).max() for x in g0) > 1e-6


def test_autograd_matches_finite_differences():
    """Central differences (h = 1e-6, rel 2e-5, abs 1e-9: tests/test_oracle_train.py::test_autograd_matches_finite_differences) on a tiny
    branch network with blur_idx 0, noise and a background: one random element per kernel and bias, branch layers included.  Handing the
    oracle its own ReLU patterns changes nothing."""
    _, spec, wts = make_model((1, 2), arch=dict(depth=3, width=8, skips=[1], param_depth=2, param_width=4))
    rng = np.random.default_rng(0)
    wts = [np.asarray(x, np.float64) + (0.05 * rng.standard_normal(x.shape) if x.ndim == 1 else 0) for x in wts]       # biases off zero
    ro, rd, z, params, cone, color, alpha = small_batch(spec, n=6, S=5)
    okw = LOSSES["alpha_smape"][0]
    noise = 0.1 * orc.noise_normals(len(z), z.shape[1], 4).astype(np.float64)
    kw = dict(blur_idx=0, composite_bkgd=True, bkgd=BKGD, noise=noise)
    f = lambda w: bro.step_gradients(w, spec, ro, rd, z, params, cone, color, alpha, okw, **kw)
    val, c, a, grad = f(wts)
    assert len(grad) == len(wts) == 2 * len(orc.layer_table(spec)) and sum(n.startswith("param_") for n, _, _ in orc.layer_table(spec)) == 4
    h = 1e-6
    for j, x in enumerate(wts):
        idx = tuple(int(rng.integers(0, s)) for s in x.shape)
        up, down = [y.copy() for y in wts], [y.copy() for y in wts]
        up[j][idx] += h; down[j][idx] -= h
        fd = (f(up)[0] - f(down)[0]) / (2 * h)
        assert abs(fd - grad[j][idx]) <= 2e-5 * abs(fd) + 1e-9, (j, idx, fd, grad[j][idx])
    masks, branch_masks, sigma_mask = bro.own_masks(wts, spec, ro, rd, z, params, cone, blur_idx=0, noise=noise, dtype=torch.float64)
    assert len(masks) == 3 + 1 + 1 and len(branch_masks) == 4 and all(m.shape == (z.size, 4) for m in branch_masks)
    val2, c2, a2, grad2 = bro.step_gradients(wts, spec, ro, rd, z, params, cone, color, alpha, okw, masks=masks, branch_masks=branch_masks, sigma_mask=sigma_mask, **kw)
    assert val2 == val and all(np.array_equal(x, y) for x, y in zip(grad, grad2))


@pytest.mark.parametrize("case", bro.GPU_CASES, ids=[c[0] for c in bro.GPU_CASES])
def test_the_gpu_cases_are_fair(case):
    """Every case of tests/test_gpu_train_branches.py::test_gradients_of_every_layer_match_float64_autograd -- same model, batch and seeds --
    with the ReLU patterns of a float32 torch forward of the oracle itself: every layer's float32-vs-float64 floor is <= 5e-4, every layer
    has a gradient, the largest is > 1e-6.  So the GPU test's bars can be met by a correct float32 step."""
    model, spec, wts, (ro, rd, t, cone, params, color, alpha), kn, seed = bro.case_setup(case)
    n, S = bro.N_RAYS, bro.N_SAMPLES
    z = orc.z_values_perturbed(t, S, seed, F) if kn["perturb"] else orc.z_values(t, S, F)
    noise = kn["noise_std"] * orc.noise_normals(n, S, seed, dtype=F).astype(np.float64) if kn["noise_std"] > 0 else None
    masks, branch_masks, sigma_mask = bro.own_masks(wts, spec, ro, rd, z, params, cone, blur_idx=kn["blur"], noise=noise)
    assert len(branch_masks) == bro.n_branch_relu(spec) > 0
    okw = LOSSES[kn["loss_name"]][0]
    kw = dict(blur_idx=kn["blur"], map_exr=kn["map_exr"], composite_bkgd=kn["bkgd"], bkgd=BKGD, masks=masks, branch_masks=branch_masks, sigma_mask=sigma_mask, noise=noise)
    flat = lambda g: np.concatenate([np.asarray(x, np.float64).ravel() for x in g])
    want = flat(bro.step_gradients(wts, spec, ro, rd, z, params, cone, color, alpha, okw, **kw)[3])
    f32 = flat(bro.step_gradients(wts, spec, ro, rd, z, params, cone, color, alpha, okw, dtype=torch.float32, **kw)[3])
    rows = bro.floors(spec, want, f32)
    for name, floor, biggest in rows:
        print(f"  {name:<24} floor {floor:.2e} max {biggest:.3e}")
    assert len(rows) == 2 * len(model.layer_table()) and want.size == model.n_weight_floats()
    assert np.abs(want).max() > 1e-6 and all(r[2] > 0 for r in rows)
    assert all(r[1] <= 5e-4 for r in rows), [r for r in rows if r[1] > 5e-4]


def create_ex(desc, n_floats, max_rays=0, samples=64):
    from nerf_tex_amd import _lib
    desc.kind = _lib.KIND_PARAMNERF_EX
    blob, h = np.zeros(max(1, n_floats), np.float32), C.c_void_p()
    rc = _lib.lib.ntx_trainer_create_flex_ex(C.byref(desc), blob.ctypes.data_as(C.POINTER(C.c_float)), n_floats, 0, max_rays, samples, C.byref(h))
    assert rc != _lib.NTX_OK and not h.value
    return rc


@pytest.mark.parametrize("npar,arch", ARCHS, ids=ARCH_IDS)
def test_the_entry_accepts(npar, arch):
    """Every architecture above passes the check of `ntx_trainer_create_flex_ex`: max_rays = 0 is then NTX_E_INVALID, before any device is
    asked for; so are samples per ray outside 2..1024 and a wrong weight count."""
    from nerf_tex_amd import _lib
    model, _, _ = make_model(npar, arch=arch)
    n = model.n_weight_floats()
    assert n == _lib.lib.ntx_weight_count(C.byref(model.desc()))
    assert create_ex(model.desc(), n) == _lib.NTX_E_INVALID
    assert create_ex(model.desc(), n, max_rays=4, samples=1) == _lib.NTX_E_INVALID and create_ex(model.desc(), n, max_rays=4, samples=1025) == _lib.NTX_E_INVALID
    assert create_ex(model.desc(), n - 1, max_rays=4) == _lib.NTX_E_INVALID and b"floats" in _lib.lib.ntx_last_error()


def test_what_the_entry_refuses():
    """NTX_E_UNSUPPORTED although max_rays = 0 would be NTX_E_INVALID: param_depth 5 and -1, param_width 129 and 1, an IPE model, a skip at
    depth - 1, width 258; a descriptor that does not say it is the extended one."""
    from nerf_tex_amd import _lib
    base, _, _ = make_model((1, 6), arch=dict(depth=6, param_depth=2))

    def desc(**kw):
        d = base.desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert create_ex(desc(), 1000) == _lib.NTX_E_INVALID
    ipe, _, _ = make_model((1, 3), kind="IPE")
    for name, d in (("pd 5", desc(param_depth=5)), ("pd -1", desc(param_depth=-1)), ("pw 129", desc(param_width=129)), ("pw 1", desc(param_width=1)), ("ipe", ipe.desc()),
                    ("skip at depth-1", desc(skip=5)), ("skip mask with depth-1", desc(skip=_lib.SKIP_MASK | 0b100010)), ("width 258", desc(width=258))):
        assert create_ex(d, 1000) == _lib.NTX_E_UNSUPPORTED, name
    assert create_ex(desc(param_depth=0, param_width=0), 1000) == _lib.NTX_E_INVALID          # param_width counts only where there are layers
    plain, h, blob = desc(), C.c_void_p(), np.zeros(1000, np.float32)
    plain.kind = 0
    assert _lib.lib.ntx_trainer_create_flex_ex(C.byref(plain), blob.ctypes.data_as(C.POINTER(C.c_float)), 1000, 0, 0, 64, C.byref(h)) == _lib.NTX_E_UNSUPPORTED


def test_the_chooser_with_branches():
    """`trainer_class_for(m, branches=True)` is `BranchTrainer` for a model with branches; the default still raises NTX_E_UNSUPPORTED for it;
    models without branches are picked as before under either value."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer, Trainer, trainer_class_for
    assert issubclass(BranchTrainer, FlexTrainer)
    for npar, arch in ARCHS:
        m = make_model(npar, arch=arch)[0]
        assert trainer_class_for(m, branches=True) is BranchTrainer
        with pytest.raises(_lib.NtxError) as e:
            trainer_class_for(m)
        assert e.value.code == _lib.NTX_E_UNSUPPORTED
    for branches in (False, True):
        assert trainer_class_for(make_model((1, 6))[0], branches=branches) is Trainer
        assert trainer_class_for(make_model((1, 6), arch=dict(depth=6))[0], branches=branches) is FlexTrainer
        assert trainer_class_for(make_model((0, 0), arch=dict(depth=5, skips=[2], param_depth=2))[0], branches=branches) is FlexTrainer      # no parameters: no branches
        assert trainer_class_for(make_model((0, 0), kind="Nerf")[0], branches=branches) is FlexTrainer
        with pytest.raises(_lib.NtxError) as e:
            trainer_class_for(make_model((1, 6), arch=dict(depth=6, skips=[5], param_depth=1))[0], branches=branches)
        assert e.value.code == _lib.NTX_E_UNSUPPORTED
