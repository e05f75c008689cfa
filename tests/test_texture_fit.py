"""Learnable parameter textures on the CPU: the new entry is declared, bound and exported and refuses NULL without a device; `texture_lookup`
is `oracle.instancer_oracle.interpolate2d` bit for bit in float32; its autograd gradient is its adjoint; `apply_textures` touches only its
columns; and the scenes of tests/test_gpu_texture_fit.py are fair (decided here, from the oracle alone)."""

import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import instancer_oracle as io
from tests import texture_fit_common as tfc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_bound_and_exported():
    from nerf_tex_amd import _lib
    assert "ntx_instancer_sample_uv" in _lib.SYMBOLS and len(_lib.SYMBOLS["ntx_instancer_sample_uv"][1]) == 10
    assert hasattr(C.CDLL(_lib.LIB_PATH), "ntx_instancer_sample_uv") and callable(_lib.lib.ntx_instancer_sample_uv)


def test_the_prototype_is_declared_and_the_abi_is_still_7():
    from nerf_tex_amd import _lib
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "nerftex.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ntx_instancer_sample_uv\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m, "include/nerftex.h does not declare ntx_instancer_sample_uv"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0] == "ntx_instancer *inst" and args[8] == "float *uv_out" and args[9] == "uint8_t *found_out", args
    assert header.rstrip().endswith("#endif") and header.index("ntx_instancer_sample_uv") > header.index("ntx_trainer_weight_cotangent")      # appended
    assert _lib.lib.ntx_abi_version() == _lib.ABI_VERSION == 7 and re.search(r"#define\s+NTX_ABI_VERSION\s+7\b", header)


def test_null_arguments_are_refused_without_a_device():
    """inst NULL: NTX_E_INVALID, whatever else is passed, and not NTX_E_NODEVICE / NTX_E_HIP on a machine without a GPU."""
    from nerf_tex_amd import _lib
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    for n_rays, n_pts in ((1, 1), (0, 1), (1, 0), (-1, 1)):
        assert _lib.lib.ntx_instancer_sample_uv(None, p, p, p, p, n_rays, n_pts, 0.5, p, p) == _lib.NTX_E_INVALID
        assert b"NULL" in _lib.lib.ntx_last_error()
    assert not any(buf)


# ---- texture_lookup = interpolate2d ----------------------------------------------------------------------------------------------------------
LOOKUP_SHAPES = [(1, 1), (2, 3), (12, 16), (1, 7)]


def coordinates(n):
    """Coordinates along an axis of n texels: 0 and 1, the texel centres, a hair below and above every texel boundary, and values outside [0, 1]
    on both sides (below zero truncation and floor differ)."""
    vals = [0.0, 1.0, 0.5, 0.3137, -0.0, -1e-3, -0.3, -1.0, -2.6, 1.0 + 1e-3, 1.2, 2.5, np.nextafter(F(1), F(0)), np.nextafter(F(1), F(2)), np.nextafter(F(0), F(1)),
            -np.nextafter(F(0), F(1))]
    for k in range(n):
        c = F(k) / F(max(n - 1, 1))
        vals += [c, np.nextafter(c, F(-1)), np.nextafter(c, F(2))]
    return np.unique(np.asarray(vals, F))


@pytest.mark.parametrize("shape", LOOKUP_SHAPES, ids=[f"{r}x{c}" for r, c in LOOKUP_SHAPES])
def test_texture_lookup_is_interpolate2d_bit_for_bit(shape):
    from nerf_tex_amd.fit import texture_lookup
    tex = tfc.texels(3, shape)
    us, vs = coordinates(shape[0]), coordinates(shape[1])
    uv = np.stack(np.meshgrid(us, vs, indexing="ij"), -1).reshape(-1, 2).astype(F)
    found = np.ones(len(uv), bool); found[::7] = False
    want = np.asarray([io.interpolate2d(x, tex) if f else F(1.0) for x, f in zip(uv, found)], F)
    got = texture_lookup(torch.as_tensor(tex), torch.as_tensor(uv), torch.as_tensor(found)).numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert len(np.unique(want)) > (1 if shape == (1, 1) else 2 * shape[0] * shape[1] if shape[0] * shape[1] < 8 else 15)     # the cases tell texels apart
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert not len(bad), (len(bad), uv[bad[:5]], got[bad[:5]], want[bad[:5]])
    # leading dimensions are kept, and a uint8 `found` (the C entry's) is taken like a bool one
    again = texture_lookup(torch.as_tensor(tex), torch.as_tensor(uv).reshape(len(us), len(vs), 2), torch.as_tensor(found.astype(np.uint8)).reshape(len(us), len(vs)))
    assert np.array_equal(again.numpy().reshape(-1), got)


@pytest.mark.parametrize("shape", LOOKUP_SHAPES, ids=[f"{r}x{c}" for r, c in LOOKUP_SHAPES])
def test_the_gradient_is_the_adjoint(shape):
    """<L(T), g> = <T, L^T g> in float64 for random T and g, L the linear part of the lookup (the lookup is affine: 1 where nothing is found)."""
    from nerf_tex_amd.fit import texture_lookup
    rng = np.random.default_rng(shape[0] * 31 + shape[1])
    n = 500
    uv = torch.as_tensor(rng.uniform(-0.2, 1.2, size=(n, 2)))
    found = torch.as_tensor(rng.uniform(size=n) < 0.8)
    T, g = torch.as_tensor(rng.normal(size=shape)), torch.as_tensor(rng.normal(size=n))
    linear = texture_lookup(T, uv, found) - texture_lookup(torch.zeros_like(T), uv, found)
    adj = torch.as_tensor(tfc.lookup_adjoint(shape, uv.numpy(), found.numpy(), g.numpy(), torch.float64))
    lhs, rhs = float((linear * g).sum()), float((T * adj).sum())
    assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= 1e-12 * max(abs(lhs), abs(rhs)), (lhs, rhs)
    leaf = T.clone().requires_grad_(True)                                                        # at another T: the same gradient
    (texture_lookup(leaf, uv, found) * g).sum().backward()
    assert np.allclose(leaf.grad.numpy(), adj.numpy(), rtol=1e-12, atol=1e-14)


def test_apply_textures_leaves_every_other_column_alone():
    from nerf_tex_amd.fit import apply_textures, texture_lookup
    rng = np.random.default_rng(4)
    n, S, P = 5, 9, 7
    pm = rng.normal(size=(n, S, P)).astype(F)
    pm[0, 0, 3] = np.nan; pm[1, 2, 4] = np.inf; pm[2, 2, 6] = -0.0
    uv = torch.as_tensor(rng.uniform(0, 1, size=(n, S, 2)).astype(F)); found = torch.as_tensor(rng.uniform(size=(n, S)) < 0.7)
    tex = [torch.as_tensor(tfc.texels(1, (12, 16))), torch.as_tensor(tfc.texels(2, (4, 3)))]
    out = apply_textures(torch.as_tensor(pm), [5, 0], tex, uv, found)
    assert out.shape == (n, S, P) and out.dtype == torch.float32 and out.data_ptr() != torch.as_tensor(pm).data_ptr()
    out = out.numpy()
    for c in (1, 2, 3, 4, 6):
        assert out[..., c].tobytes() == pm[..., c].tobytes(), c
    for c, t in ((5, tex[0]), (0, tex[1])):
        want = pm[..., c] * texture_lookup(t, uv, found).numpy()
        assert np.array_equal(out[..., c], want) and not np.array_equal(out[..., c], pm[..., c])
        assert np.array_equal(out[..., c][~found.numpy()], pm[..., c][~found.numpy()])           # nothing within reach: the parameter as given
    with pytest.raises(ValueError):
        apply_textures(torch.as_tensor(pm), [5, 0], tex[:1], uv, found)


def test_neutral_texture_is_one_texel_of_one():
    """The pixels of a 1 x 1 image of 255: through `load_texture`, unchanged by this feature, the 1 x 1 channel matrix holding 1.0."""
    from nerf_tex_amd.instancer import load_texture, neutral_texture, parse_textures
    t = neutral_texture()
    assert t.dtype == np.uint8 and t.shape == (1, 1) and t[0, 0] == 255
    one = np.ones((1, 1), F)
    assert len(load_texture(t)) == 1 and load_texture(t)[0].dtype == np.float32 and np.array_equal(load_texture(t)[0], one) and F(255) / F(255) == 1
    n, ld, ls, idx, mats = parse_textures([t, "", "light", t])
    assert (n, ld, ls, idx) == (6, 2, -1, [0, 5]) and all(np.array_equal(m, one) for m in mats)
    assert np.array_equal(io.texture_from_pixels(t)[0], one)                                     # the oracle's loadTexture reads it the same way
    # float32 input is still pixels, as before this feature: cast to uint8, divided by 255
    assert np.array_equal(load_texture(np.full((2, 3), 255.0, F))[0], np.ones((3, 2), F)) and np.array_equal(load_texture(np.ones((1, 1), F))[0], np.full((1, 1), F(1) / F(255)))


# ---- the GPU file's scenes, judged here ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", tfc.UV_CASES, ids=tfc.UV_IDS)
def test_the_uv_cases_are_fair(case):
    """From the oracle alone: in every case at least a tenth of the in-patch samples find the sheet and one does not (the one sample of 1 x 1
    finds it); rays that miss have no in-patch sample.  (The GPU test asserts the same on the GPU's own t and dists before it compares.)"""
    cid, n, S, mean, method, scale, miss_every, seed = case
    box, tr, sheet = tfc.scene()
    o, d = tfc.rays(seed, n, miss_every)
    t, dists = tfc.oracle_march(box, tr, sheet, o, d, tfc.parameters(61, n), S, tfc.STEP, 8, mean, method, scale)
    uv, found = tfc.oracle_uv(sheet, tfc.max_extent(box, scale), o, d, t, dists, tfc.STEP, mean)
    inside = dists > 0
    if n * S == 1:
        assert inside.all() and found.all()
    else:
        tfc.fair_uv(found, dists)
    if miss_every:
        assert not inside[::miss_every].any() and inside.any()
    assert not uv[~found].any()


def test_the_gradient_case_is_fair():
    """The GPU file's gradient case on the CPU: dL/d params_map from the float64 restatement of the instanced step (the trainer's stand-in) on
    the oracle's buffers, pushed through the lookup's adjoint in float64 and in float32 -- the float32 restatement alone sits 2x inside
    `pgc.fair`'s guards for both textures, and some texels of the 12 x 16 texture are read by no sample."""
    from tests import instanced_train_common as itc
    from tests import param_grad_common as pgc
    from tests.common import make_model
    g_ = tfc.GRAD
    n, S = g_["n"], g_["S"]
    box, tr, sheet = tfc.scene()
    o, d = tfc.rays(g_["seed"], n)
    bufs = list(tfc.oracle_march(box, tr, sheet, o, d, tfc.parameters(g_["seed"], n), S, tfc.STEP, 8, patch_scale=tfc.PATCH_SCALE, full=True))
    uv, found = tfc.oracle_uv(sheet, tfc.max_extent(box, tfc.PATCH_SCALE), o, d, bufs[2], bufs[3], tfc.STEP, False)
    tex = [tfc.texels(g_["tex_seed"] + i, s) for i, s in enumerate(tfc.SHAPES)]
    from nerf_tex_amd.fit import apply_textures
    neutral = bufs[9].copy()
    bufs[9] = apply_textures(torch.as_tensor(neutral), [0, 1], [torch.as_tensor(t) for t in tex], torch.as_tensor(uv), torch.as_tensor(found)).numpy()
    _, spec, wts = make_model(pgc.SMALL[0], dense_media=True, arch=pgc.SMALL[1])
    cone = np.random.default_rng(2).uniform(1e-3, 5e-3, size=n).astype(F)
    out = itc.restated(wts, spec, bufs, bufs[8], cone, itc.quadratic_head(n), patch_scale=tfc.PATCH_SCALE, density_scale=tfc.DENSITY_SCALE)
    want = tfc.texture_gradients(tfc.SHAPES, [0, 1], uv, found, neutral, out.param_grad, torch.float64)
    f32 = tfc.texture_gradients(tfc.SHAPES, [0, 1], uv, found, neutral, out.param_grad, torch.float32)
    for w, f in zip(want, f32):
        pgc.fair(w.reshape(-1, 1), f.reshape(-1, 1), margin=pgc.MARGIN)
    touched = tfc.lookup_adjoint(tfc.SHAPES[0], uv, found, np.ones(found.shape), torch.float64) != 0
    assert 10 < touched.sum() < touched.size and not want[0][~touched].any()
