"""Learnable parameter textures on the GPU (`ntx_instancer_sample_uv`, `nerf_tex_amd.fit.texture_lookup` / `apply_textures` / `TextureFitter`):
uv and found against the oracle's point query bit for bit, params_map against the textured instancer's own bit for bit, texels.grad against the
float64 adjoint of the lookup, the refusals, a side stream, and a fit end to end.  `-m gpu`.  The scenes are tests/texture_fit_common.py's,
judged fair on the CPU by tests/test_texture_fit.py."""

import ctypes as C

import numpy as np
import pytest

from tests import texture_fit_common as tfc
from tests.test_gpu_instancer import gpu_instancer, random_pixels

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
SENTINEL = -7.25


def dev():
    return torch.device("cuda", 0)


def make_instancer(textures, patch_scale, mean=False, method="nearest", **kw):
    """The scene with the wavy sheet as its instancer mesh; "T" entries of `textures` are neutral textures."""
    from nerf_tex_amd.instancer import neutral_texture
    box, tr, sheet = tfc.scene()
    textures = [neutral_texture() if isinstance(t, str) and t == "T" else t for t in textures]
    inst = gpu_instancer(box, tr, textures=textures, instance_sampling_method=method, use_mean_distance=mean, instancer_mesh=sheet, patch_scale=patch_scale, **kw)
    return inst, box, sheet


@pytest.mark.parametrize("case", tfc.UV_CASES, ids=tfc.UV_IDS)
def test_uv_and_found_are_the_oracles_point_query(case):
    cid, n, S, mean, method, scale, miss_every, seed = case
    inst, box, sheet = make_instancer(tfc.TEXTURES[1], scale, mean, method)
    assert inst.patch_max_extent == tfc.max_extent(box, scale)
    o, d = tfc.rays(seed, n, miss_every)
    bufs = inst.get_model_input(o, d, tfc.parameters(61, n), S, tfc.STEP, seed=8)
    uv, found = inst.sample_uv(o, d, bufs, tfc.STEP)
    assert uv.shape == (n, S, 2) and uv.dtype == torch.float32 and found.shape == (n, S) and found.dtype == torch.bool and uv.is_cuda and found.is_cuda
    t, dists, uv, found = bufs[2].cpu().numpy(), bufs[3].cpu().numpy(), uv.cpu().numpy(), found.cpu().numpy()
    want_uv, want_found = tfc.oracle_uv(sheet, inst.patch_max_extent, o, d, t, dists, tfc.STEP, mean)
    inside = dists > 0
    print(f"{cid}: {int(inside.sum())} in-patch samples of {n * S}, {int(want_found.sum())} find the sheet")
    if n * S == 1:
        assert inside.all() and want_found.all()
    else:
        tfc.fair_uv(want_found, dists)
    if miss_every:
        assert not inside[::miss_every].any()
    assert np.array_equal(found, want_found), int((found != want_found).sum())
    assert np.array_equal(uv, want_uv), (int((uv != want_uv).any(-1).sum()), np.abs(uv - want_uv).max())
    assert not uv[~inside].any() and not found[~inside].any() and (~inside).any() == (n * S > 1)   # outside every patch: exact zeros
    assert len(np.unique(uv[found], axis=0)) >= min(20, int(found.sum()))


@pytest.mark.parametrize("n_tex", [1, 2])
def test_params_map_is_the_textured_instancers(n_tex):
    """A textured instancer that makes a lookup per step against a neutral one + `sample_uv` + `apply_textures`: every buffer equal, params_map
    included.  The mode switch (ntx_instancer.hip: tex_interp = n_tex < S with n_tex = max(uint32(n_texture_samples * total), min_texture_samples))
    is held on the per-step side by min_texture_samples >= S alone, whatever a ray's length in its patches is."""
    from nerf_tex_amd.fit import apply_textures
    from nerf_tex_amd.instancer import load_texture
    n, S, scale = 70, 33, tfc.REACH
    pixels = [random_pixels(1), random_pixels(2, h=9, w=7)][:n_tex]
    entries = lambda tex: list(tex) + [""] * (4 - n_tex) + ["light"]
    tkw = dict(n_texture_samples=10 ** 6, min_texture_samples=64)
    assert tkw["min_texture_samples"] >= S                                                       # n_tex >= min_texture_samples >= S on every ray: a lookup per step
    textured, _, _ = make_instancer(entries(pixels), scale, **tkw)
    neutral, _, _ = make_instancer(entries(["T"] * n_tex), scale, **tkw)
    assert textured.tex_idx == neutral.tex_idx == list(range(n_tex)) and textured.n_parameters == neutral.n_parameters == 7
    o, d = tfc.rays(61, n)
    par = np.random.default_rng(3).uniform(0.3, 2.0, size=(n, 7)).astype(F)
    want = textured.get_model_input(o, d, par, S, tfc.STEP, seed=8)
    bufs = neutral.get_model_input(o, d, par, S, tfc.STEP, seed=8)
    uv, found = neutral.sample_uv(o, d, bufs, tfc.STEP)
    mats = [torch.as_tensor(load_texture(px)[0], device=dev()) for px in pixels]
    assert [tuple(m.shape) for m in mats] == [(16, 12), (7, 9)][:n_tex]
    field = apply_textures(bufs[9], neutral.tex_idx, mats, uv, found)
    inside, fnd = (bufs[3] > 0).cpu().numpy(), found.cpu().numpy()
    tfc.fair_uv(fnd, bufs[3].cpu().numpy())
    got_pm, want_pm, plain = field.cpu().numpy(), want[9].cpu().numpy(), bufs[9].cpu().numpy()
    assert np.array_equal(plain[..., :4], np.repeat(par[:, None, :4], S, 1))                     # neutral: params_map untextured
    ratio = want_pm[..., 0][fnd] / plain[..., 0][fnd]
    assert ratio.min() < 0.5 and ratio.max() > 0.7 and len(np.unique(ratio)) > 100               # the texture shows
    assert np.array_equal(got_pm, want_pm), (int((got_pm != want_pm).sum()), np.abs(got_pm - want_pm).max())
    for k in range(9):
        assert torch.equal(bufs[k], want[k]), k
    assert inside.sum() > 500


def test_texel_gradients_against_the_float64_adjoint():
    """texels.grad after a `DifferentiableInstanceRender` step against the float64 adjoint of the lookup applied to the trainer's own
    `sample_parameter_gradients()`, per texture at the standing bar: rel-Linf <= max(1e-4, 4 x the float32 CPU restatement's floor) under
    `pgc.fair`'s guards; texels no sample reads have gradient exactly 0."""
    from nerf_tex_amd.autograd import DifferentiableInstanceRender
    from nerf_tex_amd.fit import apply_textures
    from nerf_tex_amd.train import FlexTrainer
    from tests import instanced_train_common as itc
    from tests import param_grad_common as pgc
    from tests.common import make_model
    g_ = tfc.GRAD
    n, S = g_["n"], g_["S"]
    inst, box, sheet = make_instancer(tfc.TEXTURES[2], tfc.PATCH_SCALE)
    model = make_model(pgc.SMALL[0], dense_media=True, arch=pgc.SMALL[1])[0]
    tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=False, param_gradients="only")
    o, d = tfc.rays(g_["seed"], n)
    bufs = inst.get_model_input(o, d, tfc.parameters(g_["seed"], n), S, tfc.STEP, seed=8)
    uv, found = inst.sample_uv(o, d, bufs, tfc.STEP)
    tex = [torch.as_tensor(tfc.texels(g_["tex_seed"] + i, s), device=dev()).requires_grad_(True) for i, s in enumerate(tfc.SHAPES)]
    field = apply_textures(bufs[9], inst.tex_idx, tex, uv, found)
    cone = torch.as_tensor(np.random.default_rng(2).uniform(1e-3, 5e-3, size=n).astype(F), device=dev())
    color, alpha = DifferentiableInstanceRender(tr, patch_scale=tfc.PATCH_SCALE, density_scale=tfc.DENSITY_SCALE)(bufs, cone, params_map=field, hit=inst.last_hit)
    itc.quadratic_head(n)(color, alpha).backward()
    g = tr.sample_parameter_gradients().cpu().numpy()
    got = [t.grad.cpu().numpy() for t in tex]
    uv_, found_, plain = uv.cpu().numpy(), found.cpu().numpy(), bufs[9].cpu().numpy()
    assert tr.last_live > 500 and np.abs(g[..., :2]).max() > 0
    want = tfc.texture_gradients(tfc.SHAPES, inst.tex_idx, uv_, found_, plain, g, torch.float64)
    f32 = tfc.texture_gradients(tfc.SHAPES, inst.tex_idx, uv_, found_, plain, g, torch.float32)
    res = tfc.check_texture_gradients(got, want, f32)
    print("texture gradients: rel-Linf", [float(r.errs[0]) for r in res], "float32 floors", [float(r.floors[0]) for r in res])
    touched = tfc.lookup_adjoint(tfc.SHAPES[0], uv_, found_, np.ones(found_.shape), torch.float64) != 0
    assert 10 < touched.sum() < touched.size and not got[0][~touched].any()


def test_refusals_write_nothing():
    from nerf_tex_amd import _lib
    n, S = 6, 5
    z = lambda *shape, dt=torch.float32: torch.full(shape, SENTINEL if dt == torch.float32 else 113, device=dev(), dtype=dt)
    o, d = (torch.as_tensor(a, device=dev()) for a in tfc.rays(61, n))
    t, dists, uv, found = torch.full((n, S), 4.0, device=dev()), torch.full((n, S), 0.04, device=dev()), z(n, S, 2), z(n, S, dt=torch.uint8)

    def call(inst, n_rays, n_pts, uv_ptr=None):
        rc = _lib.lib.ntx_instancer_sample_uv(inst._h, o.data_ptr(), d.data_ptr(), t.data_ptr(), dists.data_ptr(), n_rays, n_pts, tfc.STEP,
                                              uv.data_ptr() if uv_ptr is None else uv_ptr, found.data_ptr())
        return rc, _lib.lib.ntx_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool((uv == SENTINEL).all()) and bool((found == 113).all())

    box, tr, sheet = tfc.scene()
    bare = gpu_instancer(box, tr, textures=["", "", "", "", "light"], instance_sampling_method="nearest")
    rc, msg = call(bare, n, S)
    assert rc == _lib.NTX_E_INVALID and "parameter textures" in msg and untouched()
    rc, msg = call(bare, n, 0)                                                                   # the header's order: NULL arguments, the sizes, then the textures
    assert rc == _lib.NTX_E_INVALID and "n_pts" in msg and untouched()
    rc, msg = call(bare, n, 0, uv_ptr=C.c_void_p(None))
    assert rc == _lib.NTX_E_INVALID and "NULL" in msg and untouched()
    with pytest.raises(_lib.NtxError) as e:
        bare.sample_uv(o, d, (None, None, t, dists), tfc.STEP)
    assert e.value.code == _lib.NTX_E_INVALID
    inst, _, _ = make_instancer(tfc.TEXTURES[1], tfc.PATCH_SCALE)
    for n_pts in (0, 4097):
        rc, msg = call(inst, n, n_pts)
        assert rc == _lib.NTX_E_INVALID and "n_pts" in msg and untouched()
    rc, msg = call(inst, -1, S)
    assert rc == _lib.NTX_E_INVALID and untouched()
    rc, msg = call(inst, n, S, uv_ptr=C.c_void_p(None))
    assert rc == _lib.NTX_E_INVALID and "NULL" in msg and untouched()
    assert call(inst, 0, S)[0] == _lib.NTX_OK and untouched()                                    # nothing to do: no launch
    assert call(inst, n, S)[0] == _lib.NTX_OK                                                    # and the call the refusals were variations of
    torch.cuda.synchronize()
    assert bool((found <= 1).all()) and bool(found.any()) and bool((uv != SENTINEL).all())       # every element of both outputs is written


def test_a_side_stream_gives_the_default_streams_bits():
    from tests import stream_common as sc
    n, S = 70, 33
    inst, _, _ = make_instancer(tfc.TEXTURES[1], tfc.REACH, mean=True)
    o, d = (torch.as_tensor(a, device=dev()) for a in tfc.rays(61, n))
    bufs = inst.get_model_input(o, d, tfc.parameters(61, n), S, tfc.STEP, seed=8)
    uv0, found0 = inst.sample_uv(o, d, bufs, tfc.STEP)
    torch.cuda.synchronize()
    s = sc.side_stream()
    with torch.cuda.stream(s):
        uv1, found1 = inst.sample_uv(o, d, bufs, tfc.STEP)
    s.synchronize()
    assert found0.any() and not found0.all()
    sc.same_bytes(sc.as_bytes([uv1, found1]), sc.as_bytes([uv0, found0]), "sample_uv on a side stream")
    # the march and the lookup both on the side stream while the null stream is busy (tests/stream_common.py's trap B): the entry runs on
    # the march's stream, and nothing waits for the null stream or the device
    par = torch.as_tensor(tfc.parameters(61, n), device=dev())
    torch.cuda.synchronize()
    busy = torch.cuda.Event()
    sc.delay(100.0)
    busy.record()
    with torch.cuda.stream(s):
        bufs2 = inst.get_model_input(o, d, par, S, tfc.STEP, seed=8)
        uv2, found2 = inst.sample_uv(o, d, bufs2, tfc.STEP)
        snaps = [uv2.clone(), found2.clone()]
    s.synchronize()
    still_busy = not busy.query()
    torch.cuda.synchronize()
    assert still_busy, "the delay on the null stream had completed behind s.synchronize(): something waited for the null stream or the device"
    sc.same_bytes(sc.as_bytes(snaps), sc.as_bytes([uv0, found0]), "march and sample_uv on a side stream, busy null stream")


# the class's default lrate; Adam moves a texel by at most lrate an iteration, the start is up to 0.38 off: 400 iterations are ten times that way
# (docs/DESIGN_instancer.md: why a small rate and enough iterations, for the texels few samples read)
E2E = dict(shape=(4, 3), batches=2, rays=128, S=32, start=0.6, lrate=1e-2, n_iters=400)


def fit_a_texture(e):
    """The end-to-end fit with the settings `e`: (loss history, the batches' count of `sample_uv` calls, the fitted texture, the teacher, the mask of
    texels a sample reads)."""
    from nerf_tex_amd.fit import TextureFitter, apply_textures
    from nerf_tex_amd.train import FlexTrainer
    from tests import param_grad_common as pgc
    from tests.common import make_model
    n, S, B = e["rays"], e["S"], e["batches"]
    inst, _, _ = make_instancer(tfc.TEXTURES[1], tfc.PATCH_SCALE, n_texture_samples=10 ** 6)
    model = make_model(pgc.SMALL[0], dense_media=True, arch=pgc.SMALL[1])[0]
    tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=False, param_gradients="only")
    fitter = TextureFitter(tr, inst, [e["shape"]], lrate=e["lrate"], bounds=(0., 1.), patch_scale=tfc.PATCH_SCALE, density_scale=tfc.DENSITY_SCALE, step_size=tfc.STEP, seed=40)
    teacher = torch.as_tensor(tfc.texels(9, e["shape"]), device=dev())
    batches, touched = [], np.zeros(e["shape"], bool)
    for k in range(B):
        o, d = tfc.rays(70 + k, n)
        par = tfc.parameters(61, n)
        cone = np.random.default_rng(k).uniform(1e-3, 5e-3, size=n).astype(F)
        bufs = inst.get_model_input(o, d, par, S, tfc.STEP, seed=fitter.seed + k)
        uv, found = inst.sample_uv(o, d, bufs, tfc.STEP)
        field = apply_textures(bufs[9], inst.tex_idx, [teacher], uv, found)
        color, alpha = tr.forward_instanced(bufs[:9] + (field,), cone, patch_scale=tfc.PATCH_SCALE, density_scale=tfc.DENSITY_SCALE, hit=inst.last_hit)
        assert tr.last_live > 300 and float(alpha.max()) > 0.3
        batches.append(dict(rays_o=o, rays_d=d, parameters=par, cone_scale=cone, color_true=color.clone(), alpha_true=alpha.clone()))
        touched |= tfc.lookup_adjoint(e["shape"], uv.cpu().numpy(), found.cpu().numpy(), np.ones(found.shape), torch.float64) != 0
    calls = []
    real = inst.sample_uv
    inst.sample_uv = lambda *a, **kw: (calls.append(1), real(*a, **kw))[1]
    mse = lambda color_true, alpha_true, color_pred, alpha_pred: torch.mean((color_pred - color_true) ** 2) + torch.mean((alpha_pred - alpha_true) ** 2)
    textures, history = fitter.fit(batches, mse, init=e["start"], n_iters=e["n_iters"])
    return history, len(calls), textures, teacher.cpu().numpy(), touched


def test_a_texture_is_fitted_end_to_end():
    """A teacher 4 x 3 texture on the geometry parameter renders 2 batches of 128 rays x 32 samples; a `TextureFitter` starts from a constant.  The
    final loss of each batch is below its first, the final max texel error over the texels a sample reads is below the initial one (no ratio
    is fixed: the run's figures are in profiles/texture_fit/fit_e2e.md), and `sample_uv` runs once per batch."""
    e = E2E
    B = e["batches"]
    history, calls, textures, teacher, touched = fit_a_texture(e)
    assert calls == B and len(history) == e["n_iters"] and len(textures) == 1 and tuple(textures[0].shape) == e["shape"]
    err = lambda t: float(np.abs(np.asarray(t, np.float64) - teacher)[touched].max())
    first, last = history[:B], history[-B:]
    err0, err1 = err(np.full(e["shape"], e["start"])), err(textures[0].cpu().numpy())
    print(f"texture fit: loss {first} -> {last} over {e['n_iters']} iterations; max texel error over {int(touched.sum())} read texels {err0:.4f} -> {err1:.4f}")
    assert touched.sum() >= 6 and np.isfinite(history).all()
    assert all(b < a for a, b in zip(first, last)), (first, last)
    assert err1 < err0, (err0, err1)
    assert float(textures[0].min()) >= 0.0 and float(textures[0].max()) <= 1.0
