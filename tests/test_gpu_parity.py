"""Parity of the HIP kernels (through the C ABI) against the CPU oracle.  `-m gpu` only.

Bar (BASELINE.json): rel-L-inf <= 1e-4 against the float64 restatement of the reference; the
tolerance is written next to each assert.  Integer/index work (culling, scatter) must be exact.
"""

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from tests.common import importance_depths, TOL, camera_rays, make_model, random_samples

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def dev():
    return torch.device("cuda", 0)


def to_dev(*arrs):
    return [torch.as_tensor(a, device=dev()) for a in arrs]


def test_native_library_is_loaded():
    from nerf_tex_amd import _lib
    assert _lib.lib.ntx_abi_version() == _lib.ABI_VERSION == 7
    with open("/proc/self/maps") as f:
        assert "libnerftex_hip.so" in f.read()


@pytest.mark.parametrize("d,nf", [(3, 10), (3, 4), (6, 4), (1, 4)])
def test_fourier_features(d, nf):
    from nerf_tex_amd.layer import FourierFeatures
    rng = np.random.default_rng(0)
    x = rng.uniform(-3, 3, size=(1000, d)).astype(np.float32)
    out = FourierFeatures(nf)(to_dev(x)[0]).cpu().numpy()
    ref = orc.fourier_features(x, nf, np.float64)
    assert out.shape == ref.shape
    # sin/cos of arguments up to 2^9 * 3 rad, <= 2 ulp of 1.0
    assert np.max(np.abs(out - ref)) <= 2.5e-7


@pytest.mark.parametrize("family,h,w", [("carpet", 40, 56), ("grass", 33, 17)])
def test_generate_rays(family, h, w):
    from nerf_tex_amd.ray_sampler import Proxy
    from nerf_tex_amd.proxy import AABB
    from nerf_tex_amd import synthetic
    fam = synthetic.FAMILIES[family]
    (ro, rd, t, cone), c2w, focal = camera_rays(family, h, w, np.float64)
    o, d, tt, cc = Proxy(h, w, focal, AABB(fam["b_0"], fam["b_1"]))((0, h * w), c2w)
    o, d, tt, cc = [v.cpu().numpy() for v in (o, d, tt, cc)]
    assert np.max(np.abs(o - ro)) <= 1e-6
    assert np.max(np.abs(d - rd)) <= 1e-6          # unit vectors, float32 rounding
    hit = np.isfinite(t[:, 0])
    assert hit.any() and (~hit).any()
    # hit/miss classification may only differ on rays grazing the box (t1 - t0 ~ 0)
    mism = np.isfinite(tt[:, 0]) != hit
    if mism.any():
        both = np.where(mism)[0]
        span = np.where(hit[both], t[both, 1] - t[both, 0], tt[both, 1] - tt[both, 0])
        assert np.all(np.abs(span) < 1e-4)
    ok = hit & ~mism
    assert np.max(np.abs(tt[ok] - t[ok]) / np.abs(t[ok])) <= 1e-5
    assert np.all(np.isinf(tt[~hit & ~mism]))
    assert np.max(np.abs(cc - cone) / cone) <= 1e-5


@pytest.mark.parametrize("S", [2, 32, 64, 100, 128])
@pytest.mark.parametrize("flags", [(False, False), (True, True)])
def test_composite(S, flags):
    from nerf_tex_amd.renderer import Renderer
    map_exr, bk = flags
    rng = np.random.default_rng(S)
    n = 257
    color = rng.normal(size=(n, S, 3)).astype(np.float32) * 2
    sigma = (rng.normal(size=(n, S)) * 20).astype(np.float32)
    sigma[0] = 1e6            # fully opaque first sample: transmittance floor 1e-10 (renderer.py:198)
    sigma[1] = -5.0           # relu -> empty ray
    z = np.sort(rng.uniform(2, 6, size=(n, S)), -1).astype(np.float32)
    rays_d = (rng.normal(size=(n, 3)) * 2).astype(np.float32)     # |d| != 1 (renderer.py:180)
    r = Renderer(model=None, map_exr=map_exr, perturb=False)
    c, a, w = r.map_model_output(*to_dev(color, sigma, z, rays_d), bk, [0.2, 0.5, 1.0])
    rc, ra, rw, _ = orc.map_model_output(color, sigma, z, rays_d, bk, [0.2, 0.5, 1.0], map_exr, None, np.float64)
    scale = max(1.0, float(np.max(np.abs(rc))))
    assert np.max(np.abs(w.cpu().numpy() - rw)) <= 1e-5                 # float32 exp/scan rounding
    assert np.max(np.abs(a.cpu().numpy() - ra)) <= 1e-5
    assert np.max(np.abs(c.cpu().numpy() - rc)) / scale <= 1e-5
    assert abs(float(a[1])) == 0.0


FAMS = [("ParamNerf", (1, 6)), ("ParamNerf", (1, 4)), ("ParamNerf", (2, 3)), ("Nerf", (0, 0))]


@pytest.mark.parametrize("kind,npar", FAMS)
@pytest.mark.parametrize("m", [1, 31, 4096 + 17])
def test_mlp_forward(kind, npar, m):
    model, spec, w = make_model(npar, kind)
    pos, dirs, params = random_samples(m, sum(npar))
    color, alpha = model(tuple(to_dev(pos, dirs, params)))
    rc, ra = orc.model_forward(w, spec, pos, dirs, params, np.float64)
    out = np.concatenate([color.cpu().numpy(), alpha.cpu().numpy()], -1)
    ref = np.concatenate([rc, ra], -1)
    err = orc.rel_linf(out, ref)
    assert err <= TOL, err          # north-star gate
    assert err <= 2e-5, err         # what exact-f32 MFMA should actually reach on glorot weights


@pytest.mark.parametrize("kind,npar", FAMS)
def test_mlp_forward_at_the_edge_of_the_encoder_domain(kind, npar):
    """The fused encoders evaluate sin_q alone, whose domain is |2^f x| < 2^17 (include/nerftex.h: |pos| < 256 at pos_freq 10):
    positions uniform in [-250, 250] against the float64 network on the same float32 points, at test_mlp_forward's bars."""
    m = 4096 + 17
    model, spec, w = make_model(npar, kind)
    pos, dirs, params = random_samples(m, sum(npar), box=250.0)
    assert 200 < float(np.abs(pos).max()) < 256
    color, alpha = model(tuple(to_dev(pos, dirs, params)))
    rc, ra = orc.model_forward(w, spec, pos, dirs, params, np.float64)
    err = orc.rel_linf(np.concatenate([color.cpu().numpy(), alpha.cpu().numpy()], -1), np.concatenate([rc, ra], -1))
    assert err <= TOL, err
    assert err <= 2e-5, err


@pytest.mark.parametrize("family,S", [("carpet", 32), ("carpet", 64), ("grass", 128), ("fur", 64), ("grass_filtered", 48)])
@pytest.mark.parametrize("bk", [False, True])
def test_render_rays_camera(family, S, bk):
    """Renderer.__call__ on a true camera grid (hits and misses), batch of 2 views' worth of rays."""
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.renderer import Renderer
    fam = synthetic.FAMILIES[family]
    model, spec, w = make_model(fam["n_parameters"], dense_media=True)
    h, wd = 24, 20
    (ro, rd, t, cone), _, _ = camera_rays(family, h, wd)
    B = 2
    params = np.stack([np.asarray(fam["params"], np.float32), np.asarray(fam["params"], np.float32) * 0.5])
    batch = lambda a: np.stack([a, a])
    r = Renderer(model=model, n_samples=S, perturb=False, blur_idx=fam["blur_idx"])
    out = r(*to_dev(batch(ro), batch(rd), batch(t)), parameters=to_dev(params)[0], cone_scale=to_dev(batch(cone))[0],
            composite_bkgd=bk, bkgd_color=[1, 1, 1.])
    r.raise_if_nonfinite()
    ref = orc.renderer_call(w, spec, batch(ro), batch(rd), batch(t), params, batch(cone), S, bk, (1., 1., 1.),
                            fam["blur_idx"], False, dtype=np.float64)
    c = out["color_pred"].cpu().numpy(); a = out["alpha_pred"].cpu().numpy()
    assert c.shape == (B, h * wd, 3) and a.shape == (B, h * wd)
    miss = ~np.isfinite(batch(t)[..., 0])
    assert miss.any() and (~miss).any()
    # culled rays are exact: 0 (or the background colour) and alpha 0  (renderer.py:81-86)
    assert np.all(a[miss] == 0.0)
    assert np.all(c[miss] == (1.0 if bk else 0.0))
    got = np.concatenate([c, a[..., None]], -1); want = np.concatenate([ref["color_pred"], ref["alpha_pred"][..., None]], -1)
    err = orc.rel_linf(got, want)
    assert err <= TOL, err
    assert float(np.max(want[..., 3])) > 0.3     # the dense-media weights give genuinely opaque-ish rays


def test_render_per_ray_params_and_zvals():
    """rays_per_param_row = 1 path (HW = 1) and caller-supplied z_vals (stratified jitter stand-in)."""
    from nerf_tex_amd.renderer import Renderer
    from nerf_tex_amd import synthetic
    model, spec, w = make_model((1, 6), dense_media=True)
    n, S = 70, 64
    fam = synthetic.FAMILIES["carpet"]
    ro, rd, t, cone = synthetic.all_hit_rays(n, fam["b_0"], fam["b_1"], fam["cam"])
    rng = np.random.default_rng(5)
    params = rng.uniform(0, 1, size=(n, 7)).astype(np.float32)
    z0 = orc.z_values(t, S, np.float32)
    lo, up = orc.jitter_bounds(z0)
    z = (lo + (up - lo) * rng.uniform(size=z0.shape).astype(np.float32)).astype(np.float32)
    r = Renderer(model=model, n_samples=S, perturb=True)
    out = r(*to_dev(ro[:, None], rd[:, None], t[:, None]), parameters=to_dev(params)[0],
            cone_scale=to_dev(cone[:, None])[0], z_vals=to_dev(z)[0])
    ref = orc.render_rays(w, spec, ro, rd, t, params, cone, S, False, (1, 1, 1.), z_override=z, dtype=np.float64)
    got = np.concatenate([out["color_pred"].cpu().numpy()[:, 0], out["alpha_pred"].cpu().numpy()], -1)
    want = np.concatenate([ref["color_pred"], ref["alpha_pred"][:, None]], -1)
    assert orc.rel_linf(got, want) <= TOL


def test_unsupported_model_fails_loudly():
    from nerf_tex_amd import _lib
    from nerf_tex_amd.model import ParamNerf
    from tests.common import EMB
    m = ParamNerf(EMB(10), EMB(4), EMB(4), [5, 3])["model"]        # more geometry parameters than the generic family's 4 slots
    with pytest.raises(_lib.NtxError) as e:
        m.ctx(0)
    assert e.value.code == _lib.NTX_E_UNSUPPORTED


def test_full_size_properties():
    """BASELINE config 1 size (800x800x64 carpet, all-hit rays): size-independent properties.
    (a) alpha in [0,1], colour <= alpha (premultiplied sigmoid colours); (b) the image does not depend
    on how the rays are split across calls (what sharding across GPUs relies on): bit-identical."""
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.renderer import Renderer
    fam = synthetic.FAMILIES["carpet"]
    model, spec, w = make_model((1, 6), dense_media=True)
    n, S = 800 * 800, 64
    ro, rd, t, cone = synthetic.all_hit_rays(n, fam["b_0"], fam["b_1"], fam["cam"])
    params = np.asarray([fam["params"]], np.float32)
    r = Renderer(model=model, n_samples=S, perturb=False)
    dro, drd, dt, dcone = to_dev(ro, rd, t, cone)
    full = r(dro[None], drd[None], dt[None], parameters=to_dev(params)[0], cone_scale=dcone[None])
    c, a = full["color_pred"][0], full["alpha_pred"][0]
    assert torch.isfinite(c).all() and torch.isfinite(a).all()
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 + 1e-6
    assert bool((c <= a[:, None] + 1e-6).all())
    # split into 3 uneven shards
    cuts = [0, 100_003, 400_000, n]
    parts_c, parts_a = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        o = r(dro[None, lo:hi], drd[None, lo:hi], dt[None, lo:hi], parameters=to_dev(params)[0], cone_scale=dcone[None, lo:hi])
        parts_c.append(o["color_pred"][0]); parts_a.append(o["alpha_pred"][0])
    assert torch.equal(torch.cat(parts_c), c) and torch.equal(torch.cat(parts_a), a)
    # spot-check 256 rays of the full-size render against the oracle
    idx = np.random.default_rng(0).choice(n, 256, replace=False)
    ref = orc.render_rays(w, spec, ro[idx], rd[idx], t[idx], np.repeat(params, 256, 0), cone[idx], S, False,
                          (1, 1, 1.), dtype=np.float64)
    got = np.concatenate([c[idx].cpu().numpy(), a[idx].cpu().numpy()[:, None]], -1)
    want = np.concatenate([ref["color_pred"], ref["alpha_pred"][:, None]], -1)
    assert orc.rel_linf(got, want) <= TOL


@pytest.mark.parametrize("h,w,f", [(64, 48, 1), (64, 48, 2), (50, 37, 2), (96, 96, 4), (33, 65, 3)])
@pytest.mark.parametrize("exr", [False, True])
def test_image_epilogue(h, w, f, exr):
    """logger.py:128-144 + interpolate.py:68-82."""
    from nerf_tex_amd.render import image_epilogue
    rng = np.random.default_rng(h * w + f)
    a = rng.uniform(0, 1, size=(h, w, 1)); a[rng.uniform(size=(h, w, 1)) < 0.3] = 0.0
    rgba = np.concatenate([rng.uniform(0, 1, size=(h, w, 3)) * a, a], -1).astype(np.float32)
    out, u8 = image_epilogue(to_dev(rgba)[0], f, write_exr=exr, uint8=True)
    ref = orc.image_epilogue(rgba, f, exr, np.float64)
    assert out.shape == ref.shape
    assert np.max(np.abs(out.cpu().numpy() - ref)) <= 2e-5 * max(1.0, float(np.abs(ref).max()))
    ref8 = orc.to_uint8(ref)
    d8 = np.abs(u8.cpu().numpy().astype(int) - ref8.astype(int))
    assert d8.max() <= 1 and (d8 > 0).mean() < 0.01          # float32 vs float64 may straddle a truncation boundary


@pytest.mark.parametrize("family,S,NI,fine", [("carpet", 32, 32, False), ("carpet", 64, 128, True), ("grass_filtered", 48, 17, False)])
@pytest.mark.parametrize("det", [True, False])
def test_hierarchical_sampling(family, S, NI, fine, det):
    """n_importance > 0 (renderer.py:125-138, sample_pdf 589-617): coarse pass -> weights ->
    inverse-CDF depths -> merged sorted depths -> fine pass (optionally with model_fine)."""
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.renderer import Renderer
    fam = synthetic.FAMILIES[family]
    model, spec, w = make_model(fam["n_parameters"], dense_media=True)
    model_f, w_f = None, None
    if fine:
        model_f, _, w_f = make_model(fam["n_parameters"], seed=5, dense_media=True)
    h, wd = 12, 10
    (ro, rd, t, cone), _, _ = camera_rays(family, h, wd)
    n = h * wd
    params = np.asarray([fam["params"]], np.float32)
    rng = np.random.default_rng(NI)
    u = None if det else rng.uniform(size=(n, NI)).astype(np.float32)
    # perturb=True is what makes the reference use the deterministic u (`det=self.perturb`); the coarse jitter
    # itself is pinned by passing the un-jittered depths explicitly
    z0 = orc.z_values(np.where(np.isfinite(t), t, 0), S, np.float32)
    r = Renderer(model=model, model_fine=model_f, n_samples=S, n_importance=NI, perturb=det, blur_idx=fam["blur_idx"])
    out = r(*to_dev(ro[None], rd[None], t[None]), parameters=to_dev(params)[0], cone_scale=to_dev(cone[None])[0],
            z_vals=to_dev(z0)[0], u=None if det else to_dev(u)[0])
    r.raise_if_nonfinite()
    hit = np.isfinite(t[:, 0])
    ref = orc.render_rays_hierarchical(w, w_f, spec, ro[hit], rd[hit], t[hit], np.repeat(params, hit.sum(), 0), cone[hit], S, NI,
                                       False, (1, 1, 1.), perturb=det, u=None if det else u[hit], blur_idx=fam["blur_idx"], dtype=np.float64)
    zg = r._last_z.cpu().numpy()[hit]
    assert np.all(np.diff(zg, axis=-1) >= 0)
    for k in ("color_pred", "alpha_pred", "color_pred_coarse", "alpha_pred_coarse"):
        assert out[k].shape[1] == n
    # (1) coarse pass: the strict gate
    got_c = np.concatenate([out["color_pred_coarse"][0].cpu().numpy()[hit], out["alpha_pred_coarse"][0].cpu().numpy()[hit][:, None]], -1)
    want_c = np.concatenate([ref["color_pred_coarse"], ref["alpha_pred_coarse"][:, None]], -1)
    assert orc.rel_linf(got_c, want_c) <= TOL
    # (2) the sampler on ITS inputs: every one of the n_importance depths of every ray against sample_pdf evaluated in float64 on
    # the kernel's own float32 coarse weights, within the float32 conditioning of the reference's formula (oracle sample_pdf:
    # return_conditioning -- tight wherever a bin holds weight, the whole bin in the empty bins of this dense medium, where
    # `denom < 1e-5 -> 1` and searchsorted are decided by the last bit; the float32 restatement ITSELF sits 6e-3 from float64
    # end to end on this case for that reason, so an end-to-end figure against float64 measures the reference, not the kernel)
    w_hip = r._last_weights.cpu().numpy()[hit].astype(np.float64)
    z0h = z0[hit].astype(np.float64)
    zs, allowed = orc.sample_pdf(0.5 * (z0h[:, 1:] + z0h[:, :-1]), w_hip[:, 1:-1], NI, det=det, u=None if det else u[hit], dtype=np.float64,
                                 return_conditioning=True)
    order = np.argsort(zs, axis=-1, kind="stable")
    zs, allowed = np.take_along_axis(zs, order, -1), np.take_along_axis(allowed, order, -1)
    dz = np.abs(importance_depths(zg, z0[hit]) - zs)
    assert np.all(dz <= allowed), float((dz / allowed).max())
    bin_w = (t[hit][:, 1] - t[hit][:, 0])[:, None] / (S - 1)
    assert np.mean(allowed < 1e-3 * bin_w) > 0.9                 # ... and the bound is not vacuous: 1e-3 of a bin for > 90 % of the samples
    # (3) fine pass: the oracle on the kernel's own depths, every ray, the strict gate
    ref2 = orc.render_rays(w_f if fine else w, spec, ro[hit], rd[hit], t[hit], np.repeat(params, hit.sum(), 0), cone[hit], S + NI,
                           False, (1, 1, 1.), fam["blur_idx"], z_override=zg, dtype=np.float64)
    got = np.concatenate([out["color_pred"][0].cpu().numpy()[hit], out["alpha_pred"][0].cpu().numpy()[hit][:, None]], -1)
    want = np.concatenate([ref2["color_pred"], ref2["alpha_pred"][:, None]], -1)
    assert orc.rel_linf(got, want) <= TOL
    assert np.all(out["alpha_pred"][0].cpu().numpy()[~hit] == 0)


def test_edge_cases_empty_culled_minimal():
    """Empty input, every ray culled, the smallest legal sample count, a sample count with a ragged last batch,
    NaN inputs raising through the check_numerics flag, n_samples < 2 refused."""
    from nerf_tex_amd import _lib, synthetic
    from nerf_tex_amd.renderer import Renderer
    fam = synthetic.FAMILIES["carpet"]
    model, spec, w = make_model((1, 6), dense_media=True)
    params = to_dev(np.asarray([fam["params"]], np.float32))[0]
    r = Renderer(model=model, n_samples=64, perturb=False)
    z3 = lambda n, k: torch.zeros((1, n, k), device=dev())
    out = r(z3(0, 3), z3(0, 3), z3(0, 2), parameters=params, cone_scale=z3(0, 1))                    # no rays at all
    assert out["color_pred"].shape == (1, 0, 3) and out["alpha_pred"].shape == (1, 0)
    ro, rd, t, cone = synthetic.all_hit_rays(37, fam["b_0"], fam["b_1"], fam["cam"])
    tinf = np.full_like(t, np.inf)
    out = r(*to_dev(ro[None], rd[None], tinf[None]), parameters=params, cone_scale=to_dev(cone[None])[0], composite_bkgd=True,
            bkgd_color=[.2, .4, .6])
    assert torch.all(out["alpha_pred"] == 0) and torch.allclose(out["color_pred"][0], torch.tensor([.2, .4, .6], device=dev()).expand(37, 3))
    for S in (2, 3, 33, 97):                                                                       # ragged batches of 32
        rr = Renderer(model=model, n_samples=S, perturb=False)
        o = rr(*to_dev(ro[None], rd[None], t[None]), parameters=params, cone_scale=to_dev(cone[None])[0])
        got = np.concatenate([o["color_pred"][0].cpu().numpy(), o["alpha_pred"][0].cpu().numpy()[:, None]], -1)
        # few samples -> nearly empty image (max |ref| ~ 0.2), where the float32 rounding of the sample positions is visible
        # against the all-float64 image: the strict gate holds against the float32 restatement AND against the float64 network
        # on the float32 points (oracle render_rays: points_dtype); the all-float64 image adds the input rounding, measured
        # oracle to oracle, and nothing more
        pr37 = np.repeat(np.asarray([fam["params"]], np.float32), 37, 0)
        cat = lambda ref: np.concatenate([ref["color_pred"], ref["alpha_pred"][:, None]], -1).astype(np.float64)
        w32 = cat(orc.render_rays(w, spec, ro, rd, t, pr37, cone, S, False, (1, 1, 1.), dtype=np.float32))
        wn = cat(orc.render_rays(w, spec, ro, rd, t, pr37, cone, S, False, (1, 1, 1.), dtype=np.float64, points_dtype=np.float32))
        w64 = cat(orc.render_rays(w, spec, ro, rd, t, pr37, cone, S, False, (1, 1, 1.), dtype=np.float64))
        scale = float(np.abs(w64).max())
        err_net = float(np.abs(got - wn).max()) / scale
        assert float(np.abs(got - w32).max()) / scale <= TOL, S
        assert err_net <= TOL, S
        assert float(np.abs(got - w64).max()) / scale <= err_net + float(np.abs(wn - w64).max()) / scale * (1 + 1e-6) + 1e-9, S
    bad = ro.copy(); bad[5, 0] = np.nan
    o = r(*to_dev(bad[None], rd[None], t[None]), parameters=params, cone_scale=to_dev(cone[None])[0])
    with pytest.raises(FloatingPointError):                                                        # renderer.py:140-141
        r.raise_if_nonfinite()
    with pytest.raises(_lib.NtxError) as e:
        Renderer(model=model, n_samples=1, perturb=False)(*to_dev(ro[None], rd[None], t[None]), parameters=params,
                                                          cone_scale=to_dev(cone[None])[0])
    assert e.value.code == _lib.NTX_E_INVALID


@pytest.mark.parametrize("family", ["carpet", "grass_filtered"])
def test_direction_hoisting_is_bit_identical(family, monkeypatch):
    """ntx_render_rays evaluates the colour layer's direction segment once per ray (dir_block, through LDS) instead of once per
    sample; a context created with NERFTEX_NO_DIR_HOIST evaluates it per sample.  Same bits, and a blur_idx on an
    APPEARANCE parameter (per-sample scaling, renderer.py:155-158) takes the per-sample path by itself."""
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.renderer import Renderer
    fam = synthetic.FAMILIES[family]
    h, wd, S = 20, 24, 64
    (ro, rd, t, cone), _, _ = camera_rays(family, h, wd)
    params = np.asarray([fam["params"]], np.float32)
    args = to_dev(ro[None], rd[None], t[None])
    kw = dict(parameters=to_dev(params)[0], cone_scale=to_dev(cone[None])[0])

    def render(blur_idx):
        model, spec, w = make_model(fam["n_parameters"], dense_media=True)
        out = Renderer(model=model, n_samples=S, perturb=False, blur_idx=blur_idx)(*args, **kw)
        return torch.cat([out["color_pred"][0], out["alpha_pred"][0][:, None]], -1).cpu().numpy(), spec, w

    got, spec, w = render(fam["blur_idx"])
    monkeypatch.setenv("NERFTEX_NO_DIR_HOIST", "1")
    plain, _, _ = render(fam["blur_idx"])
    monkeypatch.delenv("NERFTEX_NO_DIR_HOIST")
    assert np.array_equal(got, plain)
    # blur on the last (appearance) parameter: not hoistable
    bi = sum(fam["n_parameters"]) - 1
    got2, _, _ = render(bi)
    ref = orc.renderer_call(w, spec, ro[None], rd[None], t[None], params, cone[None], S, False, (1., 1., 1.), bi, False,
                            dtype=np.float64)
    want = np.concatenate([ref["color_pred"][0], ref["alpha_pred"][0][:, None]], -1)
    assert orc.rel_linf(got2, want) <= TOL
    assert not np.array_equal(got2, got)
