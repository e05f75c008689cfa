"""The stand-alone kernels of nerf_tex_amd/csrc/ntx_small_kernels.h (`ntx_sample_pdf`, `ntx_composite`, `ntx_fourier_features`,
`ntx_image_epilogue`) at their chunk edges, argument limits and large arguments, each against the float64 oracle on the kernel's
own float32 inputs.  `-m gpu`.

Tolerances are the suite's existing ones (1e-5 composite, 2e-5 epilogue, 2.5e-7 sine, the oracle's own `allowed` for the sampler)
plus exact-equality / 1-ulp conditions where the arithmetic cannot round.  The inputs of the sampler cases and the float32
emulation of its arithmetic are in tests/kernel_emulation.py, shared with the CPU tests of tests/test_oracle.py."""

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from tests import kernel_emulation as emu
from tests.common import importance_depths

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRID_RAYS = 2048 * 4            # composite / sample_pdf: the grid is capped at 2048 workgroups of 4 waves, one ray per wave and pass
MANY_RAYS = 2 * GRID_RAYS + 5   # 16 389: every wave takes two rays, five of them a third
ORACLE_ROWS = 800


def dev():
    return torch.device("cuda", 0)


def to_dev(*arrs):
    return [torch.as_tensor(np.ascontiguousarray(a), device=dev()) for a in arrs]


def stream():
    return torch.cuda.current_stream(dev()).cuda_stream


def ptr(t):
    return t.data_ptr() if t is not None else None


def ulp_distance(a, b):
    """float32 arrays of one sign -> how many representable values apart"""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


# ---------------------------------------------------------------------------------------------
# 1. ntx_sample_pdf
# ---------------------------------------------------------------------------------------------
SENTINEL = -7.25


def sample_pdf(t, z, w, u, S, NI, flags=0, seed=0, opts=None, n=None):
    """ntx_sample_pdf on host arrays (z, u: None = NULL) -> (return code, z_out [n, S + NI] as numpy, pre-filled with SENTINEL)"""
    from nerf_tex_amd import _lib
    n = len(t) if n is None else n
    dt, dw = to_dev(np.asarray(t, np.float32), np.asarray(w, np.float32))
    dz = to_dev(np.asarray(z, np.float32))[0] if z is not None else None
    du = to_dev(np.asarray(u, np.float32))[0] if u is not None else None
    out = torch.full((max(len(t), 1), S + NI), SENTINEL, device=dev(), dtype=torch.float32)
    with torch.cuda.device(dev()):
        rc = _lib.lib.ntx_sample_pdf(ptr(dt), ptr(dz), ptr(dw), ptr(du), n, S, NI, flags, seed, opts, ptr(out), stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def coarse_depths(t, S, perturb, seed=0, ray_index=None):
    from nerf_tex_amd.renderer import Renderer
    return Renderer.sample_depths(to_dev(np.asarray(t, np.float32))[0], S, perturb=perturb, seed=seed, ray_index=ray_index).cpu().numpy()


@pytest.mark.parametrize("order", ["seeded", "sorted"])
@pytest.mark.parametrize("weight", [0.0, 0.25, 0.013])
@pytest.mark.parametrize("S", [66, 130])
def test_sample_pdf_exact_dyadic(S, weight, order):
    """64 / 128 equal interior weights (one chunk / two chunks of the CDF scan), depths 2 + i/32, u = k/1024 holding 0, 1 and every
    CDF entry.  Nothing rounds: each lane sums one or two equal values and the butterfly doubles them, pdf = 1/64 or 1/128, every
    partial sum and midpoint is exact and the interpolation has dyadic operands.  So the sum, the scan and the carry are pinned to
    the bit: at most 1 ulp from the float64 result rounded to float32 (tests/test_oracle.py: the float32 emulation of the kernel's
    arithmetic equals it bit for bit, and the float64 oracle equals rational arithmetic).  `sorted` u takes the merge path of the
    final sort, `seeded` the rank sort.  Importance depths coincide with coarse depths, bin midpoints and each other here (ties)."""
    from nerf_tex_amd import _lib
    t, z, w, u = emu.dyadic_case(S, weight)
    if order == "sorted":
        u = np.sort(u, -1)
    NI = u.shape[1]
    rc, zo = sample_pdf(t, z, w, u, S, NI)
    assert rc == _lib.NTX_OK
    assert not np.isnan(zo).any() and np.all(np.diff(zo, axis=-1) >= 0)
    got = importance_depths(zo, z)                                       # asserts that every coarse depth is there
    z64 = z.astype(np.float64)
    want = orc.sample_pdf(0.5 * (z64[:, 1:] + z64[:, :-1]), w.astype(np.float64)[:, 1:-1], NI, det=False, u=u.astype(np.float64), dtype=np.float64)
    want = np.sort(want, -1).astype(np.float32)
    d = ulp_distance(got, want)
    print("dyadic", S, weight, order, "max ulp", int(d.max()))
    assert d.max() <= 1, int(d.max())


def pdf_case(S, NI, pattern, n=48):
    rng = np.random.default_rng(1000 * S + NI + 17 * emu.PDF_PATTERNS.index(pattern))
    t = emu.pdf_rays(n, rng)
    w = emu.pdf_weights(pattern, n, S, rng)
    u = rng.uniform(size=(n, NI)).astype(np.float32)
    return t, w, u


RAY_INDEX = (1000, 16, 40)      # a sharded call's global ray indices (ntx_render_opts): the jitter is keyed by them


@pytest.mark.parametrize("pattern", emu.PDF_PATTERNS)
@pytest.mark.parametrize("S,NI", emu.PDF_SHAPES)
def test_sample_pdf_general(S, NI, pattern):
    """Every importance depth within the float32 conditioning (`allowed`) of float64 orc.sample_pdf on the kernel's own float32 inputs
    (test_hierarchical_sampling part (2)), at the ragged last chunks S - 2 = 63, 65, 129 and at the LDS limit S = NI = 512; the
    deterministic u (merge path) and seeded draws (rank sort); depths given, and NULL with `t` with and without NTX_FLAG_PERTURB --
    the merged row then holds, bit for bit, what ntx_sample_depths gives for the same flags, seed and opts.
    The bound is not vacuous: S >= 4 has `allowed` < 0.1 coarse bin for >= 90 % of the samples (kernel_emulation.pdf_check)."""
    from nerf_tex_amd import _lib
    t, w, u = pdf_case(S, NI, pattern)
    for zmode in ("given", "lin", "jitter"):
        if zmode == "given":
            z = orc.z_values_perturbed(t, S, seed=5, dtype=np.float32)
            z_in, flags, seed, opts = z, 0, 0, None
        elif zmode == "lin":
            z = coarse_depths(t, S, False)
            z_in, flags, seed, opts = None, 0, 0, None
        else:
            z = coarse_depths(t, S, True, seed=77, ray_index=RAY_INDEX)
            z_in, flags, seed, opts = None, _lib.FLAG_PERTURB, 77, _lib.render_opts(ray_index=RAY_INDEX)
        assert np.all(np.diff(z, axis=-1) >= 0)
        for det in (True, False):
            rc, zo = sample_pdf(t, z_in, w, None if det else u, S, NI, flags, seed, opts)
            assert rc == _lib.NTX_OK
            assert not np.isnan(zo).any() and np.all(np.diff(zo, axis=-1) >= 0), (zmode, det)
            ratio, share = emu.pdf_check(importance_depths(zo, z), z, w, t, NI, det, u)
            print("sample_pdf", S, NI, pattern, zmode, "det" if det else "u", f"max dz/allowed {ratio:.3f} share {share:.3f}")


@pytest.mark.parametrize("det", [True, False])
def test_sample_pdf_more_rays_than_waves(det):
    """16 389 rays on the 8192 waves of the capped grid: the grid-stride loop re-uses the LDS arrays, with a `continue` for the culled
    third of the rays (t0 = inf) in it.  Culled rows are all zero, every other row is non-decreasing and holds the coarse depths;
    the oracle runs on 800 hit rows that hold the first and the last."""
    from nerf_tex_amd import _lib
    S, NI, n = 67, 33, MANY_RAYS
    rng = np.random.default_rng(67 + det)
    t = emu.pdf_rays(n, rng)
    culled = rng.uniform(size=n) < 1 / 3
    culled[[0, n - 1]] = False                                           # the block edges are hit rays
    t[culled] = np.inf
    w = emu.pdf_weights("floor", n, S, rng)
    u = rng.uniform(size=(n, NI)).astype(np.float32)
    z = coarse_depths(t, S, True, seed=9)
    rc, zo = sample_pdf(t, None, w, None if det else u, S, NI, _lib.FLAG_PERTURB, 9)
    assert rc == _lib.NTX_OK
    assert culled.any() and np.all(zo[culled] == 0.0)
    hit = ~culled
    assert not np.isnan(zo[hit]).any() and np.all(np.diff(zo[hit], axis=-1) >= 0)
    idx = np.nonzero(hit)[0]
    sel = np.unique(np.concatenate([idx[:8], idx[-8:], rng.choice(idx, size=ORACLE_ROWS - 16, replace=False)]))
    assert sel[0] == idx[0] and sel[-1] == idx[-1] and idx[-1] >= 2 * GRID_RAYS
    ratio, share = emu.pdf_check(importance_depths(zo[sel], z[sel]), z[sel], w[sel], t[sel], NI, det, u[sel])
    print("sample_pdf many rays", "det" if det else "u", f"max dz/allowed {ratio:.3f} share {share:.3f}")
    # the rows the oracle does not see: every one holds its coarse depths, and NI more inside the ray
    rest = np.setdiff1d(idx, sel)
    imp = importance_depths(zo[rest], z[rest])
    assert imp.shape == (rest.size, NI)
    assert np.all(imp >= z[rest][:, :1]) and np.all(imp <= z[rest][:, -1:])


def test_sample_pdf_argument_limits():
    """n_samples outside [3, 512] and n_importance outside [1, 512] are refused before anything is written; no rays is not an error."""
    from nerf_tex_amd import _lib
    rng = np.random.default_rng(0)
    n = 5
    t = emu.pdf_rays(n, rng)
    for S, NI in [(2, 8), (513, 8), (16, 0), (16, 513)]:
        w = np.full((n, S), 0.1, np.float32)
        rc, zo = sample_pdf(t, None, w, None, S, NI)
        assert rc == _lib.NTX_E_INVALID, (S, NI)
        assert np.all(zo == SENTINEL), (S, NI)
    rc, zo = sample_pdf(t, None, np.full((n, 16), 0.1, np.float32), None, 16, 8, n=0)
    assert rc == _lib.NTX_OK and np.all(zo == SENTINEL)


@pytest.mark.parametrize("S,NI", [(3, 1), (66, 64), (130, 200)])
def test_sample_pdf_ties(S, NI):
    """Rows whose depths all hold one value: every bin has width 0, so the row comes back as S + NI copies of the value, by the
    merge (deterministic u) and by the rank sort (drawn u) alike."""
    from nerf_tex_amd import _lib
    rng = np.random.default_rng(S)
    vals = np.asarray([2.0, 3.1415927, 1e-3, 250.0], np.float32)
    n = vals.size
    z = np.repeat(vals[:, None], S, 1)
    t = np.stack([vals, vals], -1)
    w = emu.pdf_weights("floor", n, S, rng)
    u = rng.uniform(size=(n, NI)).astype(np.float32)
    for uu in (None, u):
        rc, zo = sample_pdf(t, z, w, uu, S, NI)
        assert rc == _lib.NTX_OK
        assert np.array_equal(zo, np.repeat(vals[:, None], S + NI, 1))


# ---------------------------------------------------------------------------------------------
# 2. ntx_composite
# ---------------------------------------------------------------------------------------------
BKGD = [0.2, 0.5, 1.0]


def composite(color, sigma, z, rays_d, map_exr, bk, weights=True, n_samples=None):
    """ntx_composite on host arrays -> (return code, colour [n,3], alpha [n], weights [n,S] or None), outputs pre-filled with SENTINEL"""
    from nerf_tex_amd import _lib
    n, S = sigma.shape
    dc, ds, dz, dd = to_dev(color, sigma, z, rays_d)
    c = torch.full((n, 3), SENTINEL, device=dev()); a = torch.full((n,), SENTINEL, device=dev())
    w = torch.full((n, S), SENTINEL, device=dev()) if weights else None
    flags = (_lib.FLAG_MAP_EXR if map_exr else 0) | (_lib.FLAG_COMPOSITE_BKGD if bk else 0)
    with torch.cuda.device(dev()):
        rc = _lib.lib.ntx_composite(ptr(dc), ptr(ds), ptr(dz), ptr(dd), n, S if n_samples is None else n_samples, flags, _lib.f3(BKGD),
                                    ptr(c), ptr(a), ptr(w), stream())
    torch.cuda.synchronize()
    return rc, c.cpu().numpy(), a.cpu().numpy(), (w.cpu().numpy() if weights else None)


def composite_inputs(n, S, seed):
    """As test_composite (tests/test_gpu_parity.py), plus row 2 with every depth equal and row 3 with an infinite density in front"""
    rng = np.random.default_rng(seed)
    color = rng.normal(size=(n, S, 3)).astype(np.float32) * 2
    sigma = (rng.normal(size=(n, S)) * 20).astype(np.float32)
    sigma[0] = 1e6            # fully opaque first sample: transmittance floor 1e-10 (renderer.py:198)
    sigma[1] = -5.0           # relu -> empty ray
    z = np.sort(rng.uniform(2, 6, size=(n, S)), -1).astype(np.float32)
    z[2] = 3.5                # dist = 0 everywhere: alpha and weights exactly 0
    z[3] = np.linspace(2, 6, S).astype(np.float32)
    sigma[3] = np.abs(sigma[3]); sigma[3, 0] = np.inf      # alpha_0 = 1 exactly; the samples behind see the 1e-10 floor
    rays_d = (rng.normal(size=(n, 3)) * 2).astype(np.float32)     # |d| != 1 (renderer.py:180)
    return color, sigma, z, rays_d


def check_composite(got, inputs, map_exr, bk):
    c, a, w = got
    color, sigma, z, rays_d = inputs
    with np.errstate(over="ignore"):
        rc, ra, rw, _ = orc.map_model_output(color, sigma, z, rays_d, bk, BKGD, map_exr, None, np.float64)
    scale = max(1.0, float(np.max(np.abs(rc))))
    errs = (float(np.max(np.abs(w - rw))) if w is not None else 0.0, float(np.max(np.abs(a - ra))), float(np.max(np.abs(c - rc))) / scale)
    assert errs[0] <= 1e-5, errs                # float32 exp/scan rounding: the bars of test_composite
    assert errs[1] <= 1e-5, errs
    assert errs[2] <= 1e-5, errs
    return errs


@pytest.mark.parametrize("flags", [(False, False), (True, True)])
@pytest.mark.parametrize("S", [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096])
def test_composite_chunk_edges(S, flags):
    """One valid lane in the last chunk of 64 (S = 65 / 129 / 257), one missing (63 / 127 / 255), and long rows whose float32
    transmittance product crosses 16 / 64 chunks (the float32 restatement itself is within 9.5e-7 / 4.5e-6 of float64 there)."""
    from nerf_tex_amd import _lib
    map_exr, bk = flags
    inputs = composite_inputs(257, S, S)
    rc, c, a, w = composite(*inputs, map_exr, bk)
    assert rc == _lib.NTX_OK
    errs = check_composite((c, a, w), inputs, map_exr, bk)
    print("composite", S, flags, "weights %.2e alpha %.2e colour %.2e" % errs)
    assert a[1] == 0.0 and np.all(w[1] == 0.0)
    assert a[2] == 0.0 and np.all(w[2] == 0.0)
    assert w[3, 0] == 1.0 and np.all(w[3, 1:] <= 1e-10 * (1 + 1e-6))


def test_composite_more_rays_than_waves():
    """16 389 rays at S = 65 on the capped grid of 8192 waves, every ray against float64"""
    from nerf_tex_amd import _lib
    inputs = composite_inputs(MANY_RAYS, 65, 11)
    rc, c, a, w = composite(*inputs, False, True)
    assert rc == _lib.NTX_OK
    print("composite many rays: weights %.2e alpha %.2e colour %.2e" % check_composite((c, a, w), inputs, False, True))


@pytest.mark.parametrize("S", [2, 65, 1000])
def test_composite_without_weights_out(S):
    """weights_out = NULL: the same colour and alpha bits as the call that also writes the weights"""
    from nerf_tex_amd import _lib
    inputs = composite_inputs(300, S, 5 + S)
    rc1, c1, a1, _ = composite(*inputs, False, True)
    rc2, c2, a2, w2 = composite(*inputs, False, True, weights=False)
    assert rc1 == rc2 == _lib.NTX_OK and w2 is None
    assert np.array_equal(c1.view(np.uint32), c2.view(np.uint32)) and np.array_equal(a1.view(np.uint32), a2.view(np.uint32))


@pytest.mark.parametrize("S,at", [(2, 0), (64, 63), (65, 64), (200, 70)])
def test_composite_propagates_nan_density(S, at):
    """A NaN density at one sample of one ray: tf.nn.relu propagates it (as np.maximum in the oracle does), so that ray's colour and
    alpha are NaN -- which renderer.py:140-141 then reports -- and its neighbours are untouched."""
    from nerf_tex_amd import _lib
    color, sigma, z, rays_d = composite_inputs(40, S, 3)
    ray = 17
    clean = composite(color, sigma, z, rays_d, False, False)
    sigma = sigma.copy(); sigma[ray, at] = np.nan
    rc, c, a, w = composite(color, sigma, z, rays_d, False, False)
    with np.errstate(all="ignore"):
        ref_c, ref_a, _, _ = orc.map_model_output(color, sigma, z, rays_d, False, BKGD, False, None, np.float64)
    assert rc == _lib.NTX_OK
    assert np.isnan(ref_a[ray]) and np.isnan(ref_c[ray]).all()            # what the reference computes
    assert np.isnan(a[ray]) and np.isnan(c[ray]).all()
    others = np.arange(40) != ray
    assert np.isfinite(ref_a[others]).all()
    assert np.array_equal(a[others], clean[2][others]) and np.array_equal(c[others], clean[1][others])
    assert np.array_equal(w[others], clean[3][others])


def test_composite_refuses_one_sample():
    from nerf_tex_amd import _lib
    color, sigma, z, rays_d = composite_inputs(8, 4, 0)
    rc, c, a, w = composite(color, sigma, z, rays_d, False, False, n_samples=1)
    assert rc == _lib.NTX_E_INVALID
    assert np.all(c == SENTINEL) and np.all(a == SENTINEL) and np.all(w == SENTINEL)


# ---------------------------------------------------------------------------------------------
# 3. ntx_fourier_features
# ---------------------------------------------------------------------------------------------
def fourier(x, nf, m=None, d=None):
    from nerf_tex_amd import _lib
    x = np.asarray(x, np.float32)
    rows, cols = x.shape
    dx = to_dev(x)[0]
    out = torch.full((rows, cols * (1 + 2 * max(nf, 0))), SENTINEL, device=dev())
    with torch.cuda.device(dev()):
        rc = _lib.lib.ntx_fourier_features(ptr(dx), rows if m is None else m, cols if d is None else d, nf, ptr(out), stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("nf", [0, 10, 17, 18, 24, 30])
@pytest.mark.parametrize("d", [1, 3, 6])
def test_fourier_features_every_band(d, nf):
    """n_freq up to the entry point's limit of 30: arguments 2^k x up to 3 * 2^29, exact in float32, against float64 sin / cos of the
    same argument.  The bar is test_fourier_features' 2.5e-7 at every band: sin_q serves |2^k x| < 2^17 and the device library's
    sinf / cosf the rest (the three-step reduction of sin_q alone is 6e-7 off at band 20 and returns 1e14 at band 30:
    tests/test_oracle.py::test_sin_q_emulation_range).  Measured on an MI355X: <= 9.2e-8 at every band, the library sine included."""
    from nerf_tex_amd import _lib
    rng = np.random.default_rng(100 * d + nf)
    x = rng.uniform(-3, 3, size=(1000, d)).astype(np.float32)
    rc, out = fourier(x, nf)
    assert rc == _lib.NTX_OK
    ref = orc.fourier_features(x, nf, np.float64)
    assert out.shape == ref.shape
    assert np.array_equal(out[:, :d], x)
    err = np.abs(out - ref)
    per_band = [float(err[:, d + 2 * k * d: d + 2 * (k + 1) * d].max()) for k in range(nf)]
    print("fourier", d, nf, "per band:", " ".join("%.1e" % e for e in per_band))
    assert max(per_band, default=0.0) <= 2.5e-7, per_band


def test_fourier_features_large_positions():
    """|x| of 1e3, 1e5 and 1e7 at n_freq 4: the same bar on both sides of the 2^17 switch-over"""
    from nerf_tex_amd import _lib
    rng = np.random.default_rng(4)
    mag = np.repeat(np.asarray([1e3, 1e5, 1e7]), 200)[:, None]
    x = (mag * rng.uniform(0.5, 1.0, size=(600, 3)) * rng.choice([-1.0, 1.0], size=(600, 3))).astype(np.float32)
    x = np.concatenate([x, np.asarray([[131071.99, -131072.0, 131072.01], [65536.0, -65535.996, 32768.0]], np.float32)])
    rc, out = fourier(x, 4)
    assert rc == _lib.NTX_OK
    err = np.abs(out - orc.fourier_features(x, 4, np.float64))
    print("fourier large |x|: %.2e" % err.max())
    assert err.max() <= 2.5e-7


def test_fourier_features_nonfinite():
    """inf, -inf and NaN: x is copied through, every sin / cos entry of that component is NaN, the rest of the row is untouched"""
    from nerf_tex_amd import _lib
    rng = np.random.default_rng(5)
    d, nf = 3, 18
    x = rng.uniform(-3, 3, size=(70, d)).astype(np.float32)
    rc, clean = fourier(x, nf)
    bad = x.copy()
    spots = [(3, 0, np.inf), (20, 1, -np.inf), (64, 2, np.nan), (69, 0, np.nan)]
    for r, c, v in spots:
        bad[r, c] = v
    rc2, out = fourier(bad, nf)
    assert rc == rc2 == _lib.NTX_OK
    assert np.array_equal(out[:, :d], bad, equal_nan=True)
    feat = out[:, d:].reshape(-1, 2 * nf, d); feat0 = clean[:, d:].reshape(-1, 2 * nf, d)
    mask = np.zeros(feat.shape, bool)
    for r, c, _ in spots:
        mask[r, :, c] = True
    assert np.isnan(feat[mask]).all()
    assert np.array_equal(feat[~mask], feat0[~mask])


def test_fourier_features_argument_limits():
    from nerf_tex_amd import _lib
    x = np.ones((4, 3), np.float32)
    rc, out = fourier(x, 31)
    assert rc == _lib.NTX_E_INVALID and np.all(out == SENTINEL)
    rc, out = fourier(x, 4, d=0)
    assert rc == _lib.NTX_E_INVALID and np.all(out == SENTINEL)
    rc, out = fourier(x, 4, m=0)
    assert rc == _lib.NTX_OK and np.all(out == SENTINEL)


# ---------------------------------------------------------------------------------------------
# 4. ntx_image_epilogue
# ---------------------------------------------------------------------------------------------
def epilogue(rgba, f, unpremultiply, want_f32=True, want_u8=True):
    from nerf_tex_amd import _lib
    h, w = rgba.shape[:2]
    ff = max(f, 1)
    oh, ow = -(-h // ff), -(-w // ff)
    src = to_dev(np.asarray(rgba, np.float32))[0]
    out = torch.full((oh, ow, 4), SENTINEL, device=dev()) if want_f32 else None
    u8 = torch.full((oh, ow, 4), 99, device=dev(), dtype=torch.uint8) if want_u8 else None
    with torch.cuda.device(dev()):
        rc = _lib.lib.ntx_image_epilogue(ptr(src), h, w, f, 1 if unpremultiply else 0, ptr(out), ptr(u8), stream())
    torch.cuda.synchronize()
    return rc, (out.cpu().numpy() if want_f32 else None), (u8.cpu().numpy() if want_u8 else None)


def epilogue_image(h, w, f):
    """As test_image_epilogue (tests/test_gpu_parity.py); pixel (0, 0) always has alpha > 0, so a 1 x 1 image is not empty"""
    rng = np.random.default_rng(h * w + f)
    a = rng.uniform(0, 1, size=(h, w, 1)); a[rng.uniform(size=(h, w, 1)) < 0.3] = 0.0
    a[0, 0, 0] = 0.75
    return np.concatenate([rng.uniform(0, 1, size=(h, w, 3)) * a, a], -1).astype(np.float32)


EPILOGUE_SHAPES = [(47, 95, 5), (100, 130, 8), (129, 200, 16), (16, 16, 16), (1, 1, 16), (3, 200, 7), (200, 3, 16), (1, 1, 1), (5, 7, 2)]


@pytest.mark.parametrize("unpremultiply", [True, False])
@pytest.mark.parametrize("h,w,f", EPILOGUE_SHAPES)
def test_image_epilogue_factors_and_small_images(h, w, f, unpremultiply):
    """Factors up to the limit of 16 (48 taps fill the kernel's tap array), images smaller than the filter, one pixel.  float32
    against float64 at test_image_epilogue's bar (the float32 restatement is within 1.8e-6 of float64 on these shapes); and the
    uint8 output equals orc.to_uint8 of the float32 output OF THE SAME CALL exactly -- both come from one accumulator."""
    from nerf_tex_amd import _lib
    rgba = epilogue_image(h, w, f)
    rc, out, u8 = epilogue(rgba, f, unpremultiply)
    assert rc == _lib.NTX_OK
    ref = orc.image_epilogue(rgba, f, not unpremultiply, np.float64)
    assert out.shape == ref.shape
    err = float(np.max(np.abs(out - ref))) / max(1.0, float(np.abs(ref).max()))
    print("epilogue", h, w, f, unpremultiply, "%.2e" % err)
    assert err <= 2e-5
    assert np.array_equal(u8, orc.to_uint8(out))
    if (h, w) == (1, 1):
        assert out[0, 0, 3] > 0
    # one output only: the other's bits are unchanged
    rc1, only_f32, none8 = epilogue(rgba, f, unpremultiply, want_u8=False)
    rc2, none32, only_u8 = epilogue(rgba, f, unpremultiply, want_f32=False)
    assert rc1 == rc2 == _lib.NTX_OK and none8 is None and none32 is None
    assert np.array_equal(only_f32.view(np.uint32), out.view(np.uint32)) and np.array_equal(only_u8, u8)


def test_image_epilogue_uint8_saturates():
    """tf.image.convert_image_dtype saturates: above 1 -> 255, below 0 -> 0, NaN -> 0; x * 255.5 is truncated, not rounded"""
    from nerf_tex_amd import _lib
    vals = np.asarray([1.5, -0.2, np.nan, np.inf, -np.inf, 1.0, 0.5, 0.9999, 0.0, 1.7 / 255.5, 1e30, -1e30], np.float32)
    want = np.asarray([255, 0, 0, 255, 0, 255, 127, 255, 0, 1, 255, 0], np.uint8)
    rgba = vals.reshape(1, 3, 4)
    rc, out, u8 = epilogue(rgba, 1, False)
    assert rc == _lib.NTX_OK
    assert np.array_equal(out, rgba, equal_nan=True)
    assert np.array_equal(u8.ravel(), want)
    assert np.array_equal(u8, orc.to_uint8(out))


def test_image_epilogue_argument_limits():
    from nerf_tex_amd import _lib
    rgba = epilogue_image(20, 20, 1)
    for f in (17, 0):
        rc, out, u8 = epilogue(rgba, f, True)
        assert rc == _lib.NTX_E_INVALID, f
        assert np.all(out == SENTINEL) and np.all(u8 == 99)
    rc, _, _ = epilogue(rgba, 2, True, want_f32=False, want_u8=False)
    assert rc == _lib.NTX_E_INVALID
