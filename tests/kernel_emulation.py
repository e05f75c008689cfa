"""numpy float32 emulations of two pieces of device arithmetic, and the seeded inputs the CPU and the GPU tests of the
stand-alone kernels share (tests/test_oracle.py, tests/test_gpu_standalone_edges.py).

An emulation states the kernel's OWN order of operations (which the oracle, a restatement of the reference, does not), one
rounding per operation: a float32 product or sum is formed in float64 -- exact for a product, and for an FMA the one
rounding the hardware does -- and rounded to float32 once."""

from fractions import Fraction

import numpy as np

from oracle import nerftex_oracle as orc

F32, F64 = np.float32, np.float64


def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def sin_q_f32(x, q):
    """sin_q of nerf_tex_amd/csrc/ntx_device.h, operation for operation: sin(x + q pi/2) by a three-step Cody-Waite
    reduction and the cephes polynomials."""
    x = np.asarray(x, F32)
    n = np.rint(x * F32(float.fromhex("0x1.45f306p-1")))
    r = _fma(-n, F32(float.fromhex("0x1.921fb6p+0")), x)
    r = _fma(-n, F32(float.fromhex("-0x1.777a5cp-25")), r)
    r = _fma(-n, F32(float.fromhex("-0x1.ee59dap-50")), r)
    qq = n.astype(np.int64) + int(q)
    r2 = r * r
    ps = _fma(r2, F32(-1.9515295891e-4), F32(8.3321608736e-3))
    ps = _fma(r2, ps, F32(-1.6666654611e-1))
    s = _fma(r * r2, ps, r)
    pc = _fma(r2, F32(2.443315711809948e-5), F32(-1.388731625493765e-3))
    pc = _fma(r2, pc, F32(4.166664568298827e-2))
    c = _fma(r2 * r2, pc, _fma(r2, F32(-0.5), F32(1.0)))
    v = np.where(qq & 1, c, s)
    return np.where(qq & 2, -v, v).astype(F32)


def sin_q_band_errors(n_bands=31, n=200_000, seed=0):
    """max |sin_q - float64 sin / cos| of the float32 argument 2^k x, x uniform in [-3, 3], for every band k."""
    x = np.random.default_rng(seed).uniform(-3, 3, n).astype(F32)
    out = []
    for k in range(n_bands):
        y = x * F32(2.0 ** k)                                         # exact: a power of two
        with np.errstate(all="ignore"):
            e = max(np.max(np.abs(sin_q_f32(y, 0).astype(F64) - np.sin(y.astype(F64)))),
                    np.max(np.abs(sin_q_f32(y, 1).astype(F64) - np.cos(y.astype(F64)))))
        out.append(float(e))
    return out


def sample_pdf_f32(z, w, u=None, n_imp=None):
    """sample_pdf_kernel of nerf_tex_amd/csrc/ntx_small_kernels.h for rays with given depths, in its own order: per-lane
    strided sums of the S-2 interior weights (+1e-5), xor butterfly over the 64 lanes, the pdf, a Hillis-Steele scan per
    chunk of 64 with the carry between chunks, searchsorted(side='right') and the interpolation.
    z [n,S], w [n,S], u [n,NI] or None (the deterministic linspace over n_imp) -> the NI importance depths [n,NI], unsorted."""
    z = np.asarray(z, F32); w = np.asarray(w, F32)
    n, S = z.shape
    NB = S - 1
    lanes = np.arange(64)
    part = np.zeros((n, 64), F32)
    for i0 in range(0, S - 2, 64):
        i = i0 + lanes
        ok = i < S - 2
        term = np.where(ok, w[:, 1 + np.minimum(i, S - 3)] + F32(1e-5), F32(0))
        part = np.where(ok, part + term, part).astype(F32)
    for d in (32, 16, 8, 4, 2, 1):
        part = (part + part[:, lanes ^ d]).astype(F32)
    total = part[:, :1]
    cdf = np.zeros((n, NB), F32)
    carry = np.zeros((n, 1), F32)
    for i0 in range(0, S - 2, 64):
        i = i0 + lanes
        ok = i < S - 2
        p = np.where(ok, (w[:, 1 + np.minimum(i, S - 3)] + F32(1e-5)) / total, F32(0)).astype(F32)
        d = 1
        while d < 64:
            v = np.concatenate([np.zeros((n, d), F32), p[:, :-d]], 1)
            p = np.where(lanes >= d, p + v, p).astype(F32)
            d <<= 1
        cdf[:, 1 + i[ok]] = (carry + p)[:, ok]
        carry = (carry + p[:, 63:]).astype(F32)
    bins = (F32(0.5) * (z[:, 1:] + z[:, :-1])).astype(F32)
    if u is None:
        du = F32(1.0) / F32(n_imp - 1) if n_imp > 1 else F32(0)
        k = np.arange(n_imp)
        uu = (du * k.astype(F32)).astype(F32)
        uu[0] = 0.0
        if n_imp > 1:
            uu[-1] = 1.0
        u = np.broadcast_to(uu, (n, n_imp))
    u = np.asarray(u, F32)
    lo = np.stack([np.searchsorted(c, x, side="right") for c, x in zip(cdf, u)])
    below = np.maximum(lo - 1, 0); above = np.minimum(lo, NB - 1)
    c0 = np.take_along_axis(cdf, below, 1); c1 = np.take_along_axis(cdf, above, 1)
    b0 = np.take_along_axis(bins, below, 1); b1 = np.take_along_axis(bins, above, 1)
    denom = (c1 - c0).astype(F32)
    denom = np.where(denom < F32(1e-5), F32(1), denom)
    tt = ((u - c0) / denom).astype(F32)
    return (b0 + (tt * (b1 - b0)).astype(F32)).astype(F32)


def sample_pdf_exact(z, w, u):
    """Brute-force inverse CDF of renderer.sample_pdf in rational arithmetic, one sample at a time: bins = the midpoints of
    z, pdf over the interior weights + 1e-5 (the float32 constant the kernel adds is NOT used: callers pass weights for which
    the pdf is uniform whatever the constant).  z [S], w [S], u [NI] sequences of Fractions -> list of Fractions."""
    S = len(z)
    ws = [Fraction(x) + Fraction(1, 100000) for x in w[1:S - 1]]
    tot = sum(ws)
    cdf = [Fraction(0)]
    for x in ws:
        cdf.append(cdf[-1] + x / tot)
    bins = [(z[i] + z[i + 1]) / 2 for i in range(S - 1)]
    out = []
    for uk in u:
        ind = sum(1 for c in cdf if c <= uk)                          # searchsorted(side='right')
        below, above = max(0, ind - 1), min(len(cdf) - 1, ind)
        den = cdf[above] - cdf[below]
        if den < Fraction(1, 100000):
            den = Fraction(1)
        out.append(bins[below] + (uk - cdf[below]) / den * (bins[above] - bins[below]))
    return out


# ---------------------------------------------------------------------------------------------
# seeded inputs of the sample_pdf cases
# ---------------------------------------------------------------------------------------------
def dyadic_case(S, weight, seed=0):
    """An exact case: S - 2 = 64 or 128 equal interior weights, depths 2 + i/32, u = k/1024 for seeded k that hold 0, 1024
    and every CDF entry.  Nothing rounds in the kernel's float32 arithmetic (tests/test_gpu_standalone_edges.py says why).
    -> (t [1,2], z [1,S], w [1,S], u [1,NI]) float32, u in a seeded order (not sorted)."""
    assert S - 2 in (64, 128)
    rng = np.random.default_rng(seed + S)
    step = 1024 // (S - 2)
    k = np.arange(0, 1025, step)
    NI = 128 if S == 66 else 200
    rest = np.setdiff1d(np.arange(1025), k)
    k = np.concatenate([k, rng.choice(rest, size=NI - k.size, replace=False)])
    rng.shuffle(k)
    z = (2.0 + np.arange(S) / 32.0).astype(F32)[None]
    w = np.full((1, S), weight, F32)
    u = (k / 1024.0).astype(F32)[None]
    t = np.asarray([[z[0, 0], z[0, -1]]], F32)
    return t, z, w, u


PDF_SHAPES = [(3, 1), (3, 7), (4, 64), (64, 64), (65, 65), (66, 64), (67, 129), (130, 200), (257, 64), (512, 512)]
PDF_PATTERNS = ["floor", "spike", "zero"]


def pdf_weights(pattern, n, S, rng):
    if pattern == "floor":
        return (rng.uniform(0.2, 1.0, size=(n, S)) / S).astype(F32)
    w = np.zeros((n, S), F32)
    if pattern == "spike":
        w[np.arange(n), rng.integers(1, S - 1, size=n)] = 0.9          # an interior sample: the end weights are not part of the pdf
    return w


def pdf_rays(n, rng):
    t0 = rng.uniform(2.0, 4.0, size=n)
    return np.stack([t0, t0 + rng.uniform(0.5, 3.0, size=n)], -1).astype(F32)


def pdf_check(z_imp, z, w, t, NI, det, u, min_share=0.9):
    """The general check of one sample_pdf call: the NI importance depths z_imp [n,NI] (sorted per ray) against float64
    orc.sample_pdf on the float32 inputs z, w (and u), every depth within the oracle's own `allowed`; and the bound is not
    vacuous (S >= 4: `allowed` < 0.1 coarse bin for >= min_share of the samples).  Returns (largest ratio, share)."""
    z64 = np.asarray(z, F64); S = z64.shape[1]
    zs, allowed = orc.sample_pdf(0.5 * (z64[:, 1:] + z64[:, :-1]), np.asarray(w, F64)[:, 1:-1], NI, det=det,
                                 u=None if det else np.asarray(u, F64), dtype=F64, return_conditioning=True)
    order = np.argsort(zs, axis=-1, kind="stable")
    zs, allowed = np.take_along_axis(zs, order, -1), np.take_along_axis(allowed, order, -1)
    dz = np.abs(np.asarray(z_imp, F64) - zs)
    ratio = float((dz / allowed).max())
    assert np.all(dz <= allowed), ratio
    bin_w = (np.asarray(t, F64)[:, 1] - np.asarray(t, F64)[:, 0])[:, None] / (S - 1)
    share = float(np.mean(allowed < 0.1 * bin_w))
    if S >= 4:
        assert share >= min_share, share
    elif NI == 7 and det:
        assert share >= 6 / 7 - 1e-12, share                           # u = 1 sits on the last CDF entry
    return ratio, share


if __name__ == "__main__":      # python -m tests.kernel_emulation: the table behind the 2^17 switch-over of fourier_kernel
    for k, e in enumerate(sin_q_band_errors()):
        print(f"band {k:2d}  |2^k x| <= {3 * 2.0 ** k:.3g}  max |sin_q - float64| = {e:.2e}{'' if e <= 2.5e-7 else '   > 2.5e-7'}")
