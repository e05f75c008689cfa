"""What the tests of the distortion loss share (tests/test_ray_distortion.py on the CPU, tests/test_gpu_ray_distortion.py on the GPU;
`ntx_ray_distortion`, `nerf_tex_amd.loss.ray_distortion` / `distortion` / `Distortion`): the formula of include/nerftex.h
restated twice -- the float64 pair sum with its analytic gradient (the reference), and the O(S) form in float32 with sequential scans and the
shift by the first live depth (what any float32 evaluation of that form is off by: the FLOOR) -- the case table, and the gate.

THE GATE, everywhere: error <= max(4 floors, 5e-7), and never beyond 1e-4; errors and floors are rel-Linf over the batch, max|x - ref| /
max|ref|.  Four float32 floors is the project's standing convention; 5e-7 is 4 ulp of float32, for the tiny cases whose
floor is a single rounding; 1e-4 is the house bar and the cap.  tests/test_ray_distortion.py holds every floor <= 2.5e-5, so four floors
never reach the cap.

Appended for the calls past the capped grid and the liveness an instanced step produces: `PATCH_PATTERNS`, `live_limit_case`, `large_base` /
`cycled` / `large_scale` / `large_reference` (the float64 reference is computed on the 257 base rows alone and cycled)."""

import functools

import numpy as np

F = np.float32
ULP4, CAP, FLOOR_GUARD = 5e-7, 1e-4, 2.5e-5


def gate(floor):
    return min(max(4.0 * floor, ULP4), CAP)


def rel_linf(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(x - ref).max() / max(np.abs(ref).max(), 1e-300))


# ---- the formula, twice -----------------------------------------------------------------------------------------------------------------
def live_mask(z, live=None):
    """A sample is live iff its depth is finite and (where `live` is given) live > 0."""
    m = np.isfinite(np.asarray(z))
    return m if live is None else m & (np.nan_to_num(np.asarray(live), nan=0.0) > 0)


def default_widths(z):
    """delta_i = z_{i+1} - z_i, delta_{S-1} = delta_{S-2}; 0 for S == 1 (in z's dtype)."""
    z = np.asarray(z)
    if z.shape[1] == 1:
        return np.zeros_like(z)
    with np.errstate(invalid="ignore"):
        d = z[:, 1:] - z[:, :-1]
    return np.concatenate([d, d[:, -1:]], 1)


def pairwise64(w, z, widths=None, live=None, ray_scale=None, rows=64):
    """(loss [N], grad [N, S]) in float64: L = sum_ij w_i w_j |z_i - z_j| + (1/3) sum_i w_i^2 delta_i over the live samples and
    dL/dw_k = 2 sum_j w_j |z_k - z_j| + (2/3) w_k delta_k, 0 at a sample that is not live; both times ray_scale, and 0 on a ray without a live
    sample whatever ray_scale holds.  The pair sum is taken `rows` samples at a time (a ray of 4096 samples is 16 M pairs)."""
    lv = live_mask(z, live)
    sel = lambda a: np.where(lv, np.nan_to_num(np.asarray(a, np.float64), nan=0.0, posinf=0.0, neginf=0.0), 0.0)
    w64, z64 = sel(w), sel(z)
    d64 = sel(default_widths(np.asarray(z, np.float64)) if widths is None else widths)
    n, S = w64.shape
    inner = np.zeros((n, S))
    for k0 in range(0, S, rows):
        k1 = min(S, k0 + rows)
        inner[:, k0:k1] = np.einsum("nj,nkj->nk", w64, np.abs(z64[:, k0:k1, None] - z64[:, None, :]))     # (w is 0 where a sample is not live)
    loss = (w64 * inner).sum(1) + (w64 * w64 * d64).sum(1) / 3.0
    grad = np.where(lv, 2.0 * inner + (2.0 / 3.0) * w64 * d64, 0.0)
    scale = np.ones(n) if ray_scale is None else np.asarray(ray_scale, np.float64)
    any_live = lv.any(1)
    scale = np.where(any_live, np.nan_to_num(scale, nan=0.0, posinf=0.0, neginf=0.0), 0.0)            # (selected, not multiplied, where no sample is live)
    return loss * scale, grad * scale[:, None]


def linear_form(w, z, widths=None, live=None, ray_scale=None, dtype=F, shift=True):
    """The O(S) form in `dtype` with SEQUENTIAL scans (numpy's cumsum adds front to back in the array's type): m = z - z_first (shift=False:
    m = z), exclusive prefix sums W_<, M_< of w and w m, suffix sums as totals less the inclusive ones,
        inner_k = (m_k W_<k - M_<k) + (M_>k - m_k W_>k),   L = 2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 delta_i,
        dL/dw_k = 2 inner_k + (2/3) w_k delta_k.
    Returns (loss [N], grad [N, S]) in `dtype`."""
    T = dtype
    lv = live_mask(z, live)
    sel = lambda a: np.where(lv, np.nan_to_num(np.asarray(a, T), nan=0.0, posinf=0.0, neginf=0.0), T(0)).astype(T)
    wv, zv = sel(w), sel(z)
    dv = sel(default_widths(np.asarray(z, T)) if widths is None else widths)
    n, S = wv.shape
    first = np.where(lv.any(1), lv.argmax(1), 0)
    z_first = zv[np.arange(n), first][:, None] if shift else np.zeros((n, 1), T)
    m = np.where(lv, zv - z_first, T(0)).astype(T)
    wm = (wv * m).astype(T)
    W_in, M_in = np.cumsum(wv, 1, dtype=T), np.cumsum(wm, 1, dtype=T)
    W_lt, M_lt = np.concatenate([np.zeros((n, 1), T), W_in[:, :-1]], 1), np.concatenate([np.zeros((n, 1), T), M_in[:, :-1]], 1)
    W_gt, M_gt = (W_in[:, -1:] - W_in).astype(T), (M_in[:, -1:] - M_in).astype(T)
    before = ((m * W_lt).astype(T) - M_lt).astype(T)
    behind = (M_gt - (m * W_gt).astype(T)).astype(T)
    pair = np.cumsum((wv * before).astype(T), 1, dtype=T)[:, -1]
    own = np.cumsum(((wv * wv).astype(T) * dv).astype(T), 1, dtype=T)[:, -1]
    loss = (T(2) * pair + T(1.0 / 3.0) * own).astype(T)
    grad = np.where(lv, T(2) * (before + behind).astype(T) + T(2.0 / 3.0) * (wv * dv).astype(T), T(0)).astype(T)
    any_live = lv.any(1)
    scale = np.ones(n, T) if ray_scale is None else np.asarray(ray_scale, T)
    scale = np.where(any_live, np.nan_to_num(scale, nan=0.0, posinf=0.0, neginf=0.0), T(0)).astype(T)
    return (loss * scale).astype(T), (grad * scale[:, None]).astype(T)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def composite_weights(sigma, dists):
    """w = a * cumprod(1 - a + 1e-10, exclusive), a = 1 - exp(-relu(sigma) dists): the composite's weights, restated (float64)."""
    a = 1.0 - np.exp(-np.maximum(sigma, 0.0) * dists)
    trans = np.cumprod(1.0 - a + 1e-10, 1)
    return a * np.concatenate([np.ones_like(trans[:, :1]), trans[:, :-1]], 1)


def ray_batch(n, S, family, near=(2.0, 6.0), span=(0.5, 2.0), seed=0):
    """(w [n, S], z [n, S]) float32: jittered depths between a per-ray near and near + span, and the composite's weights of random densities
    along them -- "smooth": a broad bump of moderate density, every sample with some weight; "peaky": a few samples a ray of a density that
    saturates the ray there, most weights tiny or exactly 0."""
    rng = np.random.default_rng(seed)
    lo = rng.uniform(*near, size=(n, 1))
    sp = rng.uniform(*span, size=(n, 1))
    z = (lo + sp * (np.arange(S)[None, :] + rng.uniform(0.05, 0.95, size=(n, S))) / S).astype(F)
    z64 = z.astype(np.float64)
    d = default_widths(z64) if S > 1 else sp
    u = (z64 - lo) / sp
    if family == "smooth":
        sigma = rng.uniform(0.5, 4.0, size=(n, 1)) / sp * np.exp(-((u - rng.uniform(0.3, 0.7, size=(n, 1))) / 0.35) ** 2) * rng.uniform(0.5, 1.5, size=(n, S))
    else:
        sigma = np.where(rng.uniform(size=(n, S)) < min(1.0, 3.0 / S), rng.uniform(200.0, 4000.0, size=(n, S)) * S / sp, rng.uniform(0.0, 0.02, size=(n, S)) / sp)
        sigma[rng.uniform(size=(n, S)) < 0.2] = 0.0
    return composite_weights(sigma, d).astype(F), z


# (id, N, S, family, near, span, widths: None = the depths' differences | "given")
SAMPLE_COUNTS = [1, 2, 3, 63, 64, 65, 128, 129, 255, 1024, 4096]
RAY_COUNTS = {1: 3, 2: 1, 3: 5, 63: 9, 64: 257, 65: 257, 128: 3, 129: 5, 255: 9, 1024: 3, 4096: 5}       # rays a workgroup (4) do not divide N
NEAR, SPAN = (2.0, 6.0), (0.5, 2.0)


def parity_cases():
    rows = []
    for k, S in enumerate(SAMPLE_COUNTS):
        fam = ("smooth", "peaky")[k % 2]
        rows.append((f"S{S}_N{RAY_COUNTS[S]}_{fam}", RAY_COUNTS[S], S, fam, NEAR, SPAN, "given" if S == 1 or S == 128 else None))
    rows.append(("S65_N9_smooth", 9, 65, "smooth", NEAR, SPAN, None))
    rows.append(("S129_N3_peaky_widths", 3, 129, "peaky", NEAR, SPAN, "given"))
    rows.append(("S256_N5_near500", 5, 256, "smooth", (500.0, 500.0), (0.5, 0.5), None))
    rows.append(("S65_N257_smooth", 257, 65, "smooth", NEAR, SPAN, None))          # the base of the calls past the capped grid (`large_base`)
    return rows


CASES = parity_cases()
CASE_IDS = [c[0] for c in CASES]
NEAR500 = [c for c in CASES if c[0] == "S256_N5_near500"][0]


@functools.lru_cache(maxsize=None)
def _case_inputs(cid):
    _, n, S, fam, near, span, wd = [c for c in CASES if c[0] == cid][0]
    seed = 1000 + 7 * S + n
    w, z = ray_batch(n, S, fam, near, span, seed)
    rng = np.random.default_rng(seed + 1)
    widths = None
    if wd == "given":                       # lengths along an un-normalised direction, as a trainer's dists are
        base = default_widths(z) if S > 1 else rng.uniform(0.01, 0.1, size=(n, 1)).astype(F)
        widths = (base * rng.uniform(0.8, 1.6, size=(n, 1)).astype(F)).astype(F)
    scale = rng.uniform(0.5, 2.0, size=n).astype(F)
    return w, z, widths, scale


def case_inputs(case):
    """(w, z, widths or None, ray_scale) of a case, float32; the arrays are shared between the tests: do not write them."""
    return _case_inputs(case[0])


@functools.lru_cache(maxsize=None)
def _case_reference(cid):
    w, z, widths, scale = _case_inputs(cid)
    return pairwise64(w, z, widths, None, scale)


def case_reference(case):
    """(loss, grad) of the case in float64, computed once."""
    return _case_reference(case[0])


@functools.lru_cache(maxsize=None)
def _case_floor(cid):
    w, z, widths, scale = _case_inputs(cid)
    want = _case_reference(cid)
    got = linear_form(w, z, widths, None, scale)
    return rel_linf(got[0], want[0]), rel_linf(got[1], want[1])


def floor(case):
    """(floor of the loss, floor of the gradient): the float32 restatement's rel-Linf against float64."""
    return _case_floor(case[0])


def held(got_loss, got_grad, want, floors, label, report=print):
    """The figures, printed; then the gate."""
    e = (rel_linf(got_loss, want[0]) if got_loss is not None else 0.0, rel_linf(got_grad, want[1]) if got_grad is not None else 0.0)
    report(f"| {label} | loss {e[0]:.2e} floor {floors[0]:.2e} gate {gate(floors[0]):.1e} | grad {e[1]:.2e} floor {floors[1]:.2e} gate {gate(floors[1]):.1e} |")
    assert e[0] <= gate(floors[0]) and e[1] <= gate(floors[1]), (label, e, floors)
    return e


# ---- liveness ----------------------------------------------------------------------------------------------------------------------------
LIVE_N, LIVE_S = 5, 200                      # four chunks, the last one short
LIVE_PATTERNS = ["all_dead", "one_in_last_chunk", "first_behind_chunk0", "random35"]
# ... and as the patches of an instanced step leave a ray (seeded by the list index: append only): a whole dead chunk BETWEEN live ones (pass 2's
# empty-chunk branch entered with carries that are not zero), whole dead chunks BEHIND the last live sample, patches that end on the chunk edges
PATCH_PATTERNS = ["dead_chunk_between", "dead_tail", "patch_ends_on_chunk_edges", "two_short_patches"]
LIVE_PATTERNS += PATCH_PATTERNS


@functools.lru_cache(maxsize=None)
def live_case(pattern):
    """(w, z, widths, live, ray_scale) float32 with NaN in w, z and widths wherever a sample is not live, and the mask [n, S]."""
    n, S = LIVE_N, LIVE_S
    w, z = ray_batch(n, S, "smooth", NEAR, SPAN, seed=77)
    rng = np.random.default_rng(78 + LIVE_PATTERNS.index(pattern))
    widths = (default_widths(z) * rng.uniform(0.8, 1.6, size=(n, 1)).astype(F)).astype(F)
    mask = np.zeros((n, S), bool)
    if pattern == "one_in_last_chunk":
        mask[np.arange(n), 192 + rng.integers(0, S - 192, size=n)] = True
    elif pattern == "first_behind_chunk0":
        mask[:, 64:] = rng.uniform(size=(n, S - 64)) < 0.5
        mask[0, :130] = False                                                     # ... and behind chunk 1 on one ray
        mask[:, 150] = True
    elif pattern == "random35":
        mask = rng.uniform(size=(n, S)) < 0.35
    elif pattern == "dead_chunk_between":                                         # two patches, chunk [64, 128) entirely dead between them
        mask[:, :64] = rng.uniform(size=(n, 64)) < 0.6
        mask[:, 128:] = rng.uniform(size=(n, S - 128)) < 0.6
        mask[:, [5, 190]] = True
    elif pattern == "dead_tail":                                                  # the ray leaves its patch early: nothing behind sample 70
        mask[:, :70] = rng.uniform(size=(n, 70)) < 0.7
        mask[:, [3, 69]] = True
    elif pattern == "patch_ends_on_chunk_edges":
        mask[:, 37:64] = True
        mask[:, 128:192] = True
    elif pattern == "two_short_patches":
        mask[:, 10:14] = True
        mask[:, 150:153] = True
    return _live_pack(w, z, widths, mask, rng)


def _live_pack(w, z, widths, mask, rng):
    n, S = mask.shape
    live = np.where(mask, widths, F(0)).astype(F)                                 # dists in the role of live: > 0 inside a patch
    live[~mask & (rng.uniform(size=(n, S)) < 0.3)] = F(-1.0)
    w, z, widths = (np.where(mask, a, F(np.nan)).astype(F) for a in (w, z, widths))
    scale = rng.uniform(0.5, 2.0, size=n).astype(F)
    return w, z, widths, live, scale, mask


LIMIT_N, LIMIT_S, LIMIT_LIVE = 3, 4096, ((100, 1000), (3000, 4090))                # 31 whole dead chunks, 1024 .. 3007, between live ones
LIMIT_SEED = 91                                                                  # (of the weights: the one to change if a floor passes FLOOR_GUARD)


@functools.lru_cache(maxsize=None)
def live_limit_case():
    """`live_case`'s tuple at the sample limit: 3 rays of 4096 samples, live exactly in [100, 1000) and [3000, 4090)."""
    n, S = LIMIT_N, LIMIT_S
    w, z = ray_batch(n, S, "smooth", NEAR, SPAN, seed=LIMIT_SEED)
    rng = np.random.default_rng(LIMIT_SEED + 1)
    widths = (default_widths(z) * rng.uniform(0.8, 1.6, size=(n, 1)).astype(F)).astype(F)
    mask = np.zeros((n, S), bool)
    for a, b in LIMIT_LIVE:
        mask[:, a:b] = True
    return _live_pack(w, z, widths, mask, rng)


@functools.lru_cache(maxsize=None)
def live_figures(pattern):
    """(float64 reference, float32 floors) of `live_case(pattern)` -- "limit": of `live_limit_case()` --, computed once."""
    w, z, widths, live, scale, _ = live_limit_case() if pattern == "limit" else live_case(pattern)
    want, f32 = pairwise64(w, z, widths, live, scale), linear_form(w, z, widths, live, scale)
    return want, (rel_linf(f32[0], want[0]), rel_linf(f32[1], want[1]))


# ---- past the capped grid: 256 * 8 workgroups of four waves, a ray a wave; from 8193 rays on a wave takes a second ray ---------------------
GRID_RAYS = 256 * 8 * 4
LARGE_N = [GRID_RAYS, GRID_RAYS + 1, 2 * GRID_RAYS + 5]      # one pass exactly; one wave's second ray; three passes for five waves
LARGE_BASE = "S65_N257_smooth"                               # 257 is prime and 8192 mod 257 = 225: a wave meets another base row in every pass
MISSED, PARTIAL, NAN_W = 0, 1, 130                           # the replaced rows of the base; MISSED and NAN_W have no live sample
PARTIAL_LIVE = 30


@functools.lru_cache(maxsize=None)
def large_base():
    """(w, z, dead [257], (loss, grad) float64 without a ray_scale, floors) of the base batch: the case's rays with three rows replaced -- a
    missed ray (depths inf, weights 0), a ray finite only in its first 30 samples, a ray with NaN weights behind depths that are not finite."""
    case = [c for c in CASES if c[0] == LARGE_BASE][0]
    w, z, widths, _ = case_inputs(case)
    assert widths is None
    w, z = w.copy(), z.copy()
    w[MISSED], z[MISSED] = 0.0, np.inf
    z[PARTIAL, PARTIAL_LIVE:] = np.inf
    w[NAN_W], z[NAN_W, ::2], z[NAN_W, 1::2] = np.nan, np.inf, np.nan
    dead = ~np.isfinite(z).any(1)
    return w, z, dead, pairwise64(w, z), floor(case)


def cycled(a, n):
    """Row k of the result is row k mod len(a) of a."""
    return np.asarray(a)[np.arange(n) % len(a)]


def large_scale(n, dead, seed=5):
    """A per-ray ray_scale over the whole large batch, NaN on the rays without a live sample."""
    scale = np.random.default_rng(seed + n).uniform(0.5, 2.0, size=n).astype(F)
    scale[cycled(dead, n)] = np.nan
    return scale


def large_reference(n, scale):
    """The float64 reference of the 257 base rows, cycled, times `scale`; zeros on the dead rows whatever `scale` holds there."""
    _, _, dead, (loss, grad), _ = large_base()
    s = np.where(cycled(dead, n), 0.0, np.nan_to_num(np.asarray(scale, np.float64), nan=0.0))
    return cycled(loss, n) * s, cycled(grad, n) * s[:, None]


# ---- the loss a trainer takes, stated with the pair sum in torch ---------------------------------------------------------------------------
def pairwise_torch(weights, z_vals, widths=None, ray_scale=None):
    """The per-ray distortion as the textbook torch expression ([N, S, S] intermediates; autograd gives its gradient): the parent's own way
    to this loss.  Depths that are not finite count as not live."""
    import torch
    z = torch.as_tensor(z_vals, device=weights.device, dtype=weights.dtype)
    lv = torch.isfinite(z)
    zero = torch.zeros_like(z)
    zz, w = torch.where(lv, z, zero), torch.where(lv, weights, zero)
    if widths is None:                                  # (0 where the neighbouring depth is not finite)
        d = z[:, 1:] - z[:, :-1]
        d = torch.cat([d, d[:, -1:]], 1) if z.shape[1] > 1 else zero
        d = torch.where(torch.isfinite(d), d, zero)
    else:
        d = torch.as_tensor(widths, device=weights.device, dtype=weights.dtype)
    d = torch.where(lv, d, zero)
    val = (w[:, :, None] * w[:, None, :] * (zz[:, :, None] - zz[:, None, :]).abs()).sum((1, 2)) + (w * w * d).sum(1) / 3.0
    if ray_scale is not None:
        val = val * torch.where(lv.any(1), torch.as_tensor(ray_scale, device=weights.device, dtype=weights.dtype), torch.zeros_like(val))
    return val


def span_scale(z):
    """1 / (z[n, -1] - z[n, 0]) in torch, 0 where that is not finite (a missed ray)."""
    import torch
    s = 1.0 / (z[:, -1] - z[:, 0])
    return torch.where(torch.isfinite(s), s, torch.zeros_like(s))


def pairwise_loss(base, weight=0.1):
    """`Distortion(base, weight, normalize=True)` stated with `pairwise_torch`: a callable loss that names `weights` and `z_vals`."""
    import torch

    def loss(color_true=None, alpha_true=None, color_pred=None, alpha_pred=None, weights=None, z_vals=None):
        z = torch.as_tensor(z_vals, device=weights.device, dtype=weights.dtype)
        return base(color_true=color_true, alpha_true=alpha_true, color_pred=color_pred, alpha_pred=alpha_pred) + weight * (pairwise_torch(weights, z) * span_scale(z)).mean()
    return loss


# ---- as_callable's reference ----------------------------------------------------------------------------------------------------------------
LOSS_SETTINGS = [
    ("nerf_mse", "NerfLoss", dict(loss_fn="network.loss.mse")),
    ("nerf_smape", "NerfLoss", dict(loss_fn="network.loss.smape")),
    ("alpha_smape_mse_hard", "AlphaLoss", dict(loss_fn="network.loss.smape", alpha_loss_fn="network.loss.mse")),
    ("alpha_mse_soft_gamma", "AlphaLoss", dict(loss_fn="network.loss.mse", alpha_loss_fn="network.loss.smape", gamma=0.3, use_hard_mask=False)),
    ("alpha_unfiltered", "AlphaLoss", dict(loss_fn="network.loss.smape", filter_color_loss=False)),
]


def descriptor_loss64(kind, kw, color_true, alpha_true, color_pred, alpha_pred):
    """network/loss.py:6-59 in float64 numpy."""
    fn = {"mse": lambda t, p: np.mean((t - p) ** 2), "smape": lambda t, p: np.mean(np.abs(t - p) / (t + p + 1e-2))}
    name = lambda path: path.rsplit(".", 1)[-1]
    ct, at, cp, ap = (np.asarray(x, np.float64) for x in (color_true, alpha_true, color_pred, alpha_pred))
    loss_fn = fn[name(kw.get("loss_fn", "network.loss.mse"))]
    if kind == "NerfLoss":
        return float(loss_fn(ct, cp))
    alpha_fn = fn[name(kw["alpha_loss_fn"])] if kw.get("alpha_loss_fn") else loss_fn
    if kw.get("filter_color_loss", True):
        mask = (at[:, None] > 0).astype(np.float64) if kw.get("use_hard_mask", True) else at[:, None]
        ct, cp = ct * mask, cp * mask
    return float(loss_fn(ct, cp) + kw.get("gamma", 1) * alpha_fn(at, ap))
