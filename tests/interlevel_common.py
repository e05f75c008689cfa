"""What the tests of the interlevel loss share (tests/test_ray_interlevel.py on the CPU, tests/test_gpu_ray_interlevel.py on the GPU;
`ntx_ray_interlevel`, `nerf_tex_amd.loss.ray_interlevel` / `interlevel`, `nerf_tex_amd.train.ProposalTrainer`): the formula of
include/nerftex.h restated twice -- `reference(..., dtype=float64)`, and the same statement in float32 with every sum added sequentially in
the stated order (what any float32 evaluation is off by: the FLOOR) -- a dense torch statement for autograd, the case table, and the gate.

THE GATE is tests.distortion_common.gate, imported and not edited: error <= min(max(4 floors, 5e-7), 1e-4); errors and floors are rel-Linf
over the batch.  tests/test_ray_interlevel.py holds every floor <= FLOOR_GUARD, so four floors never reach the cap, and max q >= 0.5 on every
case: a case whose loss is all zeros would pass any gate.

Inputs: `ray_batch` rays for the proposal set; the fine depths are those merged with uniform draws inside the span and sorted (exact ties
between the two sets everywhere; where a case has no more fine than proposal samples, a sorted subset of the proposal depths), or -- "free"
-- independent depths with no ties; the fine weights are the composite's weights of an independent density.  Off the merged grid
(`off_grid_inputs`): "repeats", exact repeats inside either set, and "beyond", fine samples far outside the proposal's range.  `large_base` /
`large_reference`: the 257 rows the calls past the capped grid cycle, and their float64 reference."""

import functools

import numpy as np

from tests.distortion_common import CAP, F, FLOOR_GUARD, composite_weights, default_widths, gate, ray_batch, rel_linf   # noqa: F401 (shared with the tests)

EPS = 2.0 ** -23


# ---- the formula, twice ------------------------------------------------------------------------------------------------------------------
def interval_ends(z):
    """b_k = z_{k+1}, the stored neighbour; b_last = z_last + (z_last - z_{last-1}); b_0 = z_0 for one sample (in z's dtype)."""
    z = np.asarray(z)
    if z.shape[1] == 1:
        return z.copy()
    with np.errstate(invalid="ignore"):
        last = (z[:, -1:] + (z[:, -1:] - z[:, -2:-1]).astype(z.dtype)).astype(z.dtype)
    return np.concatenate([z[:, 1:], last], 1)


def reference(w, z, wp, zp, ray_scale=None, eps=EPS, dtype=np.float64):
    """(loss [N], grad_prop [N, S_p], grad_fine [N, S], q [N, S]) in `dtype`, every sum added sequentially in the stated order (numpy's cumsum
    adds front to back in the array's type); a ray with a depth that is not finite: zeros, whatever its weights and ray_scale hold."""
    T = dtype
    w, z, wp, zp = (np.asarray(a, T) for a in (w, z, wp, zp))
    n, S = w.shape
    Sp = wp.shape[1]
    b, bp = interval_ends(z), interval_ends(zp)
    eps = T(eps)
    seq = lambda v: np.cumsum(v, dtype=T)[-1] if len(v) else T(0)
    L, gp, gf, qs = np.zeros(n, T), np.zeros((n, Sp), T), np.zeros((n, S), T), np.zeros((n, S), T)
    live = np.isfinite(z).all(1) & np.isfinite(zp).all(1)
    scale = np.ones(n, T) if ray_scale is None else np.asarray(ray_scale, T)
    for r in np.nonzero(live)[0]:
        lo = np.searchsorted(bp[r], z[r], side="right")                 # #{j : b^_j <= a_i}
        hi = np.searchsorted(zp[r], b[r], side="left")                  # #{j : z^_j < b_i}
        bound = np.array([seq(wp[r, lo[i]:hi[i]]) for i in range(S)], T)
        res = np.maximum(T(0), (w[r] - bound).astype(T)).astype(T)
        q = (res / (w[r] + eps).astype(T)).astype(T)
        qs[r] = q
        L[r] = seq((res * q).astype(T)) * scale[r]
        gf[r] = ((q * (T(2) - q).astype(T)).astype(T) * scale[r]).astype(T)
        lo = np.searchsorted(b[r], zp[r], side="right")                 # #{i : b_i <= z^_j}
        hi = np.searchsorted(z[r], bp[r], side="left")                  # #{i : a_i < b^_j}
        gp[r] = (np.array([T(-2) * seq(q[lo[j]:hi[j]]) for j in range(Sp)], T) * scale[r]).astype(T)
    return L, gp, gf, qs


def dense_torch(w, z, wp, zp, eps=EPS):
    """The per-ray loss as the textbook torch expression, an [N, S, S_p] overlap mask (autograd gives both gradients); finite depths only."""
    import torch
    ends = lambda x: x.clone() if x.shape[1] == 1 else torch.cat([x[:, 1:], x[:, -1:] + (x[:, -1:] - x[:, -2:-1])], 1)
    b, bp = ends(z), ends(zp)
    mask = (zp[:, None, :] < b[:, :, None]) & (bp[:, None, :] > z[:, :, None])
    bound = (mask.to(wp.dtype) * wp[:, None, :]).sum(-1)
    res = torch.relu(w - bound)
    return (res * res / (w + eps)).sum(-1)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
NEAR, SPAN = (2.0, 6.0), (0.5, 2.0)
# (id, N, S_p, S, family, near, span, depths: "merged" | "free" | "repeats" | "beyond")
# (S_p, S, N, family): N is no multiple of the four rays of a workgroup; two proposal samples of a smooth ray cover whatever the fine
# pass holds (max q 0.06), so that shape is peaky
_SHAPES = [(1, 1, 5, "smooth"), (1, 2, 3, "peaky"), (2, 3, 5, "peaky"), (3, 2, 9, "smooth"), (8, 16, 9, "smooth"), (63, 64, 5, "peaky"), (64, 65, 257, "smooth"),
           (65, 129, 9, "peaky"), (24, 40, 5, "smooth"), (128, 256, 7, "peaky"), (129, 128, 5, "smooth"), (1024, 2048, 3, "peaky"), (4096, 4096, 3, "smooth")]


def parity_cases():
    rows = []
    for Sp, S, n, fam in _SHAPES:
        rows.append((f"P{Sp}_S{S}_N{n}_{fam}", n, Sp, S, fam, NEAR, SPAN, "merged"))
    rows.append(("P65_S129_N5_smooth", 5, 65, 129, "smooth", NEAR, SPAN, "merged"))
    rows.append(("P64_S128_N5_near500", 5, 64, 128, "smooth", (500.0, 500.0), (0.5, 0.5), "merged"))
    rows.append(("P63_S130_N6_free", 6, 63, 130, "peaky", NEAR, SPAN, "free"))
    for how in OFF_GRID:                                # inputs off the merged grid: `off_grid_inputs`
        rows += [(f"P65_S130_N6_{how}_{fam}", 6, 65, 130, fam, NEAR, SPAN, how) for fam in ("peaky", "smooth")]
    return rows


OFF_GRID = ("repeats", "beyond")


CASES = parity_cases()
CASE_IDS = [c[0] for c in CASES]
by_id = lambda cid: [c for c in CASES if c[0] == cid][0]


def fine_set(zp, S, family, how, seed):
    """(w [n, S], z [n, S]) float32 for a proposal row set zp: the fine depths, and the composite's weights of an independent density."""
    rng = np.random.default_rng(seed)
    n, Sp = zp.shape
    z0 = zp[:, :1].astype(np.float64)
    sp = (zp[:, -1:] - zp[:, :1]).astype(np.float64) if Sp > 1 else np.full((n, 1), 0.5)
    if how == "free":
        z = np.sort((z0 + sp * rng.uniform(-0.05, 1.05, size=(n, S))).astype(F), 1)
    elif S > Sp:
        extra = (z0 + sp * rng.uniform(0.02, 0.98, size=(n, S - Sp))).astype(F)
        z = np.sort(np.concatenate([zp, extra], 1), 1)
    else:                                               # a sorted subset of the proposal depths, first sample kept
        keep = np.stack([np.sort(np.concatenate([[0], 1 + rng.permutation(Sp - 1)[:S - 1]])) for _ in range(n)]) if Sp > 1 else np.zeros((n, 1), int)
        z = np.take_along_axis(zp, keep, 1)
    z64 = z.astype(np.float64)
    d = default_widths(z64) if S > 1 else sp
    u = (z64 - z0) / sp
    if family == "smooth":
        sigma = rng.uniform(2.0, 8.0, size=(n, 1)) / sp * np.exp(-((u - rng.uniform(0.3, 0.7, size=(n, 1))) / 0.15) ** 2) * rng.uniform(0.5, 1.5, size=(n, S))
    else:
        sigma = np.where(rng.uniform(size=(n, S)) < min(1.0, 3.0 / S), rng.uniform(200.0, 4000.0, size=(n, S)) * S / sp, rng.uniform(0.0, 0.02, size=(n, S)) / sp)
    return composite_weights(sigma, d).astype(F), z


@functools.lru_cache(maxsize=None)
def _case_inputs(cid):
    _, n, Sp, S, fam, near, span, how = by_id(cid)
    seed = 2000 + 7 * S + 3 * Sp + n
    wp, zp = ray_batch(n, Sp, fam, near, span, seed)
    w, z, zp = off_grid_inputs(zp, S, fam, how, seed + 1) if how in OFF_GRID else fine_set(zp, S, fam, how, seed + 1) + (zp,)
    scale = np.random.default_rng(seed + 2).uniform(0.5, 2.0, size=n).astype(F)
    return w, z, wp, zp, scale


def case_inputs(case):
    """(w, z, wp, zp, ray_scale) of a case, float32; the arrays are shared between the tests: do not write them."""
    return _case_inputs(case[0])


@functools.lru_cache(maxsize=None)
def _case_reference(cid):
    return reference(*_case_inputs(cid))


def case_reference(case):
    """(loss, grad_prop, grad_fine, q) of the case in float64, computed once."""
    return _case_reference(case[0])


@functools.lru_cache(maxsize=None)
def _case_floor(cid):
    want, got = _case_reference(cid), reference(*_case_inputs(cid), dtype=F)
    return tuple(rel_linf(got[k], want[k]) for k in range(3))


def floor(case):
    """(floor of the loss, of dL/d proposal weights, of dL/d fine weights): the float32 restatement's rel-Linf against float64."""
    return _case_floor(case[0])


def held(got, want, floors, label, report=print):
    """The figures of (loss, grad_prop, grad_fine) -- None: not asked for --, printed; then the gate."""
    names = ("loss", "d prop", "d fine")
    e = [0.0 if got[k] is None else rel_linf(got[k], want[k]) for k in range(3)]
    report(f"| {label} | " + " | ".join(f"{names[k]} {e[k]:.2e} floor {floors[k]:.2e} gate {gate(floors[k]):.1e}" for k in range(3)) + " |")
    assert all(e[k] <= gate(floors[k]) for k in range(3)), (label, e, floors)
    return e


# ---- inputs off the merged grid ------------------------------------------------------------------------------------------------------------
N_REPEATS, N_REPEATS_PROP = 13, 6


def off_grid_inputs(zp, S, family, how, seed):
    """(w [n, S], z [n, S], zp) float32 for a proposal row set zp.
    "repeats": the merged set, then 13 fine and 6 proposal depths a ray copied from their left neighbours (zero-width intervals inside a set,
    where the two searches of a sample give lo > hi), the last two fine depths of every ray and the last two proposal depths of ray 0 equal
    (a zero LAST width), sorted again; the weights are the merged set's, so a zero-width interval holds a weight.
    "beyond": fine depths uniform in [z^_0 - span, z^_last + span], sorted: a third of them on either side overlap no proposal interval
    (bound 0, q = w / (w + eps)), and the outer proposal intervals overlap several fine ones; the density's bump lies in the fine set's range."""
    rng = np.random.default_rng(seed + 50)
    n, Sp = zp.shape
    if how == "repeats":
        w, z = fine_set(zp, S, family, "merged", seed)
        z, zp = z.copy(), zp.copy()
        for r in range(n):
            for row, count in ((z[r], N_REPEATS), (zp[r], N_REPEATS_PROP)):
                for i in np.sort(1 + rng.permutation(len(row) - 3)[:count]):          # (increasing: a run of picks repeats one depth)
                    row[i] = row[i - 1]
            v = zp[r, np.nonzero(zp[r, 1:] == zp[r, :-1])[0][0]]                      # one repeat at the SAME depth in both sets: that is where lo > hi
            i = min(int(np.searchsorted(z[r], v, side="left")), S - 4)
            z[r, i], z[r, i + 1] = v, v
        z[:, -1] = z[:, -2]
        zp[0, -1] = zp[0, -2]
        return w, np.sort(z, 1), np.sort(zp, 1)
    assert how == "beyond"
    z0 = zp[:, :1].astype(np.float64)
    sp = (zp[:, -1:] - zp[:, :1]).astype(np.float64)
    z = np.sort((z0 + sp * rng.uniform(-1.0, 2.0, size=(n, S))).astype(F), 1)
    z64 = z.astype(np.float64)
    lo, wide = z64[:, :1], z64[:, -1:] - z64[:, :1]
    u = (z64 - lo) / wide
    if family == "smooth":
        sigma = rng.uniform(2.0, 8.0, size=(n, 1)) / wide * np.exp(-((u - rng.uniform(0.3, 0.7, size=(n, 1))) / 0.15) ** 2) * rng.uniform(0.5, 1.5, size=(n, S))
    else:
        sigma = np.where(rng.uniform(size=(n, S)) < min(1.0, 3.0 / S), rng.uniform(200.0, 4000.0, size=(n, S)) * S / wide, rng.uniform(0.0, 0.02, size=(n, S)) / wide)
    return composite_weights(sigma, default_widths(z64)).astype(F), z, zp


# ---- past the capped grid (tests.distortion_common has the sizes and `cycled`) ---------------------------------------------------------------
LARGE_BASE = "P64_S65_N257_smooth"
INF_FINE, ORDINARY, NAN_PROP = 0, 1, 130                 # the replaced rows of the base: INF_FINE and NAN_PROP are not live, ORDINARY is left as it is


@functools.lru_cache(maxsize=None)
def large_base():
    """(w, z, wp, zp, dead [257], (loss, grad_prop, grad_fine) float64 without a ray_scale, floors) of the base batch: the case's rays with an
    inf in the fine depths alone on one row, and a NaN in the proposal depths alone and NaN in both sets of weights on another."""
    case = by_id(LARGE_BASE)
    w, z, wp, zp, _ = (a.copy() for a in case_inputs(case))
    z[INF_FINE, -1] = np.inf
    zp[NAN_PROP, 17], w[NAN_PROP], wp[NAN_PROP] = np.nan, np.nan, np.nan
    dead = ~(np.isfinite(z).all(1) & np.isfinite(zp).all(1))
    return w, z, wp, zp, dead, reference(w, z, wp, zp)[:3], floor(case)


def large_reference(n, scale):
    """The float64 reference of the 257 base rows, cycled, times `scale`; zeros on the dead rows whatever `scale` holds there."""
    from tests.distortion_common import cycled
    dead, want = large_base()[4:6]
    s = np.where(cycled(dead, n), 0.0, np.nan_to_num(np.asarray(scale, np.float64), nan=0.0))
    return cycled(want[0], n) * s, cycled(want[1], n) * s[:, None], cycled(want[2], n) * s[:, None]
