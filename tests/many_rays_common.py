"""What the tests of training steps with more than 1024 rays share (tests/test_train_many_rays.py on the CPU, tests/test_gpu_train_many_rays.py
on the GPU): the fixtures -- many SHORT rays, so that a step has a few thousand samples and its float64 restatement takes a fraction of a
second -- and what a fixture has to hold for a pass to mean something.

Why 1024: `live_scan_kernel` (csrc/ntx_trainer.hip) is one workgroup of 1024 threads, thread k taking the `per = ceil(n_rays / 1024)` rays
k * per .. ; `loss_sum_kernel` strides the rays by 1024; dirrow_kernel, the composite kernels, the parameter and ray folds and the depth jitter
have grids or keys of the ray count.  Up to 1024 rays `per` is 1 and no thread of either kernel sees a second ray.

No yardstick of its own: the instanced step is tests/instanced_train_common.py's float64 restatement, the whole-ray step oracle/train_oracle.py's
(tests/train_branch_oracle.py's with parameter branches), the per-parameter and per-ray gradients tests/param_grad_common.py's and
tests/input_grad_common.py's; the bars are `clc.check_layers`, `pgc.check_param_gradients`, `igc.check_input_gradients` and the 1e-5 / 1e-4 of
tests/test_gpu_train.py.  The seeds are chosen on the CPU (tests/test_train_many_rays.py), with the restatements' own float32 ReLU patterns.

Fixtures that are not the first thing one would write down, and why:
- the one-ray live masks (`MASK_SEEDS`) have seeds of their own per back end: most positions have density 0 and no gradient, as
  `itc.LIVE_MASK_SEEDS` and `fic.EDGE_SEEDS` say of their one-live-sample edges;
- `every_sample` and `every_other_range` run at a tenth of the density_scale, as `itc.edge_setup`'s dense masks do;
- at 1025 rays (513 scan ranges in all) 400 ranges with a live sample are asked for, 500 at the larger sizes;
- the whole-ray fixtures' rays are cut short (`short_rays`), and the parameter and ray gradient cases run under NerfLoss(mse) on batch seed 5:
  under AlphaLoss(smape) a single three-sample ray's own row sits 1e-3 from float64 in float32 autograd itself (seeds 3 .. 8 tried)."""

from types import SimpleNamespace

import numpy as np
import torch

from oracle import torch_cpu as tcpu
from oracle import train_oracle as tro
from tests import custom_loss_common as clc
from tests import fused_instanced_common as fic
from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests import train_branch_oracle as tbo
from tests.train_common import F, LOSSES, layer_slices, mip_batch, rel_linf, step_depths, step_noise, targets

SCAN_THREADS = 1024                                                              # live_scan_kernel's workgroup, loss_sum_kernel's stride


def per_of(n):
    """Rays per scan thread."""
    return -(-n // SCAN_THREADS)


def range_counts(live):
    """The live samples of every non-empty scan range (thread k's rays k * per .. min((k + 1) * per, n) - 1) of a live mask [n, S]."""
    n = live.shape[0]
    return np.bincount(np.arange(n) // per_of(n), live.sum(1), minlength=-(-n // per_of(n)))


# ---- 1. instanced steps -------------------------------------------------------------------------------------------------------------------------
BACKENDS = ("flex", "chain")
INST_CASE = dict(flex=itc.CASES[0], chain=fic.CASES[0])                          # both (1, 6) parameters, no blur: the same buffers
INST_S = 3
# 1023: the last scan thread's range empty at per = 1; 1024: the largest n with per = 1; 1025: per = 2, a one-ray last range and 511 threads beyond
# the end; 2049: per = 3 and a thread whose first ray is n_rays; 3000: a ragged per = 3
INST_SIZES = (1023, 1024, 1025, 2049, 3000)
MODE_SIZES = (1024, 2049)                                                        # per-sample gradients on: one per = 1 size, one per >= 2
MASK_N = 2049                                                                    # per = 3: 683 ranges of three rays, and thread 683's first ray is n_rays
MASKS = ("only_ray_0", "only_last_ray", "every_sample", "every_other_range", "one_per_range")
# (the buffers' seed, the mask's) where they are not (70 + n, 0): the first pair, buffers' seed ascending, under which a live sample of the one ray
# lies inside the back end's medium and every layer has a gradient
MASK_SEEDS = {("flex", "only_ray_0"): (2119, 1), ("flex", "only_last_ray"): (2122, 1), ("chain", "only_ray_0"): (2145, 0), ("chain", "only_last_ray"): (2123, 1)}
DENSE_MASKS = ("every_sample", "every_other_range")


def inst_setup(backend, n, seed=None):
    """`itc.case_setup`'s tuple of the back end's first case at n rays x 3 samples."""
    return itc.case_setup(INST_CASE[backend], n=n, S=INST_S, seed=70 + n if seed is None else seed)


def mask_of(name, seed=0, n=MASK_N, S=INST_S):
    """The explicit live mask [n, S] of a name."""
    per = per_of(n)
    mask = np.zeros((n, S), bool)
    rng = np.random.default_rng(seed)
    some = lambda: rng.permutation(S)[:rng.integers(1, S + 1)]                   # a seeded, non-empty choice of a ray's samples
    if name == "only_ray_0":
        mask[0, some()] = True
    elif name == "only_last_ray":
        mask[n - 1, some()] = True
    elif name == "every_sample":
        mask[:] = True
    elif name == "every_other_range":
        mask[(np.arange(n) // per) % 2 == 0] = True
    elif name == "one_per_range":
        first = np.arange(0, n, per)
        mask[first, rng.integers(0, S, size=len(first))] = True
    else:
        raise KeyError(name)
    return mask


def mask_setup(backend, name):
    """`inst_setup` at 2049 x 3 under an explicit live mask, every ray hit; (setup, the mask)."""
    bseed, mseed = MASK_SEEDS.get((backend, name), (70 + MASK_N, 0))
    model, spec, wts, bufs, hit, cone, kn, okw = inst_setup(backend, MASK_N, bseed)
    mask = mask_of(name, mseed)
    bufs, hit = itc.with_live_mask(bufs, hit, mask)
    if name in DENSE_MASKS:
        okw = dict(okw, density_scale=okw["density_scale"] / 10)
        kn = dict(kn, density_scale=okw["density_scale"])
    return (model, spec, wts, bufs, hit, cone, kn, okw), mask


def first_rays(setup, n):
    """The same setup on the first n rays' buffers."""
    model, spec, wts, bufs, hit, cone, kn, okw = setup
    N = len(hit)
    bufs = tuple(b[b[:, 0] < n] if k == 8 else b[:n] for k, b in enumerate(bufs))     # (8: the indices of the rays that are hit)
    assert all(len(b) == n for k, b in enumerate(bufs) if k != 8) and len(bufs[8]) == hit[:n].sum() and len(hit) == N
    return model, spec, wts, bufs, hit[:n], cone[:n], kn, okw


def check_random_buffers(setup):
    """What the random buffers have to hold so that a pass is not hollow; returns the live count."""
    _, _, _, bufs, hit, _, _, _ = setup
    dists, n = np.asarray(bufs[3]), len(hit)
    live = itc.live_mask(hit, dists)
    assert ((~hit) & (dists > 0).any(1)).any(), "no ray that is not hit although its dists are positive"
    assert (~live[hit]).all(1).any(), "no hit ray without a live sample"
    assert (dists[hit] < 0).any(), "no hit ray with negative dists"
    counts = range_counts(live)
    if per_of(n) >= 2:                                                           # (1025 rays are 513 ranges in all: 400 of them)
        assert (counts == 0).sum() >= 50 and (counts > 0).sum() >= (400 if n == 1025 else 500), ((counts == 0).sum(), (counts > 0).sum())
    assert live.sum() > 64 and live.sum() == len(itc.live_order(hit, dists))
    return int(live.sum())


def check_mask(setup, mask, name):
    """An explicit mask is what its name says; returns the live count."""
    _, _, _, bufs, hit, _, _, _ = setup
    n, S = mask.shape
    live = itc.live_mask(hit, bufs[3])
    assert hit.all() and np.array_equal(live, mask) and per_of(n) == 3 and len(range_counts(mask)) == 683
    rays, counts = np.nonzero(mask.any(1))[0], range_counts(mask)
    if name == "only_ray_0":
        assert list(rays) == [0]
    elif name == "only_last_ray":
        assert list(rays) == [n - 1] and counts[682] > 0 and not counts[:682].any()
    elif name == "every_sample":
        assert mask.sum() == n * S
    elif name == "every_other_range":
        assert (counts[1::2] == 0).all() and (counts[0::2] == 3 * S).all()
    elif name == "one_per_range":
        assert (counts == 1).all() and (rays % 3 == 0).all()
    return int(mask.sum())


def inst_fair(setup, samples=False, report=print):
    """A fixture's floors on the CPU, on the float32 restatement's OWN ReLU patterns: every layer's float32 floor <= 5e-4 and largest gradient
    > 1e-6 (`samples`: and every column of the per-sample parameter and input gradients, over the live samples).  Returns (worst floor, the
    float64 restatement)."""
    _, spec, w, bufs, hit, cone, kn, okw = setup
    head = itc.quadratic_head(len(hit))
    pat = igc.own_instanced_patterns(spec, w, bufs, hit, cone, okw)
    if samples:
        want, want_in = fic.restate_all(spec, w, bufs, hit, cone, okw, head, pat, torch.float64)
        f32, f32_in = fic.restate_all(spec, w, bufs, hit, cone, okw, head, pat, torch.float32)
    else:
        want, f32 = (itc.restated(w, spec, bufs, hit, cone, head, dtype=dt, **okw, **pat) for dt in (torch.float64, torch.float32))
        want_in = f32_in = None
    assert len(want.live) >= 1
    fic.fair_all(spec, want, f32, want_in, f32_in, hit, bufs, report, margin=1.0, samples=samples)
    assert all(np.abs(want.grad[sl]).max() > 1e-6 for _, sl in layer_slices(spec))
    return max(rel_linf(f32.grad[sl], want.grad[sl]) for _, sl in layer_slices(spec)), want


# ---- 2. whole-ray steps -------------------------------------------------------------------------------------------------------------------------
# the three trainers: (trainer class name, n_parameters, arch, family) -- the chain, and `clc.TRAINER_CASES`' flex_w98_skips13 and branches_f
TRAINERS = dict(chain=("Trainer", (1, 6), None, "carpet"), flex=clc.TRAINER_CASES[1][1:5], branches=clc.TRAINER_CASES[2][1:5])
assert clc.TRAINER_CASES[1][0] == "flex_w98_skips13" and clc.TRAINER_CASES[2][0] == "branches_f"
MISS_2500 = list(range(12)) + [1023, 1024, 1025] + list(range(2485, 2500))       # the front, either side of the 1024th ray, the back
# (id, n, S, loss, knobs): both `loss_term` branches at every shape; the jitter on the two-sample rays, the missed rays at 2500, the raw noise at
# S = 32 (the chain's hoisted build: dirrow_kernel on 1025 rays)
WHOLE_CASES = [(f"{n}x{S}_{loss}", n, S, loss, kn) for n, S, kn in ((1025, 2, dict(perturb=True)), (2500, 3, dict(miss=MISS_2500)), (1025, 32, dict(noise_std=0.1)))
               for loss in ("alpha_smape", "nerf_mse")]
WHOLE_IDS = [c[0] for c in WHOLE_CASES]
NO_HOIST_CASE = WHOLE_CASES[4]
MIP_CASE = ("mip_1025x2", 1025, 2, "alpha_smape", dict(blur=0, perturb=True))
WHOLE_RUNS = [(tr, c) for tr in ("chain", "flex", "branches") for c in WHOLE_CASES] + [("mip", MIP_CASE)]
WHOLE_RUN_IDS = [f"{tr}_{c[0]}" for tr, c in WHOLE_RUNS]
WHOLE_DEFAULTS = dict(perturb=False, noise_std=0.0, miss=(), blur=None, seed=11, batch_seed=3)
assert {LOSSES[c[3]][0]["kind"] for c in WHOLE_CASES} == {"alpha", "nerf"}


def short_rays(t, S, of=64):
    """The rays' [near, far] cut to the middle S / 64 of the proxy's depth: S samples at the spacing of a 64-sample ray.  (Two or three samples
    over the whole depth are steps of half the proxy: 1 - exp(-sigma dist) then carries a float32 sigma's rounding so far that float32
    autograd of the restatement itself is 2e-4 .. 4e-4 off in the predictions and up to 2e-2 in a parameter column, beyond what the bars
    take -- tests/test_gpu_train.py's `tiny` says the same of its handful of coarse steps.)  A missed ray's inf stays."""
    t = np.asarray(t, F)
    t0 = np.where(np.isfinite(t), t, 0)
    mid, half = (t0[:, 0] + t0[:, 1]) / 2, (t0[:, 1] - t0[:, 0]) * F(S / (2.0 * of))
    return np.where(np.isfinite(t), np.stack([mid - half, mid + half], 1), t).astype(F)


def whole_setup(trainer, case):
    """A whole-ray fixture: model, spec, wts, batch = (ro, rd, t, cone, params [n, P], color, alpha) with the missed rays at t = inf and
    cone_scale NaN, and the knobs."""
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    cid, n, S, loss_name, knobs = case
    kn = dict(WHOLE_DEFAULTS, **knobs)
    if trainer == "mip":
        model, spec, wts = make_model((1, 3), kind="IPE", dense_media=True)
        ro, rd, t, cone, params = mip_batch(n, 5, seed=kn["batch_seed"])
        color, alpha = targets(n, 4)
    else:
        cls, npar, arch, fam = TRAINERS[trainer]
        model, spec, wts = make_model(npar, dense_media=True, arch=arch)
        ro, rd, t, cone, params, color, alpha = tbo.branch_batch(kn["batch_seed"], n, spec, fam) if pgc.has_branches(spec) else flex_batch(kn["batch_seed"], n, S, spec, fam)
    miss = np.zeros(n, bool); miss[list(kn["miss"])] = True
    t, cone = (t.copy() if trainer == "mip" else short_rays(t, S)), cone.copy()
    t[miss] = np.inf; cone[miss] = np.nan
    return SimpleNamespace(id=cid, trainer=trainer, cls="Trainer" if trainer == "mip" else TRAINERS[trainer][0], model=model, spec=spec, wts=wts,
                           batch=(ro, rd, t, cone, params, color, alpha), n=n, S=S, loss_name=loss_name, okw=LOSSES[loss_name][0], miss=miss,
                           **{k: kn[k] for k in ("perturb", "noise_std", "blur", "seed")})


def whole_restate(fx, dtype, masks, branch_masks, sigma_mask):
    """The fixture's step on GIVEN ReLU patterns: loss, pred = [color | alpha], grad (flat)."""
    ro, rd, t, cone, params, color, alpha = fx.batch
    ipe = fx.spec.pos_encoding == "ipe"
    z, noise = step_depths(t, fx.S + 1 if ipe else fx.S, fx.seed, fx.perturb, fx.miss), step_noise(fx.n, fx.S, fx.seed, fx.noise_std)
    kw = dict(blur_idx=fx.blur, dtype=dtype, masks=masks, sigma_mask=sigma_mask, noise=noise)
    if pgc.has_branches(fx.spec):
        val, c, a, g = tbo.step_gradients(fx.wts, fx.spec, ro, rd, z, params, np.nan_to_num(cone), color, alpha, fx.okw, branch_masks=branch_masks, **kw)
    else:
        val, c, a, g = tro.step_gradients(fx.wts, fx.spec, ro, rd, z, params, np.nan_to_num(cone), color, alpha, fx.okw, **kw)
    return SimpleNamespace(loss=val, pred=np.concatenate([c, a[:, None]], -1), grad=np.concatenate([np.asarray(x, np.float64).ravel() for x in g]))


def whole_own_patterns(fx):
    """(masks, branch_masks or None, sigma_mask) of a float32 forward pass of the restatement itself, every ray taken as a hit (the missed
    ones are filtered out of the step whatever their patterns)."""
    ro, rd, t, cone, params, _, _ = fx.batch
    ipe = fx.spec.pos_encoding == "ipe"
    z, noise = step_depths(t, fx.S + 1 if ipe else fx.S, fx.seed, fx.perturb), step_noise(fx.n, fx.S, fx.seed, fx.noise_std)
    if not ipe:
        masks, branch, sigma = tbo.own_masks(fx.wts, fx.spec, ro, rd, z, params, np.nan_to_num(cone), blur_idx=fx.blur, noise=noise)
        return masks, (branch or None), sigma
    t_ = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)                # tro.render's IPE half, with the patterns kept
    kept = []
    with torch.no_grad():
        p = t_(params)
        blur = p[:, fx.blur, None] * t_(np.nan_to_num(cone)).reshape(fx.n, 1)
        rest = torch.cat([p[:, :fx.blur], p[:, fx.blur + 1:]], -1).repeat_interleave(fx.S, 0)
        mean, cov = tcpu.cone_segment_gaussians(t_(ro), t_(rd), t_(z), blur)
        dirs = (t_(rd) / torch.linalg.norm(t_(rd), dim=-1, keepdim=True)).repeat_interleave(fx.S, 0)
        _, sg = tbo.mlp([t_(x) for x in fx.wts], fx.spec, tcpu.ipe(mean.reshape(-1, 3), cov.reshape(-1, 3), fx.spec.pos_freq), dirs, rest, kept=kept)
        sg = sg.reshape(fx.n, fx.S)
        sigma = (sg if noise is None else sg + t_(noise)).numpy() > 0
    return kept, None, sigma


def whole_fair(fx, report=print):
    """A whole-ray fixture's floors on the CPU, on the restatement's own float32 patterns: every layer's floor <= 5e-4, its largest gradient
    > 1e-6, the predictions' floor <= 1e-4 and the loss's <= 1e-5.  Returns the worst floor."""
    pat = whole_own_patterns(fx)
    want, f32 = whole_restate(fx, torch.float64, *pat), whole_restate(fx, torch.float32, *pat)
    rows = [(name, rel_linf(f32.grad[sl], want.grad[sl]), float(np.abs(want.grad[sl]).max())) for name, sl in layer_slices(fx.spec)]
    e_loss, e_pred = abs(f32.loss - want.loss) / abs(want.loss), rel_linf(f32.pred, want.pred)
    report(f"{fx.trainer} {fx.id}: loss {want.loss:.9g} float32 {e_loss:.2e}; pred float32 {e_pred:.2e}")
    for r in rows:
        report(f"  {r[0]:<24} floor {r[1]:.2e} max {r[2]:.3e}")
    assert all(r[2] > 1e-6 for r in rows), "a layer without a gradient worth the name: change the seed"
    assert all(r[1] <= 5e-4 for r in rows), ("a float32 floor above 5e-4: change the seed, not the bar", [r for r in rows if r[1] > 5e-4])
    assert e_pred <= 1e-4 and e_loss <= 1e-5, (e_pred, e_loss)
    if fx.miss.any():
        assert (want.pred[fx.miss] == 0).all() and 24 <= fx.miss.sum() <= 48 and fx.miss[[0, 1024, fx.n - 1]].all()
    return max(r[1] for r in rows)


# ---- parameter and ray gradients: `pgc.case_setup`'s form, (id, n_parameters, arch, freqs, family, knobs, (step seed, batch seed)) ------------
_GRAD_ARCH = dict(chain=None, flex=dict(width=98, depth=5, skips=[1, 3]))
# 1025 rays in rows of 256: five rows, the last of one ray; 2500 rays, a row per ray, the missed rays' rows and ray gradients exactly 0
GRAD_CASES = {b: [("rows_of_256", (1, 6), a, None, "carpet", dict(n=1025, S=3, rpr=256, loss_name="nerf_mse"), (11, 5)),
                  ("a_row_per_ray", (1, 6), a, None, "carpet", dict(n=2500, S=3, rpr=1, miss=MISS_2500, loss_name="nerf_mse"), (11, 5))] for b, a in _GRAD_ARCH.items()}
GRAD_IDS = [c[0] for c in GRAD_CASES["chain"]]


def grad_setup(backend, cid):
    """`tests.fused_grad_common.case_setup` (un-normalised rays_d) of a gradient case."""
    from tests import fused_grad_common as fgc
    model, spec, wts, (ro, rd, t, cone, rows, color, alpha), kn, seed = fgc.case_setup([c for c in GRAD_CASES[backend] if c[0] == cid][0])
    return model, spec, wts, (ro, rd, short_rays(t, kn["S"]), cone, rows, color, alpha), kn, seed


def grad_restate(spec, wts, batch, kn, seed, dtype, patterns):
    """(loss, dL/d rows, dL/d rays_o, dL/d rays_d) from the two yardsticks on the same patterns."""
    p = pgc.restate(spec, wts, batch, kn, seed, dtype, *patterns)
    r = igc.restate(spec, wts, batch, kn, seed, dtype, *patterns)
    return p[0], p[2], r[2], r[3]


def grad_rows(kn, n_rows):
    """(the parameter rows with a ray that hits, the rays that hit), or None for all."""
    miss = kn["miss"]
    if not miss.any():
        return None, None
    return np.array([(~miss[r * kn["rpr"]:(r + 1) * kn["rpr"]]).any() for r in range(n_rows)]), ~miss
