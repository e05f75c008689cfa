"""The distortion loss on the compositing weights on the GPU (`ntx_ray_distortion`, `nerf_tex_amd.loss.ray_distortion` / `distortion` /
`Distortion`; include/nerftex.h has the formula, tests/distortion_common.py the float64 reference, the float32 floors and the gate).  `-m gpu`.

1. Parity at the scan's edges.  2. Liveness.  3. Fixed order.  4. The op.  5. Through a trainer.  6. One instanced case.

Measured on an MI355X (error | float32 floor, rel-Linf over the batch; the gate is max(4 floors, 5e-7) capped at 1e-4): see the table in
DESIGN section 10.3 -- every case printed by `held` below."""

import numpy as np
import pytest
import torch

from tests import distortion_common as dc
from tests import weight_loss_common as wlc

pytestmark = pytest.mark.gpu
F = np.float32


def dev():
    return torch.device("cuda", 0)


def put(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev())


def run(w, z, widths=None, live=None, scale=None, loss=True, grad=True):
    """The raw entry on numpy inputs: (loss or None, grad or None) as numpy, each output buffer optional."""
    from nerf_tex_amd import _lib
    w, z, widths, live, scale = put(w), put(z), put(widths), put(live), put(scale)
    n, S = w.shape
    L = torch.full((n,), -7.0, device=dev()) if loss else None
    G = torch.full((n, S), -7.0, device=dev()) if grad else None
    p = lambda x: None if x is None else x.data_ptr()
    _lib.check(_lib.lib.ntx_ray_distortion(p(w), p(z), p(widths), p(live), p(scale), n, S, p(L), p(G), torch.cuda.current_stream(dev()).cuda_stream))
    torch.cuda.synchronize()
    return (None if L is None else L.cpu().numpy()), (None if G is None else G.cpu().numpy())


# ---- 1. parity at the scan's edges ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", dc.CASES, ids=dc.CASE_IDS)
def test_parity_at_the_scans_edges(case):
    """Every sample count around the chunk of 64 up to the limit, ray counts the four rays of a workgroup do not divide, both families of
    weights and the near = 500 rays: loss and gradient against the float64 pair sum at the gate; each output alone is the same bits."""
    w, z, widths, scale = dc.case_inputs(case)
    L, G = run(w, z, widths, None, scale)
    dc.held(L, G, dc.case_reference(case), dc.floor(case), case[0])
    L1, _ = run(w, z, widths, None, scale, grad=False)
    _, G1 = run(w, z, widths, None, scale, loss=False)
    assert np.array_equal(L1, L) and np.array_equal(G1, G)


# ---- 2. liveness ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", dc.LIVE_PATTERNS)
def test_liveness(pattern):
    """NaN in z, w and widths at every sample that is not live: exact zeros there, everything finite, parity on the rest."""
    w, z, widths, live, scale, mask = dc.live_case(pattern)
    L, G = run(w, z, widths, live, scale)
    assert np.isfinite(L).all() and np.isfinite(G).all() and (G[~mask] == 0).all() and not np.signbit(G[~mask]).any()
    want = dc.pairwise64(w, z, widths, live, scale)
    if not mask.any():
        assert not L.any() and not G.any()
        return
    f32 = dc.linear_form(w, z, widths, live, scale)
    dc.held(L, G, want, (dc.rel_linf(f32[0], want[0]), dc.rel_linf(f32[1], want[1])), pattern)
    assert (L[~mask.any(1)] == 0).all()


def test_liveness_at_the_sample_limit():
    """S = 4096, live exactly in [100, 1000) and [3000, 4090): 31 whole dead chunks between live ones (pass 2 keeps its carries across all of
    them), one in front and a short dead tail; NaN wherever a sample is not live."""
    w, z, widths, live, scale, mask = dc.live_limit_case()
    L, G = run(w, z, widths, live, scale)
    assert np.isfinite(L).all() and np.isfinite(G).all() and (G[~mask] == 0).all() and not np.signbit(G[~mask]).any()
    want, floors = dc.live_figures("limit")
    dc.held(L, G, want, floors, "S4096 two patches")


def test_a_missed_ray_is_exact_zeros_and_moves_no_other_bit():
    """Depths inf, weights 0 and ray_scale NaN on one ray of the batch: loss exactly 0, gradient row exactly 0, every other row the bits of the
    batch without that ray's values changed."""
    case = [c for c in dc.CASES if c[0] == "S65_N9_smooth"][0]
    w, z, widths, scale = (None if a is None else a.copy() for a in dc.case_inputs(case))
    L0, G0 = run(w, z, widths, None, scale)
    k = 4
    w[k], z[k], scale[k] = 0.0, np.inf, np.nan
    L, G = run(w, z, widths, None, scale)
    others = np.arange(len(w)) != k
    assert L[k] == 0 and not G[k].any() and np.isfinite(L).all() and np.isfinite(G).all()
    assert np.array_equal(L[others], L0[others]) and np.array_equal(G[others], G0[others]) and np.abs(G0[k]).max() > 0


def test_a_ray_that_is_finite_only_in_part_stays_finite():
    """Without `widths` and `live`, depths that stop being finite halfway along a ray (and at its last sample on another): the samples
    behind are not live, the default width next to them is selected to 0, and the rest meets the gate."""
    case = [c for c in dc.CASES if c[0] == "S65_N9_smooth"][0]
    w, z, _, scale = (None if a is None else a.copy() for a in dc.case_inputs(case))
    z[2, 40:], z[5, -1], z[7, :3] = np.inf, np.inf, np.nan
    L, G = run(w, z, None, None, scale)
    mask = np.isfinite(z)
    assert np.isfinite(L).all() and np.isfinite(G).all() and (G[~mask] == 0).all()
    want, f32 = dc.pairwise64(w, z, None, None, scale), dc.linear_form(w, z, None, None, scale)
    dc.held(L, G, want, (dc.rel_linf(f32[0], want[0]), dc.rel_linf(f32[1], want[1])), "finite in part")


def test_distortion_counts_zero_on_a_ray_without_a_span():
    """`Distortion(normalize=True)`: a ray whose first and last depth are equal (and one at infinity) has no span to divide by and counts 0;
    value and gradient stay finite, and the other rays are what they are without those two."""
    from nerf_tex_amd.loss import Distortion
    case = [c for c in dc.CASES if c[0] == "S65_N9_smooth"][0]
    w, z, _, _ = (None if a is None else a.copy() for a in dc.case_inputs(case))
    z[1], z[3] = z[1, 0], np.inf
    loss = Distortion(lambda color_true, alpha_true, color_pred, alpha_pred: color_pred.sum() * 0.0, weight=1.0)
    wt = put(w).requires_grad_(True)
    val = loss(color_true=None, alpha_true=None, color_pred=torch.zeros(1, device=dev()), alpha_pred=None, weights=wt, z_vals=put(z))
    (g,) = torch.autograd.grad(val, wt)
    val = val.detach()
    keep = np.ones(len(w), bool); keep[[1, 3]] = False
    span = (z[keep, -1] - z[keep, 0]).astype(np.float64)
    want = dc.pairwise64(w[keep], z[keep], None, None, 1.0 / span)
    assert np.isfinite(float(val)) and torch.isfinite(g).all() and not g[1].any() and not g[3].any()
    assert abs(float(val) - want[0].sum() / len(w)) <= dc.CAP * want[0].sum() / len(w)                          # (the house bar: a float32 mean over the kernel's figures)
    assert dc.rel_linf(g.cpu().numpy()[keep] * len(w), want[1]) <= dc.CAP


# ---- 3. fixed order ------------------------------------------------------------------------------------------------------------------------
def test_fixed_order():
    """Two runs are the same bits; row k of a 9-ray call is the 1-ray call on row k; a ray_scale of ones is no ray_scale."""
    case = [c for c in dc.CASES if c[0] == "S255_N9_smooth"][0]
    w, z, widths, scale = dc.case_inputs(case)
    L, G = run(w, z, widths, None, scale)
    L2, G2 = run(w, z, widths, None, scale)
    assert np.array_equal(L, L2) and np.array_equal(G, G2) and np.abs(G).max() > 0
    for k in range(len(w)):
        Lk, Gk = run(w[k:k + 1], z[k:k + 1], widths, None, scale[k:k + 1])
        assert np.array_equal(Lk, L[k:k + 1]) and np.array_equal(Gk, G[k:k + 1]), k
    Ln, Gn = run(w, z, widths, None, None)
    L1, G1 = run(w, z, widths, None, np.ones(len(w), F))
    assert np.array_equal(Ln, L1) and np.array_equal(Gn, G1) and not np.array_equal(Ln, L)


@pytest.fixture(scope="module")
def base257():
    """The 257 base rows through the kernel once, without a ray_scale: what every larger call has to repeat."""
    w, z, dead, want, floors = dc.large_base()
    L, G = run(w, z)
    assert not L[dead].any() and not G[dead].any() and np.isfinite(L).all() and np.isfinite(G).all() and (np.abs(G[~dead]).max(1) > 0).all()
    dc.held(L, G, want, floors, "the 257 base rows")
    return L, G


@pytest.mark.parametrize("n", dc.LARGE_N)
def test_past_the_capped_grid(n, base257):
    """8192 rays (the capped grid exactly), 8193 (one wave takes a second ray) and 16 389 (three passes for five waves), row k = base row
    k mod 257, three base rows replaced by a missed ray, a ray finite in its first 30 samples and a ray of NaN weights: without a ray_scale
    every row is bit for bit the 257-ray call's, the dead rows exact zeros; under a per-ray ray_scale (NaN on the dead rows) the cycled
    float64 reference times that scale holds the call at the gate."""
    w, z, dead, _, floors = dc.large_base()
    W, Z, D = dc.cycled(w, n), dc.cycled(z, n), dc.cycled(dead, n)
    L, G = run(W, Z)
    assert np.array_equal(L, dc.cycled(base257[0], n)) and np.array_equal(G, dc.cycled(base257[1], n))
    assert not L[D].any() and not G[D].any() and not np.signbit(G[D]).any() and D.sum() >= 2 * (n // 257)
    scale = dc.large_scale(n, dead)
    L, G = run(W, Z, scale=scale)
    assert np.isfinite(L).all() and np.isfinite(G).all() and not L[D].any() and not G[D].any()
    dc.held(L, G, dc.large_reference(n, scale), floors, f"N{n} cycled, ray_scale")


def test_each_output_alone_past_the_capped_grid(base257):
    """N = 8193: the loss alone and the gradient alone are the bits of the call that writes both."""
    n = dc.LARGE_N[1]
    w, z, _, _, _ = dc.large_base()
    W, Z = dc.cycled(w, n), dc.cycled(z, n)
    L1, none = run(W, Z, grad=False)
    nothing, G1 = run(W, Z, loss=False)
    assert none is None and nothing is None
    assert np.array_equal(L1, dc.cycled(base257[0], n)) and np.array_equal(G1, dc.cycled(base257[1], n))


# ---- 4. the op -----------------------------------------------------------------------------------------------------------------------------
def test_the_op_under_autograd_and_no_second_order():
    """`distortion` under torch.autograd.grad with a random per-ray cotangent against float64 at the gate; `ray_distortion` is the same
    numbers; a double backward raises."""
    from nerf_tex_amd.loss import distortion, ray_distortion
    case = [c for c in dc.CASES if c[0] == "S129_N3_peaky_widths"][0]
    w, z, widths, scale = dc.case_inputs(case)
    cot = np.random.default_rng(8).normal(size=len(w)).astype(F)
    wt = put(w).requires_grad_(True)
    val = distortion(wt, put(z), widths=put(widths), ray_scale=put(scale))
    assert val.shape == (len(w),) and val.requires_grad
    (g,) = torch.autograd.grad(val, wt, put(cot))
    want = dc.case_reference(case)
    dc.held(val.detach().cpu().numpy(), g.cpu().numpy(), (want[0], want[1] * cot[:, None].astype(np.float64)), dc.floor(case), "the op")
    L, G = ray_distortion(put(w), z, widths=widths, ray_scale=scale, with_grad=True)                         # (numpy depths are taken too)
    assert torch.equal(L, val.detach()) and torch.equal(G * put(cot)[:, None], g)
    assert torch.equal(ray_distortion(put(w), put(z), widths=put(widths), ray_scale=put(scale)), L)
    wt2 = put(w).requires_grad_(True)
    (g1,) = torch.autograd.grad(distortion(wt2, put(z)).sum(), wt2, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


def test_the_op_on_a_side_stream_gives_the_default_streams_bits():
    """The launch goes to the current stream: on a non-blocking side stream, behind a delay and a late copy of the inputs into buffers that
    hold another batch, the results are the default stream's bits (the late-inputs trap of tests/stream_common.py)."""
    from nerf_tex_amd.loss import ray_distortion
    from tests import stream_common as sc
    case = [c for c in dc.CASES if c[0] == "S65_N257_peaky"][0]
    other = [c for c in dc.CASES if c[0] == "S64_N257_smooth"][0]
    w, z, _, scale = dc.case_inputs(case)
    L0, G0 = ray_distortion(put(w), put(z), ray_scale=put(scale), with_grad=True)
    torch.cuda.synchronize()
    wo, zo, _, so = dc.case_inputs(other)
    bufs = [put(np.pad(wo, ((0, 0), (0, 1)))), put(np.pad(zo, ((0, 0), (0, 1)), constant_values=9.0)), put(so)]   # (another valid batch, 257 x 65)
    staging = [put(w), put(z), put(scale)]
    s, armed = sc.side_stream(), torch.cuda.Event()
    sc.delay(sc.MIN_DELAY_MS, s)
    with torch.cuda.stream(s):
        armed.record(s)
        for b, src in zip(bufs, staging):
            b.copy_(src)
        L, G = ray_distortion(bufs[0], bufs[1], ray_scale=bufs[2], with_grad=True)
    still_blocked = not armed.query()
    s.synchronize()
    assert still_blocked, "the call waited for its stream (or the delay was too short)"
    assert torch.equal(L, L0) and torch.equal(G, G0) and float(G0.abs().max()) > 0


# ---- 5. through a trainer ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in wlc.E2E_CASES if c[0] in ("chain", "flex")], ids=["chain", "flex"])
def test_through_a_trainer(case):
    """One `gradients_step` under `Distortion(mse, weight=0.1)` beside the same step under a callable that states the same loss with the
    pair sum in torch (the parent's own path): loss and the trainer's gradient agree within 1e-4 rel-Linf, and the gradient is not the
    plain-mse step's."""
    from nerf_tex_amd import train
    from nerf_tex_amd.loss import Distortion, NerfLoss, as_callable
    model, spec, wts, batch, kn, seed, _, _ = wlc.e2e_setup(case)
    ro, rd, t, cone, rows, color, alpha = batch
    tr = getattr(train, case[1])(model, max_rays=kn["n"], n_samples=kn["S"], perturb=kn["perturb"])
    mse = as_callable(NerfLoss())

    def step(loss):
        val, _, _ = tr.gradients_step(ro, rd, t, rows, cone, color, alpha, loss, seed=seed, rays_per_param_row=kn["rpr"])
        torch.cuda.synchronize()
        return float(val.item()), tr.gradients().copy()
    got, want, plain = step(Distortion(NerfLoss(), weight=0.1)), step(dc.pairwise_loss(mse, 0.1)), step(mse)
    e_val, e_grad = abs(got[0] - want[0]) / abs(want[0]), dc.rel_linf(got[1], want[1])
    moved = dc.rel_linf(plain[1], want[1])
    print(f"| {case[0]} | loss {got[0]:.9g} pair sum {want[0]:.9g} mse alone {plain[0]:.9g} | rel {e_val:.2e} | gradient {e_grad:.2e} | the term moves it by {moved:.2e} |")
    assert e_val <= 1e-4 and e_grad <= 1e-4 and np.isfinite(got[1]).all()
    assert got[0] > plain[0] and moved > 10 * 1e-4, "the distortion term did not arrive (it has to move the gradient by more than ten bars)"


# ---- 6. one instanced case -----------------------------------------------------------------------------------------------------------------
def test_an_instanced_step():
    """`DifferentiableInstanceRender(weights=True)` + `distortion(w, t, widths=dists, live=dists)` on the instancer's buffers:
    `total.backward()` runs, the trainer's gradient is finite and equals the pair-sum statement's within 1e-4."""
    from nerf_tex_amd.autograd import DifferentiableInstanceRender
    from nerf_tex_amd.loss import distortion
    from nerf_tex_amd.train import FlexTrainer
    from tests import fused_instanced_common as fic
    model, spec, wts, bufs, hit, cone, kn, okw = wlc.instanced_setup("flex", "some")
    n, S = bufs[3].shape
    tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=False)
    k = fic.fkw(kn)
    render = DifferentiableInstanceRender(tr, k["patch_scale"], k["density_scale"], k["density_reweighting"], weights=True)
    h8 = np.asarray(hit).astype(np.uint8)
    tt, dists = put(np.asarray(bufs[2], F)), put(np.asarray(bufs[3], F))
    z_ref = torch.where(dists > 0, tt, torch.full_like(tt, float("inf")))                                   # the op's liveness, for the pair sum

    def step(term):
        c, a, w = render(bufs, cone, hit=h8, composite_bkgd=k["composite_bkgd"], bkgd_color=wlc.BKGD)
        total = ((c - 0.5) ** 2).mean() + 10.0 * term(w).mean()                              # (the rays are 0.14 long: a term one can see)
        total.backward()
        torch.cuda.synchronize()
        return float(total.item()), tr.gradients().copy(), w.detach()
    got = step(lambda w: distortion(w, tt, widths=dists, live=dists))
    want = step(lambda w: dc.pairwise_torch(w, z_ref, widths=dists))
    plain = step(lambda w: torch.zeros(n, device=dev()) * w.sum())
    e_val, e_grad, moved = abs(got[0] - want[0]) / abs(want[0]), dc.rel_linf(got[1], want[1]), dc.rel_linf(plain[1], want[1])
    print(f"| instanced flex | total {got[0]:.9g} pair sum {want[0]:.9g} | rel {e_val:.2e} | gradient {e_grad:.2e} | the term moves it by {moved:.2e} |")
    assert torch.equal(got[2], want[2]) and float(got[2].max()) > 1e-3
    assert np.isfinite(got[1]).all() and e_val <= 1e-4 and e_grad <= 1e-4 and moved > 10 * 1e-4
