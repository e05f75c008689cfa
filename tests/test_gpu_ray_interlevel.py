"""The interlevel loss on the GPU (`ntx_ray_interlevel`, `nerf_tex_amd.loss.ray_interlevel` / `interlevel`, `nerf_tex_amd.train.ProposalTrainer`;
include/nerftex.h has the formula, tests/interlevel_common.py the float64 reference, the float32 floors and the gate).  `-m gpu`.

1. Parity at the edges.  2. Exact zeros and equalities.  3. Bit reproducibility.  4. Refusals.  5. The op.  6. Through the trainers.

Measured on an MI355X (error | float32 floor, rel-Linf over the batch; the gate is max(4 floors, 5e-7) capped at 1e-4): see the table in
DESIGN section 10.4 -- every case printed by `held` below."""

import numpy as np
import pytest
import torch

from tests import distortion_common as dc
from tests import interlevel_common as ic

pytestmark = pytest.mark.gpu
F = np.float32


def dev():
    return torch.device("cuda", 0)


def put(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev())


def run(w, z, wp, zp, scale=None, outs=(True, True, True), eps=ic.EPS):
    """The raw entry on numpy inputs, on the current stream: [loss, grad_prop, grad_fine] as numpy (None where `outs` leaves the buffer out)."""
    from nerf_tex_amd import _lib
    w, z, wp, zp, scale = put(w), put(z), put(wp), put(zp), put(scale)
    (n, S), Sp = w.shape, wp.shape[1]
    bufs = [torch.full(shape, -7.0, device=dev()) if on else None for shape, on in zip(((n,), (n, Sp), (n, S)), outs)]
    p = lambda x: None if x is None else x.data_ptr()
    torch.cuda.synchronize()
    _lib.check(_lib.lib.ntx_ray_interlevel(p(w), p(z), S, p(wp), p(zp), Sp, p(scale), eps, n, *(p(b) for b in bufs), torch.cuda.current_stream(dev()).cuda_stream))
    torch.cuda.synchronize()
    return [None if b is None else b.cpu().numpy() for b in bufs]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 1. parity at the edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ic.CASES, ids=ic.CASE_IDS)
def test_parity_at_the_edges(case):
    """Sample counts from one to the limit on both sides and around the chunk of 64, more proposal than fine samples, ray counts the four rays of
    a workgroup do not divide, both families, near = 500, and depths without ties: all three outputs against float64 at the gate."""
    w, z, wp, zp, scale = ic.case_inputs(case)
    got = run(w, z, wp, zp, scale)
    ic.held(got, ic.case_reference(case), ic.floor(case), case[0])


# ---- 2. exact zeros and equalities ---------------------------------------------------------------------------------------------------------
def test_a_proposal_that_covers_twice_the_fine_weights_costs_nothing():
    """Every fine depth also a proposal depth (a sorted subset), the proposal weight of each interval twice the fine weight it covers: loss and
    both gradients exactly 0."""
    rng = np.random.default_rng(4)
    n, Sp, S = 7, 96, 40
    _, zp = ic.ray_batch(n, Sp, "smooth", seed=41)
    keep = np.stack([np.sort(np.concatenate([[0], 1 + rng.permutation(Sp - 1)[:S - 1]])) for _ in range(n)])
    z = np.take_along_axis(zp, keep, 1)
    w = rng.uniform(0.0, 0.02, size=(n, S)).astype(F)
    wp = np.zeros((n, Sp), F)
    for r in range(n):                                   # fine interval i covers the proposal intervals keep[i] .. keep[i+1] - 1: its first one pays
        wp[r, keep[r]] = 2 * w[r]
    L, gp, gf = run(w, z, wp, zp, None)
    assert not L.any() and not gp.any() and not gf.any()
    want = ic.reference(w, z, wp, zp)
    assert not want[0].any() and not want[1].any() and not want[2].any()


def test_identical_histograms_cost_nothing():
    w, z, _, _, scale = ic.case_inputs(ic.by_id("P64_S65_N257_smooth"))
    L, gp, gf = run(w, z, w, z, scale)
    assert not L.any() and not gp.any() and not gf.any() and np.abs(w).max() > 0


def test_rays_that_are_not_live_are_exact_zeros_and_move_no_other_bit():
    """Depths inf on three rays of a batch -- on the fine set, on the proposal set, on both -- with NaN in their ray_scale and NaN in their weights:
    exact zeros on those rays, the other rays the bits of the batch before."""
    w, z, wp, zp, scale = (a.copy() for a in ic.case_inputs(ic.by_id("P65_S129_N9_peaky")))
    before = run(w, z, wp, zp, scale)
    dead = [1, 4, 8]
    z[1], zp[4], z[8], zp[8] = np.inf, np.inf, np.inf, np.inf
    z[1, :5] = 1.0                                                              # (one depth that is not finite is enough)
    w[dead], wp[dead], scale[dead] = np.nan, np.nan, np.nan
    got = run(w, z, wp, zp, scale)
    others = np.setdiff1d(np.arange(len(w)), dead)
    for a, b in zip(got, before):
        assert np.isfinite(a).all() and not a[dead].any() and np.array_equal(a[others], b[others]) and np.abs(b[dead]).max() > 0


def test_a_single_sample_on_either_side():
    """S == 1: the interval has no width (b_0 = a_0) and overlaps nothing.  One fine sample: bound 0, q = w / (w + eps).  One proposal sample:
    its gradient is exactly 0 and every fine sample is unbounded."""
    rng = np.random.default_rng(9)
    n = 6
    wp, zp = ic.ray_batch(n, 33, "smooth", seed=3)
    w1, z1 = rng.uniform(0.1, 0.9, size=(n, 1)).astype(F), zp[:, 7:8].copy()
    L, gp, gf = run(w1, z1, wp, zp)
    q = w1 / (w1 + F(ic.EPS))
    assert np.array_equal(L, (w1 * q)[:, 0]) and not gp.any() and np.array_equal(gf, q * (F(2) - q))
    w, z = ic.fine_set(zp, 50, "smooth", "merged", 10)
    L, gp, gf = run(w, z, wp[:, 7:8].copy(), zp[:, 7:8].copy())
    want, f32 = ic.reference(w, z, wp[:, 7:8], zp[:, 7:8]), ic.reference(w, z, wp[:, 7:8], zp[:, 7:8], dtype=F)
    assert not gp.any() and not want[1].any() and want[3].max() >= 0.5
    ic.held((L, None, gf), want, tuple(ic.rel_linf(f32[k], want[k]) for k in range(3)), "one proposal sample")


# ---- 3. bit reproducibility ----------------------------------------------------------------------------------------------------------------
def test_fixed_order():
    """The same bits twice; row k of the batch alone and inside a batch of another size; with each subset of the outputs left out; a ray_scale of
    ones against none; on a non-default stream."""
    w, z, wp, zp, scale = ic.case_inputs(ic.by_id("P128_S256_N7_peaky"))
    got = run(w, z, wp, zp, scale)
    assert same(run(w, z, wp, zp, scale), got) and all(np.abs(g).max() > 0 for g in got)
    for k in range(len(w)):
        one = run(w[k:k + 1], z[k:k + 1], wp[k:k + 1], zp[k:k + 1], scale[k:k + 1])
        assert same(one, [g[k:k + 1] for g in got]), k
    rep = lambda a: np.concatenate([a[2:5]] * 3 + [a[:1]])                       # 10 rays: rows 2..4 three times over, then row 0
    more = run(*(rep(a) for a in (w, z, wp, zp, scale)))
    assert same(more, [rep(g) for g in got])
    for outs in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)]:
        part = run(w, z, wp, zp, scale, outs=outs)
        assert all((p is None) == (not on) and (p is None or np.array_equal(p, g)) for p, g, on in zip(part, got, outs)), outs
    none, ones = run(w, z, wp, zp, None), run(w, z, wp, zp, np.ones(len(w), F))
    assert same(none, ones) and not np.array_equal(none[0], got[0])
    s = torch.cuda.Stream(device=dev())
    with torch.cuda.stream(s):
        side = run(w, z, wp, zp, scale)
    assert same(side, got)


@pytest.fixture(scope="module")
def base257():
    """The 257 base rows through the kernel once, without a ray_scale: what every larger call has to repeat."""
    w, z, wp, zp, dead, want, floors = ic.large_base()
    got = run(w, z, wp, zp)
    assert all(np.isfinite(g).all() and not g[dead].any() for g in got) and (got[0][~dead] > 0).all()
    ic.held(got, want, floors, "the 257 base rows")
    return got


@pytest.mark.parametrize("n", dc.LARGE_N)
def test_past_the_capped_grid(n, base257):
    """8192 rays (the capped grid exactly), 8193 (one wave takes a second ray and writes its `q_row` again) and 16 389 (three passes for five
    waves), row k = base row k mod 257; one base row has an inf in its fine depths alone, one a NaN in its proposal depths alone and NaN
    weights (the `continue` that skips the closing fence), so a wave that meets a dead ray goes on to a live one.  Without a ray_scale every
    row is bit for bit the 257-ray call's, the dead rows exact zeros; under a per-ray ray_scale (NaN on the dead rows) the cycled float64
    reference times that scale holds all three outputs at the gate."""
    w, z, wp, zp, dead, _, floors = ic.large_base()
    big = [dc.cycled(a, n) for a in (w, z, wp, zp)]
    D = dc.cycled(dead, n)
    got = run(*big)
    assert same(got, [dc.cycled(g, n) for g in base257])
    assert all(not g[D].any() and not np.signbit(g[D]).any() for g in got) and D.sum() >= 2 * (n // 257)
    scale = dc.large_scale(n, dead)
    got = run(*big, scale)
    assert all(np.isfinite(g).all() and not g[D].any() for g in got)
    ic.held(got, ic.large_reference(n, scale), floors, f"N{n} cycled, ray_scale")


def test_each_output_alone_past_the_capped_grid(base257):
    """N = 8193: each of the three outputs alone is the bits of the call that writes all of them."""
    n = dc.LARGE_N[1]
    big = [dc.cycled(a, n) for a in ic.large_base()[:4]]
    for k, outs in enumerate([(1, 0, 0), (0, 1, 0), (0, 0, 1)]):
        part = run(*big, outs=outs)
        assert [p is None for p in part] == [not on for on in outs] and np.array_equal(part[k], dc.cycled(base257[k], n)), outs


def test_the_op_on_a_side_stream_gives_the_default_streams_bits():
    """The launch goes to the current stream: on a non-blocking side stream, behind a delay and a late copy of the inputs into buffers that
    hold another batch, the results are the default stream's bits (the late-inputs trap of tests/stream_common.py)."""
    from nerf_tex_amd.loss import ray_interlevel
    from tests import stream_common as sc
    w, z, wp, zp, scale = ic.case_inputs(ic.by_id("P64_S65_N257_smooth"))
    want = ray_interlevel(put(w), put(z), put(wp), put(zp), ray_scale=put(scale), with_grad=True)
    torch.cuda.synchronize()
    staging = [put(a) for a in (w, z, wp, zp, scale)]
    bufs = [torch.flip(a, (0,)).contiguous() for a in staging]                   # (another valid batch: the rays in reverse)
    s, armed = sc.side_stream(), torch.cuda.Event()
    sc.delay(sc.MIN_DELAY_MS, s)
    with torch.cuda.stream(s):
        armed.record(s)
        for b, src in zip(bufs, staging):
            b.copy_(src)
        got = ray_interlevel(bufs[0], bufs[1], bufs[2], bufs[3], ray_scale=bufs[4], with_grad=True)
    still_blocked = not armed.query()
    s.synchronize()
    assert still_blocked, "the call waited for its stream (or the delay was too short)"
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and float(want[1].abs().max()) > 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_a_refused_call_writes_nothing():
    """Each NTX_E_INVALID case with at least one output pointer given leaves the sentinel-filled outputs untouched; n_rays = 0 is NTX_OK."""
    from nerf_tex_amd import _lib
    w, z, wp, zp, scale = (put(a) for a in ic.case_inputs(ic.by_id("P8_S16_N9_smooth")))
    (n, S), Sp = w.shape, wp.shape[1]
    outs = [torch.full((n,), -7.0, device=dev()), torch.full((n, Sp), -7.0, device=dev()), torch.full((n, S), -7.0, device=dev())]
    p = lambda x: None if x is None else x.data_ptr()
    L, gp, gf = (p(o) for o in outs)
    W, Z, WP, ZP, RS, eps = p(w), p(z), p(wp), p(zp), p(scale), ic.EPS
    bad = {
        "weights NULL": (None, Z, S, WP, ZP, Sp, RS, eps, n, L, gp, gf),
        "z_vals NULL": (W, None, S, WP, ZP, Sp, RS, eps, n, L, None, gf),
        "weights_prop NULL": (W, Z, S, None, ZP, Sp, RS, eps, n, L, gp, None),
        "z_prop NULL": (W, Z, S, WP, None, Sp, RS, eps, n, None, gp, gf),
        "S = 0": (W, Z, 0, WP, ZP, Sp, RS, eps, n, L, gp, gf),
        "S = 4097": (W, Z, 4097, WP, ZP, Sp, RS, eps, n, L, gp, gf),
        "S_p = 0": (W, Z, S, WP, ZP, 0, RS, eps, n, L, gp, gf),
        "S_p = 4097": (W, Z, S, WP, ZP, 4097, RS, eps, n, L, gp, gf),
        "n_rays < 0": (W, Z, S, WP, ZP, Sp, RS, eps, -1, L, gp, gf),
        "n_rays = 2^31": (W, Z, S, WP, ZP, Sp, RS, eps, 2 ** 31, L, gp, gf),
        "eps = 0": (W, Z, S, WP, ZP, Sp, RS, 0.0, n, L, gp, gf),
        "eps < 0": (W, Z, S, WP, ZP, Sp, RS, -1.0, n, L, gp, gf),
        "eps inf": (W, Z, S, WP, ZP, Sp, RS, float("inf"), n, L, gp, gf),
        "eps nan": (W, Z, S, WP, ZP, Sp, RS, float("nan"), n, L, gp, gf),
    }
    for what, args in bad.items():
        assert _lib.lib.ntx_ray_interlevel(*args, None) == _lib.NTX_E_INVALID, what
    assert _lib.lib.ntx_ray_interlevel(W, Z, S, WP, ZP, Sp, RS, eps, n, None, None, None, None) == _lib.NTX_E_INVALID
    assert _lib.lib.ntx_ray_interlevel(W, Z, S, WP, ZP, Sp, RS, eps, 0, L, gp, gf, None) == _lib.NTX_OK
    torch.cuda.synchronize()
    assert all(bool((o == -7.0).all()) for o in outs)


# ---- 5. the op -----------------------------------------------------------------------------------------------------------------------------
def test_the_op_under_autograd_and_no_second_order():
    """`interlevel` under torch.autograd.grad with a random per-ray cotangent against torch float64 autograd of the dense statement, at the gate;
    the detached-fine use gives the proposal's gradient alone; `ray_interlevel` is the same numbers; a double backward raises."""
    from nerf_tex_amd.loss import interlevel, ray_interlevel
    case = ic.by_id("P24_S40_N5_smooth")
    w, z, wp, zp, scale = ic.case_inputs(case)
    cot = np.random.default_rng(8).normal(size=len(w)).astype(F)
    t64 = lambda a, g=False: torch.tensor(a.astype(np.float64), requires_grad=g)
    w64, wp64 = t64(w, True), t64(wp, True)
    val64 = ic.dense_torch(w64, t64(z), wp64, t64(zp)) * t64(scale)
    g64 = torch.autograd.grad(val64, (wp64, w64), t64(cot))
    want = (val64.detach().numpy(), g64[0].numpy(), g64[1].numpy())
    wt, wpt = put(w).requires_grad_(True), put(wp).requires_grad_(True)
    val = interlevel(wt, put(z), wpt, put(zp), ray_scale=put(scale))
    assert val.shape == (len(w),) and val.requires_grad
    g_prop, g_fine = torch.autograd.grad(val, (wpt, wt), put(cot))
    ic.held((val.detach().cpu().numpy(), g_prop.cpu().numpy(), g_fine.cpu().numpy()), want, ic.floor(case), "the op")
    L, GP, GF = ray_interlevel(put(w), z, put(wp), zp, ray_scale=scale, with_grad=True)                        # (numpy depths are taken too)
    assert torch.equal(L, val.detach()) and torch.equal(GP * put(cot)[:, None], g_prop) and torch.equal(GF * put(cot)[:, None], g_fine)
    assert torch.equal(ray_interlevel(put(w), put(z), put(wp), put(zp), ray_scale=put(scale)), L)
    wp2 = put(wp).requires_grad_(True)                                                                       # the mip-NeRF 360 use
    val2 = interlevel(wt.detach(), put(z), wp2, put(zp), ray_scale=put(scale))
    (g2,) = torch.autograd.grad(val2, wp2, put(cot))
    assert torch.equal(g2, g_prop) and torch.equal(val2.detach(), L)
    wp3 = put(wp).requires_grad_(True)
    (g1,) = torch.autograd.grad(interlevel(put(w), put(z), wp3, put(zp)).sum(), wp3, create_graph=True)
    with pytest.raises(RuntimeError):
        g1.sum().backward()


# ---- 6. through the trainers ---------------------------------------------------------------------------------------------------------------
N_RAYS, S_PROP, N_IMP, LAMBDA = 24, 8, 8, 0.5
SMALL = dict(width=64, depth=3, skips=[1])
OTHER = dict(width=128, depth=4, skips=[2])


def pair(fine_arch=SMALL):
    from tests.common import make_model
    prop = make_model((0, 0), kind="Nerf", seed=0, dense_media=True, arch=SMALL)
    fine = make_model((0, 0), kind="Nerf", seed=1, dense_media=True, arch=fine_arch)
    return prop[0], fine[0], fine[1]


def the_batch(spec):
    from tests.train_flex_common import flex_batch
    ro, rd, t, cone, params, color, alpha = flex_batch(14, N_RAYS, S_PROP, spec, "carpet")
    t = t.copy()
    t[5] = np.inf                                                                 # one ray misses its proxy: it counts in both means
    u = np.random.default_rng(2).uniform(size=(N_RAYS, N_IMP)).astype(F)
    return (ro, rd, t, params, cone, color, alpha), u


def charbonnier(color_true, alpha_true, color_pred, alpha_pred):
    return torch.sqrt((color_pred - color_true) ** 2 + 1e-3).mean() + 0.5 * ((alpha_pred - alpha_true) ** 2).mean()


def colour_slices(model):
    """(name, slice) of the layers only the colour depends on, in the order of the trainer's flat gradient (kernel, then bias, per layer)."""
    out, p = [], 0
    for name, i, o in model.layer_table():
        if name.startswith("color") or name == "feature":
            out.append((name, slice(p, p + i * o + o)))
        p += i * o + o
    return out, p


@pytest.mark.parametrize("setting", [("descriptor", True, SMALL), ("descriptor", False, SMALL), ("callable", True, SMALL), ("callable", False, OTHER),
                                     ("descriptor", True, OTHER)], ids=["descriptor-perturb", "descriptor-fixed", "callable-perturb", "callable-fixed-other", "descriptor-perturb-other"])
def test_one_step_is_its_pieces_by_hand(setting):
    """The proposal network's gradient is bit for bit what `forward(return_weights)` -> `ray_interlevel` -> `backward(d_weights=)` leaves, its
    colour layers take exact zeros; the fine network's gradient is bit for bit a plain trainer's step with z_vals = the merged depths under the
    same loss; the value is the sum of the two terms."""
    from nerf_tex_amd.loss import NerfLoss, ray_interlevel
    from nerf_tex_amd.train import ProposalTrainer, trainer_for
    kind, perturb, arch = setting
    prop, fine, spec = pair(arch)
    args, u = the_batch(spec)
    loss = NerfLoss() if kind == "descriptor" else charbonnier
    seed, S, NI = 5, S_PROP, N_IMP
    pt = ProposalTrainer(prop, fine, max_rays=N_RAYS, n_samples=S, n_importance=NI, perturb=perturb, interlevel_weight=LAMBDA)
    assert len(pt.trainers) == 2 and not pt.shared
    val, cf, af, cp, ap = pt.gradients_step(*args, loss, seed=seed, u=u)
    torch.cuda.synchronize()
    g_prop, g_fine, z_all = pt.coarse.gradients().copy(), pt.fine.gradients().copy(), pt.last_z
    ro, rd, t, params, cone, color, alpha = args
    # the proposal's side by hand
    hp = trainer_for(prop, max_rays=N_RAYS, n_samples=S, perturb=perturb)
    hf = trainer_for(fine, max_rays=N_RAYS, n_samples=S + NI, perturb=perturb)
    z_prop = hp._sample_depths(put(t), seed, S)
    c_p, a_p, w_p = hp.forward(ro, rd, t, params, cone, seed=seed, z_vals=z_prop, n_samples=S, return_weights=True)
    _, _, w_f = hf.forward(ro, rd, t, params, cone, seed=seed, z_vals=z_all, n_samples=S + NI, return_weights=True)
    w_f = w_f.clone()
    scale = torch.full((N_RAYS,), LAMBDA / N_RAYS, device=dev())
    per_ray, d_prop, _ = ray_interlevel(w_f, z_all, w_p, z_prop, ray_scale=scale, with_grad=True)
    hp.backward(torch.zeros_like(c_p), None, d_weights=d_prop)
    val_f, c_f, a_f = hf.gradients_step(ro, rd, t, params, cone, color, alpha, loss, seed=seed, z_vals=z_all, n_samples=S + NI)
    torch.cuda.synchronize()
    assert np.array_equal(hp.gradients(), g_prop) and np.isfinite(g_prop).all() and np.abs(g_prop).max() > 0
    assert np.array_equal(hf.gradients(), g_fine) and np.isfinite(g_fine).all() and np.abs(g_fine).max() > 0
    assert torch.equal(c_p, cp) and torch.equal(a_p, ap) and torch.equal(c_f, cf) and torch.equal(a_f, af)
    assert torch.equal(pt.last_interlevel, per_ray.sum().reshape(1)) and torch.equal(val, val_f + pt.last_interlevel)
    assert float(pt.last_interlevel) > 0 and float(per_ray[5]) == 0 and not d_prop[5].any()
    layers, total = colour_slices(prop)
    assert total == g_prop.size and len(layers) >= 3 and all(not g_prop[sl].any() for _, sl in layers), [(nm, float(np.abs(g_prop[sl]).max())) for nm, sl in layers]
    # the merged depths hold the proposal's
    assert all(np.isin(z_prop[r].cpu().numpy(), z_all[r].cpu().numpy()).all() for r in range(N_RAYS) if r != 5)


def test_what_the_pair_refuses():
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import ProposalTrainer
    from tests.common import make_model
    prop, fine, _ = pair()
    with pytest.raises(ValueError):
        ProposalTrainer(prop, None, max_rays=8, n_samples=8, n_importance=8)
    with pytest.raises(ValueError):
        ProposalTrainer(prop, prop, max_rays=8, n_samples=8, n_importance=8)
    ipe = make_model((1, 3), kind="IPE")[0]
    with pytest.raises(_lib.NtxError) as e:
        ProposalTrainer(prop, ipe, max_rays=8, n_samples=8, n_importance=8, blur_idx=0)
    assert e.value.code == _lib.NTX_E_UNSUPPORTED


def test_the_interlevel_term_falls_over_forty_steps():
    """40 `step`s on one fixed batch: the mean of the last five `last_interlevel` is below the mean of the first five (a falling value, not a
    converged one), everything finite, both networks moved."""
    from nerf_tex_amd.loss import NerfLoss
    from nerf_tex_amd.train import ProposalTrainer
    prop, fine, spec = pair()
    args, u = the_batch(spec)
    pt = ProposalTrainer(prop, fine, max_rays=N_RAYS, n_samples=S_PROP, n_importance=N_IMP, perturb=False, interlevel_weight=1.0)
    start = [tr.weights().copy() for tr in pt.trainers]
    terms, totals = [], []
    for _ in range(40):
        totals.append(pt.step(*args, NerfLoss(), seed=3, u=u))
        terms.append(pt.last_interlevel)
    torch.cuda.synchronize()
    terms, totals = [float(x) for x in terms], [float(x) for x in totals]
    print(f"| interlevel term | first five {np.mean(terms[:5]):.6g} | last five {np.mean(terms[-5:]):.6g} | total {np.mean(totals[:5]):.6g} -> {np.mean(totals[-5:]):.6g} |")
    assert np.isfinite(terms).all() and np.isfinite(totals).all() and np.mean(terms[-5:]) < np.mean(terms[:5])
    assert pt.iterations == 40 and all(not np.array_equal(tr.weights(), w0) for tr, w0 in zip(pt.trainers, start))


def test_configs_build_the_pair_and_checkpoints_hold_both_networks(tmp_path):
    """`Trainer.from_config`: with `sampler_loss` a `ProposalTrainer` (and with `proposal_model_config` a smaller first network), without it
    the class it built before; `save` / `restore` round-trips both networks."""
    from nerf_tex_amd.train import CoarseFineTrainer, FlexTrainer, ProposalTrainer, Trainer
    from tests.test_gpu_train_flex import carpet_config
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    cfg = carpet_config(depth=6)
    block = dict(cfg["model_config"])
    cfg = dict(cfg, model_config={"module": "network.model.CoarseFine", "model_config": block}, renderer_config=dict(cfg["renderer_config"], n_samples=16, n_importance=8))
    n = 16
    tr, _ = Trainer.from_config(cfg, max_rays=n)
    assert type(tr) is CoarseFineTrainer
    key = {"module": "nerf_tex_amd.loss.Interlevel", "weight": 0.25}
    tr, _ = Trainer.from_config(dict(cfg, sampler_loss=key), max_rays=n)
    assert type(tr) is ProposalTrainer and tr.interlevel_weight == 0.25 and tr.coarse.model.width == 256 and tr.coarse.model.depth == 6
    small = dict(block, depth=4, width=128)
    a, loss = Trainer.from_config(dict(cfg, sampler_loss=key, proposal_model_config=small), max_rays=n)
    assert type(a) is ProposalTrainer and [type(x) for x in a.trainers] == [FlexTrainer, FlexTrainer]
    assert (a.coarse.model.width, a.coarse.model.depth, a.fine.model.width, a.fine.model.depth) == (128, 4, 256, 6)
    assert (a.coarse.n_samples, a.fine.n_samples, a.coarse.model.name, a.fine.model.name) == (16, 24, "model", "model_fine")
    with pytest.raises(ValueError):
        Trainer.from_config(dict(carpet_config(depth=6), sampler_loss=key), max_rays=n)                      # no CoarseFine block, no n_importance
    _, spec, _ = make_model((1, 6), arch=dict(depth=6))
    ro, rd, t, cone, params, color, alpha = flex_batch(5, n, 16, spec, "carpet")
    for k in range(2):
        a.step(ro, rd, t, params, cone, color, alpha, loss, seed=k)
    prefix = a.save(str(tmp_path / "checkpoints" / "ckpt-2"), step=2)
    b, _ = Trainer.from_config(dict(cfg, sampler_loss=key, proposal_model_config=small), max_rays=n)
    assert not np.array_equal(a.coarse.weights(), b.coarse.weights())
    info = b.restore(prefix)
    assert info["step"] == 2 and b.iterations == 2
    for x, y in zip(a.trainers, b.trainers):
        assert np.array_equal(x.weights(), y.weights()) and all(np.array_equal(p, q) for p, q in zip(x.adam_state(), y.adam_state()))
    va, vb = a.step(ro, rd, t, params, cone, color, alpha, loss, seed=9), b.step(ro, rd, t, params, cone, color, alpha, loss, seed=9)
    torch.cuda.synchronize()
    assert torch.equal(va, vb) and np.isfinite(float(va)) and all(np.array_equal(x.weights(), y.weights()) for x, y in zip(a.trainers, b.trainers))


def test_a_trained_pair_of_different_architectures_renders():
    """`hand_weights_to_models`, then the existing `Renderer(model=proposal, model_fine=model, n_importance=...)`: a pair of different
    architectures renders finite colours."""
    from nerf_tex_amd.loss import NerfLoss
    from nerf_tex_amd.renderer import Renderer
    from nerf_tex_amd.train import ProposalTrainer
    prop, fine, spec = pair(OTHER)
    args, u = the_batch(spec)
    pt = ProposalTrainer(prop, fine, max_rays=N_RAYS, n_samples=S_PROP, n_importance=N_IMP, perturb=False)
    pt.step(*args, NerfLoss(), seed=1, u=u)
    pt.hand_weights_to_models()
    ro, rd, t, params, cone, color, alpha = args
    r = Renderer(model=prop, model_fine=fine, n_samples=S_PROP, n_importance=N_IMP, perturb=False)
    out = r(put(ro)[None], put(rd)[None], put(t)[None], None, put(cone).reshape(1, N_RAYS, 1), training=False)
    torch.cuda.synchronize()
    r.raise_if_nonfinite()
    assert tuple(out["color_pred"].shape) == (1, N_RAYS, 3) and tuple(out["color_pred_coarse"].shape) == (1, N_RAYS, 3)
    assert bool(torch.isfinite(out["color_pred"]).all()) and bool(torch.isfinite(out["alpha_pred"]).all()) and float(out["alpha_pred"].max()) > 0
