"""Camera pose fitting on the GPU (`ntx_generate_rays_posed`, `ntx_generate_rays_posed_adjoint`, `ray_sampler.posed_rays`,
`autograd.PosedRays`, `fit.PoseFitter`; DESIGN "Fitting camera poses"): the forward against `ntx_generate_rays_at` bit for bit, the adjoint
against the header's formulas in float64 within the derived bound of its fixed-order sums, its order and reproducibility, the autograd chain
against float64 autograd of the restated pipeline at the project's standing gradient bar, an end-to-end fit, and a fingerprint of what must
not move.  The scenes are chosen on the CPU (tests/test_pose_fit.py).  `-m gpu`."""


import numpy as np
import pytest

from tests import pose_common as pc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
H, W = pc.H, pc.W
RS = (1, 63, 64, 65, 256, 257)


def dev():
    return torch.device("cuda", 0)


def up(a):
    return torch.as_tensor(np.ascontiguousarray(a, F)).to(dev())


def batch_of_three(R, seed):
    """Three cameras with three focals, the middle one looking AWAY from the box -- a quarter turn to the side: the slab test is a LINE's, and the
    lines of a camera that turns its back still pass the box, at negative t -- so every t of its rays is inf in mode 0; N = 2 R + 5 rays (a short
    last pose; R = 1: three full poses), fractional locations, some outside the image."""
    from oracle import nerftex_oracle as orc
    rng = np.random.default_rng(seed)
    c2w, focal = pc.cameras(3, seed=seed)
    pos = c2w[1, :3, 3].astype(np.float64)
    c2w[1] = orc.look_at(pos, to=pos + np.cross(pos, (0., 0., 1.)), dtype=np.float64).astype(F)
    n = 3 if R == 1 else 2 * R + 5
    loc = rng.uniform(-3, H + 3, size=(n, 2)).astype(F)
    return c2w, focal, loc, n


def posed(loc, c2w, focal, R, mode):
    from nerf_tex_amd.proxy import AABB
    from nerf_tex_amd.ray_sampler import posed_rays
    kw = dict(proxy=AABB(*pc.BOX)) if mode == 0 else dict(near=2.0, far=6.0)
    outs = posed_rays(up(loc), up(c2w), up(focal), H, W, rays_per_pose=R, **kw)
    return [o.cpu().numpy() for o in outs]


def adjoint(loc, poses, focal, R, mode, g_o, g_d, stream=None):
    """`ntx_generate_rays_posed_adjoint` on device copies of the arguments: (d_poses [B,3,4], d_focal [B]) on the host."""
    from nerf_tex_amd import _lib
    B = len(focal)
    args = [up(a) for a in (np.asarray(poses)[:, :3, :], focal, loc, g_o, g_d)]
    d_poses, d_focal = torch.full((B, 3, 4), np.nan, device=dev()), torch.full((B,), np.nan, device=dev())
    torch.cuda.synchronize()
    _lib.check(_lib.lib.ntx_generate_rays_posed_adjoint(args[0].data_ptr(), args[1].data_ptr(), B, H, W, args[2].data_ptr(), len(loc), R, mode, args[3].data_ptr(),
                                                        args[4].data_ptr(), d_poses.data_ptr(), d_focal.data_ptr(), stream))
    torch.cuda.synchronize()
    return d_poses.cpu().numpy(), d_focal.cpu().numpy()


# ---- 1. forward, bit for bit ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("mode", [0, 1], ids=["proxy", "frustum"])
def test_forward_is_generate_rays_at_bit_for_bit(mode, R):
    from nerf_tex_amd.proxy import AABB
    from nerf_tex_amd.ray_sampler import Frustum, Proxy
    c2w, focal, loc, n = batch_of_three(R, seed=R)
    got = posed(loc, c2w, focal, R, mode)
    assert [g.shape for g in got] == [(n, 3), (n, 3), (n, 2), (n, 1)]
    for b in range(3):
        sl = slice(b * R, min(n, (b + 1) * R))
        one = (Proxy(H, W, float(focal[b]), AABB(*pc.BOX)) if mode == 0 else Frustum(H, W, float(focal[b]), 2.0, 6.0))(up(loc[sl]), c2w[b], device=dev())
        for g, w, name in zip(got, one, ("rays_o", "rays_d", "t", "cone_scale")):
            assert np.array_equal(g[sl], w.cpu().numpy(), equal_nan=True), (b, name)
    if mode == 0:
        t = got[2]
        assert np.isinf(t[R:min(n, 2 * R)]).all()                                   # the camera that looks away
        assert R < 63 or np.isfinite(t[:R, 0]).any()                                  # ... and one that sees it
    assert len({float(f) for f in focal}) == 3


# ---- 2. the adjoint against float64 ----------------------------------------------------------------------------------------------------------------
def held_to_the_bound(got, loc, poses, focal, R, mode, g_o, g_d, name):
    """Every entry within (ceil(R / T) + log2 T + 8) 2^-24 sum_k |term_k| of float64, term_k the summand of the header's formula; the ratio to the
    looser sum over the monomials inside a summand is printed beside it, not asserted."""
    want_p, want_f, mag_p, mag_f, mono_p, mono_f = pc.adjoint_formulas(loc, poses, focal, H, W, R, mode, g_o, g_d)
    worst = loose = 0.0
    for b in range(len(focal)):
        count = min(len(loc), (b + 1) * R) - b * R
        for g, w, m, mono in ((got[0][b], want_p[b], mag_p[b], mono_p[b]), (got[1][b], want_f[b], mag_f[b], mono_f[b])):
            err = np.abs(np.asarray(g, np.float64) - w)
            worst = max(worst, float(np.max(np.where(np.asarray(m) > 0, err / np.maximum(pc.adjoint_bound(count, m), 1e-300), 0.0))))
            loose = max(loose, float(np.max(np.where(np.asarray(mono) > 0, err / np.maximum(pc.adjoint_bound(count, mono), 1e-300), 0.0))))
            assert (np.asarray(g)[np.asarray(m) == 0] == 0).all()
    print(f"ADJERR {name}: largest |got - float64| / bound = {worst:.2e} (over the monomials' magnitudes: {loose:.2e})")
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and worst <= 1.0, worst
    return worst


@pytest.mark.parametrize("R", RS)
@pytest.mark.parametrize("mode", [0, 1], ids=["proxy", "frustum"])
def test_adjoint_within_the_derived_bound_of_float64(mode, R):
    c2w, focal, loc, n = batch_of_three(R, seed=R)
    rng = np.random.default_rng(R + 100)
    g_o, g_d = rng.normal(size=(n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    got = adjoint(loc, c2w, focal, R, mode, g_o, g_d)
    held_to_the_bound(got, loc, c2w, focal, R, mode, g_o, g_d, f"mode {mode} R {R}")


@pytest.mark.parametrize("mode", [0, 1], ids=["proxy", "frustum"])
def test_adjoint_of_one_pose_with_70001_rays(mode):
    """69 trips of the 1024 lanes, the last a partial one."""
    n = 70001
    rng = np.random.default_rng(7)
    c2w, focal = pc.cameras(1, seed=7)
    loc = rng.uniform(-3, H + 3, size=(n, 2)).astype(F)
    g_o, g_d = rng.normal(size=(n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    got = adjoint(loc, c2w, focal, n, mode, g_o, g_d)
    held_to_the_bound(got, loc, c2w, focal, n, mode, g_o, g_d, f"mode {mode} R {n}")


@pytest.mark.parametrize("mode", [0, 1], ids=["proxy", "frustum"])
def test_zero_cotangents_add_exact_zeros(mode):
    """Rays with zero cotangents appended to a pose's rays change no bit (within a trip of the lanes and across one); a pose whose cotangents
    are all zero gets exact zeros, beside poses that do not."""
    rng = np.random.default_rng(3)
    c2w, focal = pc.cameras(3, seed=3)
    for n, more in ((257, 40), (1000, 100), (5, 2000)):
        loc = rng.uniform(-3, H + 3, size=(n + more, 2)).astype(F)
        g_o, g_d = rng.normal(size=(n + more, 3)).astype(F), rng.normal(size=(n + more, 3)).astype(F)
        g_o[n:] = 0; g_d[n:] = 0
        g_d[n + 1] = -0.0
        base = adjoint(loc[:n], c2w[:1], focal[:1], n, mode, g_o[:n], g_d[:n])
        longer = adjoint(loc, c2w[:1], focal[:1], n + more, mode, g_o, g_d)
        assert np.array_equal(base[0], longer[0]) and np.array_equal(base[1], longer[1]) and np.abs(base[0]).min() > 0
    R = 65
    loc = rng.uniform(-3, H + 3, size=(3 * R, 2)).astype(F)
    g_o, g_d = rng.normal(size=(3 * R, 3)).astype(F), rng.normal(size=(3 * R, 3)).astype(F)
    g_o[R:2 * R] = 0; g_d[R:2 * R] = 0
    d_poses, d_focal = adjoint(loc, c2w, focal, R, mode, g_o, g_d)
    assert not d_poses[1].any() and d_focal[1] == 0 and not np.signbit(d_poses[1]).any() and not np.signbit(d_focal[1])      # +0, every bit
    assert np.abs(d_poses[0]).min() > 0 and np.abs(d_poses[2]).min() > 0 and d_focal[0] != 0 and d_focal[2] != 0


# ---- 3. order and reproducibility --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["proxy", "frustum"])
def test_a_poses_numbers_do_not_depend_on_the_batch(mode):
    """Two calls: identical bits.  Pose b's thirteen numbers out of a batch of five (the last pose short) are the bits it gets as a batch of
    one, for b first, middle and last."""
    R, B, short = 300, 5, 77
    n = (B - 1) * R + short
    rng = np.random.default_rng(11)
    c2w, focal = pc.cameras(B, seed=11)
    loc = rng.uniform(-3, H + 3, size=(n, 2)).astype(F)
    g_o, g_d = rng.normal(size=(n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    first = adjoint(loc, c2w, focal, R, mode, g_o, g_d)
    again = adjoint(loc, c2w, focal, R, mode, g_o, g_d)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    for b in (0, 2, 4):
        sl = slice(b * R, min(n, (b + 1) * R))
        count = sl.stop - sl.start
        alone = adjoint(loc[sl], c2w[b:b + 1], focal[b:b + 1], count, mode, g_o[sl], g_d[sl])
        assert np.array_equal(alone[0][0], first[0][b]) and alone[1][0] == first[1][b], b
        if count == R:                                                             # ... and with room for more rays per pose than it has
            roomy = adjoint(loc[sl], c2w[b:b + 1], focal[b:b + 1], R + 50, mode, g_o[sl], g_d[sl])
            assert np.array_equal(roomy[0], alone[0]) and np.array_equal(roomy[1], alone[1])


@pytest.mark.parametrize("mode", [0, 1], ids=["proxy", "frustum"])
def test_both_entries_run_on_the_stream_they_are_given(mode):
    """On a side stream of torch's (non-blocking: the null stream does not wait for it) the inputs are written BEHIND a long matrix product
    on that stream, over values that give other results; an entry that launched anywhere else would read those.  The results are the null
    stream's bits."""
    from nerf_tex_amd import _lib
    R, B = 129, 3
    n = B * R
    rng = np.random.default_rng(5)
    c2w, focal = pc.cameras(B, seed=5)
    loc = rng.uniform(0, H, size=(n, 2)).astype(F)
    g_o, g_d = rng.normal(size=(n, 3)).astype(F), rng.normal(size=(n, 3)).astype(F)
    want_rays = posed(loc, c2w, focal, R, mode)
    want_adj = adjoint(loc, c2w, focal, R, mode, g_o, g_d)
    real = [up(a) for a in (c2w[:, :3, :], focal, loc, g_o, g_d)]
    work = [torch.full_like(a, 3.0) for a in real]                                 # valid cameras of another kind: other rays, other sums
    outs = [torch.zeros((n, 3), device=dev()), torch.zeros((n, 3), device=dev()), torch.zeros((n, 2), device=dev()), torch.zeros((n, 1), device=dev())]
    d_poses, d_focal = torch.zeros((B, 3, 4), device=dev()), torch.zeros((B,), device=dev())
    big = torch.randn((4096, 4096), device=dev())
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev())
    b0, b1 = _lib.f3(pc.BOX[0]), _lib.f3(pc.BOX[1])
    with torch.cuda.stream(side):
        for _ in range(4):
            big = big @ big * 1e-3
        for w, r in zip(work, real):
            w.copy_(r)
        s = torch.cuda.current_stream(dev()).cuda_stream
        assert s == side.cuda_stream and s != 0
        _lib.check(_lib.lib.ntx_generate_rays_posed(work[0].data_ptr(), work[1].data_ptr(), B, H, W, work[2].data_ptr(), n, R, mode, b0, b1, 2.0, 6.0,
                                                    *[o.data_ptr() for o in outs], s))
        _lib.check(_lib.lib.ntx_generate_rays_posed_adjoint(work[0].data_ptr(), work[1].data_ptr(), B, H, W, work[2].data_ptr(), n, R, mode, work[3].data_ptr(),
                                                            work[4].data_ptr(), d_poses.data_ptr(), d_focal.data_ptr(), s))
    side.synchronize()
    for o, w in zip(outs, want_rays):
        assert np.array_equal(o.cpu().numpy(), w, equal_nan=True)
    assert np.array_equal(d_poses.cpu().numpy(), want_adj[0]) and np.array_equal(d_focal.cpu().numpy(), want_adj[1])


# ---- 4. the autograd chain ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [False, True], ids=["flex", "fused_chain"])
def test_the_autograd_chain_matches_float64_autograd_of_the_pipeline(fused, monkeypatch):
    """PosedRays -> DifferentiableRender(trainer) -> a torch mse on colour and alpha -> backward(), float32 on the device, 2 poses x 33 rays x 8
    samples: poses.grad [2,3,4] and focal.grad [2] against float64 autograd of the WHOLE restated pipeline (tests/pose_common.py in front of
    `oracle.train_oracle.render`) on the ReLU patterns the trainer kept, per column at the project's standing bar: rel-Linf <= max(1e-4, 4
    float32 floors), the floor what float32 autograd of the same pipeline is off by, under the project's guards (floor <= 5e-4, every column's
    gradient > 1e-6): `pgc.check_param_gradients`.  With
    poses and focal that do not require grad the adjoint is never launched and the rays are the same bits."""
    from oracle import nerftex_oracle as orc
    from nerf_tex_amd import _lib
    from nerf_tex_amd.autograd import DifferentiableRender, PosedRays
    from nerf_tex_amd.proxy import AABB
    from nerf_tex_amd.ray_sampler import posed_rays
    from nerf_tex_amd.train import FlexTrainer, Trainer, trainer_for
    from tests import custom_loss_common as clc
    from tests import param_grad_common as pgc
    model, spec, wts, sc = pc.chain_setup(fused)
    B, R, S = pc.CHAIN["poses"], pc.CHAIN["rays"], pc.CHAIN["S"]
    n = B * R
    tr = trainer_for(model, input_gradients="only", fused=fused, max_rays=n, n_samples=S, perturb=False)
    assert type(tr) is (Trainer if fused else FlexTrainer)
    launches = []
    real = _lib.lib.ntx_generate_rays_posed_adjoint
    monkeypatch.setattr(_lib.lib, "ntx_generate_rays_posed_adjoint", lambda *a: (launches.append(1), real(*a))[1])
    render = DifferentiableRender(tr)
    box = AABB(*pc.BOX)
    loc, rows, color, alpha = up(sc["loc"]), up(sc["rows"]), up(sc["color"]), up(sc["alpha"])

    def run(grad):
        poses, focal = up(sc["poses"]).requires_grad_(grad), up(sc["focal"]).requires_grad_(grad)
        rays = posed_rays(loc, poses, focal, H, W, proxy=box)
        assert rays[0].requires_grad == rays[1].requires_grad == grad and not rays[2].requires_grad and not rays[3].requires_grad
        cp, ap = render(rays[0], rays[1], rays[2], rows, rays[3].reshape(-1), rays_per_param_row=R)
        val = pc.mse_loss(color, alpha, cp, ap)
        val.backward()
        torch.cuda.synchronize()
        return poses, focal, [r.detach().cpu().numpy() for r in rays], float(val.detach())

    _, _, rays0, val0 = run(False)
    assert not launches
    poses, focal, rays1, val = run(True)
    assert len(launches) == 1 and val == val0 and all(np.array_equal(a, b) for a, b in zip(rays0, rays1))
    assert issubclass(PosedRays, torch.autograd.Function)
    got = pc.columns(poses.grad.cpu().numpy(), focal.grad.cpu().numpy())
    t = rays1[2]
    assert np.isfinite(t).all()
    z = orc.z_values(t, S, F)
    masks, _, sigma_mask = clc.chain_patterns(tr, n, S, None) if fused else pgc.trainer_patterns(tr, spec, n, S, None)
    args = (H, W, R, S, *pc.BOX, sc["rows"], sc["color"], sc["alpha"])
    kw = dict(z=z, masks=masks, sigma_mask=sigma_mask)
    want = pc.restated_pose_gradients(wts, spec, sc["loc"].reshape(-1, 2), sc["poses"], sc["focal"], *args, dtype=torch.float64, **kw)
    f32 = pc.restated_pose_gradients(wts, spec, sc["loc"].reshape(-1, 2), sc["poses"], sc["focal"], *args, dtype=torch.float32, **kw)
    want_c, f32_c = pc.columns(*want[1:]), pc.columns(*f32[1:])
    print(f"CHAIN {'fused' if fused else 'flex'}: loss {val:.9g} want {want[0]:.9g}")
    assert abs(val - want[0]) <= 1e-4 * abs(want[0])
    res = pgc.check_param_gradients(got, want_c, f32_c)                              # per column: err <= max(1e-4, 4 floors), floor <= 5e-4, max |grad| > 1e-6
    print(f"CHAINERR {'fused' if fused else 'flex'} worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")


# ---- 5. a fit ------------------------------------------------------------------------------------------------------------------------------------
def test_a_fit_lowers_the_loss_and_its_first_gradient_is_float64s():
    """Teacher: synthetic weights with dense media on the carpet architecture; 2 poses x 64 rays x 16 samples at fixed in-box pixels, the targets
    rendered at the true poses by the fitter's own trainer; the start 2 degrees and 0.05 off; 40 iterations.

    NO scene with random weights lets the float64 fit halve the pose errors (tests/test_pose_fit.py, tools/pose_fit_sweep.py,
    profiles/pose_fit/fit_e2e.md: the loss is saturated half a degree from the truth), so, as the issue provides for that case, this asserts the loss decrease
    and the first step's gradient, not the pose errors: every loss finite, the last below the first, and dL/d omega, dL/d tau of the first
    step against float64 autograd of the restated pipeline through `compose_poses`, per column at the standing bar
    (`pgc.check_param_gradients` on the six columns of [omega | tau]).  The trajectory is printed
    beside float64's."""
    from oracle import nerftex_oracle as orc
    from nerf_tex_amd.fit import PoseFitter, compose_poses
    from nerf_tex_amd.proxy import AABB
    from tests import param_grad_common as pgc
    f = pc.FIT
    model, spec, wts, batch, true, start, focal = pc.fit_setup()
    B, R, S = f["poses"], f["rays"], f["S"]
    n = B * R
    fitter = PoseFitter(model, H, W, focal, proxy=AABB(*pc.BOX), n_samples=S, max_rays=n, lrate=f["lrate"])
    with torch.no_grad():
        rays = fitter.rays(up(batch["image_plane_loc"]), up(true), up(focal))
        assert torch.isfinite(rays[2]).all()
        color, alpha = fitter.trainer.forward(rays[0], rays[1], rays[2], up(batch["parameters"]), rays[3].reshape(-1), rays_per_param_row=R)
    batch["color"], batch["alpha"] = color.cpu().numpy().reshape(B, R, 3), alpha.cpu().numpy().reshape(B, R)
    # the first step's gradient
    omega, tau = (torch.zeros((B, 3), device=dev(), requires_grad=True) for _ in range(2))
    dbatch = {k: up(v) for k, v in batch.items()}
    val = float(fitter.step(dbatch, pc.mse_loss, compose_poses(up(start), omega, tau), up(focal)))
    got = np.concatenate([omega.grad.cpu().numpy(), tau.grad.cpu().numpy()], 1).astype(np.float64)
    with torch.no_grad():
        t = fitter.rays(dbatch["image_plane_loc"], up(start), up(focal))[2].cpu().numpy()
    assert np.isfinite(t).all()
    masks, _, sigma_mask = pgc.trainer_patterns(fitter.trainer, spec, n, S, None)

    z = orc.z_values(t, S, F)
    want_val, want = pc.restated_first_step(spec, wts, batch, start, focal, torch.float64, z, masks, sigma_mask)
    _, f32 = pc.restated_first_step(spec, wts, batch, start, focal, torch.float32, z, masks, sigma_mask)
    print(f"FIT first step: loss {val:.9g} want {want_val:.9g}")
    assert abs(val - want_val) <= 1e-4 * abs(want_val)
    res = pgc.check_param_gradients(got, want, f32)                                  # the six columns of [omega | tau] over the two poses
    print(f"FITGRAD worst err {res.errs.max():.2e} worst floor {res.floors.max():.2e}")
    # the fit
    track = []
    c2w, focal_out, history = fitter.fit(batch, pc.mse_loss, start, f["n_iters"], callback=lambda it, c, fo: track.append(c.cpu().numpy()) if it % 10 == 0 else None)
    torch.cuda.synchronize()
    c2w = c2w.cpu().numpy()
    rot0, tr0 = pc.pose_errors(start, true)
    rot, trn = pc.pose_errors(c2w, true)
    for k, c in enumerate(track):
        r_, t_ = pc.pose_errors(c, true)
        print(f"FITTRACK {10 * k:3d} loss {history[10 * k]:.6e} rotation {r_[0]:.4f} {r_[1]:.4f} translation {t_[0]:.5f} {t_[1]:.5f}")
    print(f"FITTRACK end loss {history[-1]:.6e} rotation {rot[0]:.4f} {rot[1]:.4f} translation {trn[0]:.5f} {trn[1]:.5f}")
    assert len(history) == f["n_iters"] and np.isfinite(history).all() and np.isfinite(c2w).all()
    assert abs(history[0] - val) <= 1e-6 * val                                      # the loss of a step is taken before its update
    assert history[-1] < history[0]
    assert tuple(c2w.shape) == (B, 4, 4) and np.array_equal(focal_out.cpu().numpy(), focal)
    R3 = c2w[:, :3, :3].astype(np.float64)
    assert np.abs(R3 @ R3.transpose(0, 2, 1) - np.eye(3)).max() <= 1e-5              # (look_at's own matrices are orthonormal to 2e-6)


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------------------------------
def test_nothing_else_moves():
    """`ntx_generate_rays_at` on one fixed input and one plain `gradients_step` of a default trainer, before and after a PoseFitter (with
    `fit_focal`: the focal moves too) has been created and stepped in this process: the same bits."""
    from nerf_tex_amd.fit import PoseFitter
    from nerf_tex_amd.loss import AlphaLoss
    from nerf_tex_amd.proxy import AABB
    from nerf_tex_amd.ray_sampler import Proxy
    from nerf_tex_amd.train import Trainer
    from tests.common import make_model
    model, spec, wts = make_model((1, 6), dense_media=True)
    c2w, focal = pc.cameras(2, seed=9)
    rng = np.random.default_rng(9)
    loc = rng.uniform(0, H, size=(2, 40, 2)).astype(F)
    color, alpha = rng.uniform(0, 1, (80, 3)).astype(F), rng.uniform(0, 1, 80).astype(F)
    rows = np.asarray([(1, 1, 1, .1, 0, 0, 1)], F)

    def fingerprint():
        rays = Proxy(H, W, float(focal[0]), AABB(*pc.BOX))(up(loc.reshape(-1, 2)), c2w[0], device=dev())
        tr = Trainer(model, max_rays=80, n_samples=16, perturb=False)
        val, cp, ap = tr.gradients_step(rays[0], rays[1], rays[2], rows, rays[3], color, alpha, AlphaLoss(loss_fn="network.loss.smape", alpha_loss_fn="network.loss.mse"),
                                        rays_per_param_row=80)
        torch.cuda.synchronize()
        return [r.cpu().numpy().tobytes() for r in rays] + [val.cpu().numpy().tobytes(), cp.cpu().numpy().tobytes(), ap.cpu().numpy().tobytes(), tr.gradients().tobytes()]

    before = fingerprint()
    fitter = PoseFitter(model, H, W, focal, proxy=AABB(*pc.BOX), n_samples=16, max_rays=80, lrate=1e-4, fit_focal=True)
    batch = dict(image_plane_loc=loc, parameters=np.repeat(rows, 2, 0), color=color.reshape(2, 40, 3), alpha=alpha.reshape(2, 40))
    _, focal_out, history = fitter.fit(batch, pc.mse_loss, c2w, 2)
    assert len(history) == 2 and np.isfinite(history).all()
    moved = focal_out.cpu().numpy() / focal                                        # with fit_focal Adam has taken two steps of 1e-4 on log f
    assert np.isfinite(moved).all() and (moved != 1).all() and np.abs(np.log(moved)).max() <= 2.1e-4
    assert fingerprint() == before
