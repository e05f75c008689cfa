"""What the tests of camera pose fitting share (tests/test_pose_fit.py on the CPU, tests/test_gpu_pose_fit.py on the GPU; `ntx_generate_rays_posed`,
`ntx_generate_rays_posed_adjoint`, `ray_sampler.posed_rays`, `autograd.PosedRays`, `fit.PoseFitter`): a torch restatement of the oracle's
`rays_from_camera` / `proxy_rays` / `frustum_rays` for a BATCH of cameras, differentiable in the poses and the focals; the header's adjoint formulas
in numpy float64 with the sum of the magnitudes of their terms; the derived bound of the kernel's fixed-order sums; the restated pipeline (rays in
front of `oracle.train_oracle.render`, the step restatement tests/input_grad_common.py uses) and the end-to-end fit's scene.

TEST INFRASTRUCTURE ONLY.  tests/test_pose_fit.py holds `rays_torch` against the oracle's numpy functions, and `adjoint_formulas` against float64
autograd of `rays_torch`."""

import numpy as np
import torch

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro

F = np.float32
ADJ_T = 1024                                                                     # the adjoint kernel's partial sums per pose (include/nerftex.h)


# ---- the rays of B cameras ---------------------------------------------------------------------------------------------------------------------
def rays_torch(loc, poses, focal, height, width, rays_per_pose, mode):
    """(rays_o [N,3], rays_d [N,3], cone_scale [N,1]) of `orc.rays_from_camera` -- and, mode 0, `orc.proxy_rays`' normalisation -- for ray k under
    pose k // rays_per_pose, as a torch expression in the dtype of `poses` [B,3,4] (or [B,4,4]) and `focal` [B]; `loc` [N,2] = (row, col)."""
    dt = poses.dtype
    loc = torch.as_tensor(np.asarray(loc)).to(dt)
    idx = torch.arange(loc.shape[0]) // int(rays_per_pose)
    f = focal.to(dt)[idx]
    d0 = (loc[:, 1] + 0.5 - 0.5 * width) / f
    d1 = -(loc[:, 0] + 0.5 - 0.5 * height) / f
    dirs = torch.stack([d0, d1, -torch.ones_like(d0)], -1)
    rays_d = torch.sum(dirs[:, None, :] * poses[idx][:, :3, :3], -1)
    rays_o = poses[idx][:, :3, 3]
    norm_xy = torch.sqrt(torch.sum(dirs[:, :2] * dirs[:, :2], -1))
    norm = torch.sqrt(torch.sum(dirs * dirs, -1))
    cone = torch.cos(torch.atan(norm_xy)) / norm / f
    if mode == 0:
        rays_d = rays_d / torch.sqrt(torch.sum(rays_d * rays_d, -1, keepdim=True))
    return rays_o, rays_d, cone[:, None]


def oracle_rays(loc, poses, focal, height, width, rays_per_pose, mode, b_0=None, b_1=None, near=0.0, far=0.0, dtype=np.float64):
    """The oracle's own functions, pose by pose: (rays_o, rays_d, t, cone_scale) concatenated."""
    loc, outs = np.asarray(loc), []
    for b in range(len(poses)):
        rows = loc[b * rays_per_pose:(b + 1) * rays_per_pose]
        c2w = np.concatenate([np.asarray(poses[b], dtype)[:3], np.asarray([[0, 0, 0, 1.]], dtype)])
        outs.append(orc.proxy_rays(rows, height, width, focal[b], c2w, b_0, b_1, dtype) if mode == 0 else
                    orc.frustum_rays(rows, height, width, focal[b], c2w, near, far, dtype))
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(4))


# ---- the adjoint, as include/nerftex.h states it -----------------------------------------------------------------------------------------------
def adjoint_formulas(loc, poses, focal, height, width, rays_per_pose, mode, g_o, g_d):
    """(d_poses [B,3,4], d_focal [B], mag_poses [B,3,4], mag_focal [B], mono_poses, mono_focal) in float64: the header's formulas, ray by ray, and
    beside every sum the sum over the rays of |term_k|, term_k the SUMMAND of the header's formula -- g_v[r] dc[c], g_o[r], g_v . (d0 R[:,0] +
    d1 R[:,1]) / f -- which is what `adjoint_bound` multiplies.  mono_*: the looser sum of the magnitudes of the monomials INSIDE a summand
    (g_d[r] dc[c] / |v| and n[r] n[j] g_d[j] dc[c] / |v| for dR in mode 0), printed beside the bound's ratio to show how much cancellation inside a
    ray's own term there is; nothing is asserted on it."""
    loc, P, f = np.asarray(loc, np.float64), np.asarray(poses, np.float64)[:, :3, :], np.asarray(focal, np.float64)
    g_o, g_d = np.asarray(g_o, np.float64), np.asarray(g_d, np.float64)
    B = len(P)
    d_poses, mag_poses, d_focal, mag_focal = np.zeros((B, 3, 4)), np.zeros((B, 3, 4)), np.zeros(B), np.zeros(B)
    mono_poses, mono_focal = np.zeros((B, 3, 4)), np.zeros(B)
    for b in range(B):
        sl = slice(b * rays_per_pose, min(len(loc), (b + 1) * rays_per_pose))
        R = P[b, :, :3]
        d0, d1 = (loc[sl, 1] + 0.5 - 0.5 * width) / f[b], -(loc[sl, 0] + 0.5 - 0.5 * height) / f[b]
        dc = np.stack([d0, d1, -np.ones_like(d0)], -1)                               # [n, 3]
        go, gd = g_o[sl], g_d[sl]
        if mode == 0:
            v = dc @ R.T
            ln = np.sqrt(np.sum(v * v, -1, keepdims=True))
            n = v / ln
            gv = (gd - n * np.sum(n * gd, -1, keepdims=True)) / ln
            gv_mag = (np.abs(gd) + np.abs(n) * np.sum(np.abs(n * gd), -1, keepdims=True)) / ln
        else:
            gv, gv_mag = gd, np.abs(gd)
        d_poses[b, :, :3] = gv.T @ dc
        mag_poses[b, :, :3] = np.abs(gv).T @ np.abs(dc)
        mono_poses[b, :, :3] = gv_mag.T @ np.abs(dc)
        d_poses[b, :, 3] = go.sum(0)
        mag_poses[b, :, 3] = mono_poses[b, :, 3] = np.abs(go).sum(0)
        q = dc[:, :1] * R[None, :, 0] + dc[:, 1:2] * R[None, :, 1]                    # d0 R[:,0] + d1 R[:,1]
        q_mag = np.abs(dc[:, :1] * R[None, :, 0]) + np.abs(dc[:, 1:2] * R[None, :, 1])
        d_focal[b] = -np.sum(gv * q) / f[b]
        mag_focal[b] = np.sum(np.abs(np.sum(gv * q, -1))) / f[b]
        mono_focal[b] = np.sum(gv_mag * q_mag) / f[b]
    return d_poses, d_focal, mag_poses, mag_focal, mono_poses, mono_focal


def adjoint_bound(count, magnitude, T=ADJ_T):
    """(ceil(R / T) + log2 T + 8) 2^-24 sum |term|: a lane adds at most ceil(R / T) terms one after the other, the butterfly and the tree add
    log2 T levels, and a term carries a few roundings of its own.  Worst case of the fixed-order float32 sum; derived, not measured."""
    return (-(-int(count) // T) + np.log2(T) + 8) * 2.0 ** -24 * np.asarray(magnitude, np.float64)


def autograd_adjoint(loc, poses, focal, height, width, rays_per_pose, mode, g_o, g_d, dtype=torch.float64):
    """(d_poses [B,3,4], d_focal [B]) by torch autograd of `rays_torch` under the cotangents g_o, g_d."""
    P = torch.tensor(np.asarray(poses)[:, :3, :], dtype=dtype, requires_grad=True)
    f = torch.tensor(np.asarray(focal), dtype=dtype, requires_grad=True)
    ro, rd, _ = rays_torch(loc, P, f, height, width, rays_per_pose, mode)
    (torch.sum(ro * torch.as_tensor(np.asarray(g_o)).to(dtype)) + torch.sum(rd * torch.as_tensor(np.asarray(g_d)).to(dtype))).backward()
    return P.grad.numpy().astype(np.float64), f.grad.numpy().astype(np.float64)


# ---- cameras -----------------------------------------------------------------------------------------------------------------------------------
def cameras(n, seed=0, dtype=np.float32, radius=None):
    """`n` look-at cameras on a sphere around the origin, [n,4,4], and slightly different focals [n] for a `width` of 64."""
    rng = np.random.default_rng(seed)
    radius = RADIUS if radius is None else radius
    out = []
    for _ in range(n):
        az, el = rng.uniform(0, 2 * np.pi), rng.uniform(0.2, 0.9)
        out.append(orc.look_at((radius * np.cos(el) * np.cos(az), radius * np.cos(el) * np.sin(az), radius * np.sin(el)), dtype=np.float64))
    focal = np.asarray([orc.focal_from_angle(64, 0.55) * (1 + 0.07 * k) for k in range(n)])
    return np.stack(out).astype(dtype), focal.astype(dtype)


def rotation_about(axis, degrees):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = np.deg2rad(degrees)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def perturbed(c2w, degrees, shift, seed):
    """Every pose of `c2w` [B,4,4] rotated by `degrees` about a random axis (on the left: the camera turns in the world) and moved by `shift`
    in a random direction."""
    rng = np.random.default_rng(seed)
    out = np.asarray(c2w, np.float64).copy()
    for b in range(len(out)):
        out[b, :3, :3] = rotation_about(rng.normal(size=3), degrees) @ out[b, :3, :3]
        d = rng.normal(size=3)
        out[b, :3, 3] += shift * d / np.linalg.norm(d)
    return out


def pose_errors(c2w, true):
    """(rotation error in degrees [B], translation error [B]) of the poses `c2w` against `true`."""
    c2w, true = np.asarray(c2w, np.float64), np.asarray(true, np.float64)
    cos = (np.trace(np.einsum("bij,bkj->bik", c2w[:, :3, :3], true[:, :3, :3]), axis1=1, axis2=2) - 1) / 2
    return np.rad2deg(np.arccos(np.clip(cos, -1, 1))), np.linalg.norm(c2w[:, :3, 3] - true[:, :3, 3], axis=1)


# ---- the pipeline: rays in front of the restated step -------------------------------------------------------------------------------------------
def mse_loss(color_true, alpha_true, color_pred, alpha_pred):
    """The torch loss of the chain and fit tests, on either side: mse on colour plus mse on alpha."""
    return torch.mean((color_pred - color_true) ** 2) + torch.mean((alpha_pred - alpha_true) ** 2)


def restated_pipeline(wts, spec, loc, poses, focal, height, width, rays_per_pose, n_samples, b_0, b_1, rows, color, alpha, dtype=torch.float64, z=None,
                      masks=None, sigma_mask=None, loss=mse_loss):
    """(loss, [color | alpha] [N,4], rays_o, rays_d) of rays -> render -> loss as ONE torch graph in `dtype`: `rays_torch` (mode 0) in front of
    `tro.render`, the step restatement of tests/input_grad_common.py.  `poses` [B,3,4] / [B,4,4] and `focal` [B] are torch tensors (the caller's
    leaves or expressions of them).  The depths are constants: `z` [N,S] as given (inf: a ray that misses), or placed between the box's range of
    the rays at their present values.  `rows` [B,P]: a parameter row per pose.  Rays that miss are filtered out, predict 0 and count in the loss."""
    np_dt = np.float64 if dtype == torch.float64 else np.float32
    ro, rd, cone = rays_torch(loc, poses.to(dtype), focal.to(dtype), height, width, rays_per_pose, 0)
    n = ro.shape[0]
    if z is None:
        t = orc.aabb(ro.detach().numpy(), rd.detach().numpy(), b_0, b_1, np_dt)
        z = orc.z_values(np.where(np.isfinite(t), t, 0).astype(np_dt), n_samples, np_dt)
        z[~np.isfinite(t[:, 0])] = np.inf
    z = np.asarray(z)
    hit = np.isfinite(z).all(1)
    t_ = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    per_ray = t_(np.repeat(np.asarray(rows), int(rays_per_pose), 0)[:n])
    c, a = torch.zeros((n, 3), dtype=dtype), torch.zeros((n,), dtype=dtype)
    if hit.any():
        idx = torch.as_tensor(np.nonzero(hit)[0])
        S = z.shape[1]
        mk = None if masks is None else [t_(np.asarray(m).reshape(n, S, -1)[hit]).flatten(0, 1) for m in masks]
        sm = None if sigma_mask is None else t_(np.asarray(sigma_mask)[hit])
        ch, ah = tro.render([t_(x) for x in wts], spec, ro[idx], rd[idx], t_(z[hit]), per_ray[idx], cone.detach()[idx], None, False, False, (1., 1., 1.), mk, sm, None)
        c, a = c.index_put((idx,), ch), a.index_put((idx,), ah)
    val = loss(color_true=t_(color), alpha_true=t_(alpha), color_pred=c, alpha_pred=a)
    return val, torch.cat([c, a[:, None]], -1), ro, rd


def restated_pose_gradients(wts, spec, loc, poses, focal, *args, dtype=torch.float64, **kw):
    """(loss, d_poses [B,3,4], d_focal [B]) of `restated_pipeline` by autograd, the twelve numbers of every pose and its focal as the leaves."""
    P = torch.tensor(np.asarray(poses)[:, :3, :], dtype=dtype, requires_grad=True)
    f = torch.tensor(np.asarray(focal), dtype=dtype, requires_grad=True)
    val, _, _, _ = restated_pipeline(wts, spec, loc, P, f, *args, dtype=dtype, **kw)
    val.backward()
    return float(val.detach()), P.grad.numpy().astype(np.float64), f.grad.numpy().astype(np.float64)


def columns(d_poses, d_focal):
    """[B,3,4] and [B] as thirteen columns over the poses: what `pgc.check_param_gradients` holds to the bar column by column."""
    return np.concatenate([np.asarray(d_poses, np.float64).reshape(len(d_focal), 12), np.asarray(d_focal, np.float64).reshape(-1, 1)], 1)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------
# A SMALL scene on purpose: a box of side 1 seen from distance 2.  A float32 ray position carries rounding in proportion to |o| + |d z|, which the
# tenth Fourier band multiplies by 2^9; the carpet family's own box (side 3 from distance 6) puts the float32 floor of the WHOLE pipeline at the
# project's guard of 5e-4, this one about three times inside it.
BOX = ((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))
RADIUS = 2.0
H = W = 64


def in_box_pixels(c2w, focal, rays, seed, margin=0.15):
    """`rays` (row, col) locations per pose, [B,rays,2] float32, whose rays pass the box `margin` inside its faces seen from `c2w`: pixels that
    stay hits while a fit moves the camera by a few degrees."""
    rng = np.random.default_rng(seed)
    inner = tuple(tuple(np.sign(v) * (abs(v) - margin) for v in b) for b in BOX)
    grid = orc.full_pixels(H, W)
    out = []
    for b in range(len(c2w)):
        _, _, t, _ = orc.proxy_rays(grid, H, W, focal[b], c2w[b], *inner, np.float64)
        ok = np.nonzero(np.isfinite(t[:, 0]))[0]
        assert len(ok) >= rays, (len(ok), rays)
        out.append(grid[np.sort(rng.choice(ok, rays, replace=False))])
    return np.stack(out).astype(F)


# the autograd chain's case (2 poses x 33 rays x 8 samples) on a small network and on the fused chain's 8 x 256
CHAIN = dict(poses=2, rays=33, S=8, seed=1, small=dict(width=64, depth=3, skips=[1]))


def chain_setup(fused):
    """(model, spec, weights, scene) of the autograd chain's case; scene: loc [B,R,2], poses [B,3,4], focal [B], rows [B,P], color, alpha."""
    from tests.common import make_model
    c = CHAIN
    model, spec, wts = make_model((1, 6), dense_media=True, arch=None if fused else c["small"])
    c2w, focal = cameras(c["poses"], seed=c["seed"])
    loc = in_box_pixels(c2w, focal, c["rays"], c["seed"])
    rng = np.random.default_rng(c["seed"])
    n = c["poses"] * c["rays"]
    rows = np.tile(np.asarray([(1, 1, 1, .1, 0, 0, 1)], F), (c["poses"], 1))
    scene = dict(loc=loc, poses=np.ascontiguousarray(c2w[:, :3, :]), focal=focal, rows=rows, color=rng.uniform(0, 1, (n, 3)).astype(F), alpha=rng.uniform(0, 1, n).astype(F))
    return model, spec, wts, scene


# the end-to-end fit: a teacher with dense media on the carpet architecture renders 2 poses x 64 rays x 16 samples at the true poses; the fit starts
# 2 degrees and 0.05 off; lrate 1e-3, PoseFitter's default: 40 Adam steps can cover 0.04 rad = 2.3 degrees and 0.04 units.  The seeds are chosen on the CPU
# (tests/test_pose_fit.py: the first step's float32 floors twice inside the project's guard; the float64 fit's loss falls by a third).
FIT = dict(poses=2, rays=64, S=16, seed=1, start_seed=2, degrees=2.0, shift=0.05, lrate=1e-3, n_iters=40)


def fit_setup():
    """(model, spec, weights, batch dict for `PoseFitter.fit`, true c2w [B,4,4] float64, start c2w [B,4,4] float32, focal [B])."""
    from tests.common import make_model
    f = FIT
    model, spec, wts = make_model((1, 6), dense_media=True)
    true, focal = cameras(f["poses"], seed=f["seed"])
    start = perturbed(true, f["degrees"], f["shift"], f["start_seed"]).astype(F)
    loc = in_box_pixels(true, focal, f["rays"], f["seed"])
    rows = np.tile(np.asarray([(1, 1, 1, .1, 0, 0, 1)], F), (f["poses"], 1))
    batch = dict(image_plane_loc=loc, parameters=rows)
    return model, spec, wts, batch, true.astype(np.float64), start, focal


def restated_targets(spec, wts, batch, c2w, focal, dtype=torch.float64):
    """The teacher's images at the poses `c2w`: (color [B,R,3], alpha [B,R]) float32 from the float64 pipeline."""
    B, R = batch["image_plane_loc"].shape[:2]
    with torch.no_grad():
        _, pred, _, _ = restated_pipeline(wts, spec, batch["image_plane_loc"].reshape(-1, 2), torch.tensor(np.asarray(c2w), dtype=dtype), torch.tensor(np.asarray(focal), dtype=dtype),
                                          H, W, R, FIT["S"], *BOX, batch["parameters"], np.zeros((B * R, 3)), np.zeros(B * R), dtype=dtype)
    return pred[:, :3].numpy().astype(F).reshape(B, R, 3), pred[:, 3].numpy().astype(F).reshape(B, R)


def restated_fit(spec, wts, batch, start, focal, n_iters, lrate, dtype=torch.float64):
    """`PoseFitter.fit` on the CPU: the same parametrisation (`nerf_tex_amd.fit.compose_poses`), the same torch Adam, autograd of the restated
    pipeline in `dtype` (free ReLU branches).  Returns (c2w [B,4,4], the loss of every step before its update, the poses before every step)."""
    from nerf_tex_amd.fit import compose_poses
    B, R = batch["image_plane_loc"].shape[:2]
    c2w0 = torch.tensor(np.asarray(start), dtype=dtype)
    omega, tau = (torch.zeros((B, 3), dtype=dtype, requires_grad=True) for _ in range(2))
    f = torch.tensor(np.asarray(focal), dtype=dtype)
    opt = torch.optim.Adam([omega, tau], lr=lrate)
    losses, track = [], []
    for _ in range(n_iters):
        opt.zero_grad(set_to_none=True)
        c2w = compose_poses(c2w0, omega, tau)
        track.append(c2w.detach().numpy().copy())
        val, _, _, _ = restated_pipeline(wts, spec, batch["image_plane_loc"].reshape(-1, 2), c2w, f, H, W, R, FIT["S"], *BOX, batch["parameters"],
                                         batch["color"].reshape(-1, 3), batch["alpha"].reshape(-1), dtype=dtype)
        val.backward()
        opt.step()
        losses.append(float(val.detach()))
    with torch.no_grad():
        return compose_poses(c2w0, omega, tau).numpy(), losses, track


def restated_first_step(spec, wts, batch, start, focal, dtype=torch.float64, z=None, masks=None, sigma_mask=None):
    """(loss, [dL/d omega | dL/d tau] [B,6]) of the fit's first step: autograd of the restated pipeline through `compose_poses` at omega = tau = 0."""
    from nerf_tex_amd.fit import compose_poses
    B, R = batch["image_plane_loc"].shape[:2]
    om, ta = (torch.zeros((B, 3), dtype=dtype, requires_grad=True) for _ in range(2))
    val, _, _, _ = restated_pipeline(wts, spec, batch["image_plane_loc"].reshape(-1, 2), compose_poses(torch.tensor(np.asarray(start), dtype=dtype), om, ta),
                                     torch.tensor(np.asarray(focal), dtype=dtype), H, W, R, FIT["S"], *BOX, batch["parameters"], batch["color"].reshape(-1, 3),
                                     batch["alpha"].reshape(-1), dtype=dtype, z=z, masks=masks, sigma_mask=sigma_mask)
    val.backward()
    return float(val.detach()), np.concatenate([om.grad.numpy(), ta.grad.numpy()], 1).astype(np.float64)


def own_fit_patterns(spec, wts, batch, start, focal):
    """(z [N,S], masks, sigma_mask) of a float32 pass of the restatement at the start poses: the CPU's stand-in for what the trainer keeps."""
    from tests import train_branch_oracle as tbo
    B, R = batch["image_plane_loc"].shape[:2]
    ro, rd, t, cone = oracle_rays(batch["image_plane_loc"].reshape(-1, 2), np.asarray(start, F)[:, :3, :], focal, H, W, R, 0, *BOX, dtype=F)
    assert np.isfinite(t).all()
    z = orc.z_values(t, FIT["S"], F)
    masks, _, sigma_mask = tbo.own_masks(wts, spec, ro, rd, z, np.repeat(batch["parameters"], R, 0), cone)
    return z, masks, sigma_mask
