"""A MipRenderer training step restated on the CPU for the tests of the IPE trainer: MipRenderer.render_rays / get_cone_segment_gaussians /
map_model_output (network/renderer.py:356-473) and IntegratedPositionalEncoding (network/layer.py:25-41) in torch, so that float64 autograd
stands in for tf.GradientTape.  The MLP is oracle/train_oracle.py's masked one with the encoding swapped; the losses are its own.

TEST INFRASTRUCTURE ONLY (nothing under nerf_tex_amd/ imports it)."""

from __future__ import annotations

import math

import numpy as np
import torch

from oracle import torch_cpu
from oracle import train_oracle as tro


def cone_segment_gaussians(rays_o, rays_d, z, radii):
    """renderer.py:411-437: z [n, S+1] edges, radii [n, 1] -> mean [n, S, 3], diagonal covariance [n, S, 3]."""
    t0, t1 = z[:, :-1], z[:, 1:]
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    den = 3 * mu ** 2 + hw ** 2
    t_mean = mu + (2 * mu * hw ** 2) / den
    t_var = hw ** 2 / 3 - (4 / 15) * ((hw ** 4 * (12 * mu ** 2 - hw ** 2)) / den ** 2)
    r_var = radii ** 2 * (mu ** 2 / 4 + (5 / 12) * hw ** 2 - 4 / 15 * hw ** 4 / den)
    mean = rays_o[:, None, :] + rays_d[:, None, :] * t_mean[..., None]
    d_mag_sq = torch.clamp(torch.sum(rays_d ** 2, -1, keepdim=True), min=1e-10)
    null = 1 - rays_d ** 2 / d_mag_sq
    cov = t_var[..., None] * (rays_d ** 2)[:, None, :] + r_var[..., None] * null[:, None, :]
    return mean, cov


def ipe(mean, cov, n_freq):
    """layer.py:31-41 on [M, 3] means and covariances: [sin(y) e^(-y_var/2) | sin(y + pi/2) e^(-y_var/2)], y = 2^f x_c at index 3 f + c."""
    freq = torch.as_tensor(2.0 ** np.arange(n_freq), dtype=mean.dtype)
    y = (mean[:, None, :] * freq[:, None]).reshape(-1, 3 * n_freq)
    y_var = (cov[:, None, :] * freq[:, None] ** 2).reshape(-1, 3 * n_freq)
    return torch.sin(torch.cat([y, y + 0.5 * math.pi], -1)) * torch.exp(-0.5 * torch.cat([y_var, y_var], -1))


def model_forward(w, spec, mean, cov, dirs, params, masks=None):
    """ParamNerf (model.py:58-125) with pos_map = IPE(mean, cov) | FourierFeatures(geometry parameters); `masks` as
    train_oracle.model_forward_masked (the float32 pass's ReLU pattern), or None for the network's own ReLUs."""
    ff = torch_cpu.fourier_features
    g, a = spec.n_geo, spec.n_app
    pos_map = ipe(mean, cov, spec.pos_freq); dir_map = ff(dirs, spec.dir_freq)
    if g > 0:
        pos_map = torch.cat([pos_map, ff(params[:, :g], spec.param_freq)], -1)
    if a > 0:
        dir_map = torch.cat([dir_map, ff(params[:, g:g + a], spec.param_freq)], -1)
    it = iter(range(0, len(w) - 2, 2))
    mk = iter(masks) if masks is not None else None
    act = lambda x: x * next(mk) if mk is not None else torch.relu(x)
    h = pos_map
    for i in range(spec.depth):
        j = next(it)
        h = act(torch.addmm(w[j + 1], h, w[j]))
        if i in spec.skips:
            h = torch.cat([pos_map, h], -1)
    alpha = torch.addmm(w[-1], h, w[-2])
    j = next(it)
    h = torch.cat([dir_map, torch.addmm(w[j + 1], h, w[j])], -1)
    for _ in range(spec.color_depth):
        j = next(it)
        h = act(torch.addmm(w[j + 1], h, w[j]))
    j = next(it)
    h = act(torch.addmm(w[j + 1], h, w[j]))
    j = next(it)
    return torch.addmm(w[j + 1], h, w[j]), alpha


def render(w, spec, rays_o, rays_d, z, parameters, cone_scale, blur_idx, map_exr=False, composite_bkgd=False, bkgd=(1., 1., 1.), masks=None,
           sigma_mask=None, noise=None):
    """MipRenderer.render_rays (renderer.py:365-409) + map_model_output (:439-473) on given edges z [n, S+1]; parameters [n, P+1]."""
    n, S = z.shape[0], z.shape[1] - 1
    rays_d_n = rays_d / torch.linalg.norm(rays_d, dim=-1, keepdim=True)
    blur = parameters[:, blur_idx, None] * cone_scale.reshape(n, 1)
    params = torch.cat([parameters[:, :blur_idx], parameters[:, blur_idx + 1:]], -1)
    mean, cov = cone_segment_gaussians(rays_o, rays_d, z, blur)
    color, alpha = model_forward(w, spec, mean.reshape(-1, 3), cov.reshape(-1, 3), rays_d_n.repeat_interleave(S, 0), params.repeat_interleave(S, 0), masks)
    color, alpha = color.reshape(n, S, 3), alpha.reshape(n, S)
    if noise is not None:
        alpha = alpha + noise
    dists = (z[:, 1:] - z[:, :-1]) * torch.linalg.norm(rays_d, dim=-1, keepdim=True)
    rgb = torch.nn.functional.elu(color) + 1 if map_exr else torch.sigmoid(color)
    am = 1. - torch.exp(-(torch.relu(alpha) if sigma_mask is None else alpha * sigma_mask) * dists)
    trans = torch.cumprod(1. - am + 1e-10, -1)
    wts = am * torch.cat([torch.ones_like(trans[:, :1]), trans[:, :-1]], -1)
    c = torch.sum(wts[..., None] * rgb, -2); a = torch.sum(wts, -1)
    if composite_bkgd:
        c = c + (1. - a[..., None]) * torch.as_tensor(bkgd, dtype=c.dtype)
    return c, a


def step_gradients(w_np, spec, rays_o, rays_d, z, parameters, cone_scale, color_true, alpha_true, loss, blur_idx, masks=None, sigma_mask=None, noise=None,
                   composite_bkgd=False, bkgd=(1., 1., 1.), chunk_rays=None, dtype=torch.float64):
    """(loss, color_pred, alpha_pred, gradients in get_weights() order) of one MipRenderer step under float64 autograd.  Rays with a non-finite
    z are filtered out and 0 / the background scattered back (Renderer.__call__, renderer.py:58-86); the loss runs over all rays.  The batch is
    evaluated `chunk_rays` rays at a time (the losses are means over rays: each chunk's loss enters weighted by its share of the rays).
    `masks`: [M, width] 0/1 per ReLU layer, `sigma_mask` / `noise`: [n, S]."""
    w = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in w_np]
    z = np.asarray(z)
    n, S = z.shape[0], z.shape[1] - 1
    hit = np.isfinite(z).all(1)
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    kw = {k: v for k, v in loss.items() if k != "kind"}
    bk = np.asarray(bkgd, np.float64)
    chunk_rays = chunk_rays or n
    total, cs, al = 0.0, [], []
    grads = [np.zeros(np.shape(a)) for a in w_np]
    for r0 in range(0, n, chunk_rays):
        r1 = min(n, r0 + chunk_rays)
        h = hit[r0:r1]
        rows = np.repeat(h, S)
        sel = lambda x: None if x is None else t_(np.asarray(x)[r0:r1][h])
        mrows = lambda x: t_(np.asarray(x)[r0 * S:r1 * S][rows])
        c = torch.zeros((r1 - r0, 3), dtype=dtype); a = torch.zeros((r1 - r0,), dtype=dtype)
        if h.any():
            ch, ah = render(w, spec, sel(rays_o), sel(rays_d), sel(z), sel(parameters), sel(np.asarray(cone_scale).reshape(n, 1)), blur_idx, False,
                            composite_bkgd, bkgd, None if masks is None else [mrows(m) for m in masks], sel(sigma_mask), sel(noise))
            idx = torch.as_tensor(np.nonzero(h)[0])
            c = c.index_put((idx,), ch); a = a.index_put((idx,), ah)
        if composite_bkgd:
            c = c + torch.as_tensor((~h)[:, None] * bk[None, :], dtype=dtype)
        ct, at = t_(np.asarray(color_true)[r0:r1]), None if alpha_true is None else t_(np.asarray(alpha_true)[r0:r1])
        val = tro.nerf_loss(ct, c, **kw) if loss["kind"] == "nerf" else tro.alpha_loss(ct, at, c, a, **kw)
        share = (r1 - r0) / n
        if h.any():
            (val * share).backward()
            for k, x in enumerate(w):
                grads[k] += x.grad.numpy()
                x.grad = None
        total += float(val.detach()) * share
        cs.append(c.detach().numpy()); al.append(a.detach().numpy())
    return total, np.concatenate(cs), np.concatenate(al), grads
