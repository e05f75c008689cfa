"""One training step of the reference restated on the CPU: network/train.py:61-67 over network/renderer.py:92-213 (Renderer) or :356-473 (MipRenderer) and
network/loss.py:6-59, with torch autograd in FLOAT64 standing in for tf.GradientTape, and TF 2.4's Adam + ExponentialDecay (train.py:49-52) written out.

TEST INFRASTRUCTURE ONLY (the rules of nerftex_oracle.py: nothing under nerf_tex_amd/ imports it).  PARITY UNPINNED: TensorFlow cannot
run here and the reference ships no gradients; the forward pass is torch_cpu.py's (checked against nerftex_oracle.py in
tests/test_oracle.py), the gradients are whatever autograd derives from it -- no hand-written adjoint on this side, which is the point:
the kernels' hand-written backward pass is compared with it."""

from __future__ import annotations

import numpy as np
import torch

from . import torch_cpu


def mse(y_true, y_pred):                                                                  # loss.py:51-54
    return torch.mean((y_true - y_pred) ** 2)


def smape(y_true, y_pred, eps=1e-2):                                                      # loss.py:56-59
    return torch.mean(torch.abs(y_true - y_pred) / (y_true + y_pred + eps))


LOSS_FNS = {"mse": mse, "smape": smape}


def nerf_loss(color_true, color_pred, loss_fn="mse"):                                    # loss.py:6-19 (no coarse pass)
    return LOSS_FNS[loss_fn](color_true, color_pred)


def alpha_loss(color_true, alpha_true, color_pred, alpha_pred, loss_fn="mse", alpha_loss_fn=None, gamma=1.0, filter_color_loss=True, use_hard_mask=True):
    """loss.py:21-49 (no coarse pass)."""
    fn, afn = LOSS_FNS[loss_fn], LOSS_FNS[alpha_loss_fn or loss_fn]
    if filter_color_loss:
        mask = (alpha_true[..., None] > 0).to(color_true.dtype) if use_hard_mask else alpha_true[..., None]
        color_true = color_true * mask
        color_pred = color_pred * mask
    return fn(color_true, color_pred) + gamma * afn(alpha_true, alpha_pred)


composite = torch_cpu.composite


def fourier_dists(z, rays_d):
    """renderer.py:174-180: a sample reaches to the next one, the last as far as the one before it; times |d|."""
    dists = z[:, 1:] - z[:, :-1]
    return torch.cat([dists, dists[:, -1:]], -1) * torch.linalg.norm(rays_d, dim=-1, keepdim=True)


def mip_dists(z, rays_d):
    """renderer.py:441-444: the S segments between the S + 1 edges; times |d|."""
    return (z[:, 1:] - z[:, :-1]) * torch.linalg.norm(rays_d, dim=-1, keepdim=True)


def render(w, spec, rays_o, rays_d, z, parameters, cone_scale, blur_idx=None, map_exr=False, composite_bkgd=False, bkgd=(1., 1., 1.), masks=None,
           sigma_mask=None, noise=None):
    """render_rays on GIVEN depths (the depths themselves, renderer.py:101-111 / 374-383, are the caller's: with perturb they come from the
    product's restated generator, nerftex_oracle.sample_depths), by the model's position encoding:
    "fourier": Renderer.render_rays (renderer.py:114-213) on sample depths z [n, S];
    "ipe": MipRenderer.render_rays (:365-409) + map_model_output (:439-473) on segment edges z [n, S + 1]; parameters [n, P + 1] hold the blur
    parameter at `blur_idx`, the model sees the other P.
    `masks` / `sigma_mask`: torch_cpu.mlp's and torch_cpu.composite's."""
    n = z.shape[0]
    rays_d_n = rays_d / torch.linalg.norm(rays_d, dim=-1, keepdim=True)
    if spec.pos_encoding == "ipe":
        if blur_idx is None:
            raise ValueError("an IPE model is rendered by the MipRenderer, which needs blur_idx")
        S = z.shape[1] - 1
        blur = parameters[:, blur_idx, None] * cone_scale.reshape(n, 1)
        params = torch.cat([parameters[:, :blur_idx], parameters[:, blur_idx + 1:]], -1).repeat_interleave(S, 0)
        mean, cov = torch_cpu.cone_segment_gaussians(rays_o, rays_d, z, blur)
        pos_map = torch_cpu.ipe(mean.reshape(-1, 3), cov.reshape(-1, 3), spec.pos_freq)
        dists = mip_dists(z, rays_d)
    else:
        S = z.shape[1]
        pts = rays_o[:, None, :] + rays_d[:, None, :] * z[:, :, None]
        params = parameters.repeat_interleave(S, 0)
        if blur_idx is not None:
            scale = (cone_scale.reshape(n, 1, 1) * z[:, :, None]).reshape(-1, 1)
            params = torch.cat([params[:, :blur_idx], params[:, blur_idx, None] * scale, params[:, blur_idx + 1:]], -1)
        pos_map = torch_cpu.fourier_features(pts.reshape(-1, 3), spec.pos_freq)
        dists = fourier_dists(z, rays_d)
    color, alpha = torch_cpu.mlp(w, spec, pos_map, rays_d_n.repeat_interleave(S, 0), params, masks)
    return composite(color.reshape(n, S, 3), alpha.reshape(n, S), dists, map_exr, composite_bkgd, bkgd, sigma_mask, noise)


def _loss(loss, color_true, alpha_true, c, a):
    kw = {k: v for k, v in loss.items() if k != "kind"}
    return nerf_loss(color_true, c, **kw) if loss["kind"] == "nerf" else alpha_loss(color_true, alpha_true, c, a, **kw)


def composite_gradients(raw_rgb, sigma, z, rays_d, color_true, alpha_true, loss, map_exr=False, composite_bkgd=False, bkgd=(1., 1., 1.), noise=None,
                        dtype=torch.float64, mip=False):
    """The Renderer's composite and the loss alone under autograd: (loss, color_pred, alpha_pred, dL/d raw_rgb [n, S, 3], dL/d sigma [n, S]) for GIVEN raw
    network outputs -- what a hand-written adjoint of renderer.py:170-213 + loss.py is compared with, apart from the network's own rounding.
    `mip`: the MipRenderer's composite (renderer.py:439-473): `z` [n, S + 1] holds the segment edges and a sample's length is its segment's."""
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    rgb = torch.tensor(np.asarray(raw_rgb), dtype=dtype, requires_grad=True); sg = torch.tensor(np.asarray(sigma), dtype=dtype, requires_grad=True)
    if np.shape(z)[-1] != sg.shape[-1] + (1 if mip else 0):
        raise ValueError(f"{np.shape(z)[-1]} depths for {sg.shape[-1]} samples (mip={mip})")
    c, a = composite(rgb, sg, (mip_dists if mip else fourier_dists)(t_(z), t_(rays_d)), map_exr, composite_bkgd, bkgd, None, t_(noise))
    val = _loss(loss, t_(color_true), t_(alpha_true), c, a)
    val.backward()
    return float(val.detach()), c.detach().numpy(), a.detach().numpy(), rgb.grad.numpy(), sg.grad.numpy()


def step_gradients(w_np, spec, rays_o, rays_d, z, parameters, cone_scale, color_true, alpha_true, loss, blur_idx=None, map_exr=False,
                   composite_bkgd=False, bkgd=(1., 1., 1.), dtype=torch.float64, masks=None, sigma_mask=None, noise=None, chunk_rays=None, workers=1):
    """(loss, color_pred, alpha_pred, gradients in get_weights() order as a list of arrays) of one step; `loss` = dict(kind='nerf'|'alpha', **kwargs).
    Renderer.__call__ (renderer.py:58-86): rays whose depths are not finite (t = inf: they miss the proxy) are filtered out, the rest
    rendered, the results scattered back into zeros -- plus the background colour for the filtered ones when compositing -- and the loss runs
    over ALL rays.
    `masks` [M, width] per ReLU layer / `sigma_mask` [n, S]: the ReLU patterns of a float32 forward pass (torch_cpu.mlp), 0/1 or bool; `noise`
    [n, S]: the density regulariser's draws (raw_noise_std * N(0,1), renderer.py:190-192).
    `chunk_rays`: for a batch too large for one autograd pass in float64 (the configs' 1024 rays x 256 samples).  The losses of loss.py are
    MEANS over the rays, so the batch's loss and gradient are the ray-count-weighted sums of its chunks' -- evaluated `chunk_rays` rays at a
    time (bounded memory, minutes of CPU; `workers` chunks at once on Python threads: the matrices of a chunk are too small to keep every
    BLAS thread busy; the masks reach the working dtype a chunk at a time: 67 MB each as bool at that batch, 537 MB in float64), added up
    in chunk order."""
    z = np.asarray(z)
    n, S = z.shape[0], z.shape[1] - (spec.pos_encoding == "ipe")
    hit_all = np.isfinite(z).all(1)
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)

    def one(r0):
        r1 = min(n, r0 + (chunk_rays or n))
        hit = hit_all[r0:r1]
        sub = lambda x: None if x is None else t_(np.asarray(x)[r0:r1][hit])
        mk = None if masks is None else [sub(m.reshape(n, S, -1)).flatten(0, 1) for m in map(np.asarray, masks)]
        w = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in w_np]
        c = torch.zeros((r1 - r0, 3), dtype=dtype); a = torch.zeros((r1 - r0,), dtype=dtype)
        if hit.any():
            ch, ah = render(w, spec, sub(rays_o), sub(rays_d), sub(z), sub(parameters), sub(cone_scale), blur_idx, map_exr, composite_bkgd, bkgd, mk,
                            sub(sigma_mask), sub(noise))
            idx = torch.as_tensor(np.nonzero(hit)[0])
            c = c.index_put((idx,), ch); a = a.index_put((idx,), ah)
        if composite_bkgd:
            c = c + torch.as_tensor((~hit)[:, None] * np.asarray(bkgd, np.float64)[None, :], dtype=dtype)
        val = _loss(loss, t_(np.asarray(color_true)[r0:r1]), None if alpha_true is None else t_(np.asarray(alpha_true)[r0:r1]), c, a)
        if val.requires_grad:
            val.backward()
        return (r1 - r0) / n, float(val.detach()), c.detach().numpy(), a.detach().numpy(), [np.zeros(x.shape) if x.grad is None else x.grad.numpy() for x in w]

    starts = list(range(0, n, chunk_rays or n))
    if len(starts) == 1:
        return one(0)[1:]
    if workers > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(workers) as ex:
            parts = list(ex.map(one, starts))
    else:
        parts = map(one, starts)
    total, grads, cs, al = 0.0, None, [], []
    for wgt, val, c, a, g in parts:                                                      # in chunk order, whatever order they finished in
        total += val * wgt
        grads = [x * wgt for x in g] if grads is None else [acc + x * wgt for acc, x in zip(grads, g)]
        cs.append(c); al.append(a)
    return total, np.concatenate(cs), np.concatenate(al), grads


def adam_step(w, g, m, v, iterations, lrate, decay_steps=0.0, decay_rate=0.1, beta_1=0.9, beta_2=0.999, epsilon=1e-7, dtype=np.float64):
    """tf.keras.optimizers.Adam (TF 2.4 ApplyAdam, non-amsgrad) under ExponentialDecay (train.py:49-52): flat arrays in, (w, m, v) out."""
    w, g, m, v = (np.asarray(x, dtype) for x in (w, g, m, v))
    lr = lrate * decay_rate ** (iterations / decay_steps) if decay_steps > 0 else lrate
    t = iterations + 1.0
    # Keras holds beta_1 / beta_2 as float32 hyper-parameters and forms 1 - beta in float32 (optimizer_v2/adam.py: _prepare_local):
    # 1 - 0.999f = 9.99987e-4, not 1e-3
    b1, b2 = np.float32(beta_1), np.float32(beta_2)
    omb1, omb2 = float(np.float32(1) - b1), float(np.float32(1) - b2)
    lr_t = lr * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t)
    m = m + (g - m) * omb1
    v = v + (g * g - v) * omb2
    return w - lr_t * m / (np.sqrt(v) + epsilon), m, v


def step_gradients_chunked(w_np, spec, rays_o, rays_d, z, parameters, cone_scale, color_true, alpha_true, loss, chunk_rays=16, masks=None, sigma_mask=None,
                           noise=None, workers=None, **kw):
    """`step_gradients` 16 rays at a time on NTX_ORACLE_WORKERS threads (default 4): what bench.py's parity block calls."""
    import os
    if workers is None:
        workers = int(os.environ.get("NTX_ORACLE_WORKERS", "4"))
    return step_gradients(w_np, spec, rays_o, rays_d, z, parameters, cone_scale, color_true, alpha_true, loss, masks=masks, sigma_mask=sigma_mask, noise=noise,
                          chunk_rays=chunk_rays, workers=workers, **kw)


def step_gradients_coarse_fine(w_coarse_np, w_fine_np, spec, rays_o, rays_d, z_coarse, z_fine, parameters, cone_scale, color_true, alpha_true, loss,
                               masks_coarse=None, sigma_mask_coarse=None, masks_fine=None, sigma_mask_fine=None, noise_coarse=None, noise_fine=None, dtype=torch.float64, **kw):
    """A step with n_importance > 0 (renderer.py:125-138, loss.py:15-16, 41-47): the coarse pass on z_coarse, the fine pass on z_fine -- GIVEN:
    the sampler carries no gradient (`tf.stop_gradient`, :129) and is restated and tested on its own (nerftex_oracle.sample_pdf) --, the
    loss of both added.  w_fine_np None: one network runs both passes (model_fine is None, :132) and its gradient is the sum.
    Returns (loss, (color, alpha) fine, (color, alpha) coarse, gradients of the coarse network, of the fine one (None when shared))."""
    t_ = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype)
    wc = [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in w_coarse_np]
    wf = wc if w_fine_np is None else [torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in w_fine_np]
    mk = lambda m: None if m is None else [t_(x) for x in m]
    args = (t_(rays_o), t_(rays_d))
    c1, a1 = render(wc, spec, *args, t_(z_coarse), t_(parameters), t_(cone_scale), masks=mk(masks_coarse), sigma_mask=t_(sigma_mask_coarse), noise=t_(noise_coarse), **kw)
    c2, a2 = render(wf, spec, *args, t_(z_fine), t_(parameters), t_(cone_scale), masks=mk(masks_fine), sigma_mask=t_(sigma_mask_fine), noise=t_(noise_fine), **kw)
    val = _loss(loss, t_(color_true), t_(alpha_true), c2, a2) + _loss(loss, t_(color_true), t_(alpha_true), c1, a1)
    val.backward()
    g = lambda w: [x.grad.numpy() for x in w]
    return float(val.detach()), (c2.detach().numpy(), a2.detach().numpy()), (c1.detach().numpy(), a1.detach().numpy()), g(wc), None if w_fine_np is None else g(wf)
