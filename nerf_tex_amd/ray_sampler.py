"""Ray generation (reference: network/ray_sampler.py)."""

from __future__ import annotations

import ctypes as C
from typing import Any, Tuple

import numpy as np


def _generate(pixel_range, height: int, width: int, focal: float, c2w, mode: int, b0, b1,
              near: float, far: float, device=None):
    """`pixel_range`: a pixel set of `pixel_sampler.Full` -- (first, count[, run_length, run_stride]) of the row-major grid -- or, as in
    the reference (ray_sampler.py:17, 25), any [n,2] tensor of (row, col) image-plane locations (`Independent`, `Proxy`, `Full.as_tensor`)."""
    import torch
    from . import _lib
    loc = None
    if hasattr(pixel_range, "shape"):                                # image_plane_loc tensor: tf.cast(image_plane_loc, tf.float32)
        loc = torch.as_tensor(pixel_range)
        if loc.dim() != 2 or loc.shape[1] != 2:
            raise ValueError(f"image_plane_loc must be [n,2], got {tuple(loc.shape)}")
        if device is None and loc.is_cuda:
            device = loc.device
        first, count, run, stride = 0, loc.shape[0], 1, 1
    else:
        first, count, run, stride = pixel_range if len(pixel_range) == 4 else (pixel_range[0], pixel_range[1], max(1, pixel_range[1]), max(1, pixel_range[1]))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    rays_o = torch.empty((count, 3), device=dev, dtype=torch.float32)
    rays_d = torch.empty((count, 3), device=dev, dtype=torch.float32)
    t = torch.empty((count, 2), device=dev, dtype=torch.float32)
    cone = torch.empty((count, 1), device=dev, dtype=torch.float32)
    c2w_h = np.ascontiguousarray(np.asarray(c2w.detach().cpu() if hasattr(c2w, "detach") else c2w, dtype=np.float32))
    if c2w_h.shape != (4, 4):
        raise ValueError(f"c2w must be 4x4, got {c2w_h.shape}")
    if loc is not None:
        loc = loc.to(device=dev, dtype=torch.float32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(_lib.lib.ntx_generate_rays_at(c2w_h.ctypes.data_as(C.POINTER(C.c_float)), height, width, float(np.float32(focal)),
                                                     loc.data_ptr(), count, mode, _lib.f3(b0) if b0 is not None else None,
                                                     _lib.f3(b1) if b1 is not None else None, float(near), float(far),
                                                     rays_o.data_ptr(), rays_d.data_ptr(), t.data_ptr(), cone.data_ptr(),
                                                     torch.cuda.current_stream(dev).cuda_stream))
        return rays_o, rays_d, t, cone
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.ntx_generate_rays_strided(c2w_h.ctypes.data_as(C.POINTER(C.c_float)), height, width,
                                                      float(np.float32(focal)), first, count, run, stride, mode,
                                                      _lib.f3(b0) if b0 is not None else None,
                                                      _lib.f3(b1) if b1 is not None else None, float(near), float(far),
                                                      rays_o.data_ptr(), rays_d.data_ptr(), t.data_ptr(), cone.data_ptr(),
                                                      torch.cuda.current_stream(dev).cuda_stream))
    return rays_o, rays_d, t, cone


class Frustum:
    """network.ray_sampler.Frustum (ray_sampler.py:6-21)."""

    def __init__(self, height: int, width: int, focal: float, near: float, far: float, **kwargs) -> None:
        self.height, self.width, self.focal, self.near, self.far = height, width, focal, near, far

    def __call__(self, image_plane_loc, c2w, device=None):
        return _generate(image_plane_loc, self.height, self.width, self.focal, c2w, 1, None, None, self.near,
                         self.far, device)


class Proxy:
    """network.ray_sampler.Proxy (ray_sampler.py:23-37): normalised rays_d and the proxy's t-range."""

    def __init__(self, height: int, width: int, focal: float, proxy: Any, **kwargs) -> None:
        self.height, self.width, self.focal, self.proxy = height, width, focal, proxy

    def __call__(self, image_plane_loc, c2w, device=None):
        """`image_plane_loc`: the (first_pixel, n_pixels[, run_length, run_stride]) pixel set produced by `pixel_sampler.Full`, or an
        [n,2] tensor of (row, col) as the reference's pixel samplers return it."""
        return _generate(image_plane_loc, self.height, self.width, self.focal, c2w, 0, self.proxy.b_0,
                         self.proxy.b_1, 0.0, 0.0, device)


def posed_rays(image_plane_loc, poses, focal, height: int, width: int, proxy: Any = None, near=None, far=None, rays_per_pose=None):
    """The rays of a BATCH of cameras whose poses live on the device (`ntx_generate_rays_posed`): `Proxy.__call__` (`proxy`: an AABB) or
    `Frustum.__call__` (`near`, `far`) for B cameras in one launch on the current stream, without a host round trip for the poses, and
    differentiable in them -- `poses` [B,4,4] or [B,3,4] (c2w) and `focal` (a float, or a tensor [B]) that require grad receive theirs from
    dL/d rays_o and dL/d rays_d (`nerf_tex_amd.autograd.PosedRays`, `ntx_generate_rays_posed_adjoint`); t and cone_scale are constants.
    `image_plane_loc`: [B,R,2] (row, col), or [N,2] with `rays_per_pose` (ray k belongs to pose k // rays_per_pose; the last pose may have
    fewer).  All tensors on the GPU.  Returns (rays_o [N,3], rays_d [N,3], t [N,2], cone_scale [N,1]); with the same matrix and focal they
    are `Proxy.__call__`'s / `Frustum.__call__`'s bit for bit."""
    import torch
    from .autograd import _posed_rays_function
    if (proxy is None) == (near is None and far is None) or (near is None) != (far is None):
        raise ValueError("give either proxy (an AABB: normalised rays_d and the box's t range) or near and far (a frustum), not both and not neither")
    if not (isinstance(poses, torch.Tensor) and isinstance(image_plane_loc, torch.Tensor) and poses.is_cuda and image_plane_loc.is_cuda):
        raise ValueError("posed_rays runs on the GPU: poses and image_plane_loc are CUDA(ROCm) tensors")
    if poses.dim() != 3 or tuple(poses.shape[1:]) not in ((4, 4), (3, 4)):
        raise ValueError(f"poses must be [B,4,4] or [B,3,4], got {tuple(poses.shape)}")
    B = int(poses.shape[0])
    loc = image_plane_loc
    if loc.dim() == 3 and loc.shape[-1] == 2 and rays_per_pose is None:
        if int(loc.shape[0]) != B:
            raise ValueError(f"image_plane_loc holds {int(loc.shape[0])} images, poses {B}")
        rays_per_pose = int(loc.shape[1])
        loc = loc.reshape(-1, 2)
    elif loc.dim() != 2 or loc.shape[-1] != 2 or rays_per_pose is None:
        raise ValueError(f"image_plane_loc must be [B,R,2], or [N,2] with rays_per_pose; got {tuple(loc.shape)}")
    n, rays_per_pose = int(loc.shape[0]), int(rays_per_pose)
    if B < 1 or rays_per_pose < 1 or (n > 0 and (n - 1) // rays_per_pose + 1 != B):
        raise ValueError(f"{n} rays at {rays_per_pose} per pose do not make {B} poses")
    dev = poses.device
    if not isinstance(focal, torch.Tensor):
        focal = torch.full((B,), float(np.float32(focal)), device=dev, dtype=torch.float32)
    elif focal.dim() == 0:
        focal = focal.expand(B)
    if tuple(focal.shape) != (B,) or focal.device != dev or loc.device != dev:
        raise ValueError(f"focal must be a float or a tensor [B] on the poses' device, got {tuple(focal.shape)} on {focal.device}")
    mode = 0 if proxy is not None else 1
    consts = (int(height), int(width), mode, None if proxy is None else tuple(proxy.b_0), None if proxy is None else tuple(proxy.b_1),
              0.0 if near is None else float(near), 0.0 if far is None else float(far))
    return _posed_rays_function().apply(poses[:, :3, :].to(torch.float32).contiguous(), focal.to(torch.float32).contiguous(),
                                        loc.detach().to(torch.float32).contiguous(), rays_per_pose, consts)
