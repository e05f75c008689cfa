"""What the tests of learnable parameter textures share (tests/test_texture_fit.py on the CPU, tests/test_gpu_texture_fit.py on the GPU): the
scene -- the 24 patches of tests/test_gpu_instancer.py's texture tests over the 9 x 9 wavy sheet --, the restatement of
`ntx_instancer_sample_uv` from the oracle's point query, and the float64 adjoint of the lookup.

TEST INFRASTRUCTURE ONLY.  The restatement is `oracle.instancer_oracle.closest_point_on_mesh` + the barycentric mix of `get_parameters` at the
float32 point the kernel forms (o + t_pt * d, t_pt = t or `get_mean_distance(t, step)`)."""

import numpy as np

from oracle import instancer_oracle as io

F = np.float32
STEP, PATCH_SCALE, DENSITY_SCALE = 0.04, 0.35, 40.0           # the march's step; InstanceRenderer's two scales (tests/test_gpu_instancer.py's end-to-end test)
# the lookup radius is patch_max_extent = |max(b_0, b_1)| * patch_scale = sqrt(3) * patch_scale of the INSTANCER (0.61 at 0.35: every sample
# finds the sheet); REACH is the instancer's patch_scale at which some samples in a patch lie further from the sheet than that
REACH = 0.12
# (id, rays, samples, use_mean_distance, method, the instancer's patch_scale, every k-th ray aimed away from the scene, ray seed).  One sample
# cannot both find the sheet and not: the 1 x 1 case has to find it, every other case is held to `fair_uv`
UV_CASES = [("70x33", 70, 33, False, "nearest", REACH, 0, 61), ("70x33_mean", 70, 33, True, "nearest", REACH, 0, 61), ("1x1", 1, 1, False, "nearest", REACH, 0, 62),
            ("3x130", 3, 130, True, "nearest", REACH, 0, 62), ("blend", 40, 33, False, "nearest_blend", REACH, 0, 61), ("misses", 40, 33, False, "nearest", REACH, 3, 61),
            ("wide_reach", 40, 33, False, "nearest", PATCH_SCALE, 0, 61)]
UV_IDS = [c[0] for c in UV_CASES]
TEXTURES = {1: ["T", "", "", "", "light"], 2: ["T", "T", "", "", "light"]}      # P = 7 = the (1, 6) model's; "T": an image entry
SHAPES = [(12, 16), (4, 3)]
# the gradient test: (rays, samples, ray seed, texel seed); chosen on the CPU (tests/test_texture_fit.py::test_the_gradient_case_is_fair)
GRAD = dict(n=70, S=33, seed=61, tex_seed=5)


def scene():
    """(box keywords, patch -> world matrices, the wavy sheet (vertices, faces, uv))."""
    from tests.test_gpu_instancer import wavy_sheet
    from tests.test_oracle_instancer import random_scene
    spec0 = random_scene(61, k=24, method="nearest")
    box = dict(b_0=spec0.b_0.tolist(), b_1=spec0.b_1.tolist())
    tr = [np.linalg.inv(m.astype(np.float64)).astype(F) for m in spec0.inv]
    return box, tr, wavy_sheet()


def rays(seed, n, miss_every=0):
    from tests.test_oracle_instancer import random_rays
    o, d = random_rays(seed, n)
    if miss_every:
        d[::miss_every] = F([0, 0, 1])                        # the origins lie above the scene: straight up meets nothing
    return o, d


def parameters(seed, n, P=7):
    rng = np.random.default_rng(seed)
    par = np.repeat(rng.uniform(0.3, 1.0, size=(1, P)), n, 0).astype(F)
    par[:, P - 3:] = F([0.3, -0.2, 0.9])
    return par


def texels(seed, shape):
    return np.random.default_rng(seed).uniform(0.2, 1.0, size=shape).astype(F)


def max_extent(box, patch_scale):
    """Instancer.patch_max_extent for a scene with an instancer mesh (instancer.cpp:69, :246)."""
    e = np.maximum(np.asarray(box["b_0"], F), np.asarray(box["b_1"], F))
    return F(F(np.sqrt(e[0] * e[0] + (e[1] * e[1] + e[2] * e[2]))) * F(patch_scale))


def oracle_uv(tex_mesh, radius, o, d, t, dists, step, mean):
    """(uv [n,S,2] float32, found [n,S] bool) as `ntx_instancer_sample_uv` defines them, from the oracle's point query."""
    v, f, uv = (np.asarray(a) for a in tex_mesh)
    v, uv, f = v.astype(F), uv.astype(F), f.astype(np.int64)
    o, d, t, dists = (np.asarray(a, F) for a in (o, d, t, dists))
    n, S = t.shape
    out, found = np.zeros((n, S, 2), F), np.zeros((n, S), bool)
    for r, s in np.argwhere((dists > 0) & np.isfinite(t)):
        t_pt = io.get_mean_distance(t[r, s], F(step)) if mean else t[r, s]
        p = (o[r] + t_pt * d[r]).astype(F)
        k, uvw = io.closest_point_on_mesh(v, f, p, radius)
        if k is not None:
            out[r, s], found[r, s] = io._bary_mix(uv, f[k], uvw), True
    return out, found


def oracle_march(box, tr, tex_mesh, o, d, par, S, step, seed, mean=False, method="nearest", patch_scale=REACH, full=False):
    """t and dists of the scene's march on the CPU (the restatement the GPU instancer is held to bit for bit), untextured; `full`: all ten
    buffers, `hit` as a mask."""
    n_par = par.shape[1]
    spec = io.make_spec(box["b_0"], box["b_1"], tr, textures=[""] * (n_par - 3) + ["light"], instance_sampling_method=method, use_mean_distance=mean,
                        mesh=(tex_mesh[0], tex_mesh[1]), patch_scale=patch_scale)
    spec.patch_scale = patch_scale
    n = o.shape[0]
    out = io.get_model_input(spec, o, d, par, S, step, io.offset_uniforms(n, seed), io.choice_uniforms(n, S, seed))
    return tuple(out) if full else (out[2], out[3])


def texture_gradients(shapes, tex_idx, uv, found, params_map, g, dtype):
    """dL/d texels of every texture from dL/d params_map `g` [n,S,P]: column tex_idx[i] of the field is params_map[..., tex_idx[i]] times the
    lookup, so the gradient is lookup^T (g[..., idx] * params_map[..., idx])."""
    g, pm = np.asarray(g, np.float64), np.asarray(params_map, np.float64)
    return [lookup_adjoint(s, uv, found, g[..., k] * pm[..., k], dtype) for s, k in zip(shapes, tex_idx)]


def check_texture_gradients(got, want, f32, report=print):
    """`pgc.check_param_gradients` per texture: its texels as the rows of one column."""
    from tests import param_grad_common as pgc
    return [pgc.check_param_gradients(np.asarray(a, np.float64).reshape(-1, 1), b.reshape(-1, 1), c.reshape(-1, 1), report) for a, b, c in zip(got, want, f32)]


def fair_uv(found, dists):
    """What a uv case has to show, from the oracle alone: at least a tenth of the in-patch samples find the mesh, and at least one does not."""
    inside = np.asarray(dists) > 0
    assert inside.sum() > 0 and found[inside].sum() * 10 >= inside.sum(), (int(inside.sum()), int(found.sum()))
    assert (~found[inside]).any(), "every in-patch sample finds the mesh: the reach is not tested"


def lookup_adjoint(shape, uv, found, g, dtype):
    """lookup^T g: the gradient of <texture_lookup(T), g> at the texels, on the CPU in `dtype` (torch autograd of the lookup; the lookup is
    affine in T, so the gradient does not depend on T)."""
    import torch
    from nerf_tex_amd.fit import texture_lookup
    T = torch.zeros(shape, dtype=dtype, requires_grad=True)
    val = texture_lookup(T, torch.as_tensor(np.asarray(uv), dtype=dtype), torch.as_tensor(np.asarray(found)))
    (val * torch.as_tensor(np.asarray(g), dtype=dtype)).sum().backward()
    return T.grad.numpy().astype(np.float64)
