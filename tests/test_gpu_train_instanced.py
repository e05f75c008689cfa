"""The differentiable InstanceRenderer tail on the GPU (`ntx_train_forward_instanced` + `ntx_train_backward`, `FlexTrainer.forward_instanced`,
`nerf_tex_amd.autograd.DifferentiableInstanceRender`) against the float64 restatement of tests/instanced_train_common.py.  `-m gpu`."""

import ctypes as C

import numpy as np
import pytest

from tests import custom_loss_common as clc
from tests import instanced_train_common as itc
from tests import param_grad_common as pgc
from tests.train_common import BKGD, F, rel_linf
from tests.train_flex_common import n_relu

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dev():
    return torch.device("cuda", 0)


def make_trainer(case, model, n, S, mode=False, max_rays=None):
    from nerf_tex_amd import train
    kn = itc.knobs_of(case)
    return getattr(train, case[1])(model, max_rays=max_rays or n, n_samples=max(S, 2), perturb=False, blur_idx=case[4], map_exr=kn["map_exr"], param_gradients=mode)


def fkw(kn):
    return dict(patch_scale=itc.PATCH_SCALE, density_scale=kn["density_scale"], density_reweighting=kn["density_reweighting"], composite_bkgd=kn["composite_bkgd"], bkgd_color=BKGD)


def step(tr, bufs, hit, cone, kn, head, spoil=None):
    """forward_instanced, the head and its cotangents in torch on the device, backward.  `spoil`: rays whose cotangents are made NaN.
    Returns pred [n, 4], the weight gradient, the head's value."""
    c, a = tr.forward_instanced(bufs, cone, hit=hit.astype(np.uint8), **fkw(kn))
    cd, ad = c.detach().requires_grad_(True), a.detach().requires_grad_(True)
    val = head(cd, ad)
    dc, da = torch.autograd.grad(val, (cd, ad))
    if spoil is not None:
        dc, da = dc.clone(), da.clone()
        dc[spoil] = float("nan"); da[spoil] = float("nan")
    tr.backward(dc, da)
    torch.cuda.synchronize()
    return np.concatenate([c.cpu().numpy(), a.cpu().numpy()[:, None]], -1), tr.gradients(), float(val.item())


def patterns(tr, spec, bufs, hit, kn):
    """The ReLU patterns of the step the trainer has just taken, in compact row order (`activation`'s rows are the compact rows), and the sign
    of the scaled density.  The live order is computed on the host."""
    live = itc.live_order(hit, bufs[3])
    M = len(live)
    assert tr.last_live == M
    if M == 0:
        return dict(masks=[], branch_masks=None, sigma_mask=np.zeros(0, bool))
    masks = [tr.activation(k, M) > 0 for k in range(n_relu(spec))]
    branch = None
    if pgc.has_branches(spec):
        slots = ([32 + j for j in range(spec.param_layers)] if spec.n_geo > 0 else []) + ([48 + j for j in range(spec.param_layers)] if spec.n_app > 0 else [])
        branch = [tr.activation(k, M) > 0 for k in slots]
    sg = tr.activation(64, M)[:, 0]
    aw = bufs[6].reshape(-1)[live] if kn["density_reweighting"] else F(1)
    return dict(masks=masks, branch_masks=branch, sigma_mask=(sg * aw * F(kn["density_scale"])) > 0)


def restate_both(spec, w, bufs, hit, cone, okw, head, pat):
    want = itc.restated(w, spec, bufs, hit, cone, head, **okw, **pat)
    f32 = itc.restated(w, spec, bufs, hit, cone, head, dtype=torch.float32, **okw, **pat)
    return want, f32


def check_pred(got, want, f32, what=""):
    err, floor = rel_linf(got, want.pred), rel_linf(f32.pred, want.pred)
    print(f"{what} pred err {err:.2e} floor {floor:.2e}")
    assert err <= max(1e-4, 4 * floor), (err, floor)


def checked_step(setup, case=itc.CASES[0], mode=False):
    """A step on a fresh trainer, its predictions and every layer's gradient held to the restatement.  Returns what the callers go on with."""
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    tr = make_trainer(case, model, n, S, mode)
    head = itc.quadratic_head(n)
    pred, got, val = step(tr, bufs, hit, cone, kn, head)
    pat = patterns(tr, spec, bufs, hit, kn)
    want, f32 = restate_both(spec, w, bufs, hit, cone, okw, head, pat)
    print(f"{n} x {S}, {tr.last_live} live: loss {val:.9g} want {want.loss:.9g}")
    check_pred(pred, want, f32)
    assert np.all(pred[~hit] == 0)
    if tr.last_live > 0:
        clc.check_layers(got, spec, want, f32)
    return tr, pred, got, want, f32, head


def render_instanced(model, bufs, hit, cone, case, kn):
    """`ntx_render_instanced` on the same buffers: (color | alpha) [n, 4]."""
    from nerf_tex_amd import _lib
    n, S = bufs[3].shape
    d = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), device=dev()).to(dt).contiguous()
    t_ = [d(bufs[0]), d(bufs[1]), d(bufs[2]), d(bufs[3]), d(bufs[4].reshape(n, 3)), d(bufs[5].reshape(n)), d(bufs[6]) if kn["density_reweighting"] else None,
          d(bufs[7], torch.int32), d(hit, torch.uint8), d(bufs[9]), d(cone)]
    col = torch.full((n, 3), float("nan"), device=dev()); alp = torch.full((n,), float("nan"), device=dev())
    flags = (_lib.FLAG_MAP_EXR if kn["map_exr"] else 0) | (_lib.FLAG_COMPOSITE_BKGD if kn["composite_bkgd"] else 0)
    model.reserve(0, n)
    _lib.check(_lib.lib.ntx_render_instanced(model.ctx(0), *[None if x is None else x.data_ptr() for x in t_], n, S, -1 if case[4] is None else case[4], itc.PATCH_SCALE,
                                             kn["density_scale"], flags, _lib.f3(BKGD), None, None, col.data_ptr(), alp.data_ptr(), None, torch.cuda.current_stream(dev()).cuda_stream))
    torch.cuda.synchronize()
    return np.concatenate([col.cpu().numpy(), alp.cpu().numpy()[:, None]], -1)


# ---- 1, 2. predictions and every layer's weight gradient ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", itc.CASES, ids=itc.CASE_IDS)
def test_predictions_and_weight_gradients(case):
    """Predictions within max(1e-4, 4 float32 floors) of the restatement and of `ntx_render_instanced` on the same buffers; every layer's
    gradient within `check_layers`' bars of float64 autograd branched by the activations the trainer kept in compact row order.  The cases
    cover alpha_weight NULL, map_exr + background (an un-hit ray predicts 0 under it), blur_idx on a geometry and on an appearance parameter,
    a hit ray without a live sample, negative dists, and parameter branches."""
    setup = itc.case_setup(case)
    model, spec, w, bufs, hit, cone, kn, okw = setup
    assert (~hit).any() and (bufs[3][hit] < 0).any() and (~itc.live_mask(hit, bufs[3])[hit]).all(1).any()
    tr, pred, got, want, f32, _ = checked_step(setup, case)
    if not pgc.has_branches(spec):                         # (the render side takes parameter branches through another descriptor: the restatement holds them)
        rendered = render_instanced(model, bufs, hit, cone, case, kn)
        err, floor = rel_linf(pred, rendered), rel_linf(f32.pred, want.pred)
        print(f"against ntx_render_instanced: {err:.2e}")
        assert err <= max(1e-4, 4 * floor), (err, floor)


# ---- 3. edges ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edge", itc.EDGES, ids=itc.EDGE_IDS)
def test_sample_and_live_count_edges(edge):
    """S = 1, 64, 65, 130 (the composite's chunk of 64) and M' = 0, 1, 31, 32, 33, 2047, 2048, 2049 (a wave's rows, the weight gradients' range
    of 2048 rows) by an explicit live mask.  M' = 0: the predictions are the appended sample's alone and every weight gradient is exactly 0."""
    setup = itc.edge_setup(edge)
    tr, pred, got, want, f32, _ = checked_step(setup)
    if edge[1] == "live":
        assert tr.last_live == edge[2]
    if tr.last_live == 0:
        assert not got.any() and np.abs(want.grad).max() == 0


def test_a_ray_that_is_not_hit_takes_no_gradient_whatever_its_cotangent():
    """hit == 0 with positive dists and a NaN cotangent: the ray predicts 0, and every gradient is bit for bit the clean run's."""
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(itc.CASES[0])
    n, S = bufs[3].shape
    dead = np.nonzero(~hit)[0]
    assert len(dead) and (bufs[3][dead] > 0).any()
    tr = make_trainer(itc.CASES[0], model, n, S, mode=True)
    head = itc.quadratic_head(n)
    pred, got, _ = step(tr, bufs, hit, cone, kn, head)
    pg = tr.sample_parameter_gradients().cpu().numpy()
    pred2, got2, _ = step(tr, bufs, hit, cone, kn, head, spoil=torch.as_tensor(dead, device=dev()))
    pg2 = tr.sample_parameter_gradients().cpu().numpy()
    assert np.all(pred[dead] == 0) and np.array_equal(pred, pred2)
    assert np.isfinite(got2).all() and np.array_equal(got, got2) and np.array_equal(pg, pg2) and np.abs(got).max() > 0


def test_nothing_is_read_at_a_sample_that_is_not_live():
    """NaN in pts / rays_d_map / t / alpha_weight / params_map at every element that is not live: predictions, weight gradients and parameter
    gradients bit for bit the zero-filled run's."""
    case = itc.CASES[1]                                    # blur_idx on: t is read too
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    live = itc.live_mask(hit, bufs[3])

    def filled(value):
        out = list(bufs)
        for k in (0, 1, 2, 6, 9):
            b = out[k].copy()
            b[~live] = value
            out[k] = b
        return tuple(out)

    tr = make_trainer(case, model, n, S, mode=True)
    head = itc.quadratic_head(n)
    res = []
    for value in (0.0, np.nan):
        pred, got, _ = step(tr, filled(value), hit, cone, kn, head)
        res.append((pred, got, tr.sample_parameter_gradients().cpu().numpy()))
    assert all(np.isfinite(x).all() for x in res[1]) and np.abs(res[0][1]).max() > 0
    for a, b in zip(*res):
        assert np.array_equal(a, b)


# ---- 4. parameter gradients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [itc.CASES[0], itc.CASES[1], itc.CASES[2], itc.CASES[4]], ids=[itc.CASE_IDS[i] for i in (0, 1, 2, 4)])
def test_sample_parameter_gradients(case):
    """`sample_parameter_gradients()` [N, S, P] per column at `check_param_gradients`' bar against float64 autograd on params_map, exactly 0
    where the sample is not live; mode 1's weight gradients are bit for bit mode 0's; mode 2 leaves the gradient buffer untouched and gives
    the same parameter gradients.  One case has parameter branches (param_depth 2)."""
    setup = itc.case_setup(case)
    model, spec, w, bufs, hit, cone, kn, okw = setup
    n, S = bufs[3].shape
    P = sum(case[2])
    tr, pred, got, want, f32, head = checked_step(setup, case, mode=True)
    pg = tr.sample_parameter_gradients().cpu().numpy()
    assert pg.shape == (n, S, P)
    live = itc.live_mask(hit, bufs[3])
    assert np.all(pg[~live] == 0) and np.all(want.param_grad[~live] == 0)
    pgc.check_param_gradients(pg.reshape(-1, P), want.param_grad.reshape(-1, P), f32.param_grad.reshape(-1, P))
    tr.set_param_gradients(False)
    pred0, got0, _ = step(tr, bufs, hit, cone, kn, head)
    assert np.array_equal(got0, got) and np.array_equal(pred0, pred)
    tr.set_param_gradients("only")
    marker = np.arange(tr.n_weights, dtype=F)
    from nerf_tex_amd import _lib
    tr._set(_lib.TRAINER_GRADIENTS, marker)
    pred2, got2, _ = step(tr, bufs, hit, cone, kn, head)
    assert np.array_equal(got2, marker) and np.array_equal(pred2, pred)
    assert np.array_equal(tr.sample_parameter_gradients().cpu().numpy(), pg)


# ---- 5. capacity independence ------------------------------------------------------------------------------------------------------------------
def test_gradients_do_not_depend_on_the_capacity():
    """Two trainers of different max_rays: bit-identical predictions, weight gradients and parameter gradients on the same step, which is
    also reproducible on one of them."""
    case = itc.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case, n=40, S=70)        # 2800 samples, M' off 32
    n, S = bufs[3].shape
    head = itc.quadratic_head(n)
    res = []
    for cap in (n, n, 3 * n + 7):
        tr = make_trainer(case, model, n, S, mode=True, max_rays=cap) if not res or cap != n else tr
        pred, got, _ = step(tr, bufs, hit, cone, kn, head)
        res.append((pred, got, tr.sample_parameter_gradients().cpu().numpy()))
    assert np.abs(res[0][1]).max() > 0
    for other in res[1:]:
        for a, b in zip(res[0], other):
            assert np.array_equal(a, b)


# ---- 6. contract and error codes -----------------------------------------------------------------------------------------------------------------
def raw_args(bufs, hit_mask, cone_scale, **over):
    """The argument list of `ntx_train_forward_instanced` behind the handle, as device tensors (kept by the caller) and their pointers."""
    n, S = bufs[3].shape
    d = lambda a, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(a), device=dev()).to(dt).contiguous()
    keep = dict(rd=d(bufs[0]), pts=d(bufs[1]), t=d(bufs[2]), dists=d(bufs[3]), cl=d(bufs[4].reshape(n, 3)), al=d(bufs[5].reshape(n)), aw=d(bufs[6]), hit=d(hit_mask, torch.uint8),
                pm=d(bufs[9]), cone=d(cone_scale), color=torch.empty((n, 3), device=dev()), alpha=torch.empty(n, device=dev()))
    a = dict({k: v.data_ptr() for k, v in keep.items()}, n=n, S=S, blur=-1, patch_scale=itc.PATCH_SCALE, density_scale=1.0, flags=0)
    a.update(over)
    order = ("rd", "pts", "t", "dists", "cl", "al", "aw", "hit", "pm", "cone", "n", "S", "blur", "patch_scale", "density_scale", "flags")
    return keep, [a[k] for k in order] + [None, a["color"], a["alpha"], None, torch.cuda.current_stream(dev()).cuda_stream]


def test_contract_and_error_codes():
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import Trainer
    from tests.common import make_model
    from tests.train_flex_common import flex_batch
    lib, INV, UNS = _lib.lib, _lib.NTX_E_INVALID, _lib.NTX_E_UNSUPPORTED
    case = itc.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case, n=9, S=12)
    n, S = bufs[3].shape
    tr = make_trainer(case, model, n, S, mode=True)
    stream = torch.cuda.current_stream(dev()).cuda_stream
    ones = torch.ones((n, 3), device=dev())
    alive = []                                             # the buffers of every forward, kept to the end: a pending step reads them again

    def fwd(**over):
        kept, args = raw_args(bufs, hit, cone, **over)
        alive.append(kept)
        return lib.ntx_train_forward_instanced(tr._h, *args)
    back = lambda: lib.ntx_train_backward(tr._h, ones.data_ptr(), None, stream)
    # backward without a forward; one backward per forward; a NULL d_color leaves the step pending
    assert back() == INV
    keep, args = raw_args(bufs, hit, cone)
    assert lib.ntx_train_forward_instanced(tr._h, *args) == 0
    assert lib.ntx_train_backward(tr._h, None, None, stream) == INV and back() == 0 and back() == INV
    # each flag and size error
    for over in (dict(S=0), dict(S=1025), dict(n=n + 1), dict(n=0), dict(patch_scale=0.0), dict(patch_scale=-1.0), dict(blur=0, cone=None), dict(blur=0, t=None),
                 dict(blur=sum(case[2])), dict(flags=_lib.FLAG_PERTURB), dict(flags=_lib.FLAG_RAW_NOISE), dict(rd=None), dict(pts=None), dict(dists=None), dict(cl=None),
                 dict(al=None), dict(hit=None), dict(pm=None)):
        assert fwd(**over) == INV, over
        assert back() == INV, over                         # a refused forward leaves nothing pending
    assert fwd(aw=None) == 0 and fwd(t=None, cone=None) == 0 and back() == 0
    # n_rays * n_samples beyond the capacity although either fits
    big = itc.case_setup(case, n=9, S=13)
    keep2, args2 = raw_args(big[3], big[4], big[5])
    assert lib.ntx_train_forward_instanced(tr._h, *args2) == INV
    # the two parameter-gradient getters refuse each other's steps; either forward replaces the other's pending step
    ptr, i64, i0, i1 = C.c_void_p(), C.c_int64(), C.c_int(), C.c_int()
    plain = lambda: lib.ntx_trainer_param_gradients(tr._h, C.byref(ptr), C.byref(i64), C.byref(i0))
    sample = lambda: lib.ntx_trainer_sample_param_gradients(tr._h, C.byref(ptr), C.byref(i64), C.byref(i0), C.byref(i1))
    assert sample() == 0 and (i64.value, i0.value, i1.value) == (n, S, sum(case[2])) and plain() == INV
    ro, rd, t, cone_p, params, _, _ = flex_batch(3, n, S, spec, "carpet")
    tr.forward_instanced(bufs, cone, hit=hit, **fkw(kn))
    c, a = tr.forward(ro, rd, t, params, cone_p)           # replaces the pending instanced step: the backward is the plain one
    tr.backward(torch.ones_like(c))
    assert plain() == 0 and sample() == INV
    tr.forward(ro, rd, t, params, cone_p)
    c, a = tr.forward_instanced(bufs, cone, hit=hit, **fkw(kn))
    tr.backward(torch.ones_like(c))
    assert sample() == 0 and plain() == INV
    tr.set_param_gradients(False)
    assert sample() == INV and plain() == INV
    torch.cuda.synchronize()
    # a handle of ntx_trainer_create: the message names the layer-by-layer entries
    chain_model, _, _ = make_model((1, 6), dense_media=True)
    chain = Trainer(chain_model, max_rays=n, n_samples=S, perturb=False)
    assert lib.ntx_train_forward_instanced(chain._h, *args) == UNS
    assert b"ntx_trainer_create_flex" in lib.ntx_last_error()


# ---- 7. the autograd op ------------------------------------------------------------------------------------------------------------------------------
def test_differentiable_instance_render():
    """A torch loss plus a regulariser on params_map: `.grad` is the native per-sample term plus the regulariser's own; the weight gradient is
    the plain pair's; a second backward raises; params_map.requires_grad without param_gradients raises ValueError."""
    from nerf_tex_amd.autograd import DifferentiableInstanceRender
    case = itc.CASES[0]
    model, spec, w, bufs, hit, cone, kn, okw = itc.case_setup(case)
    n, S = bufs[3].shape
    tr = make_trainer(case, model, n, S, mode=True)
    head = itc.quadratic_head(n)
    pred, got, val = step(tr, bufs, hit, cone, kn, head)
    native = tr.sample_parameter_gradients()
    render = DifferentiableInstanceRender(tr, itc.PATCH_SCALE, density_scale=kn["density_scale"], density_reweighting=kn["density_reweighting"])
    regulariser = lambda p: 0.01 * (p ** 2).sum() + 0.003 * p.sum()
    field = torch.tensor(bufs[9], device=dev(), requires_grad=True)
    c, a = render(bufs, cone, params_map=field, hit=hit, composite_bkgd=kn["composite_bkgd"], bkgd_color=BKGD)
    assert c.requires_grad and a.requires_grad and tr.last_live == len(itc.live_order(hit, bufs[3]))
    total = head(c, a) + regulariser(field)
    total.backward(retain_graph=True)
    torch.cuda.synchronize()
    leaf = torch.tensor(bufs[9], device=dev(), requires_grad=True)
    own, = torch.autograd.grad(regulariser(leaf), leaf)
    assert field.grad.shape == (n, S, sum(case[2])) and native.abs().max() > 0
    assert torch.equal(field.grad, native + own) and np.array_equal(tr.gradients(), got)
    assert np.array_equal(np.concatenate([c.detach().cpu().numpy(), a.detach().cpu().numpy()[:, None]], -1), pred)
    with pytest.raises(RuntimeError):
        total.backward()
    tr.set_param_gradients(False)
    with pytest.raises(ValueError):
        render(bufs, cone, params_map=torch.tensor(bufs[9], device=dev(), requires_grad=True), hit=hit)
    c, a = render(bufs, cone, hit=hit)                     # params_map from the tuple, no gradient to it: the weights' alone
    head(c, a).backward()
    torch.cuda.synchronize()
    assert np.array_equal(tr.gradients(), got)
