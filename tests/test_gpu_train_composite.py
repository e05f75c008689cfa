"""`composite_loss_kernel` (csrc/ntx_trainer.hip) on its own: the kernel every training step of every trainer runs -- the composite of a ray,
the ray's term of the loss, and the hand-written adjoint the whole way back starts from -- over every loss setting, both colour maps, the
background term, the density regulariser, the chunks of 64 samples its scans work in up to the 1024 samples a ray may have, rays that miss
the proxy, the weights it hands the importance sampler, and Adam away from a run's first steps.  `-m gpu`.

The kernel is isolated with what the handle already offers: `ntx_trainer_activation` 11 / 10 are the raw colour and density the step's own
network produced, 30 the adjoint the kernel made of them; float64 autograd of the composite and the loss alone on those SAME float32 values
(`tro.composite_gradients`, proved against finite differences in tests/test_oracle_train.py) is what it is held to, so the network's rounding
stays out.  One 8 x 256 trainer per family is made for 16 rays x 1024 samples and serves every case; a regime (thin, saturated, raw colours
either side of 0) is steered by the head biases -- raised, not scaled, as tests/test_gpu_train.py test_saturated_rays_keep_their_gradient has it --
and asserted on what the step predicted before anything else is.

The bars are the project's (test_saturated_rays_keep_their_gradient): dL/d raw colour within 5e-6 and dL/d raw density within 5e-5 rel-Linf
over the batch, loss and predictions within 1e-5.  A case named in FLOOR_GATED is held to four times what float32 torch autograd of the same
composite makes of the same inputs instead (check_gradients' convention); profiles/train_composite/adjoint_errors.md has every case's figures.
And ray by ray: a hit ray's adjoint relative to THAT ray's largest float64 entry within four times the batch's bar, for every ray whose largest
entry is at least 1e-3 of the batch's -- the oracle alone decides which, and no case may leave out more than a quarter of its hit rays."""

from types import SimpleNamespace

import numpy as np
import pytest

from oracle import nerftex_oracle as orc
from oracle import train_oracle as tro
from tests.common import make_model
from tests.train_common import BKGD, LOSSES, adjoint_errors, layer_slices, make_loss, raw_outputs, rel_linf, restated_step, step_depths, step_noise, step_pred

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = np.float32
CAP_RAYS, CAP_S = 16, 1024                                                        # 16 384 samples: a few MB a layer
GATES = dict(drgb=5e-6, dsigma=5e-5)                                               # test_saturated_rays_keep_their_gradient's
# case label -> the adjoints ("drgb", "dsigma") held to 4 x the float32 floor measured beside them instead of GATES
# (profiles/train_composite/adjoint_errors.md).  Thin rays of 256 samples and more: a sample's opacity 1 - exp(-sigma dist) is 1e-3 .. 1e-2 and
# its float32 value carries the exponential's half ulp, 3e-8, as 3e-6 .. 3e-5 of itself -- in the kernel as in torch; the colour adjoint w dC rgb'
# is proportional to it sample by sample.
FLOOR_GATED = {"edge S256 thin exr0": ("drgb",), "edge S1023 thin exr0": ("drgb",), "edge S1024 thin exr1": ("drgb",)}
# (loss, flags) -> the jitter and noise seed of a test_loss_options case whose default one (31 + k) gives a batch on which float32 torch autograd
# of the restated step, branched like float64, is ITSELF 1.0e-4 / 1.7e-4 from float64 in alpha.bias (455 samples' dL/dsigma cancel to a
# fraction of their terms): the first of 131 + k, 231 + k on which it is within half the end-to-end bar in every layer (3.1e-5, 4.4e-5) --
# the seed changes, not the bar (tests/train_flex_common.py check_against_float64)
JITTER = {("alpha_mse_unfiltered", (False, True)): 135, ("alpha_smape_smape", (True, True)): 238}
# A regime: (the density head's weights, the shift of alpha.bias, the shift of color.bias).  "dense": tests.common.make_model's dense_media
# head (scaled x32: sigma -18 .. 6 along the carpet family's rays, one sample in eight above 0); "plain": the unscaled head (sigma -0.3 .. 0.4).
# The raw colours of both lie in -0.9 .. 0: color.bias + 0.45 puts a good third of them above 0, where elu + 1 takes its other branch.
REGIMES = dict(mixed=("dense", 2.0, 0.45),             # alpha_pred 0.03 .. 0.97 over the rays
               thin=("plain", 0.3, 0.45),              # sigma -0.1 .. 0.7: nine samples in ten contribute, alpha_pred 0.2 .. 0.75
               saturated=("dense", 10.0, 0.45),        # most rays end opaque, the others at 0.99 .. 0.9999
               saturated_S2=("dense", 12.0, 0.45))     # (two samples a ray: the same at + 12)
EDGES = [2, 3, 63, 64, 65, 127, 128, 129, 256, 257, 1023, 1024]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]               # (map_exr, background)


def dev():
    return torch.device("cuda", 0)


def ray_batch(n, seed, fam="carpet", ipe=False):
    """Rays of a family's box (all hit) with per-ray parameters and seeded targets: colours in (0.05, 1), alpha targets strictly inside (0, 1)
    but for ONE ray's 0 -- the masks of AlphaLoss take their other branch on it, and a hard-masked ray is the only one a case may have to
    leave out of the ray-by-ray colour check."""
    from nerf_tex_amd import synthetic
    from tests.train_common import mip_batch
    rng = np.random.default_rng(1000 + seed)
    if ipe:
        ro, rd, t, cone, params = mip_batch(n, 5, seed=seed)
    else:
        f = synthetic.FAMILIES[fam]
        ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"], seed=seed + 1)
        params = (np.asarray([f["params"]], F) * rng.uniform(0.8, 1.2, size=(n, len(f["params"])))).astype(F)
    color = rng.uniform(0.05, 1, size=(n, 3)).astype(F)
    alpha = rng.uniform(0.3, 0.95, size=n).astype(F)
    alpha[n // 2] = 0
    return ro, rd, t, cone, params, color, alpha


def regime_blob(h, regime):
    head, alpha_shift, color_shift = REGIMES[regime]
    blob = h.blobs[head].copy()
    sl = dict(layer_slices(h.spec))
    blob[sl["alpha.bias"]] += F(alpha_shift); blob[sl["color.bias"]] += F(color_shift)
    return blob


def head_blobs(npar, kind):
    kw = dict(kind=kind) if kind else {}
    return {head: np.asarray(make_model(npar, dense_media=head == "dense", **kw)[0].get_blob(), F).reshape(-1).copy() for head in ("dense", "plain")}


@pytest.fixture(scope="module")
def chain():
    """The one Fourier chain trainer of this module: 16 rays x 1024 samples; a case sets its weights, map_exr and noise."""
    from nerf_tex_amd.train import Trainer
    model, spec, _ = make_model((1, 6), dense_media=True)
    return SimpleNamespace(tr=Trainer(model, max_rays=CAP_RAYS, n_samples=CAP_S, perturb=True), spec=spec, blobs=head_blobs((1, 6), None), blur=None, ipe=False)


@pytest.fixture(scope="module")
def mip():
    """The one IPE trainer: the blur parameter in the middle of the row (slot 2 of 5)."""
    from nerf_tex_amd.train import Trainer
    model, spec, _ = make_model((1, 3), kind="IPE", dense_media=True)
    return SimpleNamespace(tr=Trainer(model, max_rays=CAP_RAYS, n_samples=CAP_S, perturb=True, blur_idx=2), spec=spec, blobs=head_blobs((1, 3), "IPE"), blur=2, ipe=True)


def take_step(h, batch, S, loss_name, *, map_exr=False, bkgd=False, noise_std=0.0, regime="mixed", seed=11, miss=None):
    """One `gradients_step` of the shared trainer at `S` samples a ray with the regime's weights; returns what the checks need."""
    ro, rd, t, cone, params, color, alpha = batch
    n = len(t)
    miss = np.zeros(n, bool) if miss is None else np.asarray(miss, bool)
    t = t.copy(); t[miss] = np.inf
    cone = cone.copy(); cone[miss] = np.nan                                       # whatever a ray sampler leaves there
    tr = h.tr
    blob = regime_blob(h, regime)
    tr.set_weights(blob)
    tr.map_exr, tr.raw_noise_std = bool(map_exr), float(noise_std)
    okw, loss = make_loss(loss_name)
    val, cp, ap = tr.gradients_step(ro, rd, t, params, cone, color, alpha, loss, composite_bkgd=bkgd, bkgd_color=BKGD, seed=seed, n_samples=S)
    torch.cuda.synchronize()
    z, noise = step_depths(t, S + 1 if h.ipe else S, seed, True, miss), step_noise(n, S, seed, noise_std)
    return SimpleNamespace(h=h, tr=tr, n=n, S=S, okw=okw, loss_name=loss_name, val=float(val.item()), pred=step_pred(cp, ap), z=z, noise=noise, miss=miss, t=t, cone=cone,
                           batch=batch, wts=orc.split_blob(h.spec, blob), map_exr=map_exr, bkgd=bkgd, noise_std=noise_std, seed=seed)


def check_regime(st, regime):
    """The batch is what its name says, by what the step itself predicted and kept."""
    hit = ~st.miss
    ap = st.pred[hit, 3]
    if regime == "saturated":
        assert (ap > 0.99999).sum() >= hit.sum() / 4, ap
    if regime == "thin":
        assert ap.max() < 0.9 and ap.max() > 0.05, ap
    if st.map_exr:
        raw = raw_outputs(st.tr, st.n, st.S)[0][hit]
        assert (raw > 0).mean() >= 0.1 and (raw < 0).mean() >= 0.1, ((raw > 0).mean(), (raw < 0).mean())
    if st.okw.get("use_hard_mask") is False:
        at = st.batch[6]
        assert (at == 0).any() and ((at > 0) & (at < 1)).any()


def check_composite(st, label):
    """Loss, predictions and the adjoint of the step `st` against float64 on the step's own raw outputs; one markdown row of figures first."""
    rd, color, alpha = st.batch[1], st.batch[5], st.batch[6]
    e = adjoint_errors(st.tr, rd, st.z, color, alpha, st.okw, map_exr=st.map_exr, bkgd=st.bkgd, bkgd_color=BKGD, noise=st.noise, miss=st.miss, floors=True)
    n_hit = int((~st.miss).sum())
    e_loss, e_pred = abs(st.val - e["loss"]) / (abs(e["loss"]) + 1e-7), rel_linf(st.pred, e["pred"])
    floored = FLOOR_GATED.get(label, ())
    print(f"| {label} | {e['e_drgb']:.2e} | {e['f_drgb']:.2e} | {e['e_dsigma']:.2e} | {e['f_dsigma']:.2e} | {np.nanmax(e['ray_drgb']):.2e} | {np.nanmax(e['f_ray_drgb']):.2e} | "
          f"{np.nanmax(e['ray_dsigma']):.2e} | {np.nanmax(e['f_ray_dsigma']):.2e} | {e['left_out']}/{n_hit} | {e_loss:.2e} | {e_pred:.2e} | {' '.join(floored) or '-'} |")
    assert np.isfinite(e["adj"]).all() and np.isfinite(st.pred).all() and np.isfinite(st.val)
    assert np.abs(e["want"][..., :3]).max() > 1e-8 and np.abs(e["want"][..., 3]).max() > 1e-8                 # a gradient worth the name, both ways
    assert 4 * e["left_out"] <= n_hit, (e["ray_drgb"], e["ray_dsigma"])                                       # (a condition on the batch, not on the kernel)
    assert e_loss <= 1e-5 and e_pred <= 1e-5, (e_loss, e_pred)
    for key in ("drgb", "dsigma"):
        gate = 4 * e["f_" + key] if key in floored else GATES[key]
        assert e["e_" + key] <= gate, (label, key, e["e_" + key], gate, e["f_" + key])
        assert np.nanmax(e["ray_" + key]) <= 4 * gate, (label, key, e["ray_" + key], gate, e["f_ray_" + key])
    # where the oracle's colour adjoint of a ray is exactly 0 (a masked ray) so is the kernel's: nothing was formed as a difference
    zero = ~st.miss & (np.abs(e["want"][..., :3]).max((1, 2)) == 0)
    assert (e["adj"][zero][..., :3] == 0).all()
    return e


def check_end_to_end(st, label, gate_layers=1e-4):
    """The whole step against the restated one (tests/train_common.py restated_step), at check_gradients' bars."""
    ro, rd, _, _, params, color, alpha = st.batch
    want = restated_step(st.tr, st.h.spec, st.wts, ro, rd, st.t, params, st.cone, color, alpha, st.okw, seed=st.seed, perturb=True, noise_std=st.noise_std, miss=st.miss,
                         blur_idx=st.h.blur, bkgd=st.bkgd, bkgd_color=BKGD, S=st.S, map_exr=st.map_exr)
    assert np.array_equal(want.z, st.z, equal_nan=True)
    worst = max(want.layers, key=want.layers.get)
    e_loss, e_pred = abs(st.val - want.loss) / (abs(want.loss) + 1e-7), rel_linf(st.pred, want.pred)
    print(f"| {label} end to end | loss {e_loss:.1e} | pred {e_pred:.1e} | worst layer {worst} {want.layers[worst]:.1e} | gate {gate_layers:.1e} | max grad {np.abs(want.grad).max():.1e} |")
    tiny = 5.0 if st.n * st.S < 100 else 1.0                                       # check_gradients: a handful of coarse steps, nothing averages out
    assert np.isfinite(want.got).all() and np.abs(want.grad).max() > 1e-6
    assert e_loss <= (1e-5 if st.n * st.S >= 1000 else 1e-4) * tiny and e_pred <= 1e-4 * tiny, (e_loss, e_pred)
    assert max(want.layers.values()) <= gate_layers * tiny, {k: v for k, v in want.layers.items() if v > 1e-5}
    return want


# ---- 1. every loss setting x colour map x background ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS, ids=lambda f: f"exr{int(f[0])}_bk{int(f[1])}")
@pytest.mark.parametrize("loss_name", sorted(LOSSES))
def test_loss_options(chain, loss_name, flags):
    """7 rays (two workgroups of four waves, the second with one idle) x 65 samples (one lane of a second chunk), jittered, every other case
    under the density regulariser: the loss, the predictions and the adjoint alone, and every layer's gradient end to end at 1e-4."""
    map_exr, bkgd = flags
    k = sorted(LOSSES).index(loss_name) + FLAGS.index(flags)
    label = f"loss {loss_name} exr{int(map_exr)} bk{int(bkgd)}"
    st = take_step(chain, ray_batch(7, 21), 65, loss_name, map_exr=map_exr, bkgd=bkgd, noise_std=0.1 if k % 2 else 0.0, regime="mixed", seed=JITTER.get((loss_name, flags), 31 + k))
    check_regime(st, "mixed")
    check_composite(st, label)
    check_end_to_end(st, label)


# ---- 2. the chunks of the scans -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["thin", "saturated"])
@pytest.mark.parametrize("S", EDGES)
def test_chunk_edges(chain, S, regime):
    """Sample counts either side of every chunk of 64 the forward product and the reverse suffix scan work in, from 2 to the 1024 a ray may
    have (16 chunks, 15 carries back to front): thin rays, whose every sample matters, and rays that end opaque, whose gradient hangs on the
    transmittance the scan carried.  AlphaLoss(smape) as written -- smape on alpha too -- over the background, elu + 1 on every other count.
    End to end up to 257 samples (beyond, float64 autograd of the network only costs time): the plain 1e-4 plus the float32 network's own
    rounding of sigma through the exponential, 1e-5 sigma dist, as test_saturated_rays_keep_their_gradient has it."""
    map_exr = EDGES.index(S) % 2 == 1
    label = f"edge S{S} {regime} exr{int(map_exr)}"
    st = take_step(chain, ray_batch(5, 40 + S), S, "alpha_smape_smape", map_exr=map_exr, bkgd=True, regime=regime + "_S2" * (S == 2 and regime == "saturated"), seed=S)
    check_regime(st, regime)
    check_composite(st, label)
    if S <= 257:
        sigma = raw_outputs(st.tr, st.n, S)[1]
        dist = np.diff(st.z, axis=-1); dist = np.concatenate([dist, dist[:, -1:]], -1)
        check_end_to_end(st, label, 1e-4 + 1e-5 * float((np.maximum(sigma, 0) * dist).max()))


# ---- 3. rays that miss the proxy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_std", [0.0, 0.1])
@pytest.mark.parametrize("map_exr", [False, True])
def test_rays_that_miss(chain, map_exr, noise_std):
    """Rays 1 and 4 of 6 at t = inf (cone_scale NaN): their rows of the adjoint are exactly 0 -- not a rounding of it, not NaN --, they predict
    the background (0 without one) with alpha 0, the other rays' adjoint is the oracle's share of the batch, and the loss is the oracle's over
    all six.  Ray 1's targets are the background and alpha 0: every error of its term is exactly 0 and smape's sign takes its third branch.
    Then the same exactness where the prediction is not masked away: NerfLoss(smape) on six missed rays whose targets ARE the background
    has loss 0.0 and an all-zero adjoint."""
    batch = ray_batch(6, 5)
    color, alpha = batch[5].copy(), batch[6].copy()
    miss = np.zeros(6, bool); miss[[1, 4]] = True
    color[1], alpha[1], alpha[4], alpha[3] = BKGD, 0.0, 0.6, 0.45                  # (ray_batch's own zero sat on ray 3: ray 1 has it now)
    batch = batch[:5] + (color, alpha)
    label = f"miss exr{int(map_exr)} noise{noise_std}"
    for bkgd in (True, False):
        st = take_step(chain, batch, 65, "alpha_smape_smape", map_exr=map_exr, bkgd=bkgd, noise_std=noise_std, regime="mixed", seed=3, miss=miss)
        check_regime(st, "mixed")
        e = check_composite(st, f"{label} bk{int(bkgd)}")
        assert (e["adj"][miss] == 0).all() and np.abs(e["adj"][~miss]).max() > 0
        assert (st.pred[miss, 3] == 0).all() and (st.pred[miss, :3] == (np.asarray(BKGD, F) if bkgd else 0)).all()
    everything = np.ones(6, bool)
    targets = np.tile(np.asarray(BKGD, F), (6, 1))
    st = take_step(chain, batch[:5] + (targets, alpha), 65, "nerf_smape", map_exr=map_exr, bkgd=True, noise_std=noise_std, regime="mixed", seed=3, miss=everything)
    adj = st.tr.activation(30, 6 * 65)
    assert st.val == 0.0 and (adj == 0).all() and (st.pred == np.asarray(BKGD + (0.0,), F)).all()


# ---- 4. the weights handed to the importance sampler --------------------------------------------------------------------------
@pytest.mark.parametrize("regime", ["thin", "saturated"])
@pytest.mark.parametrize("S", [2, 64, 65, 1024])
def test_composite_weights(chain, S, regime):
    """`ntx_trainer_composite_weights`: the [N, S] weights a_i T_i a step leaves in a registered device buffer against the float64 composite of
    the step's own raw outputs, at the bar tests/test_gpu_standalone_edges.py test_composite_chunk_edges holds `ntx_composite`'s weights to (1e-5
    absolute); nothing behind the last ray's last sample is written, and nothing at all once the buffer is taken back."""
    from nerf_tex_amd import _lib
    n, tr = 5, chain.tr
    buf = torch.full((CAP_RAYS * CAP_S,), -7.0, device=dev())
    _lib.check(_lib.lib.ntx_trainer_composite_weights(tr._h, buf.data_ptr()))
    try:
        st = take_step(chain, ray_batch(n, 70 + S), S, "alpha_smape_smape", map_exr=S == 65, bkgd=True, regime=regime + "_S2" * (S == 2 and regime == "saturated"), seed=S)
    finally:
        _lib.check(_lib.lib.ntx_trainer_composite_weights(tr._h, None))
    check_regime(st, regime)
    got = buf.cpu().numpy()
    raw, sigma = raw_outputs(tr, n, S)
    c, a, w, _ = orc.map_model_output(raw, sigma, st.z, st.batch[1], True, BKGD, st.map_exr, None, np.float64)
    f32 = orc.map_model_output(raw, sigma, st.z, st.batch[1], True, BKGD, st.map_exr, None, np.float32)[2]
    err, floor = float(np.abs(got[:n * S].reshape(n, S) - w).max()), float(np.abs(f32 - w).max())
    print(f"| weights S{S} {regime} | {err:.1e} | {floor:.1e} | sum {np.abs(got[:n * S].reshape(n, S).sum(1) - a).max():.1e} |")
    assert (got[n * S:] == -7.0).all() and w.sum(1).max() > 0.05
    assert err <= 1e-5, (err, floor)
    assert np.abs(got[:n * S].reshape(n, S).sum(1) - st.pred[:, 3]).max() <= 1e-5                          # they are the weights alpha_pred was summed from
    buf.fill_(-7.0)
    take_step(chain, ray_batch(n, 70 + S), S, "alpha_smape_smape", bkgd=True, regime=regime, seed=S)
    assert (buf == -7.0).all()


# ---- 5. the other handles ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [2, 64, 65, 1024])
def test_mip_adjoint(mip, S):
    """The same kernel behind an IPE trainer: a sample's length is its cone segment's (renderer.py:441-444), S segments between S + 1 edges, no
    copy of the last one.  The adjoint alone, through `tro.composite_gradients(mip=True)`."""
    regime = {2: "thin", 64: "mixed", 65: "thin", 1024: "mixed"}[S]               # (the IPE model's "mixed" rays end at alpha_pred 0.9987 .. 1)
    label = f"mip S{S} {regime}"
    st = take_step(mip, ray_batch(5, 90 + S, ipe=True), S, "alpha_smape_smape", map_exr=S in (64, 1024), bkgd=True, noise_std=0.1 if S in (2, 64) else 0.0, regime=regime, seed=S)
    assert st.z.shape == (5, S + 1)
    check_regime(st, regime)
    check_composite(st, label)


@pytest.mark.parametrize("loss_name", ["alpha_smape_smape", "alpha_mse_unfiltered"])
def test_layer_by_layer_trainer(loss_name):
    """The composite behind a `FlexTrainer` (color_depth 2, one of tests/test_gpu_train_flex.py's architectures) with elu + 1 and the two loss
    settings furthest from the shipped one, through that module's `one_step` at its own gates."""
    from tests import test_gpu_train_flex as flex
    arch_id, npar, kind, arch, fam = [a for a in flex.ARCHS if a[0] == "color_depth2"][0]
    model, spec, wts = make_model(npar, kind=kind, dense_media=True, arch=arch)
    flex.one_step(model, spec, wts, fam, 45, 37, loss_name, map_exr=True, bkgd=True, perturb=True)


@pytest.mark.parametrize("loss_name", ["alpha_smape_smape", "alpha_mse_unfiltered"])
def test_branch_trainer(loss_name):
    """And behind a `BranchTrainer` (case e of tests/train_branch_oracle.py GPU_CASES, which trains with elu + 1), through
    tests/test_gpu_train_branches.py's `one_step` at its own gates."""
    from tests import test_gpu_train_branches as branches
    from tests import train_branch_oracle as bro
    case = [c for c in bro.GPU_CASES if c[0] == "e_geometry_only"][0]
    model, spec, wts, batch, kn, seed = bro.case_setup(case)
    assert kn["map_exr"]
    branches.one_step(model, spec, wts, batch, bro.N_RAYS, bro.N_SAMPLES, seed=seed, **dict(kn, loss_name=loss_name, bkgd=True))


# ---- 6. Adam away from the first steps --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hyper", [dict(), dict(beta_1=0.5, beta_2=0.9, epsilon=1e-3)], ids=["keras_defaults", "other_betas"])
@pytest.mark.parametrize("lrate_decay", [500, 0])
def test_adam_at_the_iterations_of_a_resumed_run(lrate_decay, hyper):
    """`ntx_trainer_adam_step` at the iteration counts a resumed run has (`ntx_trainer_set_iterations`): the bias correction and the
    ExponentialDecay rate are formed on the host from the count.  Weights, gradient and both moments are set, one `apply_gradients` is compared
    with `tro.adam_step` by the three assertions of test_training_step_is_bit_reproducible_and_adam_matches_its_restatement, and the count
    advances by one.  The gradient holds exact zeros: on zero moments (the weight stays, bit for bit) and on moments that still move it."""
    from nerf_tex_amd import _lib
    from nerf_tex_amd.train import FlexTrainer
    model, spec, _ = make_model((1, 6), arch=dict(depth=2, width=16, skips=[]))
    tr = FlexTrainer(model, max_rays=4, n_samples=4, lrate=5e-4, lrate_decay=lrate_decay, **hyper)
    p = tr.n_weights
    rng = np.random.default_rng(p)
    w = np.asarray(model.get_blob(), F).reshape(-1).copy()
    g = (rng.normal(size=p) * 10.0 ** rng.uniform(-5, -1, size=p)).astype(F)
    v = (g.astype(np.float64) ** 2 * rng.uniform(0.2, 5, size=p)).astype(F)
    m = (rng.normal(size=p) * np.sqrt(v)).astype(F)                               # a step of the size of the rate, over four decades of gradient
    fresh, still, coasting = np.arange(p) % 7 == 0, np.arange(p) % 7 == 1, np.arange(p) % 7 == 2
    m[fresh | still] = 0; v[fresh | still] = 0                                    # a first step's moments; `still`: and no gradient either
    g[still | coasting] = 0                                                       # `coasting`: no gradient, the moments go on moving the weight
    assert p < 5000 and (g == 0).sum() > p // 4 and ((g == 0) & (m != 0)).any() and ((g != 0) & (v == 0)).any()
    for it in (0, 1, 9, 1000, 500000):
        tr.load_state_dict(dict(weights=w, adam_m=m, adam_v=v, iterations=it))
        tr._set(_lib.TRAINER_GRADIENTS, g)
        assert tr.iterations == it and np.array_equal(tr.gradients(), g)
        tr.apply_gradients()
        torch.cuda.synchronize()
        wa, (ma, va) = tr.weights(), tr.adam_state()
        assert tr.iterations == it + 1
        ww, mm, vv = tro.adam_step(w, g, m, v, it, 5e-4, decay_steps=lrate_decay * 1e3, decay_rate=0.1, **hyper)
        g64, mb64, vb64 = g.astype(np.float64), m.astype(np.float64), v.astype(np.float64)
        assert (np.abs(ma - mm) <= 4e-7 * (np.abs(g64) + np.abs(mb64)) + 1e-30).all()                  # float32 rounding of m + (g - m)(1 - beta_1)
        assert (np.abs(va - vv) <= 4e-7 * (g64 * g64 + vb64) + 1e-38).all()
        step = ww - w.astype(np.float64)
        assert (np.abs(wa.astype(np.float64) - ww) <= 1.01 * np.spacing(np.abs(wa)) + 1e-6 * np.abs(step)).all(), it   # the updated weight, to its last place
        assert np.abs(step).max() > 1e-5
        assert np.array_equal(wa[still], w[still]) and (ma[still] == 0).all() and (va[still] == 0).all() and not np.array_equal(wa[coasting], w[coasting])
