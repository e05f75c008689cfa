"""A `ProposalTrainer` step against float64 on the GPU (`nerf_tex_amd.train.ProposalTrainer`; tests/proposal_common.py has the statement and the
bars, tests/test_proposal_step.py holds the inputs inside the guards on the CPU).  `-m gpu`.

tests/test_gpu_ray_interlevel.py pins a step bit for bit to its own pieces done by hand; here the step is stated independently: the fine
network's step on the merged depths under the caller's loss, and the proposal network's under interlevel_weight * mean of the dense [n, S, S_p]
mask statement of the fine weights, both by float64 autograd on the ReLU patterns the two trainers kept.  24 rays, 40 + 30 samples: the
interlevel kernel on 70 depths that `ntx_sample_pdf` really merged."""

import numpy as np
import pytest
import torch

from tests import custom_loss_common as clc
from tests import distortion_common as dc
from tests import interlevel_common as ic
from tests import param_grad_common as pgc
from tests import proposal_common as pc
from tests.train_common import layer_slices, rel_linf, step_pred

pytestmark = pytest.mark.gpu


def patterns_of(tr, spec, n, S):
    """(masks, sigma_mask) of the pass a trainer has just taken, chain or layer by layer."""
    masks, _, sigma_mask = pgc.trainer_patterns(tr, spec, n, S, None) if hasattr(tr, "relu_widths") else clc.chain_patterns(tr, n, S, None)
    return masks, sigma_mask


@pytest.mark.parametrize("setting", pc.SETTINGS, ids=pc.SETTING_IDS)
def test_one_step_against_float64(setting):
    """The value within 1e-5 of the two losses' sum and `last_interlevel` within 1e-5 of the second one; both predictions at 1e-4; every layer of
    the fine network and the density-side layers of the proposal network by `clc.check_layers`; the proposal's colour layers exact zeros on
    both sides; and the kernel's per-ray loss and dL/d proposal weights, as the step called it, at `dc.gate` of the float64 reference on the
    step's own weights and merged depths."""
    from nerf_tex_amd.train import ProposalTrainer
    _, route, perturb, arch = setting
    (prop, spec_p, wts_p), (fine, spec_f, wts_f) = pc.pair(arch)
    batch, u = pc.the_batch(spec_p)
    ro, rd, t, cone, params, color, alpha = batch
    n, S, NI = pc.N_RAYS, pc.S_PROP, pc.N_IMP
    pt = ProposalTrainer(prop, fine, max_rays=n, n_samples=S, n_importance=NI, perturb=perturb, interlevel_weight=pc.LAMBDA)
    with pc.KernelCall() as kernel:
        val, cf, af, cp, ap = pt.gradients_step(ro, rd, t, params, cone, color, alpha, pc.product_loss(route), seed=pc.STEP_SEED, u=u)
    torch.cuda.synchronize()
    g_prop, g_fine = pt.coarse.gradients().copy(), pt.fine.gradients().copy()
    val, term = float(val.item()), float(pt.last_interlevel.item())
    # the depths are the product's, and constants
    z_prop_t = pt.coarse._sample_depths(torch.as_tensor(t, device=cf.device), pc.STEP_SEED, S)
    z_prop, z_all = z_prop_t.cpu().numpy(), pt.last_z.cpu().numpy()
    assert z_all.shape == (n, S + NI) and np.isfinite(z_all).all() and (np.diff(z_all, axis=1) >= 0).all()
    assert all(np.isin(z_prop[r], z_all[r]).all() for r in range(n))
    # the step, stated in float64 and in float32 on the patterns the two trainers kept
    patterns = patterns_of(pt.coarse, spec_p, n, S), patterns_of(pt.fine, spec_f, n, S + NI)
    want_f, want_p = pc.restated_pair((spec_p, wts_p), (spec_f, wts_f), batch, z_prop, z_all, route, *patterns)
    f32_f, f32_p = pc.restated_pair((spec_p, wts_p), (spec_f, wts_f), batch, z_prop, z_all, route, *patterns, dtype=torch.float32)
    total = want_f.loss + want_p.loss
    e_pred = rel_linf(step_pred(cf, af), want_f.pred), rel_linf(step_pred(cp, ap), want_p.pred)
    print(f"| {setting[0]} | value {val:.9g} want {total:.9g} rel {abs(val - total) / total:.2e} | interlevel term {term:.9g} want {want_p.loss:.9g} rel "
          f"{abs(term - want_p.loss) / want_p.loss:.2e} (float32 restatement {abs(f32_p.loss - want_p.loss) / want_p.loss:.2e}) | pred fine {e_pred[0]:.2e} proposal {e_pred[1]:.2e} |")
    assert abs(val - total) <= 1e-5 * total and abs(term - want_p.loss) <= 1e-5 * want_p.loss
    assert max(e_pred) <= 1e-4
    print("the fine network")
    clc.check_layers(g_fine, spec_f, want_f, f32_f)
    print("the proposal network, density side")
    pc.check_density_layers(g_prop, spec_p, want_p, f32_p)
    colour = pc.colour_slices(spec_p)
    assert len(colour) + len(pc.density_slices(spec_p)) == len(layer_slices(spec_p)) and len(colour) >= 4
    assert all(not g_prop[sl].any() and not want_p.grad[sl].any() for _, sl in colour), [(nm, float(np.abs(g_prop[sl]).max())) for nm, sl in colour]
    # the kernel, as the step called it, on depths the sampler merged
    assert len(kernel.calls) == 1
    call = kernel.calls[0]
    assert torch.equal(call.z_all, pt.last_z) and torch.equal(call.z_prop, z_prop_t) and torch.equal(call.out[0].sum().reshape(1), pt.last_interlevel)
    w_f, w_p = call.w_fine.cpu().numpy(), call.w_prop.cpu().numpy()
    scale = np.full(n, pc.LAMBDA / n, ic.F)
    assert np.array_equal(call.kw["ray_scale"].cpu().numpy(), scale) and rel_linf(w_f, want_f.weights) <= 1e-4 and rel_linf(w_p, want_p.weights) <= 1e-4
    ref, f32 = ic.reference(w_f, z_all, w_p, z_prop, scale), ic.reference(w_f, z_all, w_p, z_prop, scale, dtype=ic.F)
    assert ref[3].max() >= 0.5 and want_p.loss > 0, "an interlevel term worth testing"
    floors = tuple(ic.rel_linf(f32[k], ref[k]) for k in range(3))
    ic.held((call.out[0].cpu().numpy(), call.out[1].cpu().numpy(), None), ref, floors, f"{setting[0]}: the step's own kernel call")
    assert max(floors) <= dc.FLOOR_GUARD
