"""A `ProposalTrainer` step against float64, without a device (tests/proposal_common.py has the statement; tests/test_gpu_proposal_step.py is
the GPU's side): on the restatement's own float32 ReLU patterns and on depths merged by the reference sampler, the four float32-vs-float64
comparisons the GPU test makes sit `pgc.MARGIN` times inside `clc.check_layers`' guards, the proposal network's colour layers are exactly zero
in float64, and the interlevel term is worth testing (max q >= 0.5, term > 0)."""

import numpy as np
import pytest
import torch

from tests import interlevel_common as ic
from tests import param_grad_common as pgc
from tests import proposal_common as pc
from tests.train_common import layer_slices, rel_linf


@pytest.mark.parametrize("setting", pc.SETTINGS, ids=pc.SETTING_IDS)
def test_the_settings_are_fair(setting):
    _, route, perturb, arch = setting
    (_, spec_p, wts_p), (_, spec_f, wts_f) = pc.pair(arch)
    batch, u = pc.the_batch(spec_p)
    z_prop, z_all = pc.cpu_depths((spec_p, wts_p), batch, perturb, u)
    n, S = z_all.shape
    assert (n, S) == (pc.N_RAYS, pc.S_PROP + pc.N_IMP) and S > 64 and np.isfinite(z_all).all() and (np.diff(z_all, axis=1) >= 0).all()
    assert all(np.isin(z_prop[r], z_all[r]).all() for r in range(n))
    patterns = pc.own_patterns(spec_p, wts_p, batch, z_prop), pc.own_patterns(spec_f, wts_f, batch, z_all)
    want_f, want_p = pc.restated_pair((spec_p, wts_p), (spec_f, wts_f), batch, z_prop, z_all, route, *patterns)
    f32_f, f32_p = pc.restated_pair((spec_p, wts_p), (spec_f, wts_f), batch, z_prop, z_all, route, *patterns, dtype=torch.float32)
    print(f"{setting[0]}: fine loss {want_f.loss:.9g} interlevel term {want_p.loss:.9g}")
    # the two values and the two predictions: float32 against float64, MARGIN times inside the bars the GPU test holds them to
    for name, a, b, bar in (("fine loss", f32_f.loss, want_f.loss, 1e-5), ("interlevel term", f32_p.loss, want_p.loss, 1e-5)):
        print(f"  {name}: float32 off by {abs(a - b) / abs(b):.2e}")
        assert abs(a - b) <= bar / pgc.MARGIN * abs(b), name
    for name, a, b in (("fine pred", f32_f.pred, want_f.pred), ("proposal pred", f32_p.pred, want_p.pred)):
        print(f"  {name}: float32 off by {rel_linf(a, b):.2e}")
        assert rel_linf(a, b) <= 1e-4 / pgc.MARGIN, name
    # the two gradients, layer by layer
    pc.fair(spec_f, want_f, f32_f)
    pc.fair(spec_p, want_p, f32_p, pc.density_slices(spec_p))
    colour = pc.colour_slices(spec_p)
    assert len(colour) >= 4 and len(colour) + len(pc.density_slices(spec_p)) == len(layer_slices(spec_p))
    assert all(not want_p.grad[sl].any() and not f32_p.grad[sl].any() for _, sl in colour), "the interlevel term reached a colour layer"
    assert all(want_f.grad[sl].any() for _, sl in layer_slices(spec_f))
    # an interlevel term worth testing, and the kernel's formula on these depths inside its guard
    ref = ic.reference(want_f.weights, z_all, want_p.weights, z_prop)
    assert ref[3].max() >= 0.5 and want_p.loss > 0
    assert abs(pc.LAMBDA * ref[0].mean() - want_p.loss) <= 1e-12 * want_p.loss                              # the dense statement is the formula
    w32 = [x.astype(ic.F) for x in (f32_f.weights, f32_p.weights)]
    want, f32 = ic.reference(w32[0], z_all, w32[1], z_prop), ic.reference(w32[0], z_all, w32[1], z_prop, dtype=ic.F)
    floors = [ic.rel_linf(f32[k], want[k]) for k in range(2)]
    print(f"  the kernel's floors on these inputs: per ray {floors[0]:.2e} d prop {floors[1]:.2e}")
    assert max(floors) <= ic.FLOOR_GUARD
