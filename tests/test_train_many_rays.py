"""Training steps of more than 1024 rays, what can be said without a GPU: every fixture of tests/test_gpu_train_many_rays.py is built and held
to the conditions that keep a pass from being hollow -- the random instancer buffers hold rays that are not hit, hit rays without a live
sample, negative dists, scan ranges with and without live samples; an explicit live mask is what its name says and has a live sample inside
the medium; every layer (and, where the GPU test reads them, every column of the per-sample, per-row and per-ray gradients) has a gradient
worth the name and a float32 floor within 5e-4, measured by float32 autograd of the same restatement on its own ReLU patterns.  A seed is changed
here, not on the GPU machine.  No GPU."""

import numpy as np
import pytest

from tests import input_grad_common as igc
from tests import instanced_train_common as itc
from tests import many_rays_common as mrc
from tests import param_grad_common as pgc

torch = pytest.importorskip("torch")


def test_the_scan_ranges_of_the_sizes():
    """What the sizes are there for: rays per scan thread, non-empty ranges, the last range's rays, threads whose first ray is n_rays."""
    seen = {}
    for n in mrc.INST_SIZES:
        per = mrc.per_of(n)
        ranges = -(-n // per)
        seen[n] = (per, ranges, n - (ranges - 1) * per, ranges < 1024 and ranges * per == n)
    assert seen == {1023: (1, 1023, 1, True), 1024: (1, 1024, 1, False), 1025: (2, 513, 1, False), 2049: (3, 683, 3, True), 3000: (3, 1000, 3, True)}
    counts = mrc.range_counts(np.ones((1025, 3), bool))
    assert len(counts) == 513 and (counts[:512] == 6).all() and counts[512] == 3


@pytest.mark.parametrize("n", mrc.INST_SIZES)
@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_the_random_buffers_are_fair(backend, n):
    """The conditions on the random buffers, and the floors of every layer on the back end's model; where the GPU test turns the per-sample
    gradients on, theirs too."""
    setup = mrc.inst_setup(backend, n)
    live = mrc.check_random_buffers(setup)
    counts = mrc.range_counts(itc.live_mask(setup[4], setup[3][3]))
    floor, want = mrc.inst_fair(setup, samples=n in mrc.MODE_SIZES)
    print(f"{backend} n {n}: {live} live, {(counts == 0).sum()} of {len(counts)} scan ranges empty, worst floor {floor:.2e}")
    assert len(want.live) == live


@pytest.mark.parametrize("name", mrc.MASKS)
@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_the_live_masks_are_fair(backend, name):
    """An explicit mask is what its name says, and the step under it has a gradient in every layer: a live sample lies inside the medium."""
    setup, mask = mrc.mask_setup(backend, name)
    live = mrc.check_mask(setup, mask, name)
    floor, want = mrc.inst_fair(setup)
    print(f"{backend} {name}: {live} live, worst floor {floor:.2e}")
    assert len(want.live) == live


def test_the_first_1024_rays_are_a_prefix():
    """`first_rays` cuts every buffer, and the live order of the first 1024 rays is the head of the 2049 rays' order."""
    setup = mrc.inst_setup("flex", 2049)
    head = mrc.first_rays(setup, 1024)
    assert len(head[4]) == len(head[5]) == 1024 and np.array_equal(head[3][8][:, 0], np.nonzero(head[4])[0])
    a, b = itc.live_order(setup[4], setup[3][3]), itc.live_order(head[4], head[3][3])
    assert len(b) > 64 and np.array_equal(a[:len(b)], b) and a[len(b)] >= 1024 * mrc.INST_S


@pytest.mark.parametrize("trainer,case", mrc.WHOLE_RUNS, ids=mrc.WHOLE_RUN_IDS)
def test_the_whole_ray_steps_are_fair(trainer, case):
    """Every whole-ray step of the three trainers, and the IPE model's: the floors of the loss, the predictions and every layer."""
    fx = mrc.whole_setup(trainer, case)
    assert fx.n > 1024 and fx.n * fx.S <= 1025 * 32
    floor = mrc.whole_fair(fx)
    print(f"{trainer} {fx.id}: worst floor {floor:.2e}")


@pytest.mark.parametrize("cid", mrc.GRAD_IDS)
@pytest.mark.parametrize("backend", mrc.BACKENDS)
def test_the_parameter_and_ray_gradient_cases_are_fair(backend, cid):
    """Every column of dL/d parameter rows and of dL/d rays_o, rays_d inside `pgc.fair`'s guards, over the rows and rays that hit."""
    model, spec, wts, batch, kn, seed = mrc.grad_setup(backend, cid)
    patterns = pgc.own_patterns(spec, wts, batch, kn, seed)
    want = mrc.grad_restate(spec, wts, batch, kn, seed, torch.float64, patterns)
    f32 = mrc.grad_restate(spec, wts, batch, kn, seed, torch.float32, patterns)
    n_rows = -(-kn["n"] // kn["rpr"])
    assert want[1].shape == (n_rows, 7) and want[2].shape == (kn["n"], 3) and kn["n"] > 1024
    row_hit, ray_hit = mrc.grad_rows(kn, n_rows)
    if cid == "rows_of_256":
        assert n_rows == 5 and kn["n"] - 4 * kn["rpr"] == 1
    else:
        assert n_rows == kn["n"] and (~row_hit).sum() == len(mrc.MISS_2500) and not want[1][~row_hit].any() and not want[2][~ray_hit].any() and not want[3][~ray_hit].any()
    pgc.fair(want[1], f32[1], rows=row_hit)
    pgc.fair(igc.columns(want[2], want[3]), igc.columns(f32[2], f32[3]), rows=ray_hit)
