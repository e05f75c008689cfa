"""The instanced step on the fused chain (`ntx_trainer_enable_instanced`, `Trainer(instanced=True)`, `trainer_for(..., instanced=True)`; DESIGN
section 10), what can be said without a GPU: the entry exists and refuses NULL, the Python surface, the contract of the chain's encoder for
compact rows restated in numpy, and every case of tests/test_gpu_fused_instanced.py 2x inside the guards of its bars.  No GPU."""

import inspect
import os
import re

import numpy as np
import pytest

from tests import fused_instanced_common as fic
from tests import input_grad_common as igc
from tests import instanced_train_common as itc

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_exported_declared_and_refuses_null():
    from nerf_tex_amd import _lib
    assert "ntx_trainer_enable_instanced" in _lib.SYMBOLS and len(_lib.SYMBOLS["ntx_trainer_enable_instanced"][1]) == 1
    assert _lib.lib.ntx_trainer_enable_instanced(None) == _lib.NTX_E_INVALID
    assert b"NULL" in _lib.lib.ntx_last_error()
    assert _lib.ABI_VERSION == 7 and _lib.lib.ntx_abi_version() == 7
    with open(os.path.join(ROOT, "include", "nerftex.h")) as f:
        header = f.read()
    assert re.search(r"int\s+ntx_trainer_enable_instanced\(ntx_trainer \*t\);", header)
    assert header.index("ntx_trainer_enable_instanced(ntx_trainer *t);") > header.index("int ntx_trainer_enable_gradients(")      # appended


def test_the_python_surface():
    """The instanced methods live on the base class, every class takes `instanced=`, and `trainer_for` hands it on."""
    from nerf_tex_amd import train
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer, Trainer
    for name in ("forward_instanced", "sample_parameter_gradients", "sample_input_gradients", "enable_instanced"):
        assert name in vars(Trainer) and name not in vars(FlexTrainer) and name not in vars(BranchTrainer), name
    for cls in (Trainer, FlexTrainer):
        p = inspect.signature(cls.__init__).parameters["instanced"]
        assert p.default is False
    seen = {}

    class Probe:
        def __init__(self, model, **kw):
            seen.update(kw)
    orig = train.trainer_class_for
    train.trainer_class_for = lambda *a, **k: Probe
    try:
        train.trainer_for(object(), fused=True, instanced=True, max_rays=4)
    finally:
        train.trainer_class_for = orig
    assert seen == dict(instanced=True, max_rays=4)


# ---- the encoder's contract ------------------------------------------------------------------------------------------------------------------
def small_compaction():
    """3 rays x 5 samples with 7 live samples (ray 1 is not hit although its dists are positive), n_parameters [2, 3]."""
    bufs, _, cone = itc.instancer_buffers((2, 3), seed=3, n=3, S=5)
    mask = np.zeros((3, 5), bool)
    mask[0, [0, 2, 3]] = True; mask[2, [0, 1, 3, 4]] = True
    bufs, hit = itc.with_live_mask(bufs, None, mask | np.array([[False], [True], [False]]))
    hit[1] = False
    assert list(itc.live_order(hit, bufs[3])) == [0, 2, 3, 10, 11, 13, 14]
    return bufs, hit, cone


@pytest.mark.parametrize("part", [0, 1], ids=["pos_map", "dir_map"])
@pytest.mark.parametrize("blur", [None, 0, 3], ids=["no_blur", "blur_geo", "blur_app"])
def test_the_encoder_writes_the_live_rows_in_o_layout_and_a_zero_tail(part, blur):
    """Lane (n, h) of the wave of a block writes compact row blk * 32 + n: element (row, feature k) of the map lands on
    o_index(row / 32, tiles, k, row % 32), every feature once; rows n_live .. 31 of the last block are zeros in all K features; the rows of
    the tiles beyond K are not written (they stay what the allocation made them)."""
    bufs, hit, cone = small_compaction()
    freqs = (10, 4, 4)
    O, tiles, K = fic.emulate_encoder(bufs, hit, cone, part, 2, 3, freqs, blur)
    want = fic.expected_rows(bufs, hit, cone, part, 2, 3, freqs, blur)
    assert want.shape == (7, K) and K == (3 * 21 + 2 * 9 if part == 0 else 3 * 9 + 3 * 9) and tiles == (K + 31) // 32 and O.size == tiles * 1024
    written = np.zeros(O.size, bool)
    for row in range(32):
        for k in range(K):
            i = fic.o_index(0, tiles, k, row)
            assert not written[i]
            written[i] = True
            assert O[i] == (want[row, k] if row < 7 else 0.0), (row, k)
    assert np.isnan(O[~written]).all() and written.sum() == 32 * K
    # o_index itself: a bijection of (tile row, sample) onto a block's floats, 16-byte groups of four consecutive samples
    idx = np.array([[fic.o_index(2, tiles, r, p) for p in range(32)] for r in range(32 * tiles)])
    assert sorted(idx.ravel()) == list(range(2 * tiles * 1024, 3 * tiles * 1024))
    assert (idx[:, 1] - idx[:, 0] == 1).all() and (idx[1, :] - idx[0, :] == 4).all()


def test_nothing_is_read_where_nothing_is_live():
    """NaN at every sample that is not live, in every buffer the encoder reads: the emulated kernel's output does not change."""
    bufs, hit, cone = small_compaction()
    live = itc.live_mask(hit, bufs[3])
    spoiled = list(bufs)
    for k in (0, 1, 2, 9):
        b = np.array(spoiled[k], copy=True)
        b[~live] = np.nan
        spoiled[k] = b
    cone2 = cone.copy(); cone2[1] = np.nan
    for part in (0, 1):
        a, _, _ = fic.emulate_encoder(bufs, hit, cone, part, 2, 3, (10, 4, 4), 3 if part else 0, fill=0.0)
        b, _, _ = fic.emulate_encoder(tuple(spoiled), hit, cone2, part, 2, 3, (10, 4, 4), 3 if part else 0, fill=0.0)
        assert np.isfinite(b).all() and np.array_equal(a, b)


def test_the_blur_columns_factor():
    """cone_scale[ray] * t[ray, s] / patch_scale, ray = m / S, in float32: against float64 to a float32 rounding or two."""
    bufs, hit, cone = small_compaction()
    S = bufs[3].shape[1]
    for m in itc.live_order(hit, bufs[3]):
        got = fic.blur_factor(cone, bufs[2], itc.PATCH_SCALE, int(m), S)
        want = float(cone[m // S]) * float(np.asarray(bufs[2]).reshape(-1)[m]) / float(np.float32(itc.PATCH_SCALE))
        assert got.dtype == np.float32 and abs(float(got) - want) <= 2 ** -22 * abs(want) and want != 0


# ---- the GPU cases are fair -------------------------------------------------------------------------------------------------------------------
def _fair(setup, samples=True):
    _, spec, w, bufs, hit, cone, kn, okw = setup
    head = itc.quadratic_head(len(hit))
    pat = igc.own_instanced_patterns(spec, w, bufs, hit, cone, okw)
    want, want_in = fic.restate_all(spec, w, bufs, hit, cone, okw, head, pat, torch.float64)
    f32, f32_in = fic.restate_all(spec, w, bufs, hit, cone, okw, head, pat, torch.float32)
    assert len(want.live) >= 1
    fic.fair_all(spec, want, f32, want_in, f32_in, hit, bufs, samples=samples)
    return want


@pytest.mark.parametrize("case", fic.CASES + [fic.WIDE_CASE], ids=fic.CASE_IDS + [fic.WIDE_CASE[0]])
def test_the_gpu_cases_are_fair(case):
    """Every parity case at its own size 2x inside the guards BEFORE any GPU run: float32 autograd of the restatement within 2.5e-4 of float64
    in every layer and in every column of the per-sample parameter and input gradients, on the restatement's own float32 ReLU patterns, and a
    gradient worth the name (2e-6) everywhere.  The buffers hold a ray that is not hit and a hit ray without a live sample."""
    setup = itc.case_setup(case)
    _, _, _, bufs, hit, _, _, _ = setup
    assert (~hit).any() and (~itc.live_mask(hit, bufs[3])[hit]).all(1).any()
    want = _fair(setup)
    assert len(want.live) >= 100


@pytest.mark.parametrize("edge", [e for e in itc.EDGES if e[2] > 0], ids=[e[0] for e in itc.EDGES if e[2] > 0])
def test_the_gpu_edges_are_fair(edge):
    """The same for the edges' weight gradients (sample counts 1 / 64 / 65 / 130, live counts 1 .. 2049) on the chain's model."""
    _fair(fic.edge_setup(edge), samples=False)
