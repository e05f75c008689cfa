"""A training step's bits, as hashes: one JSON line per case with the sha256 of the float32 loss, color_pred, alpha_pred and gradient vector of
one `gradients_step`, then of the weights and both Adam moments after two more whole steps.  The cases are the smallest seeded batches that
reach every path of the native training code (both backends, every forward-chain build, both encoders, the per-ray direction row, the
2048-sample split, the composite weights of a coarse pass, the contraction alone; behind them the parameter branches of
ntx_trainer_create_flex_ex, which a library without that entry cannot run: compare the lines in front of them; last, a step of eight ranges of
the split, whose weight gradients take the contraction's XCD-major tile numbering).  A step is bit-reproducible, so two runs on one library
print the same lines, and a change that only moves code prints what its parent prints:
    NERFTEX_LIB=<parent's libnerftex_hip.so> python tools/train_fingerprint.py > parent.jsonl
    python tools/train_fingerprint.py > new.jsonl && cmp parent.jsonl new.jsonl
Exits non-zero when a case raised, or a hashed gradient is not finite or all zero (identical but empty output must not pass)."""

import hashlib
import json
import os
import sys
import traceback

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from nerf_tex_amd import synthetic                            # noqa: E402
from tests.common import make_model                           # noqa: E402
from tests.test_gpu_train import batch                        # noqa: E402
from tests.train_common import BKGD, make_loss, mip_batch, targets   # noqa: E402
from tests.train_flex_common import ARCHS                     # noqa: E402

F = np.float32
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=F).tobytes()).hexdigest()


def fingerprint(tr, args, loss, **kw):
    """`tr`: a Trainer, FlexTrainer or CoarseFineTrainer; `args`: ro, rd, t, params, cone, color, alpha."""
    val, color, alpha = tr.gradients_step(*args, loss, seed=5, **kw)[:3]
    singles = getattr(tr, "trainers", (tr,))
    grad = np.concatenate([s.gradients() for s in singles])
    if not np.isfinite(grad).all() or not grad.any():
        raise ValueError("the gradient is not finite, or all zero")
    out = {"loss": sha(val), "color_pred": sha(color), "alpha_pred": sha(alpha), "grad": sha(grad)}
    for seed in (6, 7):
        tr.step(*args, loss, seed=seed, **kw)
    out["weights"] = sha(np.concatenate([s.weights() for s in singles]))
    for k, name in enumerate(("adam_m", "adam_v")):
        out[name] = sha(np.concatenate([s.adam_state()[k] for s in singles]))
    return out


def family_batch(fam, n, S, P, seed=3, miss=()):
    ro, rd, t, cone, params, color, alpha = batch(seed, n, S, len(synthetic.FAMILIES[fam]["params"]), fam)
    t = t.copy(); t[list(miss)] = np.inf
    return ro, rd, t, (np.ascontiguousarray(params[:, :P]) if P else None), cone, color, alpha


def chain(npar, fam, n, S, loss_name, miss=(), freqs=None, bkgd=False, **kw):
    from nerf_tex_amd.train import Trainer
    model, _, _ = make_model(npar, dense_media=True, freqs=freqs)
    tr = Trainer(model, max_rays=n, n_samples=S, **kw)
    return fingerprint(tr, family_batch(fam, n, S, sum(npar), miss=miss), make_loss(loss_name)[1], composite_bkgd=bkgd, bkgd_color=BKGD)


def ipe(blur_idx):
    from nerf_tex_amd.train import Trainer
    n, S = 16, 32
    model, _, _ = make_model((1, 3), kind="IPE", dense_media=True)
    ro, rd, t, cone, params = mip_batch(n, 5)
    t = t.copy(); t[4] = np.inf
    tr = Trainer(model, max_rays=n, n_samples=S, perturb=True, blur_idx=blur_idx)
    return fingerprint(tr, (ro, rd, t, params, cone, *targets(n, 2)), make_loss("alpha_smape")[1])


def flex(arch_id, n=45, S=37, extended=False, entry_ex=False, **kw):
    """`extended`: the same model through an ntx_model_desc_ex with param_depth 0 (kind NTX_MODEL_PARAMNERF_EX), which the C ABI takes: same bits;
    `entry_ex`: through ntx_trainer_create_flex_ex (`BranchTrainer`), which takes param_depth 0 too: same bits again"""
    from nerf_tex_amd import _lib
    from nerf_tex_amd import train
    FlexTrainer = train.BranchTrainer if entry_ex else train.FlexTrainer
    _, npar, kind, arch, fam = next(a for a in ARCHS if a[0] == arch_id)
    model, _, _ = make_model(npar, kind=kind, arch=arch, dense_media=True)
    if extended:
        plain = model.desc
        model.desc = lambda: _lib.ModelDesc(_lib.KIND_PARAMNERF_EX, *[getattr(plain(), f) for f, _ in _lib.ModelDesc._fields_[1:12]], 0, 128)
    tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=True, **kw)
    return fingerprint(tr, family_batch(fam, n, S, sum(npar)), make_loss("alpha_smape")[1])


def branches(npar, arch, fam, n=45, S=37, **kw):
    """A ParamNerf with parameter branches (param_depth > 0) through `BranchTrainer`"""
    from nerf_tex_amd.train import BranchTrainer
    from tests.train_branch_oracle import branch_batch
    model, spec, _ = make_model(npar, arch=arch, dense_media=True)
    tr = BranchTrainer(model, max_rays=n, n_samples=S, perturb=True, **kw)
    ro, rd, t, cone, params, color, alpha = branch_batch(3, n, spec, fam)
    return fingerprint(tr, (ro, rd, t, params, cone, color, alpha), make_loss("alpha_smape")[1])


def flex_ranges(n, S):
    """The 3 x 64 model of tests/test_gpu_train_flex.py::test_the_weight_gradients_split on n x S samples"""
    from nerf_tex_amd.train import FlexTrainer
    model, _, _ = make_model((1, 6), dense_media=True, arch=dict(width=64, depth=3))
    tr = FlexTrainer(model, max_rays=n, n_samples=S, perturb=True)
    return fingerprint(tr, family_batch("carpet", n, S, 7), make_loss("alpha_smape")[1])


def coarse_fine():
    from nerf_tex_amd.train import CoarseFineTrainer, FlexTrainer
    n = 16
    tr = CoarseFineTrainer(make_model((0, 0), kind="Nerf", dense_media=True)[0], make_model((0, 0), kind="Nerf", seed=1, dense_media=True)[0], max_rays=n, n_samples=16,
                           n_importance=16, perturb=True)
    assert all(isinstance(s, FlexTrainer) for s in tr.trainers)
    return fingerprint(tr, family_batch("carpet", n, 16, 0), make_loss("nerf_mse")[1])


def gemm(ak, M, N, K):
    from nerf_tex_amd import _lib
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(M + N + K)
    A, B, bias = rng.normal(size=(M, K) if ak else (K, M)).astype(F), rng.normal(size=(K, N)).astype(F), rng.normal(size=N).astype(F)
    dA, dB, db = (torch.as_tensor(x, device=dev) for x in (A, B, bias))
    out = torch.zeros((M, N), device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib.ntx_gemm_f32(dA.data_ptr(), A.shape[1], ak, dB.data_ptr(), N, 0, out.data_ptr(), N, M, N, K, db.data_ptr(), 1, torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    if not torch.isfinite(out).all() or not out.any():
        raise ValueError("the product is not finite, or all zero")
    return {"out": sha(out)}


CASES = [
    ("chain carpet 50x37 perturb alpha_smape", lambda: chain((1, 6), "carpet", 50, 37, "alpha_smape", perturb=True)),       # ragged last block, direction segment per sample, build (9, 11)
    ("chain carpet 8x64", lambda: chain((1, 6), "carpet", 8, 64, "alpha_smape", perturb=False)),                          # direction segment per ray
    ("chain grass_filtered 33x32 blur0 noise bkgd misses", lambda: chain((2, 3), "grass_filtered", 33, 32, "nerf_mse", miss=(0, 7, 32), bkgd=True, perturb=True,
                                                                         blur_idx=0, raw_noise_std=0.1)),                 # build (11, 8), blur on a geometry parameter
    ("chain carpet 8x32 blur on an appearance parameter", lambda: chain((1, 6), "carpet", 8, 32, "alpha_smape", perturb=False, blur_idx=3)),      # no hoist although S % 32 = 0
    ("chain narrow encodings (1,2) bands (4,2,2) 80x40", lambda: chain((1, 2), "carpet", 80, 40, "alpha_smape", freqs=(4, 2, 2), perturb=False)),  # build (9, 8), zero-padded streams
    ("chain three geometry parameters 20x32", lambda: chain((3, 0), "carpet", 20, 32, "alpha_smape", perturb=False)),     # pos_map of 90 features: build (12, 12)
    ("chain ipe 16x32 blur0 one miss", lambda: ipe(0)),
    ("chain ipe 16x32 blur2 one miss", lambda: ipe(2)),                                                                   # the splice in the middle of the row
    ("flex nerf_8x256", lambda: flex("nerf_8x256")),
    ("flex w98_d5_skips13", lambda: flex("w98_d5_skips13")),                                                              # unaligned operands, two skips
    ("flex color_depth0", lambda: flex("color_depth0")),
    ("flex color_depth2", lambda: flex("color_depth2")),
    ("flex depth1", lambda: flex("depth1")),
    ("flex w128_d4 grass_filtered 41x70 blur0", lambda: flex("w128_d4", 41, 70, blur_idx=0)),                            # 2870 samples: two ranges of the 2048-sample split
    ("flex w128_d4 grass_filtered 41x70 blur0, extended descriptor", lambda: flex("w128_d4", 41, 70, blur_idx=0, extended=True)),  # the line above again
    ("flex coarse + fine Nerfs 16x(16+16)", coarse_fine),                                                                 # ntx_trainer_composite_weights
    ("gemm 300x200x77 A k-contiguous", lambda: gemm(1, 300, 200, 77)),
    ("gemm 337x256x1000 A transposed", lambda: gemm(0, 337, 256, 1000)),
    # ntx_trainer_create_flex_ex: the lines above are what a library from before it prints
    ("flex w128_d4 grass_filtered 41x70 blur0, ntx_trainer_create_flex_ex", lambda: flex("w128_d4", 41, 70, blur_idx=0, entry_ex=True)),       # param_depth 0 through the new entry
    ("branches geometry only (3,0) d5 [2] pd2", lambda: branches((3, 0), dict(depth=5, skips=[2], param_depth=2), "carpet")),
    ("branches appearance only (0,5) d5 [2] pd2", lambda: branches((0, 5), dict(depth=5, skips=[2], param_depth=2), "carpet")),
    ("branches both (4,8) d6 w200 [0,4] cd2 pd4 pw100", lambda: branches((4, 8), dict(depth=6, width=200, skips=[0, 4], color_depth=2, param_depth=4, param_width=100), "carpet")),
    ("branches (2,3) d4 w128 [1,2] cd0 pd3 pw64 41x70 blur0 noise", lambda: branches((2, 3), dict(depth=4, width=128, skips=[1, 2], color_depth=0, param_depth=3, param_width=64),
                                                                                 "grass_filtered", 41, 70, blur_idx=0, raw_noise_std=0.1)),     # the branch input differs per sample
    # appended last, so that the lines above still compare with an earlier library's
    ("flex 3x64 carpet 239x64: eight ranges of the 2048-sample split", lambda: flex_ranges(239, 64)),                     # 15 296 samples: the XCD-major tile numbering of a weight gradient
]
SAME_AS = (", extended descriptor", ", ntx_trainer_create_flex_ex")               # a case named "<other case><suffix>" has to print that case's hashes


def main():
    lines = {}
    for name, run in CASES:
        try:
            lines[name] = run()
            print(json.dumps({"case": name, **lines[name]}), flush=True)
            for suffix in SAME_AS:
                if name.endswith(suffix) and lines[name] != lines[name[:-len(suffix)]]:
                    raise ValueError(f"param_depth 0{suffix} trains to other bits than through the plain descriptor and ntx_trainer_create_flex")
        except Exception:                                   # (nothing more is started on a device that may just have faulted)
            print(json.dumps({"case": name, "error": traceback.format_exc(limit=3)}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
