"""The bits of `forward` + `backward` (`ntx_train_forward` / `ntx_train_forward_instanced` / `ntx_train_backward`), as hashes: one JSON line per
case with the sha256 (16 hex digits) of the float32 predictions and gradient vector -- the three trainers of tests/custom_loss_common.py at
45 x 37 with two rays at t = inf, with and without the background / elu + 1 and the density regulariser, then five instanced steps at 23 x 70
(three on the fused chain, two layer by layer) with the per-sample parameter and input gradients.  tools/train_fingerprint.py hashes the fused
step; this is the same for the step cut in two.  Only calls a library from before `ntx_trainer_weight_cotangent` has too, so a change that must
leave a backward without a weight cotangent alone prints what its parent prints -- run it with the tree's root as the working directory, in
the parent's tree and in this one:
    (cd <parent's tree> && python <this file>) > parent.jsonl;  python tools/forward_backward_fingerprint.py > new.jsonl;  cmp parent.jsonl new.jsonl
profiles/weight_losses/forward_backward_fingerprint_{parent,new}.jsonl are such a pair.  Exits non-zero when a gradient is not finite or all zero."""

import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())

from tests import custom_loss_common as clc            # noqa: E402
from tests import fused_instanced_common as fic        # noqa: E402
from tests import instanced_train_common as itc        # noqa: E402
from tests.common import make_model                    # noqa: E402
from tests.train_common import BKGD                    # noqa: E402

F = np.float32
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=F).tobytes()).hexdigest()[:16]


def main():
    from nerf_tex_amd import _lib, train
    print(json.dumps({"lib": _lib.LIB_PATH}), file=sys.stderr)
    for case in clc.TRAINER_CASES:
        model, spec, wts, batch, kn = clc.trainer_case(case)
        ro, rd, t, cone, rows, color, alpha = batch
        n = len(t)
        t = t.copy(); t[[0, 7]] = np.inf
        for bk in (False, True):
            for noise in (0.0, 0.1):
                tr = getattr(train, case[1])(model, max_rays=n, n_samples=clc.N_SAMPLES, perturb=kn["perturb"], raw_noise_std=noise, map_exr=bk)
                c, a = tr.forward(ro, rd, t, rows, cone, seed=kn["seed"], rays_per_param_row=kn["rpr"], composite_bkgd=bk, bkgd_color=BKGD)
                rng = np.random.default_rng(3)
                gC, gA = (rng.normal(size=(n, 3)) / n).astype(F), (rng.normal(size=n) / n).astype(F)
                tr.backward(gC, gA if noise == 0.0 else None)
                torch.cuda.synchronize()
                g = tr.gradients()
                assert np.isfinite(g).all() and g.any()
                print(json.dumps({"case": case[0], "bk": bk, "noise": noise, "c": sha(c), "a": sha(a), "g": sha(g)}))
    for name, case in (("chain", fic.CASES[0]), ("chain_exr", fic.CASES[3]), ("chain_bk", fic.CASES[4]), ("flex", itc.CASES[0]), ("flex_exr_bk", itc.CASES[2])):
        if name.startswith("chain"):
            model, spec, wts = make_model(case[2], seed=0, dense_media=True)
            _, _, _, bufs, hit, cone, kn, okw = itc.case_setup(case)
            tr = fic.chain_trainer(case, model, 23, 70, pm=True, im=True)
        else:
            model, spec, wts, bufs, hit, cone, kn, okw = itc.case_setup(case)
            tr = getattr(train, case[1])(model, max_rays=23, n_samples=70, perturb=False, blur_idx=case[4], map_exr=kn["map_exr"], param_gradients=True, input_gradients=True)
        pred, g, val = fic.step(tr, bufs, hit, cone, kn, itc.quadratic_head(23))
        pg, ig = fic.sample_results(tr)
        assert np.isfinite(g).all() and g.any()
        print(json.dumps({"case": "inst_" + name, "pred": sha(pred), "g": sha(g), "pg": sha(pg), "ig": sha(ig[0]), "ig2": sha(ig[1])}))


if __name__ == "__main__":
    main()
