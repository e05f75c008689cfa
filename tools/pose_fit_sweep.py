"""The float64 side of the end-to-end pose fit (tests/pose_common.py, `FIT`), swept on the CPU: the restated fit (`restated_fit`: the same
parametrisation and torch Adam as `PoseFitter.fit`, autograd of the restated pipeline) from several start seeds at several lrates, and the loss along
the straight path from the true poses to the committed start.  It records why tests/test_gpu_pose_fit.py asserts a falling loss and the first step's
gradient and not the pose errors: with random weights no setting halves them.  No GPU is used.
    python tools/pose_fit_sweep.py [--out profiles/pose_fit/sweep_float64.json]
One JSON line."""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import pose_common as pc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--start-seeds", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--lrates", type=float, nargs="+", default=[1e-4, 3e-4, 1e-3, 2e-3, 4e-3])
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    f = dict(pc.FIT)
    out = {"what": "float64 restated pose fit, 40 Adam steps; loss first -> last, rotation error (degrees) and translation error per pose at the end", "scene": f,
           "box": pc.BOX, "camera_distance": pc.RADIUS, "fits": [], "path": []}
    halved = 0
    for ss in a.start_seeds:
        pc.FIT["start_seed"] = ss
        model, spec, wts, batch, true, start, focal = pc.fit_setup()
        batch["color"], batch["alpha"] = pc.restated_targets(spec, wts, batch, true, focal)
        rot0, tr0 = pc.pose_errors(start, true)
        for lr in a.lrates:
            c2w, losses, track = pc.restated_fit(spec, wts, batch, start, focal, f["n_iters"], lr)
            rot, tr = pc.pose_errors(c2w, true)
            both = bool((rot <= rot0 / 2).all() and (tr <= tr0 / 2).all())
            halved += both
            out["fits"].append({"start_seed": ss, "lrate": lr, "loss_first": losses[0], "loss_last": losses[-1], "loss_every_10": losses[::10], "rotation_start": rot0.tolist(),
                                "rotation_end": rot.tolist(), "translation_start": tr0.tolist(), "translation_end": tr.tolist(), "both_errors_halved": both})
    pc.FIT["start_seed"] = f["start_seed"]
    model, spec, wts, batch, true, start, focal = pc.fit_setup()
    batch["color"], batch["alpha"] = pc.restated_targets(spec, wts, batch, true, focal)
    B, R = batch["image_plane_loc"].shape[:2]
    for deg in (0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.5, 1.0, 2.0):                        # the committed perturbation, scaled: a degrees and 0.025 a units
        c2w = pc.perturbed(true, deg, f["shift"] * deg / f["degrees"], f["start_seed"])
        with torch.no_grad():
            val = pc.restated_pipeline(wts, spec, batch["image_plane_loc"].reshape(-1, 2), torch.tensor(c2w), torch.tensor(focal, dtype=torch.float64), pc.H, pc.W, R, f["S"], *pc.BOX,
                                       batch["parameters"], batch["color"].reshape(-1, 3), batch["alpha"].reshape(-1))[0]
        out["path"].append({"degrees": deg, "loss": float(val)})
    out["fits_that_halve_both_errors"] = int(halved)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
