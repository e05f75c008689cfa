"""The training composite's bits, as hashes: one JSON line per case with the sha256 (16 hex digits) of the float32 predictions, the returned
weights, slot 30 (`activation(30, ...)`, the composite's adjoint itself) and the gradient vector.  tools/train_fingerprint.py hashes the fused
step and tools/forward_backward_fingerprint.py the step cut in two; neither reaches the suffix scan's chunk edges with a weight cotangent,
S = 1024 (`MAX_TRAIN_SAMPLES`), or an instanced ray without `alpha_weight`.  This one does:
  plain      every case of tests/weight_loss_common.ADJ_CASES (5 rays; S in 2, 63, 64, 65, 129; chain, flex, branch; map_exr, background, noise)
             with its weight cotangent and without; the two S = 65 cases again with a ray at t = inf; a flex case at 4 rays x 1024 samples; a
             fused `gradients_step` under alpha_smape at S = 65 (chain) and S = 1024 (flex)
  instanced  `weight_loss_common.instanced_setup(kind, live)` for both kinds and the four LIVE settings, with and without `d_weights`; a case
             with density_reweighting=False (alpha_weight NULL); the flex kind at S = 65 and S = 1024, where -- checked on the host from `hit`
             and `dists` before anything is hashed -- one ray has its only live samples in the last chunk of 64 and one ray has hit == 0.
A change that only moves the composite's code prints what its parent prints -- with the tree's root as the working directory:
    NERFTEX_LIB=<parent's libnerftex_hip.so> python tools/composite_fingerprint.py > parent.jsonl
    python tools/composite_fingerprint.py > new.jsonl && cmp parent.jsonl new.jsonl
profiles/composite_unify/composite_fingerprint_{parent,new}.jsonl are such a pair.  Exits non-zero when a hashed gradient is not finite or all
zero (a step without a live sample has to be all zero instead)."""

import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())

from tests import fused_instanced_common as fic        # noqa: E402
from tests import instanced_train_common as itc        # noqa: E402
from tests import weight_loss_common as wlc            # noqa: E402
from tests.train_common import BKGD, make_loss, step_pred, targets   # noqa: E402

F = np.float32
sha = lambda a: hashlib.sha256(np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=F).tobytes()).hexdigest()[:16]
_TRAINERS = {}


def emit(case, grads, empty=False, **hashed):
    """One line; `grads`: the hashed arrays that are gradients (finite, and not all zero unless the step is `empty`: then all zero)."""
    for g in grads:
        if not np.isfinite(g).all() or bool(np.any(g)) == empty:
            print(json.dumps({"case": case, "error": "a hashed gradient is not finite, or all zero"}), flush=True)
            sys.exit(1)
    print(json.dumps({"case": case, **{k: sha(v) for k, v in hashed.items()}}), flush=True)


# ---- plain steps ---------------------------------------------------------------------------------------------------------------------------
def plain_trainer(kind, n, S):
    from nerf_tex_amd import train
    if (kind, n, S) not in _TRAINERS:
        _TRAINERS[kind, n, S] = getattr(train, wlc.KINDS[kind][0])(wlc.kind_model(kind)[0], max_rays=n, n_samples=S, perturb=True)
    return _TRAINERS[kind, n, S]


def plain_batch(kind, n, S, seed):
    """`wlc.adjoint_batch` for any n and S: the family's rays, all hit, per-ray parameters, the three cotangents."""
    from nerf_tex_amd import synthetic
    f = synthetic.FAMILIES[wlc.KINDS[kind][3]]
    P = sum(wlc.KINDS[kind][1])
    rng = np.random.default_rng(1000 + seed)
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], f["cam"], seed=seed + 1)
    params = (np.resize(np.asarray(f["params"], F), P)[None, :] * rng.uniform(0.8, 1.2, size=(n, P))).astype(F)
    return (ro, rd, t, cone, params), wlc.cotangents(n, S, 100 + seed)


def plain(name, tr, case, batch, cots, with_g, miss=None):
    """forward (with the weights), weight cotangent, backward, as tests/test_gpu_weight_losses.plain_sequence; a ray of `miss` at t = inf with
    NaN in its cotangents."""
    cid, kind, S, regime, exr, bk, noise_std = case
    (ro, rd, t, cone, params), (gC, gA, gW) = batch, cots
    n = len(t)
    tr.set_weights(wlc.kind_model(kind, regime)[2])
    tr.map_exr, tr.raw_noise_std = bool(exr), float(noise_std)
    if miss is not None:
        t, cone, gC, gA, gW = t.copy(), cone.copy(), gC.copy(), gA.copy(), gW.copy()
        t[miss], cone[miss] = np.inf, np.nan
        gC[miss], gA[miss], gW[miss] = np.nan, np.nan, np.nan
    cp, ap, w = tr.forward(ro, rd, t, params, cone, composite_bkgd=bk, bkgd_color=BKGD, seed=S, n_samples=S, return_weights=True)
    tr.backward(gC, gA, gW if with_g else None)
    torch.cuda.synchronize()
    adj, grad = tr.activation(30, n * S), tr.gradients()
    emit(name, (adj, grad), pred=step_pred(cp, ap), w=w, adj=adj, g=grad)


def fused(name, tr, kind, n, S):
    """One `gradients_step` under AlphaLoss(smape, smape): composite_loss_kernel, the weights through ntx_trainer_composite_weights."""
    from nerf_tex_amd import _lib
    (ro, rd, t, cone, params), _ = plain_batch(kind, n, S, 40 + S)
    tr.set_weights(wlc.kind_model(kind)[2])
    tr.map_exr, tr.raw_noise_std = False, 0.0
    buf = torch.zeros((n, S), device=torch.device("cuda", 0))
    _lib.check(_lib.lib.ntx_trainer_composite_weights(tr._h, buf.data_ptr()))
    try:
        val, cp, ap = tr.gradients_step(ro, rd, t, params, cone, *targets(n, S), make_loss("alpha_smape")[1], seed=S, n_samples=S)[:3]
    finally:
        _lib.check(_lib.lib.ntx_trainer_composite_weights(tr._h, None))
    torch.cuda.synchronize()
    adj, grad = tr.activation(30, n * S), tr.gradients()
    emit(name, (adj, grad), loss=val, pred=step_pred(cp, ap), w=buf, adj=adj, g=grad)


def plain_cases():
    for case in wlc.ADJ_CASES:
        tr = plain_trainer(case[1], wlc.CAP_RAYS, wlc.CAP_S)
        batch, cots = wlc.adjoint_batch(case)
        for with_g in (True, False):
            plain(f"plain {case[0]} g={int(with_g)}", tr, case, batch, cots, with_g)
        if case[0] in ("chain_S65", "flex_S65"):
            miss = np.zeros(wlc.ADJ_N, bool); miss[2] = True
            plain(f"plain {case[0]} g=1 ray 2 at t=inf", tr, case, batch, cots, True, miss)
    big = plain_trainer("flex", 4, 1024)
    batch, cots = plain_batch("flex", 4, 1024, 40 + 1024)
    for with_g in (True, False):
        plain(f"plain flex 4x1024 g={int(with_g)}", big, ("flex_S1024", "flex", 1024, "mixed", True, True, 0.1), batch, cots, with_g)
    fused("fused chain 5x65 alpha_smape", plain_trainer("chain", wlc.CAP_RAYS, wlc.CAP_S), "chain", wlc.ADJ_N, 65)
    fused("fused flex 4x1024 alpha_smape", big, "flex", 4, 1024)


# ---- instanced steps ---------------------------------------------------------------------------------------------------------------------------
def instanced(name, tr, bufs, hit, cone, kn, with_g):
    n, S = bufs[3].shape
    hit = np.asarray(hit, bool)
    gC, gA, gW = wlc.cotangents(n, S, 9)
    c, a, w = tr.forward_instanced(bufs, cone, hit=hit.astype(np.uint8), return_weights=True, **fic.fkw(kn))
    tr.backward(gC, gA, gW if with_g else None)
    torch.cuda.synchronize()
    M = int(itc.live_mask(hit, bufs[3]).sum())
    assert tr.last_live == M
    grad, spg = tr.gradients(), tr.sample_parameter_gradients().cpu().numpy()
    adj = tr.activation(30, M) if M else np.zeros((0, 4), F)
    emit(name, (grad, spg) + ((adj,) if M else ()), empty=M == 0, pred=step_pred(c, a), w=w, adj=adj, g=grad, pg=spg)


def instanced_trainer(kind, model, n, S, case=None):
    if kind == "chain":
        return fic.chain_trainer(wlc.INST_KINDS[kind], model, n, S, pm=True)
    from nerf_tex_amd.train import FlexTrainer
    return FlexTrainer(model, max_rays=n, n_samples=max(S, 2), perturb=False, param_gradients=True)


def chunk_edge_setup(n, S):
    """The flex kind at n x S with ray `late` live in its last chunk of 64 alone and ray `dark` at hit == 0 -- both checked from `hit` and
    `dists`, as the kernels read them."""
    model, spec, wts, bufs, hit, cone, kn, okw = itc.case_setup(wlc.INST_KINDS["flex"], n=n, S=S, seed=40 + S)
    hit, dists, c0 = np.asarray(hit, bool).copy(), np.asarray(bufs[3], F).copy(), (S - 1) // 64 * 64
    late = int(np.nonzero(hit & (dists[:, c0:] > 0).any(1))[0][0])
    dists[late, :c0] = 0
    if hit.all():
        hit[(late + 1) % n] = False
    bufs = tuple(dists if k == 3 else b for k, b in enumerate(bufs))
    mask = itc.live_mask(hit, bufs[3])
    assert mask[late, c0:].any() and not mask[late, :c0].any(), "no ray with its only live samples in the last chunk"
    assert (~hit).any() and mask.sum() > mask[late].sum(), "no ray with hit == 0, or no other live ray"
    return model, bufs, hit, cone, kn


def instanced_cases():
    for kind in sorted(wlc.INST_KINDS):
        for live in wlc.LIVE:
            model, spec, wts, bufs, hit, cone, kn, okw = wlc.instanced_setup(kind, live)
            tr = instanced_trainer(kind, model, *bufs[3].shape)
            for with_g in (True, False):
                instanced(f"instanced {kind} {live} g={int(with_g)}", tr, bufs, hit, cone, kn, with_g)
    model, spec, wts, bufs, hit, cone, kn, okw = itc.case_setup(itc.CASES[3])                   # density_reweighting=False: alpha_weight NULL
    assert not kn["density_reweighting"]
    tr = instanced_trainer("flex", model, *bufs[3].shape)
    for with_g in (True, False):
        instanced(f"instanced flex no alpha_weight g={int(with_g)}", tr, bufs, hit, cone, kn, with_g)
    for n, S in ((23, 65), (6, 1024)):
        model, bufs, hit, cone, kn = chunk_edge_setup(n, S)
        tr = instanced_trainer("flex", model, n, S)
        for with_g in (True, False):
            instanced(f"instanced flex {n}x{S} last chunk alone, hit == 0, g={int(with_g)}", tr, bufs, hit, cone, kn, with_g)


def main():
    from nerf_tex_amd import _lib
    print(json.dumps({"lib": _lib.LIB_PATH}), file=sys.stderr)
    plain_cases()
    instanced_cases()


if __name__ == "__main__":
    main()
