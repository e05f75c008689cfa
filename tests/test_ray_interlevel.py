"""The interlevel loss between a fine and a proposal histogram, without a device (`ntx_ray_interlevel`, include/nerftex.h;
tests/interlevel_common.py has the restatements, the cases and the gate): the entry is declared, bound and exported and the ABI is still 7;
the float64 reference's two analytic gradients are what central differences and the dense torch statement's autograd say; every case's
float32 floors leave the gate meaningful and its loss is worth the name (max q >= 0.5); the entry refuses bad arguments before it touches
a device."""

import os
import re

import numpy as np
import pytest
import torch

from tests import interlevel_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in ic.CASES if max(c[2], c[3]) <= 256 and c[1] <= 9]


def test_declared_bound_and_the_abi_version_stays():
    from nerf_tex_amd import _lib
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "nerftex.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+ntx_ray_interlevel\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m, "include/nerftex.h does not declare ntx_ray_interlevel"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["const float *weights", "const float *z_vals", "int n_samples", "const float *weights_prop", "const float *z_prop", "int n_prop",
                    "const float *ray_scale", "float eps", "int64_t n_rays", "float *loss_out", "float *grad_prop_out", "float *grad_fine_out", "void *stream"]
    assert len(_lib.SYMBOLS["ntx_ray_interlevel"][1]) == len(args) and hasattr(_lib.lib, "ntx_ray_interlevel")
    assert _lib.lib.ntx_abi_version() == 7


def test_the_python_names_exist():
    from nerf_tex_amd import autograd, loss, train
    assert callable(loss.ray_interlevel) and callable(loss.interlevel) and issubclass(train.ProposalTrainer, train.CoarseFineTrainer)
    assert issubclass(autograd.RayInterlevel, torch.autograd.Function)
    made = loss.Interlevel(weight=0.5)
    assert made.weight == 0.5 and made.eps == 2.0 ** -23


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_analytic_gradients_are_autograd_of_the_dense_statement(case):
    """dL/d proposal weights and dL/d fine weights of the float64 reference equal torch float64 autograd of the [N, S, S_p] mask statement."""
    w, z, wp, zp, _ = ic.case_inputs(case)
    want = ic.reference(w, z, wp, zp)
    t64 = lambda a, g=False: torch.tensor(a.astype(np.float64), requires_grad=g)
    wt, wpt = t64(w, True), t64(wp, True)
    val = ic.dense_torch(wt, t64(z), wpt, t64(zp))
    val.sum().backward()
    assert ic.rel_linf(val.detach().numpy(), want[0]) <= 1e-12
    assert ic.rel_linf(wpt.grad.numpy(), want[1]) <= 1e-12 and ic.rel_linf(wt.grad.numpy(), want[2]) <= 1e-12


def test_central_differences_confirm_both_gradients():
    """Central differences of the float64 reference, h = 1e-7, at the sample of largest q and at the proposal sample of largest gradient of
    every ray of two cases: both gradients within 1e-6 relative (q is piecewise linear in both weights: the differences are exact up to
    rounding away from a kink)."""
    for cid in ("P8_S16_N9_smooth", "P24_S40_N5_smooth"):
        w, z, wp, zp, _ = (a.astype(np.float64) for a in ic.case_inputs(ic.by_id(cid)))
        L, gp, gf, q = ic.reference(w, z, wp, zp)
        h = 1e-7
        for r in range(len(w)):
            i, j = int(np.argmax(q[r])), int(np.argmax(np.abs(gp[r])))
            for arr, k, g in ((w, i, gf[r, i]), (wp, j, gp[r, j])):
                keep = arr[r, k]
                arr[r, k] = keep + h; up = ic.reference(w, z, wp, zp)[0][r]
                arr[r, k] = keep - h; dn = ic.reference(w, z, wp, zp)[0][r]
                arr[r, k] = keep
                assert abs((up - dn) / (2 * h) - g) <= 1e-6 * max(1.0, abs(g)), (cid, r, k, (up - dn) / (2 * h), g)


@pytest.mark.parametrize("case", ic.CASES, ids=ic.CASE_IDS)
def test_floors_are_small_and_the_loss_is_worth_the_name(case):
    """Every float32 floor <= FLOOR_GUARD (four floors never reach the cap of 1e-4), and max q >= 0.5 in float64: a condition on the inputs."""
    floors, want = ic.floor(case), ic.case_reference(case)
    print(f"| {case[0]} | floors: loss {floors[0]:.2e} d prop {floors[1]:.2e} d fine {floors[2]:.2e} | max q {want[3].max():.3f} | max loss {want[0].max():.3e} |")
    assert max(floors) <= ic.FLOOR_GUARD and ic.gate(max(floors)) < ic.CAP
    assert want[3].max() >= 0.5
    assert np.abs(want[2]).max() > 0 and (case[2] == 1 or np.abs(want[1]).max() > 0)     # (one proposal sample is a zero-width interval: it overlaps nothing)


def test_ties_are_everywhere_in_the_merged_cases():
    case = ic.by_id("P24_S40_N5_peaky") if "P24_S40_N5_peaky" in ic.CASE_IDS else ic.by_id("P24_S40_N5_smooth")
    _, z, _, zp, _ = ic.case_inputs(case)
    assert all(np.isin(zp[r], z[r]).all() for r in range(len(z)))
    _, z, _, zp, _ = ic.case_inputs(ic.by_id("P63_S130_N6_free"))
    assert not any(np.isin(zp[r], z[r]).any() for r in range(len(z)))


@pytest.mark.parametrize("fam", ["peaky", "smooth"])
def test_the_off_grid_cases_are_what_they_say(fam):
    """"repeats": exact repeats inside either set (13 + the last pair a fine row, 6 a proposal row, ray 0's last proposal width zero), so that
    a sample's two searches give lo > hi somewhere; "beyond": a third of the fine samples on either side of the proposal's range, where nothing
    bounds them.  Both sorted, finite, and the dense torch statement agrees with the reference."""
    w, z, wp, zp, _ = ic.case_inputs(ic.by_id(f"P65_S130_N6_repeats_{fam}"))
    assert (np.diff(z, axis=1) >= 0).all() and (np.diff(zp, axis=1) >= 0).all()
    assert ((np.diff(z, axis=1) == 0).sum(1) >= 10).all() and ((np.diff(zp, axis=1) == 0).sum(1) >= 4).all()
    assert (z[:, -1] == z[:, -2]).all() and zp[0, -1] == zp[0, -2] and (zp[1:, -1] > zp[1:, -2]).all()
    b, bp = ic.interval_ends(z), ic.interval_ends(zp)
    crossed = [(np.searchsorted(bp[r], z[r], side="right") > np.searchsorted(zp[r], b[r], side="left")).sum() for r in range(len(z))]
    crossed_prop = [(np.searchsorted(b[r], zp[r], side="right") > np.searchsorted(z[r], bp[r], side="left")).sum() for r in range(len(z))]
    assert min(crossed) >= 1 and min(crossed_prop) >= 1, (crossed, crossed_prop)
    w, z, wp, zp, _ = ic.case_inputs(ic.by_id(f"P65_S130_N6_beyond_{fam}"))
    assert (np.diff(z, axis=1) >= 0).all()
    below, above = (z < zp[:, :1]).sum(1), (z > ic.interval_ends(zp)[:, -1:]).sum(1)
    assert (below >= 25).all() and (above >= 25).all() and ((z > zp[:, :1]) & (z < zp[:, -1:])).sum(1).min() >= 25, (below, above)
    q = ic.case_reference(ic.by_id(f"P65_S130_N6_beyond_{fam}"))[3]
    assert all(q[r, :below[r] - 1].max() > 0.99 for r in range(len(z)))                                     # nothing bounds a sample in front of the proposal's range


def test_the_large_batches_cycle_a_base_whose_rows_meet_every_wave():
    """The base of the calls past the capped grid: two of its 257 rows are not live (an inf in the fine depths alone; a NaN in the proposal
    depths alone with NaN weights), the row between them in index is ordinary; zeros where they have to be, inside the guard, worth the name."""
    from tests import distortion_common as dc
    w, z, wp, zp, dead, want, floors = ic.large_base()
    assert len(w) == 257 and np.array_equal(np.nonzero(dead)[0], [ic.INF_FINE, ic.NAN_PROP]) and not dead[ic.ORDINARY]
    assert np.isinf(z[ic.INF_FINE]).sum() == 1 and np.isfinite(zp[ic.INF_FINE]).all() and np.isfinite(w[ic.INF_FINE]).all()
    assert np.isnan(zp[ic.NAN_PROP]).sum() == 1 and np.isfinite(z[ic.NAN_PROP]).all() and np.isnan(w[ic.NAN_PROP]).all() and np.isnan(wp[ic.NAN_PROP]).all()
    assert all(np.isfinite(g).all() and not g[dead].any() for g in want) and (want[0][~dead] > 0).all() and max(floors) <= ic.FLOOR_GUARD
    f32 = ic.reference(w, z, wp, zp, dtype=ic.F)
    assert max(ic.rel_linf(f32[k], want[k]) for k in range(3)) <= ic.FLOOR_GUARD
    for n in dc.LARGE_N:
        scale = dc.large_scale(n, dead)
        got = ic.large_reference(n, scale)
        rows = np.arange(n) % 257
        assert np.isnan(scale[dead[rows]]).all() and all(np.isfinite(g).all() and not g[dead[rows]].any() for g in got)
        k = n - 1
        assert not dead[rows[k]] and all(np.array_equal(g[k], x[rows[k]] * np.float64(scale[k])) for g, x in zip(got, want))


def test_a_ray_that_is_not_live_is_zeros_in_the_reference():
    w, z, wp, zp, scale = (a.copy() for a in ic.case_inputs(ic.by_id("P8_S16_N9_smooth")))
    z[2], zp[2], w[2], scale[2] = np.inf, np.inf, np.nan, np.nan
    for T in (np.float64, ic.F):
        L, gp, gf, _ = ic.reference(w, z, wp, zp, scale, dtype=T)
        assert L[2] == 0 and not gp[2].any() and not gf[2].any() and np.isfinite(L).all() and np.isfinite(gp).all() and np.isfinite(gf).all()


def test_argument_checks_need_no_device():
    """Each NTX_E_INVALID case of the entry, with the message set, before any launch -- the buffers here are host memory the call must not
    touch -- and n_rays = 0 is NTX_OK without one."""
    from nerf_tex_amd import _lib
    fn = _lib.lib.ntx_ray_interlevel
    n, S, Sp = 3, 8, 5
    bufs = {k: np.full(n * S, -7.0, ic.F) for k in ("w", "z", "wp", "zp", "gp", "gf", "rs", "L")}
    w, z, wp, zp, gp, gf, rs, L = (bufs[k].ctypes.data for k in ("w", "z", "wp", "zp", "gp", "gf", "rs", "L"))
    eps = ic.EPS
    bad = {
        "weights NULL": (None, z, S, wp, zp, Sp, rs, eps, n, L, gp, gf),
        "z_vals NULL": (w, None, S, wp, zp, Sp, rs, eps, n, L, gp, gf),
        "weights_prop NULL": (w, z, S, None, zp, Sp, rs, eps, n, L, gp, gf),
        "z_prop NULL": (w, z, S, wp, None, Sp, rs, eps, n, L, gp, gf),
        "all outputs NULL": (w, z, S, wp, zp, Sp, rs, eps, n, None, None, None),
        "S = 0": (w, z, 0, wp, zp, Sp, rs, eps, n, L, gp, gf),
        "S = 4097": (w, z, 4097, wp, zp, Sp, rs, eps, n, L, gp, gf),
        "S_p = 0": (w, z, S, wp, zp, 0, rs, eps, n, L, gp, gf),
        "S_p = 4097": (w, z, S, wp, zp, 4097, rs, eps, n, L, gp, gf),
        "n_rays < 0": (w, z, S, wp, zp, Sp, rs, eps, -1, L, gp, gf),
        "n_rays = 2^31": (w, z, S, wp, zp, Sp, rs, eps, 2 ** 31, L, gp, gf),
        "eps = 0": (w, z, S, wp, zp, Sp, rs, 0.0, n, L, gp, gf),
        "eps < 0": (w, z, S, wp, zp, Sp, rs, -1e-7, n, L, gp, gf),
        "eps inf": (w, z, S, wp, zp, Sp, rs, float("inf"), n, L, gp, gf),
        "eps nan": (w, z, S, wp, zp, Sp, rs, float("nan"), n, L, gp, gf),
    }
    for what, args in bad.items():
        assert fn(*args, None) == _lib.NTX_E_INVALID, what
        assert _lib.lib.ntx_last_error(), what
    for args in ((w, z, S, wp, zp, Sp, rs, eps, 0, L, gp, gf), (w, z, 1, wp, zp, 4096, None, eps, 0, L, None, None), (w, z, 4096, wp, zp, 1, None, eps, 0, None, None, gf)):
        assert fn(*args, None) == _lib.NTX_OK
    assert all((a == -7.0).all() for a in bufs.values()), "a refused call has written nothing"
