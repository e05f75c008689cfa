"""What the stream-order tests share (tests/test_streams.py on the CPU, tests/test_gpu_streams.py on the GPU): the contract of
include/nerftex.h, "every entry point is asynchronous on `stream`", checked on a stream that is NOT the null stream.

Every kernel here is deterministic, so the yardstick of a case is the same call sequence on the default stream, on a fresh handle with the
same history (`reference`): the existing tests pin those bits to the float64 restatements.  A trapped run must give the same BYTES.

  trap A, late inputs (`trap_a`): every device input of the calls lives in a buffer that holds ANOTHER valid batch (same shapes, another
      seed).  On a side stream s: a delay kernel, the event `armed`, copies of the real batch into those buffers -- then the calls, under
      `torch.cuda.stream(s)`.  When the last call has returned, `armed` must not have completed: everything was enqueued while s was still
      blocked.  Work the library puts on any other stream runs early, on the other batch or on what the history call left, and the bytes differ.
  trap B, busy null stream (`trap_b`): a delay on the null stream and the event `busy` behind it; the calls and the snapshot of their results
      on s; `s.synchronize()`; `busy` must not have completed (nothing waited for the null stream or the device).  Work the library puts on
      the null stream lands behind the consumers on s: stale results.

The other batch is always a valid one: a mis-ordered kernel computes a wrong number, it does not fault.  Before a trapped call the handle
runs the same calls on a third batch (the history), in the reference run too, so that its internal buffers hold values that are not the
right ones.  The controls (tests/test_gpu_streams.py) show that both traps can see anything at all on the device at hand; and since the
runtime deals a process's streams onto a few hardware queues, where two streams on one queue simply run in turn, every side stream comes
from `side_stream()`, which has seen it run beside a busy null stream first (profiles/streams/notes.md).

The delay is `torch.cuda._sleep`, calibrated once per session: the larger of 20 ms and 10 x the host time the same calls took on the default
stream (trap A: until they were enqueued; trap B: until they had completed, since they have to complete inside it), the handle's own first
calls -- placements included -- counted too.  The binding condition is the `armed` / `busy` assertion, not the number.

This module imports without a GPU: the batches are numpy, the cases are built on first use."""

import ctypes as C
import os
import re
import time
from types import SimpleNamespace

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerftex.h")
INTEGRATION = os.path.join(ROOT, "docs", "INTEGRATION_details.md")
REAL, HISTORY, POISON = 0, 1, 2          # the seeds of a case's three batches
CAMERAS = ("carpet", "grass", "fur")     # batch k's rays come from this family's camera and box
SENTINEL = -7.25                         # what an output buffer the test owns holds before the call writes it
MIN_DELAY_MS = 20.0
DELAY_FACTOR = 10.0

# ---- the tables ---------------------------------------------------------------------------------------------------------------------------
# entry with an `ntx_stream` parameter -> one id of tests/test_gpu_streams.py that runs it off the null stream
COVERED = {
    "ntx_generate_rays": "test_trap[generate_rays-A]",
    "ntx_generate_rays_at": "test_trap[generate_rays_at-A]",
    "ntx_generate_rays_strided": "test_trap[generate_rays_strided-A]",
    "ntx_aabb_intersect": "test_trap[aabb_intersect-A]",
    "ntx_fourier_features": "test_trap[fourier_features-A]",
    "ntx_sample_depths": "test_trap[sample_depths-A]",
    "ntx_sample_noise": "test_trap[sample_noise-A]",
    "ntx_sample_pdf": "test_trap[sample_pdf_S65-A]",
    "ntx_composite": "test_trap[composite-A]",
    "ntx_image_epilogue": "test_trap[image_epilogue-A]",
    "ntx_mlp_forward": "test_trap[mlp_forward_float32-A]",
    "ntx_gemm_f32": "test_trap[gemm_f32-A]",
    "ntx_gemm_f32_ex": "test_trap[gemm_f32_ex_split_accumulate-A]",
    "ntx_render_rays": "test_trap[render_float32-A]",
    "ntx_render_instanced": "test_trap[instancer_dense-A]",
    "ntx_instancer_model_input": "test_trap[instancer_sparse_shadows-A]",
    "ntx_train_step_gradients": "test_trap[train_chain-A]",
    "ntx_trainer_adam_step": "test_trap[train_flex-A]",
    "ntx_train_forward": "test_trap[split_chain-A]",
    "ntx_train_backward": "test_trap[split_flex-A]",
    "ntx_trainer_stash_gradients": "test_trap[coarse_fine_shared-A]",
    "ntx_train_forward_instanced": "test_trap[instanced_chain-B]",
    "ntx_set_weights_device": "test_hand_off_in_stream_order[A]",
    "ntx_gather_image": "test_gather_image_on_a_side_stream[A-801-None]",
    "ntx_gather_image_ex": "test_gather_image_on_a_side_stream[A-4001-16]",
    "ntx_allreduce_mean_f32": "test_gradient_allreduce_on_a_side_stream[A]",
    "ntx_trainer_allreduce_gradients": "test_gradient_allreduce_on_a_side_stream[B]",
}
# entry -> (what it waits for, why).  "device": every stream of the device; "stream": the `stream` it was given, once; "setup": creation and
# setup entries, which allocate, upload with blocking copies (behind the null stream's work) and may free (which waits for the device).  The
# fourth convention of include/nerftex.h and docs/INTEGRATION_details.md carry the same table (tests/test_streams.py).
SYNCHRONISING = {
    "ntx_reserve": ("device", "frees the hit list a launch may still be walking"),
    "ntx_set_weights": ("device", "overwrites the weight images a launch may still be reading"),
    "ntx_trainer_get": ("device", "copies to host memory what steps on any stream leave"),
    "ntx_trainer_set": ("device", "overwrites vectors a step may still be reading"),
    "ntx_trainer_set_weights": ("device", "ntx_trainer_set of the weights"),
    "ntx_trainer_activation": ("device", "copies to host memory what the last step kept"),
    "ntx_train_forward_instanced": ("stream", "reads the live count back: the launches behind it are sized on the host"),
    "ntx_create": ("setup", "allocates and uploads the weight images"),
    "ntx_destroy": ("setup", "frees"),
    "ntx_comm_create": ("setup", "ncclCommInitRank"),
    "ntx_comm_destroy": ("setup", "ncclCommDestroy"),
    "ntx_trainer_create": ("setup", "allocates, zeroes and uploads"),
    "ntx_trainer_create_flex": ("setup", "allocates, zeroes and uploads"),
    "ntx_trainer_create_flex_ex": ("setup", "allocates, zeroes and uploads"),
    "ntx_trainer_destroy": ("setup", "frees"),
    "ntx_trainer_enable_param_gradients": ("setup", "allocates and uploads at the first enable"),
    "ntx_trainer_enable_input_gradients": ("setup", "allocates and uploads at the first enable"),
    "ntx_trainer_enable_gradients": ("setup", "allocates and uploads at the first enable"),
    "ntx_trainer_enable_instanced": ("setup", "allocates"),
    "ntx_instancer_create": ("setup", "allocates and uploads"),
    "ntx_instancer_destroy": ("setup", "frees"),
    "ntx_instancer_reserve": ("setup", "frees and allocates the workspace"),
    "ntx_instancer_set_mesh": ("setup", "frees, allocates and uploads"),
    "ntx_instancer_set_meshes": ("setup", "frees, allocates and uploads"),
    "ntx_instancer_set_parameter_textures": ("setup", "frees, allocates and uploads"),
    "ntx_instancer_set_mesh_textures": ("setup", "frees, allocates and uploads"),
}


def stream_entries(header=HEADER):
    """Names of the prototypes of include/nerftex.h with an `ntx_stream` parameter."""
    text = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    return sorted({m.group(1) for m in re.finditer(r"\b(?:int|int64_t|size_t)\s+(ntx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S) if "ntx_stream" in m.group(2)})


def documented_table(path):
    """{entry: scope} of the synchronisation table in the header's fourth convention (rows `ntx_name   scope`) or in the integration notes
    (rows `| ntx_name | scope |`), between the markers `synchronisation table` and `end of table`."""
    text = open(path).read()
    m = re.search(r"synchronisation table(.*?)end of table", text, flags=re.S)
    assert m, f"{path}: no synchronisation table"
    return {r.group(1): r.group(2) for r in re.finditer(r"^[\s*|`]*(ntx_\w+)[\s|`]+(device|stream|setup)\b", m.group(1), flags=re.M)}


# ---- batches (numpy, no device) -------------------------------------------------------------------------------------------------------------
def camera_batch(seed, n_params, h=1, w=257):
    """257 camera rays of `tests.common.camera_rays` (the field of view widened: some miss the box) and one parameter row."""
    from tests.common import camera_rays
    (ro, rd, t, cone), _, _ = camera_rays(CAMERAS[seed], h, w)
    params = np.random.default_rng(100 + seed).uniform(0.2, 1.0, size=(1, max(n_params, 1))).astype(F)
    return dict(rays_o=ro, rays_d=rd, t=t, cone=np.ascontiguousarray(cone.reshape(-1)), params=params)


def camera_fair(b):
    culled = int(np.isinf(b["t"][:, 0]).sum())
    assert 0 < culled < len(b["t"]), "a render batch needs rays that hit and rays that miss"


def train_batch(seed, n, P, fam, mip=False):
    """`tests.test_gpu_train.batch` (an IPE trainer: `tests.train_common.mip_batch`, whose rows hold the blur parameter too) with seeded rays,
    all of which hit, from a camera that batch k moves 5 k % outwards: the origins differ between batches as well."""
    from nerf_tex_amd import synthetic
    from tests.train_common import targets
    f = synthetic.FAMILIES[fam]
    cam = tuple(float(c) * (1.0 + 0.05 * seed) for c in f["cam"])
    ro, rd, t, cone = synthetic.all_hit_rays(n, f["b_0"], f["b_1"], cam, seed=seed + 1)
    if mip:
        params = np.random.default_rng(seed).uniform(0.2, 1.5, size=(n, P)).astype(F)
    else:
        params = np.tile(np.asarray([f["params"]], F)[:, :P], (n, 1)) * np.random.default_rng(seed).uniform(0.8, 1.2, size=(n, P)).astype(F)
    color, alpha = targets(n, 50 + seed)
    return dict(rays_o=ro, rays_d=rd, t=t, cone=np.ascontiguousarray(np.asarray(cone, F).reshape(-1)), params=np.ascontiguousarray(params, F), color=color, alpha=alpha)


def train_fair(b):
    assert np.isfinite(b["t"]).all() and (b["t"][:, 1] > b["t"][:, 0]).all() and np.isfinite(b["params"]).all() and (b["alpha"] > 0).any()


def instanced_batch(seed, npar, n, S, live="some"):
    """`tests.instanced_train_common.instancer_buffers` as named arrays; live = "none": the same with no live sample (n_live = 0)."""
    from tests import instanced_train_common as itc
    bufs, hit, cone = itc.instancer_buffers(npar, 20 + seed, n, S)
    if live == "none":
        bufs, hit = itc.with_live_mask(bufs, hit, np.zeros((n, S), bool))
    targets = np.random.default_rng(70 + seed).uniform(0, 1, size=(n, 4)).astype(F)
    return dict(rays_d_map=bufs[0], pts=bufs[1], t=bufs[2], dists=bufs[3], color_last=bufs[4], alpha_last=bufs[5], alpha_weight=bufs[6],
                hit=np.asarray(hit, np.uint8), params_map=bufs[9], cone=cone, target=targets)


def instanced_fair(b, live="some"):
    from tests import instanced_train_common as itc
    m = itc.live_mask(b["hit"], b["dists"])
    assert (0 < m.sum() < m.size) if live == "some" else m.sum() == 0
    assert np.isfinite(b["pts"]).all() and np.isfinite(b["params_map"]).all()


def differ_everywhere(a, b):
    """Two batches of one case: the same names, shapes and types, and no array equal."""
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, k
        assert not np.array_equal(a[k], b[k]), f"input '{k}' is the same in both batches: a late copy of it could not be seen"


# ---- the delay ------------------------------------------------------------------------------------------------------------------------------
STATS = dict(cycles_per_ms=None, longest_ms=0.0)


def dev():
    import torch
    return torch.device("cuda", 0)


def calibrate():
    """Cycles of `torch.cuda._sleep` per millisecond, measured once with events."""
    import torch
    if STATS["cycles_per_ms"] is None:
        cycles = 1_000_000
        for _ in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(); torch.cuda._sleep(cycles); b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0:
                break
            cycles *= 4
        assert ms >= 5.0, f"torch.cuda._sleep({cycles}) took {ms} ms: it does not delay on this device"
        STATS["cycles_per_ms"] = cycles / ms
    return STATS["cycles_per_ms"]


def delay(ms, stream=None):
    """A kernel that keeps `stream` (None: the current one) busy for about `ms`."""
    import torch
    STATS["longest_ms"] = max(STATS["longest_ms"], float(ms))
    cycles = int(calibrate() * ms)
    if stream is None:
        torch.cuda._sleep(cycles)
    else:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(cycles)


def delay_ms(host_seconds):
    return max(MIN_DELAY_MS, DELAY_FACTOR * 1e3 * host_seconds)


PROBE_MS = 4.0
_PROBE = {}


def runs_beside(s, other=None):
    """Whether work on `s` completes while `other` (None: the null stream) is inside a delay.  A process has a few hardware queues and the
    runtime deals its streams onto them: two streams on one queue run in the order they were fed, whatever their flags say, and neither trap
    could see anything between them."""
    import torch
    if "x" not in _PROBE:
        _PROBE["x"] = torch.zeros(64, device=dev())
        _PROBE["x"].add_(1.0)                 # (the kernel is loaded)
    torch.cuda.synchronize()
    busy = torch.cuda.Event()
    with torch.cuda.stream(other if other is not None else torch.cuda.default_stream(dev())):
        torch.cuda._sleep(int(calibrate() * PROBE_MS))
        busy.record()
    with torch.cuda.stream(s):
        _PROBE["x"].add_(1.0)
    s.synchronize()
    free = not busy.query()
    torch.cuda.synchronize()
    return free


def side_stream(beside=()):
    """A new non-blocking stream that has been SEEN to run beside the null stream (and beside the streams of `beside`): the traps' precondition,
    checked for the very stream they use.  Streams that share a queue are kept until one is found, so that the next one lands elsewhere."""
    import torch
    held = []
    for _ in range(12):
        s = torch.cuda.Stream(device=dev())
        if all(runs_beside(s, o) for o in (None,) + tuple(beside)):
            return s
        held.append(s)
    raise AssertionError(f"none of {len(held)} new streams runs beside the null stream: the traps cannot see anything on this device")


# ---- cases ----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """setup() -> state (fresh handles); inputs(seed) -> {name: numpy array}, the calls' device inputs; outputs -> {name: (shape, dtype)} of
    result buffers the test owns (filled with SENTINEL in stream order right before the calls); run(state, bufs, outs) -> list of device tensors,
    everything enqueued on the current stream and nothing waited for; after(state) -> list of numpy arrays through the synchronising getters;
    fair(batch): what a batch has to hold for the case to mean anything (the poison passes it too).  traps: which traps the case runs under;
    armed: False where an entry waits for its stream on purpose (SYNCHRONISING), so that `armed` cannot hold past the wait."""

    def __init__(self, cid, setup, inputs, run, after=None, outputs=None, fair=None, traps="AB", armed=True, entries=()):
        self.id, self.setup, self.inputs, self.run, self.after, self.outputs, self.fair, self.traps, self.armed, self.entries = \
            cid, setup, inputs, run, after, outputs or {}, fair, traps, armed, entries


def st():
    import torch
    return torch.cuda.current_stream(dev()).cuda_stream


def to_device(batch):
    import torch
    return {k: torch.as_tensor(np.ascontiguousarray(v), device=dev()) for k, v in batch.items()}


def own_outputs(case):
    import torch
    dt = {"f": torch.float32, "u8": torch.uint8, "i32": torch.int32}
    return {k: torch.zeros(shape, device=dev(), dtype=dt[kind]) for k, (shape, kind) in case.outputs.items()}


def fill_outputs(outs):
    for o in outs.values():
        o.fill_(SENTINEL if o.is_floating_point() else 113)


def as_bytes(results):
    return [np.ascontiguousarray(r.cpu().numpy() if hasattr(r, "cpu") else r) for r in results]


def same_bytes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, i, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8 if g.dtype.itemsize == 1 else np.uint32) != w.reshape(-1).view(np.uint8 if w.dtype.itemsize == 1 else np.uint32))
            raise AssertionError(f"{what}: result {i} differs from the default-stream bits in {len(bad)} of {g.size} elements, first at {int(bad[0])}: "
                                 f"{g.reshape(-1)[bad[0]]!r} != {w.reshape(-1)[bad[0]]!r}")


_REFERENCE = {}


def reference(case):
    """The default-stream run: fresh handle, the calls on the history batch, then on the real one.  Returns (results as numpy, the host seconds
    the real calls took to enqueue, the host seconds until they had completed); computed once per case."""
    import torch
    if case.id not in _REFERENCE:
        state = case.setup()
        hist, real, outs = to_device(case.inputs(HISTORY)), to_device(case.inputs(REAL)), own_outputs(case)
        case.run(state, hist, outs)
        fill_outputs(outs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = case.run(state, real, outs)
        snaps = [r.clone() for r in res]
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res = as_bytes(snaps) + (as_bytes(case.after(state)) if case.after else [])
        assert any(np.abs(np.nan_to_num(r.astype(np.float64), posinf=0, neginf=0)).max() > 0 for r in res if r.size), "the reference results are all zero"
        _REFERENCE[case.id] = (res, t1 - t0, t2 - t0)
    return _REFERENCE[case.id]


def trap_a(case):
    import torch
    want, enqueue, _ = reference(case)
    state = case.setup()
    hist, bufs, staging, outs = to_device(case.inputs(HISTORY)), to_device(case.inputs(POISON)), to_device(case.inputs(REAL)), own_outputs(case)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    case.run(state, hist, outs)
    enqueue = max(enqueue, time.perf_counter() - t0)          # (this handle's first calls, placements included, count as well)
    torch.cuda.synchronize()
    s, armed = side_stream(), torch.cuda.Event()
    delay(delay_ms(enqueue), s)
    t0 = time.perf_counter()
    with torch.cuda.stream(s):
        armed.record(s)
        for k in bufs:
            bufs[k].copy_(staging[k])
        fill_outputs(outs)
        res = case.run(state, bufs, outs)
        snaps = [r.clone() for r in res]
    still_blocked, host_ms = not armed.query(), 1e3 * (time.perf_counter() - t0)
    s.synchronize()
    torch.cuda.synchronize()
    if case.armed:
        assert still_blocked, (f"delay too short ({delay_ms(enqueue):.0f} ms), or a call waited for the stream: `armed` had completed when the last call returned, "
                               f"{host_ms:.1f} ms after the first was made")
    same_bytes(as_bytes(snaps) + (as_bytes(case.after(state)) if case.after else []), want, f"{case.id}, late inputs")


def trap_b(case):
    import torch
    want, _, complete = reference(case)
    state = case.setup()
    hist, bufs, outs = to_device(case.inputs(HISTORY)), to_device(case.inputs(REAL)), own_outputs(case)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    case.run(state, hist, outs)
    torch.cuda.synchronize()
    complete = max(complete, time.perf_counter() - t0)        # (this handle's first calls, placements included, count as well)
    s, busy = side_stream(), torch.cuda.Event()
    first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    delay(delay_ms(complete))                 # (the calls have to COMPLETE inside it: the host time until the default-stream runs had)
    busy.record()
    t0 = time.perf_counter()
    with torch.cuda.stream(s):
        first.record(s)
        fill_outputs(outs)
        res = case.run(state, bufs, outs)
        snaps = [r.clone() for r in res]
        last.record(s)
    t1 = time.perf_counter()
    s.synchronize()
    still_busy, t2 = not busy.query(), time.perf_counter()
    torch.cuda.synchronize()
    assert still_busy, (f"delay too short ({delay_ms(complete):.0f} ms), or something waited for the null stream or the device: `busy` had completed behind s.synchronize() "
                        f"(the calls took the host {1e3 * (t1 - t0):.1f} ms to make and s {first.elapsed_time(last):.1f} ms to run; s.synchronize() returned after {1e3 * (t2 - t0):.1f} ms)")
    same_bytes(as_bytes(snaps) + (as_bytes(case.after(state)) if case.after else []), want, f"{case.id}, busy null stream")


# ---- the cases' bodies ------------------------------------------------------------------------------------------------------------------------
def _fp(a):
    return np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))


def _p(t):
    return t.data_ptr() if t is not None and t.numel() else None


def _lib():
    from nerf_tex_amd import _lib as lib
    return lib


def _check(rc):
    _lib().check(rc)


def _standalone_cases():
    from nerf_tex_amd import synthetic
    from oracle import nerftex_oracle as orc
    cases = []
    fam = synthetic.FAMILIES["fur"]
    H, W = 9, 13
    c2w, focal, b0, b1 = orc.look_at(fam["cam"], dtype=F), float(orc.focal_from_angle(W, fam["angle"] * 2)), fam["b_0"], fam["b_1"]
    none = lambda: None

    def ray_outs(n):
        return dict(rays_o=((n, 3), "f"), rays_d=((n, 3), "f"), t=((n, 2), "f"), cone=((n, 1), "f"))

    ray_ptrs = lambda o: (_p(o["rays_o"]), _p(o["rays_d"]), _p(o["t"]), _p(o["cone"]))

    def gen(state, b, o):
        _check(_lib().lib.ntx_generate_rays(_fp(c2w), H, W, focal, 5, H * W - 5, 0, _fp(b0), _fp(b1), 0.0, 0.0, *ray_ptrs(o), st()))
        return list(o.values())
    cases.append(Case("generate_rays", none, lambda seed: {}, gen, outputs=ray_outs(H * W - 5)))

    def gen_at(state, b, o):
        _check(_lib().lib.ntx_generate_rays_at(_fp(c2w), H, W, focal, _p(b["loc"]), H * W, 0, _fp(b0), _fp(b1), 0.0, 0.0, *ray_ptrs(o), st()))
        return list(o.values())
    cases.append(Case("generate_rays_at", none, lambda seed: dict(loc=np.random.default_rng(seed).uniform(0, (H, W), size=(H * W, 2)).astype(F)), gen_at,
                      outputs=ray_outs(H * W)))

    R, rank, run = 3, 1, 5

    def gen_strided(state, b, o):
        n = int(_lib().lib.ntx_shard_count(H * W, run, R, rank))
        assert n == o["t"].shape[0]
        _check(_lib().lib.ntx_generate_rays_strided(_fp(c2w), H, W, focal, rank * run, n, run, R * run, 0, _fp(b0), _fp(b1), 0.0, 0.0, *ray_ptrs(o), st()))
        return list(o.values())
    n_strided = sum(min(run, H * W - q * run) for q in range((H * W + run - 1) // run) if q % R == rank)
    cases.append(Case("generate_rays_strided", none, lambda seed: {}, gen_strided, outputs=ray_outs(n_strided)))

    cam = lambda seed: {k: v for k, v in camera_batch(seed, 1).items() if k in ("rays_o", "rays_d")}

    def aabb(state, b, o):
        _check(_lib().lib.ntx_aabb_intersect(_p(b["rays_o"]), _p(b["rays_d"]), b["rays_o"].shape[0], _fp(b0), _fp(b1), _p(o["t"]), st()))
        return [o["t"]]
    cases.append(Case("aabb_intersect", none, cam, aabb, outputs=dict(t=((257, 2), "f"))))

    def samples(seed, m=300, P=7):
        from tests.common import random_samples
        pos, d, par = random_samples(m, P, seed=3 + seed)
        return dict(pos=pos, dirs=d, params=par)

    def fourier(state, b, o):
        _check(_lib().lib.ntx_fourier_features(_p(b["pos"]), 300, 3, 10, _p(o["ff"]), st()))
        return [o["ff"]]
    cases.append(Case("fourier_features", none, lambda seed: dict(pos=samples(seed)["pos"]), fourier, outputs=dict(ff=((300, 63), "f"))))

    hits = lambda seed: dict(t=train_batch(seed, 90, 7, "carpet")["t"])

    def depths(state, b, o):
        _check(_lib().lib.ntx_sample_depths(_p(b["t"]), 90, 33, _lib().FLAG_PERTURB, 7, None, _p(o["z"]), st()))
        return [o["z"]]
    cases.append(Case("sample_depths", none, hits, depths, outputs=dict(z=((90, 33), "f"))))

    def noise(state, b, o):
        opts = _lib().render_opts(raw_noise_std=0.5)
        _check(_lib().lib.ntx_sample_noise(90, 33, 7, C.byref(opts), _p(o["noise"]), st()))
        return [o["noise"]]
    cases.append(Case("sample_noise", none, lambda seed: {}, noise, outputs=dict(noise=((90, 33), "f"))))

    def pdf_inputs(seed, S=65, NI=32):
        from tests import kernel_emulation as emu
        from tests.test_gpu_standalone_edges import pdf_case
        t, w, u = pdf_case(S, NI, emu.PDF_PATTERNS[seed])
        return dict(t=np.ascontiguousarray(t, F), w=np.ascontiguousarray(w, F), u=np.ascontiguousarray(u, F))

    def pdf(state, b, o):                       # S = 65 crosses the 64-sample chunk; the coarse depths are placed again from t
        _check(_lib().lib.ntx_sample_pdf(_p(b["t"]), None, _p(b["w"]), _p(b["u"]), 48, 65, 32, _lib().FLAG_PERTURB, 9, None, _p(o["z"]), st()))
        return [o["z"]]
    cases.append(Case("sample_pdf_S65", none, pdf_inputs, pdf, outputs=dict(z=((48, 97), "f"))))

    def comp_inputs(seed):
        from tests.test_gpu_standalone_edges import composite_inputs
        color, sigma, z, rays_d = composite_inputs(37, 65, 40 + seed)
        return dict(color=color, sigma=sigma, z=z, rays_d=rays_d)

    def comp(state, b, o):
        _check(_lib().lib.ntx_composite(_p(b["color"]), _p(b["sigma"]), _p(b["z"]), _p(b["rays_d"]), 37, 65, _lib().FLAG_COMPOSITE_BKGD, _lib().f3((0.2, 0.5, 1.0)),
                                        _p(o["c"]), _p(o["a"]), _p(o["w"]), st()))
        return [o["c"], o["a"], o["w"]]
    cases.append(Case("composite", none, comp_inputs, comp, outputs=dict(c=((37, 3), "f"), a=((37,), "f"), w=((37, 65), "f"))))

    def epilogue(state, b, o):
        _check(_lib().lib.ntx_image_epilogue(_p(b["rgba"]), 19, 23, 2, 1, _p(o["f32"]), _p(o["u8"]), st()))
        return [o["f32"], o["u8"]]
    cases.append(Case("image_epilogue", none, lambda seed: dict(rgba=np.random.default_rng(seed).uniform(0, 1, size=(19, 23, 4)).astype(F)), epilogue,
                      outputs=dict(f32=((10, 12, 4), "f"), u8=((10, 12, 4), "u8"))))

    def model_state():
        from tests.common import make_model
        return make_model((1, 6), dense_media=True)[0]

    for precision in ("float32", "fp16x3"):
        def mlp(model, b, o, flags=_lib().PRECISIONS[precision]):
            _check(_lib().lib.ntx_mlp_forward(model.ctx(0), _p(b["pos"]), _p(b["dirs"]), _p(b["params"]), 300, flags, _p(o["color"]), _p(o["sigma"]), st()))
            return [o["color"], o["sigma"]]
        cases.append(Case(f"mlp_forward_{precision}", model_state, samples, mlp, outputs=dict(color=((300, 3), "f"), sigma=((300,), "f"))))

    M, N, K = 300, 200, 77                    # tests/test_gpu_train.py test_gemm_kernel_against_float64's first shape

    def gemm_inputs(seed):
        rng = np.random.default_rng(M + N + K + seed)
        return dict(A=rng.normal(size=(M, K)).astype(F), B=rng.normal(size=(K, N)).astype(F), bias=rng.normal(size=N).astype(F))

    def gemm(state, b, o):
        _check(_lib().lib.ntx_gemm_f32(_p(b["A"]), K, 1, _p(b["B"]), N, 0, _p(o["C"]), N + 3, M, N, K, _p(b["bias"]), 1, st()))
        return [o["C"]]
    cases.append(Case("gemm_f32", none, gemm_inputs, gemm, outputs=dict(C=((M, N + 3), "f"))))

    M2, N2, K2, chunk, splits = 70, 52, 100, 40, 3     # the weight-gradient form: A [K][M], K cut into 40 + 40 + 20, partial sums and column sums

    def gemm_ex_inputs(seed):
        rng = np.random.default_rng(900 + seed)
        return dict(A=rng.normal(size=(K2, M2)).astype(F), B=rng.normal(size=(K2, N2)).astype(F), C=rng.normal(size=(splits, M2, N2)).astype(F))

    def gemm_ex(state, b, o):                   # accumulate: C is read and written
        _check(_lib().lib.ntx_gemm_f32_ex(_p(b["A"]), M2, 0, _p(b["B"]), N2, _p(b["C"]), N2, M2, N2, K2, None, 0, None, 0, 1, splits, chunk, M2 * N2, _p(o["colsum"]), st()))
        return [b["C"], o["colsum"]]
    cases.append(Case("gemm_f32_ex_split_accumulate", none, gemm_ex_inputs, gemm_ex, outputs=dict(colsum=((splits, N2), "f"))))
    return cases


def _render_cases():
    def make(cid, npar=(1, 6), kind="ParamNerf", mip=False, **rkw):
        P = sum(npar) + (1 if mip else 0)

        def setup():
            from nerf_tex_amd.renderer import MipRenderer, Renderer
            from tests.common import make_model
            model = make_model(npar, kind=kind, dense_media=True)[0]
            return (MipRenderer if mip else Renderer)(model=model, n_samples=33, **rkw)

        def run(r, b, o):
            out = r(b["rays_o"][None], b["rays_d"][None], b["t"][None], parameters=b["params"], cone_scale=b["cone"][None, :, None], seed=11, training=False,
                    composite_bkgd=True, bkgd_color=[0.2, 0.5, 1.0])
            return [out[k] for k in sorted(out)] + [r._status]
        return Case(cid, setup, lambda seed: camera_batch(seed, P), run, fair=camera_fair)

    return [make("render_float32", perturb=False), make("render_fp16x3", perturb=False, precision="fp16x3"),
            make("render_perturb_noise", perturb=True, raw_noise_std=0.5),
            make("render_importance", perturb=True, n_importance=16),
            make("render_mip", npar=(1, 3), kind="IPE", mip=True, perturb=False, blur_idx=0),
            make("render_generic_family", npar=(3, 2), perturb=False)]


def instancer_scene(shadows):
    """The scene of tests/test_gpu_instancer.py test_instance_renderer_end_to_end (30 patches, nearest, a culling mesh) as an `Instancer`."""
    from tests.test_gpu_instancer import gpu_instancer
    from tests.test_oracle_instancer import random_scene
    spec0 = random_scene(21, k=30, method="nearest", mesh=True)
    box = dict(b_0=spec0.b_0.tolist(), b_1=spec0.b_1.tolist())
    tr = [np.linalg.inv(m.astype(np.float64)).astype(F) for m in spec0.inv]
    return gpu_instancer(box, tr, textures=["", "", "", "", "light"], instance_sampling_method="nearest", mesh=(spec0.mesh_v, spec0.mesh_f), cast_shadow_rays=shadows)


INST_N, INST_S, INST_STEP, INST_PATCH = 150, 64, 0.04, 0.35


def instancer_batch(seed):
    from tests.test_oracle_instancer import random_rays
    o, d = random_rays(21 + seed, INST_N)
    rng = np.random.default_rng(2 + seed)
    tt = np.tile(F([[1.0, 2.0]]), (INST_N, 1)) * F(1 + 0.125 * seed); tt[7 + seed] = np.inf
    return dict(rays_o=o, rays_d=d, params=np.repeat(rng.uniform(0.2, 1, size=(1, 7)), INST_N, 0).astype(F), cone=rng.uniform(1e-3, 5e-3, size=INST_N).astype(F), t=tt)


def _instancer_cases():
    def direct(cid, shadows, sparse):
        def setup():
            from tests.common import make_model
            return SimpleNamespace(inst=instancer_scene(shadows), model=make_model((1, 6), dense_media=True)[0])

        def run(s, b, o):                       # ntx_instancer_model_input -> ntx_render_instanced, the ten buffers made here in stream order
            import torch
            lib, n, S, P = _lib(), INST_N, INST_S, 7
            z = lambda *shape, dt=torch.float32: torch.zeros(shape, device=dev(), dtype=dt)
            rdm, pts, t, dists, cl, al, aw, iid, hit, pm = z(n, S, 3), z(n, S, 3), z(n, S), z(n, S), z(n, 3), z(n), z(n, S), z(n, S, dt=torch.int32), z(n, dt=torch.uint8), z(n, S, P)
            status, color, alpha = z(1, dt=torch.int32), z(n, 3), z(n)
            opts = lib.render_opts(flags=lib.OPT_INSTANCER_SPARSE if sparse else 0)
            _check(lib.lib.ntx_instancer_model_input(s.inst._h, _p(b["rays_o"]), _p(b["rays_d"]), _p(b["params"]), n, S, INST_STEP, 77, C.byref(opts), _p(rdm), _p(pts), _p(t),
                                                     _p(dists), _p(cl), _p(al), _p(aw), _p(iid), _p(hit), _p(pm), _p(status), st()))
            _check(lib.lib.ntx_render_instanced(s.model.ctx(0), _p(rdm), _p(pts), _p(t), _p(dists), _p(cl), _p(al), _p(aw), _p(iid), _p(hit), _p(pm), _p(b["cone"]), n, S, -1,
                                                INST_PATCH, 40.0, lib.FLAG_CHECK_NUMERICS, lib.f3((1, 1, 1)), None, None, _p(color), _p(alpha), _p(status), st()))
            return [color, alpha, dists, hit, cl, al, status] + ([] if sparse else [rdm, pts, t, aw, iid, pm])
        return Case(cid, setup, lambda seed: {k: v for k, v in instancer_batch(seed).items() if k != "t"}, run)

    def end_to_end(cid, shadows, sparse):
        def setup():
            from nerf_tex_amd.renderer import InstanceRenderer
            from tests.common import make_model
            return InstanceRenderer(model=make_model((1, 6), dense_media=True)[0], n_samples=INST_S, instancer=instancer_scene(shadows), patch_scale=INST_PATCH,
                                    step_size=INST_STEP, render_chunk=64, density_scale=40.0)

        def run(r, b, o):
            out = r(b["rays_o"][None], b["rays_d"][None], b["t"][None], parameters=b["params"][:1], cone_scale=b["cone"][None, :, None], instancer_seed=77, instancer_sparse=sparse)
            return [out["color_pred"], out["alpha_pred"], r._status]
        # the class finds the hit rays with nonzero(), which waits for its stream: the late inputs are still late, `armed` cannot hold
        return Case(cid, setup, instancer_batch, run, armed=False)

    return [direct("instancer_dense", False, False), direct("instancer_sparse_shadows", True, True),
            end_to_end("instance_renderer_sparse", False, True), end_to_end("instance_renderer_dense_shadows", True, False)]


TRAIN_N, TRAIN_S = 45, 37
FLEX_ARCH = dict(width=64, depth=3, skips=[1])
BRANCH_ARCH = dict(depth=3, width=64, skips=[1], color_depth=1, param_depth=2, param_width=128)


def make_trainer(kind, **kw):
    """A fresh trainer of `kind` on its fixed model: chain (8 x 256, (1, 6)), flex (3 x 64), branch (parameter branches), ipe (the mip chain)."""
    from nerf_tex_amd.train import BranchTrainer, FlexTrainer, Trainer
    from tests.common import make_model
    kw = dict(dict(max_rays=TRAIN_N, n_samples=TRAIN_S, perturb=False), **kw)
    if kind == "chain":
        return Trainer(make_model((1, 6), dense_media=True)[0], **kw)
    if kind == "flex":
        return FlexTrainer(make_model((1, 6), dense_media=True, arch=FLEX_ARCH)[0], **kw)
    if kind == "branch":
        return BranchTrainer(make_model((1, 4), dense_media=True, arch=BRANCH_ARCH)[0], **kw)
    if kind == "ipe":
        return Trainer(make_model((1, 3), kind="IPE", dense_media=True)[0], blur_idx=0, **kw)
    raise KeyError(kind)


TRAIN_BATCH = {"chain": (7, "carpet", False), "flex": (7, "carpet", False), "branch": (5, "grass", False), "ipe": (5, "grass_filtered", True)}


def trainer_batch(kind, seed, n=TRAIN_N):
    P, fam, mip = TRAIN_BATCH[kind]
    return train_batch(seed, n, P, fam, mip)


def the_loss():
    from tests.train_common import make_loss
    return make_loss("alpha_smape")[1]


def step_args(b):
    return b["rays_o"], b["rays_d"], b["t"], b["params"], b["cone"], b["color"], b["alpha"]


def trainer_state(tr):
    return [tr.gradients(), tr.weights(), *tr.adam_state()]


def two_steps(tr, b, o=None):
    """`gradients_step` + `apply_gradients`, twice."""
    res = []
    for k in range(2):
        res += list(tr.gradients_step(*step_args(b), the_loss(), seed=3 + k))
        tr.apply_gradients()
    return res


def quadratic_cotangents(color, alpha, b):
    """dL/d predictions of mean((c - color_true)^2) + mean((a - alpha_true)^2), made by torch on the current stream."""
    return 2.0 * (color - b["color"]) / color.numel(), 2.0 * (alpha - b["alpha"]) / alpha.numel()


def _trainer_cases():
    cases = []
    for kind in ("chain", "flex", "branch", "ipe"):
        cases.append(Case(f"train_{kind}", lambda kind=kind: make_trainer(kind), lambda seed, kind=kind: trainer_batch(kind, seed), two_steps, after=trainer_state,
                          fair=train_fair))

    def split(tr, b, o):
        color, alpha = tr.forward(*step_args(b)[:5], seed=3)
        d_color, d_alpha = quadratic_cotangents(color, alpha, b)
        tr.backward(d_color, d_alpha)
        tr.apply_gradients()
        return [color, alpha]
    for kind in ("chain", "flex"):
        cases.append(Case(f"split_{kind}", lambda kind=kind: make_trainer(kind), lambda seed, kind=kind: trainer_batch(kind, seed), split, after=trainer_state, fair=train_fair))

    def with_modes(mode):
        def run(tr, b, o):
            res = list(tr.gradients_step(*step_args(b), the_loss(), seed=3))
            res += [tr.parameter_gradients(), *tr.ray_gradients()]
            if mode is True:
                tr.apply_gradients()
            return res
        return run
    for kind in ("chain", "flex"):
        for name, mode in (("mode1", True), ("mode2", "only")):
            cases.append(Case(f"gradients_{name}_{kind}", lambda kind=kind, mode=mode: make_trainer(kind, param_gradients=mode, input_gradients=mode),
                              lambda seed, kind=kind: trainer_batch(kind, seed), with_modes(mode), after=trainer_state, fair=train_fair))

    def coarse_fine():
        from nerf_tex_amd.train import CoarseFineTrainer
        from tests.common import make_model
        return CoarseFineTrainer(make_model((1, 6), dense_media=True)[0], None, max_rays=TRAIN_N, n_samples=21, n_importance=16, perturb=True)

    def coarse_fine_steps(tr, b, o):
        res = []
        for k in range(2):
            res += list(tr.gradients_step(*step_args(b), the_loss(), seed=3 + k))
            tr.apply_gradients()
        return res + [tr.last_z]
    cases.append(Case("coarse_fine_shared", coarse_fine, lambda seed: trainer_batch("chain", seed), coarse_fine_steps, after=lambda tr: trainer_state(tr.fine), fair=train_fair))

    INST = dict(chain=(1, 6), flex=(1, 6))

    def instanced(kind, live, modes):
        def setup():
            return make_trainer(kind, max_rays=23, n_samples=70, instanced=True, **(dict(param_gradients=True, input_gradients=True) if modes else {}))

        def run(tr, b, o):
            bufs = (b["rays_d_map"], b["pts"], b["t"], b["dists"], b["color_last"], b["alpha_last"], b["alpha_weight"], None, None, b["params_map"])
            color, alpha = tr.forward_instanced(bufs, b["cone"], patch_scale=0.09, density_scale=20.0, hit=b["hit"])
            tr.backward(2.0 * (color - b["target"][:, :3]) / color.numel(), 2.0 * (alpha - b["target"][:, 3]) / alpha.numel())
            res = [color, alpha]
            if modes:
                res += [tr.sample_parameter_gradients(), *tr.sample_input_gradients()]
            tr.apply_gradients()
            return res
        inputs = lambda seed: instanced_batch(seed, INST[kind], 23, 70, live if seed == REAL else "some")
        fair = instanced_fair if live == "some" else None             # (n_live = 0: only the real batch; tests/test_streams.py looks at the pair)
        # the forward waits for its stream on purpose (SYNCHRONISING): under trap A the inputs are still late, `armed` cannot hold behind the wait
        return Case(f"instanced_{kind}" + ("_none_live" if live == "none" else "") + ("_modes" if modes else ""), setup, inputs, run, after=trainer_state, fair=fair, armed=False)
    for kind in ("chain", "flex"):
        cases += [instanced(kind, "some", False), instanced(kind, "none", False), instanced(kind, "some", True)]

    def autograd_plain(tr, b, o):
        import torch
        from nerf_tex_amd.autograd import DifferentiableRender
        params = b["params"].detach().clone().requires_grad_(True)
        color, alpha = DifferentiableRender(tr)(b["rays_o"], b["rays_d"], b["t"], params, b["cone"], seed=3)
        loss = torch.mean((color - b["color"]) ** 2) + torch.mean((alpha - b["alpha"]) ** 2)
        loss.backward()
        tr.apply_gradients()
        return [color.detach(), alpha.detach(), loss.detach(), params.grad]
    cases.append(Case("autograd_render", lambda: make_trainer("flex", param_gradients=True), lambda seed: trainer_batch("flex", seed), autograd_plain, after=trainer_state,
                      fair=train_fair))

    def autograd_instanced(tr, b, o):
        import torch
        from nerf_tex_amd.autograd import DifferentiableInstanceRender
        field = b["params_map"].detach().clone().requires_grad_(True)
        bufs = (b["rays_d_map"], b["pts"], b["t"], b["dists"], b["color_last"], b["alpha_last"], b["alpha_weight"], None, None, field)
        color, alpha = DifferentiableInstanceRender(tr, patch_scale=0.09, density_scale=20.0)(bufs, b["cone"], hit=b["hit"])
        loss = torch.mean((color - b["target"][:, :3]) ** 2) + torch.mean((alpha - b["target"][:, 3]) ** 2)
        loss.backward()
        tr.apply_gradients()
        return [color.detach(), alpha.detach(), loss.detach(), field.grad]
    cases.append(Case("autograd_instance_render", lambda: make_trainer("flex", max_rays=23, n_samples=70, param_gradients=True),
                      lambda seed: instanced_batch(seed, (1, 6), 23, 70), autograd_instanced, after=trainer_state, fair=instanced_fair, armed=False))
    return cases


_CASES = None
CASE_IDS = (["generate_rays", "generate_rays_at", "generate_rays_strided", "aabb_intersect", "fourier_features", "sample_depths", "sample_noise", "sample_pdf_S65", "composite",
             "image_epilogue", "mlp_forward_float32", "mlp_forward_fp16x3", "gemm_f32", "gemm_f32_ex_split_accumulate"] +
            ["render_float32", "render_fp16x3", "render_perturb_noise", "render_importance", "render_mip", "render_generic_family"] +
            ["instancer_dense", "instancer_sparse_shadows", "instance_renderer_sparse", "instance_renderer_dense_shadows"] +
            [f"train_{k}" for k in ("chain", "flex", "branch", "ipe")] + ["split_chain", "split_flex"] +
            [f"gradients_{m}_{k}" for k in ("chain", "flex") for m in ("mode1", "mode2")] + ["coarse_fine_shared"] +
            [f"instanced_{k}{v}" for k in ("chain", "flex") for v in ("", "_none_live", "_modes")] + ["autograd_render", "autograd_instance_render"])


def cases():
    """{id: Case}, built on first use (the bodies import the package, which needs the built library)."""
    global _CASES
    if _CASES is None:
        built = _standalone_cases() + _render_cases() + _instancer_cases() + _trainer_cases()
        _CASES = {c.id: c for c in built}
        assert list(_CASES) == CASE_IDS, (sorted(set(_CASES) ^ set(CASE_IDS)), "CASE_IDS names the cases in the order they are built")
    return _CASES


def trap_ids():
    """(case id, trap) of tests/test_gpu_streams.py::test_trap, without building a case."""
    return [(cid, trap) for cid in CASE_IDS for trap in "AB"]
