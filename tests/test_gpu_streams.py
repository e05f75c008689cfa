"""include/nerftex.h: "every entry point is asynchronous on `stream`" -- on a stream that is not the null stream.  `-m gpu`.

Every other GPU test passes `torch.cuda.current_stream()` outside any `torch.cuda.stream(...)`, i.e. the null stream, whose implicit
synchronisation orders a launch, a memset or a blocking copy that ignores the caller's stream all the same.  Here the calls run on a
non-blocking side stream under the two traps of tests/stream_common.py (late inputs; busy null stream), and the results must be the
default-stream run's, byte for byte.  The first two tests are the controls: without them the traps mean nothing."""

import numpy as np
import pytest

from tests import stream_common as sc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def dev():
    return torch.device("cuda", 0)


# ---- controls ---------------------------------------------------------------------------------------------------------------------------------
def test_control_default_stream_reads_the_old_batch_while_a_side_stream_is_delayed():
    """(a) of trap A: a copy queued on a delayed side stream has not happened when the default stream reads the buffer."""
    old, new = torch.full((4096,), 1.0, device=dev()), torch.full((4096,), 2.0, device=dev())
    torch.cuda.synchronize()
    s, armed = sc.side_stream(), torch.cuda.Event()
    sc.delay(sc.MIN_DELAY_MS, s)
    with torch.cuda.stream(s):
        armed.record(s)
        old.copy_(new)
    seen = old.clone().cpu()                                # default stream, plain torch
    assert not armed.query(), "the side stream's delay had ended before the default stream had read"
    s.synchronize()
    assert bool((seen == 1.0).all()) and bool((old == 2.0).all())


def test_control_side_stream_completes_while_the_null_stream_is_busy():
    """(b) of trap B: work on a side stream completes while the null stream is still inside its delay -- the two do not share a queue."""
    x = torch.arange(4096, device=dev(), dtype=torch.float32)
    (x * 2).clone()                                         # (the kernels are loaded: the control is about queues, not about a first launch)
    torch.cuda.synchronize()
    s, busy = sc.side_stream(), torch.cuda.Event()
    sc.delay(sc.MIN_DELAY_MS)
    busy.record()
    with torch.cuda.stream(s):
        y = (x * 2).clone()
    s.synchronize()
    assert not busy.query(), "the side stream waited for the null stream: trap B cannot be asserted on this device"
    torch.cuda.synchronize()
    assert bool((y == 2 * x).all())


# ---- cases 1-4: every entry under both traps -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,trap", sc.trap_ids(), ids=[f"{c}-{t}" for c, t in sc.trap_ids()])
def test_trap(cid, trap):
    case = sc.cases()[cid]
    (sc.trap_a if trap == "A" else sc.trap_b)(case)


# ---- case 5: first use -----------------------------------------------------------------------------------------------------------------------------
def _enable_both(tr):
    if hasattr(tr, "set_param_gradients"):
        tr.set_param_gradients(True); tr.set_input_gradients(True)
    else:
        tr.set_gradients(True, True)


# (id, the case whose calls and batch are taken, how the trainer is made -- None: the case's own setup --, what is enabled behind creation)
FIRST_USE = [("chain", "train_chain", None, None), ("flex", "train_flex", None, None), ("branch", "train_branch", None, None), ("ipe", "train_ipe", None, None),
             ("coarse_fine_stash", "coarse_fine_shared", None, None),
             ("chain_enable_instanced", "instanced_chain", lambda: sc.make_trainer("chain", max_rays=23, n_samples=70), lambda tr: tr.enable_instanced()),
             ("flex_first_instanced_step", "instanced_flex", lambda: sc.make_trainer("flex", max_rays=23, n_samples=70), None),
             ("chain_enable_gradients", "gradients_mode1_chain", lambda: sc.make_trainer("chain"), _enable_both),
             ("flex_enable_gradients", "gradients_mode1_flex", lambda: sc.make_trainer("flex"), _enable_both),
             ("flex_first_instanced_step_with_gradients", "instanced_flex_modes", lambda: sc.make_trainer("flex", max_rays=23, n_samples=70), _enable_both)]


@pytest.mark.parametrize("name,cid,make,enable", FIRST_USE, ids=[f[0] for f in FIRST_USE])
def test_first_step_on_a_side_stream_right_behind_creation(name, cid, make, enable):
    """A trainer is created while the null stream is busy -- and its instanced or gradient buffers enabled while it is busy again -- and takes
    its first steps on a side stream with no synchronisation in between: whatever creation zeroes (gradient, Adam's moments, the heads' tile,
    the chain's padded rows) and uploads, and whatever a first step places (the stash, the compaction's maps, the per-sample gradients), has
    to be there.  Creation may wait (it is a setup entry); the bits are what is asserted."""
    case = sc.cases()[cid]
    make = make or case.setup
    bufs = sc.to_device(case.inputs(sc.REAL))
    ref = make()
    if enable:
        enable(ref)
    want = sc.as_bytes(case.run(ref, bufs, {})) + sc.as_bytes(case.after(ref))
    torch.cuda.synchronize()
    s = sc.side_stream()
    sc.delay(sc.MIN_DELAY_MS)
    tr = make()
    if enable:
        sc.delay(sc.MIN_DELAY_MS)
        enable(tr)
    with torch.cuda.stream(s):
        res = [r.clone() for r in case.run(tr, bufs, {})]
    s.synchronize()
    torch.cuda.synchronize()
    sc.same_bytes(sc.as_bytes(res) + sc.as_bytes(case.after(tr)), want, f"first use: {name}")


def hand_off_sequence(tr, twin, r, b, view):
    """Two steps with Adam, the weights handed to the render context on the device, a render: everything on the current stream."""
    sc.two_steps(tr, b)
    twin.set_weights_from_trainer(tr)
    out = r(**view, training=False)
    return [out["color_pred"].clone(), out["alpha_pred"].clone()]


def hand_off_setup():
    from nerf_tex_amd.renderer import Renderer
    from tests.common import make_model
    tr = sc.make_trainer("chain")
    twin = make_model((1, 6), seed=9)[0]
    return tr, twin, Renderer(model=twin, n_samples=24, perturb=False)


def hand_off_view(b):
    return dict(rays_o=b["rays_o"][None], rays_d=b["rays_d"][None], t=b["t"][None], parameters=b["params"][:1], cone_scale=b["cone"].reshape(1, -1, 1))


def test_first_device_hand_off_of_a_context_on_a_side_stream():
    """The FIRST `ntx_set_weights_device` of a context (it places its gather tables) on a side stream while the null stream is busy, directly
    followed by a render on the same stream."""
    b = sc.to_device(sc.trainer_batch("chain", sc.REAL))
    want = sc.as_bytes(hand_off_sequence(*hand_off_setup(), b, hand_off_view(b)))
    tr, twin, r = hand_off_setup()
    torch.cuda.synchronize()
    s = sc.side_stream()
    sc.delay(sc.MIN_DELAY_MS)
    with torch.cuda.stream(s):
        got = hand_off_sequence(tr, twin, r, b, hand_off_view(b))
    s.synchronize()
    torch.cuda.synchronize()
    sc.same_bytes(sc.as_bytes(got), want, "first ntx_set_weights_device")


# ---- case 7: the hand-off in stream order ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trap", "AB")
def test_hand_off_in_stream_order(trap):
    """test_weights_reach_the_renderer_without_leaving_the_device on a side stream: step + Adam, `set_weights_from_trainer`, render."""
    def setup():
        tr, twin, r = hand_off_setup()
        warm = sc.to_device(sc.trainer_batch("chain", sc.HISTORY))
        twin.set_weights_from_trainer(tr)                      # (the tables are placed: the first use has its own test)
        r(**hand_off_view(warm), training=False)
        return tr, twin, r
    case = sc.Case("hand_off", setup, lambda seed: sc.trainer_batch("chain", seed), lambda state, b, o: hand_off_sequence(*state, b, hand_off_view(b)),
                   after=lambda state: sc.trainer_state(state[0]))
    (sc.trap_a if trap == "A" else sc.trap_b)(case)


# ---- case 6: host setters against work in flight -------------------------------------------------------------------------------------------------------
def test_set_blob_against_a_render_in_flight():
    """`Model.set_blob` (`ntx_set_weights`) while a render waits on a delayed side stream: the render in flight sees the OLD weights, the next
    one the new."""
    from nerf_tex_amd import synthetic
    from nerf_tex_amd.renderer import Renderer
    from tests.common import make_model
    model = make_model((1, 6), dense_media=True)[0]
    old, new = model.get_blob(), synthetic.synthetic_weights(model.layer_table(), seed=5, dense_media=True)
    r = Renderer(model=model, n_samples=33, perturb=False)
    b = sc.to_device(sc.camera_batch(sc.REAL, 7))
    call = lambda: [x.clone() for x in (lambda o: (o["color_pred"], o["alpha_pred"]))(r(b["rays_o"][None], b["rays_d"][None], b["t"][None], parameters=b["params"],
                                                                                        cone_scale=b["cone"][None, :, None], training=False))]
    want_old = sc.as_bytes(call())
    model.set_blob(new)
    want_new = sc.as_bytes(call())
    model.set_blob(old)
    torch.cuda.synchronize()
    assert want_old[0].tobytes() != want_new[0].tobytes()
    s = sc.side_stream()
    sc.delay(sc.MIN_DELAY_MS, s)
    with torch.cuda.stream(s):
        first = call()
    model.set_blob(new)                                         # from the host, the render still queued behind the delay
    with torch.cuda.stream(s):
        second = call()
    s.synchronize()
    torch.cuda.synchronize()
    sc.same_bytes(sc.as_bytes(first), want_old, "the render in flight when set_blob was called")
    sc.same_bytes(sc.as_bytes(second), want_new, "the render behind set_blob")


def test_load_state_dict_against_a_step_in_flight():
    """`Trainer.load_state_dict` (`ntx_trainer_set`) while a step waits on a delayed side stream: the step in flight is taken on the old state,
    then the new state is what the trainer holds and the next step starts from it."""
    b = sc.to_device(sc.trainer_batch("chain", sc.REAL))
    donor = sc.make_trainer("chain")
    sc.two_steps(donor, sc.to_device(sc.trainer_batch("chain", sc.HISTORY)))
    state = donor.state_dict()

    def sequence(tr, on):
        with on():
            first = [x.clone() for x in tr.gradients_step(*sc.step_args(b), sc.the_loss(), seed=3)]
            tr.apply_gradients()
        tr.load_state_dict(state)
        with on():
            second = [x.clone() for x in tr.gradients_step(*sc.step_args(b), sc.the_loss(), seed=4)]
            tr.apply_gradients()
        return first + second
    import contextlib
    ref = sc.make_trainer("chain")
    want = sc.as_bytes(sequence(ref, contextlib.nullcontext)) + sc.as_bytes(sc.trainer_state(ref))
    tr = sc.make_trainer("chain")
    torch.cuda.synchronize()
    s = sc.side_stream()
    sc.delay(sc.MIN_DELAY_MS, s)
    got = sequence(tr, lambda: torch.cuda.stream(s))
    s.synchronize()
    torch.cuda.synchronize()
    sc.same_bytes(sc.as_bytes(got) + sc.as_bytes(sc.trainer_state(tr)), want, "load_state_dict against a step in flight")


def parameter_texture_scene():
    """(instancer, rays and parameters, the setters to run against a call in flight): the scene of the direct instancer cases; the setters
    replace its culling mesh (`ntx_instancer_set_mesh`) and give it parameter textures (`ntx_instancer_set_parameter_textures`)."""
    import ctypes as C
    from nerf_tex_amd import _lib
    from nerf_tex_amd.instancer import _textures_struct, load_texture
    from tests.test_gpu_instancer import random_pixels, wavy_sheet
    sheet = wavy_sheet()
    b = {k: v for k, v in sc.instancer_batch(sc.REAL).items() if k in ("rays_o", "rays_d", "params")}

    def set_new(inst):
        inst.set_mesh(sheet[0], sheet[1])
        tex = load_texture(random_pixels(3))
        v, f, uv = (np.ascontiguousarray(a) for a in (sheet[0].astype(np.float32), sheet[1].astype(np.int32), sheet[2].astype(np.float32)))
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        _lib.check(_lib.lib.ntx_instancer_set_parameter_textures(inst._h, fp(v), fp(uv), v.shape[0], f.ctypes.data_as(C.POINTER(C.c_int32)), f.shape[0], float(inst.patch_max_extent),
                                                                 1, (C.c_int32 * 1)(0), _textures_struct(tex[:1]), 4, 24))
    return (lambda: sc.instancer_scene(False)), b, set_new, sc.INST_STEP


def mesh_texture_scene():
    """The scene of tests/test_gpu_instancer.py test_textured_auxiliary_meshes_bit_for_bit (a textured roof and a plain wall beside the culling
    mesh); the setters hand the same meshes over again with ANOTHER texture on the roof (`ntx_instancer_set_meshes`,
    `ntx_instancer_set_mesh_textures`)."""
    from nerf_tex_amd.instancer import Instancer, load_texture
    from tests.test_gpu_instancer import random_pixels
    from tests.test_oracle_instancer import random_rays, random_scene
    F = np.float32
    spec0 = random_scene(71, k=16, method="nearest", textures=("", "light"), mesh=True)
    tr = [np.linalg.inv(m.astype(np.float64)).astype(F) for m in spec0.inv]
    unit = lambda v: (np.asarray(v, F) / np.linalg.norm(v)).astype(F)
    roof = (F([[-1.5, -1.5, 0.9], [0.2, -1.5, 1.3], [0.2, 1.5, 1.3], [-1.5, 1.5, 0.9]]), [[0, 1, 2], [0, 2, 3]],
            np.stack([unit([-0.23, 0.05 * k, 0.97]) for k in range(4)]), F([[0.1, 0.05], [0.9, 0.2], [0.95, 0.85], [0.05, 0.9]]))
    wall = (F([[0.9, -1.5, -0.1], [0.9, 1.5, -0.1], [0.9, 1.5, 0.8], [0.9, -1.5, 0.8]]), [[0, 1, 2], [0, 2, 3]], np.tile(unit([-1, 0, 0.1]), (4, 1)))
    make = lambda: Instancer(spec0.b_0.tolist(), spec0.b_1.tolist(), textures=["", "light"], transformations=[m.tolist() for m in tr], instance_sampling_method="nearest",
                             mesh=(spec0.mesh_v, spec0.mesh_f), auxiliary_meshes=[(roof, random_pixels(5, h=10, w=14, c=3)), (wall, "")])
    n = 160
    o, d = random_rays(71, n)
    rng = np.random.default_rng(71)
    params = rng.uniform(0.2, 1.0, size=(n, 4)).astype(F)
    light = rng.normal(size=(n, 3)); light[:, 2] = np.abs(light[:, 2]) * 0.7 + 0.2
    params[:, 1:4] = light
    set_new = lambda inst: inst.set_meshes((spec0.mesh_v, spec0.mesh_f), [roof, wall], [load_texture(random_pixels(9, h=10, w=14, c=3)), None])
    return make, dict(rays_o=o, rays_d=d, params=params), set_new, 0.03


@pytest.mark.parametrize("scene", [parameter_texture_scene, mesh_texture_scene], ids=["mesh_and_parameter_textures", "meshes_and_mesh_textures"])
def test_instancer_setters_against_a_call_in_flight(scene):
    """The instancer's setup entries that replace device tables while an `ntx_instancer_model_input` waits on a delayed side stream: the call
    in flight sees the old scene, the next one the new."""
    from nerf_tex_amd import _lib
    make, batch, set_new, step = scene()
    b = sc.to_device(batch)
    n, S, P = b["rays_o"].shape[0], sc.INST_S, b["params"].shape[1]

    def march(inst):
        z = lambda *shape, dt=torch.float32: torch.zeros(shape, device=dev(), dtype=dt)
        out = [z(n, S, 3), z(n, S, 3), z(n, S), z(n, S), z(n, 3), z(n), z(n, S), z(n, S, dt=torch.int32), z(n, dt=torch.uint8), z(n, S, P), z(1, dt=torch.int32)]
        _lib.check(_lib.lib.ntx_instancer_model_input(inst._h, b["rays_o"].data_ptr(), b["rays_d"].data_ptr(), b["params"].data_ptr(), n, S, step, 77, None,
                                                      *[o.data_ptr() for o in out], torch.cuda.current_stream(dev()).cuda_stream))
        return [o.clone() for o in out]

    ref = make()
    want_old = sc.as_bytes(march(ref))
    set_new(ref)
    want_new = sc.as_bytes(march(ref))
    torch.cuda.synchronize()
    assert any(a.tobytes() != c.tobytes() for a, c in zip(want_old, want_new)), "the setters changed nothing the call reads"
    inst = make()
    torch.cuda.synchronize()
    s = sc.side_stream()
    sc.delay(sc.MIN_DELAY_MS, s)
    with torch.cuda.stream(s):
        first = march(inst)
    set_new(inst)                                               # from the host, the call still queued behind the delay
    with torch.cuda.stream(s):
        second = march(inst)
    s.synchronize()
    torch.cuda.synchronize()
    sc.same_bytes(sc.as_bytes(first), want_old, "the call in flight when the setters ran")
    sc.same_bytes(sc.as_bytes(second), want_new, "the call behind the setters")


# ---- case 8: two handles, two streams --------------------------------------------------------------------------------------------------------------------
def test_two_trainers_on_two_streams():
    """Two trainers of different architectures, enqueued alternately on two side streams, each behind its own delay: each gives its solo bits."""
    kinds = ("chain", "flex")
    batches = {k: sc.to_device(sc.trainer_batch(k, sc.REAL)) for k in kinds}
    want = {}
    for k in kinds:
        solo = sc.make_trainer(k)
        want[k] = sc.as_bytes(sc.two_steps(solo, batches[k])) + sc.as_bytes(sc.trainer_state(solo))
    trainers = {k: sc.make_trainer(k) for k in kinds}
    torch.cuda.synchronize()
    streams = {kinds[0]: sc.side_stream()}
    streams[kinds[1]] = sc.side_stream(beside=[streams[kinds[0]]])
    got = {k: [] for k in kinds}
    for k in kinds:
        sc.delay(sc.MIN_DELAY_MS, streams[k])
    for step in range(2):
        for k in kinds:
            with torch.cuda.stream(streams[k]):
                got[k] += [x.clone() for x in trainers[k].gradients_step(*sc.step_args(batches[k]), sc.the_loss(), seed=3 + step)]
                trainers[k].apply_gradients()
    for k in kinds:
        streams[k].synchronize()
    torch.cuda.synchronize()
    for k in kinds:
        sc.same_bytes(sc.as_bytes(got[k]) + sc.as_bytes(sc.trainer_state(trainers[k])), want[k], f"trainer {k} beside the other")


def test_two_render_contexts_on_two_streams():
    """Two render contexts (a tuned family and the generic one), alternately on two side streams, each behind its own delay."""
    cases = [sc.cases()["render_float32"], sc.cases()["render_generic_family"]]
    want = [sc.reference(c)[0] for c in cases]
    states = [c.setup() for c in cases]
    bufs = [sc.to_device(c.inputs(sc.REAL)) for c in cases]
    hist = [sc.to_device(c.inputs(sc.HISTORY)) for c in cases]
    for c, st_, h in zip(cases, states, hist):
        c.run(st_, h, {})
    torch.cuda.synchronize()
    streams = [sc.side_stream()]
    streams.append(sc.side_stream(beside=streams))
    for s in streams:
        sc.delay(sc.MIN_DELAY_MS, s)
    got = [None, None]
    for _ in range(2):                                           # (the second round repeats the first: same inputs, same bits)
        for i, c in enumerate(cases):
            with torch.cuda.stream(streams[i]):
                got[i] = [x.clone() for x in c.run(states[i], bufs[i], {})]
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for i, c in enumerate(cases):
        sc.same_bytes(sc.as_bytes(got[i]), want[i], f"{c.id} beside the other context")


# ---- case 9: one context moved between streams, legally ------------------------------------------------------------------------------------------------------
def test_one_context_moved_between_streams_with_an_event():
    """Render on s1, record an event, `s2.wait_event`, render on s2 (calls on one context must be stream-ordered: they are): both renders are
    the default-stream bits."""
    case = sc.cases()["render_float32"]
    want = sc.reference(case)[0]
    r = case.setup()
    b, h = sc.to_device(case.inputs(sc.REAL)), sc.to_device(case.inputs(sc.HISTORY))
    case.run(r, h, {})
    torch.cuda.synchronize()
    s1 = sc.side_stream()
    s2, done = sc.side_stream(beside=[s1]), torch.cuda.Event()
    sc.delay(sc.MIN_DELAY_MS, s1)
    with torch.cuda.stream(s1):
        first = [x.clone() for x in case.run(r, b, {})]
        done.record(s1)
    s2.wait_event(done)
    with torch.cuda.stream(s2):
        second = [x.clone() for x in case.run(r, b, {})]
    s1.synchronize(); s2.synchronize()
    torch.cuda.synchronize()
    sc.same_bytes(sc.as_bytes(first), want, "the render on s1")
    sc.same_bytes(sc.as_bytes(second), want, "the render on s2 behind the event")


# ---- case 10: the one-rank communicator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,run", [(801, None), (4001, 16)])
@pytest.mark.parametrize("trap", "AB")
def test_gather_image_on_a_side_stream(trap, n, run):
    """test_gather_image_on_a_one_rank_communicator and the uneven-shards branch (NTX_GATHER_FORCE_EXCHANGE) on a side stream."""
    from nerf_tex_amd.dist import Comm, ShardMap
    comm = Comm(0)
    shard = ShardMap(n, 1, run)
    try:
        def run_(state, b, o):
            return [comm.gather_image(b["local"], shard), comm.gather_image(b["local"], shard, force_exchange=True)]
        case = sc.Case(f"gather_{n}_{run}", lambda: None, lambda seed: dict(local=np.random.default_rng(seed).uniform(size=(n, 4)).astype(np.float32)), run_)
        (sc.trap_a if trap == "A" else sc.trap_b)(case)
        want = sc.reference(case)[0]
        assert np.array_equal(want[0], case.inputs(sc.REAL)["local"]) and np.array_equal(want[1], want[0])
    finally:
        torch.cuda.synchronize()
        comm.close()


@pytest.mark.parametrize("trap", "AB")
def test_gradient_allreduce_on_a_side_stream(trap):
    """test_gradient_allreduce_on_a_one_rank_communicator on a side stream: step, all-reduce (the mean over one rank), Adam."""
    from nerf_tex_amd.dist import Comm
    comm = Comm(0)
    try:
        def run_(tr, b, o):
            res = []
            for k in range(2):
                res += list(tr.gradients_step(*sc.step_args(b), sc.the_loss(), seed=3 + k))
                tr.sync_gradients(comm)
                tr.apply_gradients()
            return res
        case = sc.Case("allreduce", lambda: sc.make_trainer("chain"), lambda seed: sc.trainer_batch("chain", seed), run_, after=sc.trainer_state)
        (sc.trap_a if trap == "A" else sc.trap_b)(case)
        assert all(a.tobytes() == c.tobytes() for a, c in zip(sc.reference(case)[0], sc.reference(sc.cases()["train_chain"])[0])), "the mean over one rank changed the step"
    finally:
        torch.cuda.synchronize()
        comm.close()


def test_zz_report_the_delays():
    """Not a check of the library: prints what the module's delays were made of (the summary of a change quotes it)."""
    print(f"torch.cuda._sleep: {sc.calibrate():.0f} cycles per ms; longest delay used {sc.STATS['longest_ms']:.1f} ms")
    assert sc.STATS["cycles_per_ms"] > 0
