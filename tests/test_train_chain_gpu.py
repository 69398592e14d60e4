"""One training step as a real loop runs it on the MI355X (include/gsplat.h): gs_upload_gaussians_device (in place) ->
gs_render_device_async -> gs_photometric_loss_device(rgba32f = NULL) -> gs_backward_device or gs_backward_visible_device,
six steps enqueued back to back on one stream with no host wait in between, against the same six steps with a wait after
every call.  The header promises `enqueued on the context's stream, no host sync` for each of these; the other tests of
the loss and the backward wait between the calls, so work on a wrong stream (a captured graph, the tile-bucket sorter's
helper stream, a clear on the null stream, scratch allocated on first use) could hand stale data to the next call there
without any of them noticing."""
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_backward_gpu import SCENES
from test_loss_cpu import BG

pytestmark = pytest.mark.gpu

STEPS = 6
LAMBDA = 0.2
CAMERAS = (dict(pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0), dict(pos=(0.2, 0.1, -0.5), yaw=0.1, pitch=-0.05))
SENTINEL_ID = -559038737            # 0xDEADBEEF as the int32 torch fills with
SENTINEL_ROW = -12345.5
SENTINEL_COUNT = -1                 # 0xFFFFFFFF
OUTPUTS = ("numbers", "grad", "count", "ids", "rows", "dense")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def chain_inputs():
    """The dense cloud, its per-step change (positions and the SH constant term move; the size stays, so every upload after
    the renderer's own is the in-place one) and a target image, as float32 numpy arrays."""
    aos, w, h = SCENES["dense"]()
    rng = np.random.default_rng(11)
    delta = np.zeros_like(aos)
    delta[:, 0:3] = 0.004 * rng.standard_normal((len(aos), 3))
    delta[:, 12:15] = 0.02 * rng.standard_normal((len(aos), 3))
    target = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    return np.ascontiguousarray(aos, dtype=np.float32), delta, target, w, h


def new_renderer(sc, w, h, sort, timers):
    """make_renderer's context (timers on), or the same without timers: the passes replay as captured graphs."""
    if timers:
        r = make_renderer(sc, w, h, sort=sort)
    else:
        r = gs.Renderer(w, h, warmup_frames=0, sort_algorithm=sort, record_timings=False)
        r.init(sc.getResourceManager())
        r.initForScene(sc)
    r.setOutputs(rgba32f=True)
    return r


def run_chain(sort, timers, how):
    """The six steps on a fresh context; the outputs of every step back on the host as {name: [array per step]} (None where
    a step does not write that output).
    how = "waiting": the context's own stream, a wait after every torch op and every library call (the answer);
          "caller_stream": a torch stream handed to gs_set_stream, the torch ops of a step on it just before the calls
                           that read them, no host wait between the first upload and the final torch.cuda.synchronize();
          "own_stream": the context's own stream, the inputs prepared and waited for beforehand, the library calls back to
                        back, one wait at the end."""
    import torch
    aos, delta_np, target_np, w, h = chain_inputs()
    n = len(aos)
    scenes = [make_scene(aos, w, h, sh_mode=s % 3, **CAMERAS[s % 2]) for s in range(STEPS)]
    r = new_renderer(scenes[0], w, h, sort, timers)
    dev = torch.device("cuda:0")
    records0, delta = torch.tensor(aos, device=dev), torch.tensor(delta_np, device=dev)
    target0 = torch.tensor(target_np, device=dev)
    out = dict(
        numbers=[torch.full((3,), float("nan"), device=dev) for _ in range(STEPS)],
        grad=[torch.full((h, w, 4), float("nan"), device=dev) for _ in range(STEPS)],
        count=[torch.full((1,), SENTINEL_COUNT, dtype=torch.int32, device=dev) if s % 2 == 0 else None for s in range(STEPS)],
        ids=[torch.full((n,), SENTINEL_ID, dtype=torch.int32, device=dev) if s % 2 == 0 else None for s in range(STEPS)],
        rows=[torch.full((n, 84), SENTINEL_ROW, device=dev) if s % 2 == 0 else None for s in range(STEPS)],
        dense=[torch.full((n, 84), float("nan"), device=dev) if s % 2 == 1 else None for s in range(STEPS)])
    make_records = lambda s: records0 + float(s) * delta
    make_target = lambda s: target0 * (1.0 - 0.05 * s)
    waiting = how == "waiting"
    stream = torch.cuda.Stream(device=dev) if how == "caller_stream" else None
    keep = []                                                        # every step's inputs stay alive until the final wait
    if how == "own_stream":
        keep = [(make_records(s), make_target(s)) for s in range(STEPS)]
    torch.cuda.synchronize()
    if stream is not None:
        r.setStream(stream.cuda_stream)

    def wait():
        if waiting:
            torch.cuda.synchronize()
            r.synchronize()

    def steps():
        for s in range(STEPS):
            if how == "own_stream":
                records, target = keep[s]
            else:
                records = make_records(s)
                keep.append(records)
                wait()
            r.uploadDevice(records.data_ptr(), n)
            wait()
            r.drawDevice(scenes[s], None, sync=False)
            wait()
            if how != "own_stream":
                target = make_target(s)
                keep.append(target)
                wait()
            r.photometricLossDevice(None, target.data_ptr(), LAMBDA, BG, out["numbers"][s].data_ptr(), out["grad"][s].data_ptr())
            wait()
            if s % 2 == 0:
                r.backwardVisibleDevice(out["grad"][s].data_ptr(), None, out["ids"][s].data_ptr(), out["rows"][s].data_ptr(), n,
                                        out["count"][s].data_ptr())
            else:
                r.backwardDevice(out["grad"][s].data_ptr(), None, out["dense"][s].data_ptr())
            wait()

    if stream is not None:
        with torch.cuda.stream(stream):
            steps()
    else:
        steps()
    torch.cuda.synchronize()                                        # the one wait of the two unsynchronised forms
    r.synchronize()
    host = {name: [None if t is None else t.cpu().numpy() for t in out[name]] for name in OUTPUTS}
    if stream is not None:
        r.setStream(None)
    r.cleanup()
    return host


@functools.lru_cache(maxsize=None)
def answer(sort, timers):
    """The waiting form's outputs, checked not to be trivial: every step's numbers and image gradient are finite, non-zero
    and not the previous step's bits; an even step lists count > 0 splats, ascending, with non-zero rows that are not the
    bits of the even step before, and leaves the sentinel past count; an odd step's dense gradient likewise."""
    a = run_chain(sort, timers, "waiting")
    last = {}
    for s in range(STEPS):
        numbers, grad = a["numbers"][s], a["grad"][s]
        assert np.all(np.isfinite(numbers)) and numbers.all() and np.all(np.isfinite(grad)) and np.any(grad[..., :3] != 0)
        if s:
            assert not np.array_equal(bits(numbers), bits(a["numbers"][s - 1]))
            assert not np.array_equal(bits(grad), bits(a["grad"][s - 1]))
        if s % 2 == 0:
            count = int(a["count"][s].view(np.uint32)[0])
            ids, rows = a["ids"][s].view(np.uint32), a["rows"][s]
            assert 0 < count <= len(ids)
            assert np.all(np.diff(ids[:count].astype(np.int64)) > 0) and ids[count - 1] < len(ids)
            assert np.all(np.isfinite(rows[:count])) and np.any(rows[:count] != 0)
            assert np.all(a["ids"][s][count:] == SENTINEL_ID) and np.all(rows[count:] == np.float32(SENTINEL_ROW))
            new = (count, bits(ids[:count]), bits(rows[:count]))
            if "visible" in last:
                old = last["visible"]
                assert new[0] != old[0] or not np.array_equal(new[2], old[2])
            last["visible"] = new
        else:
            dense = a["dense"][s]
            assert np.all(np.isfinite(dense)) and np.any(dense != 0)
            if "dense" in last:
                assert not np.array_equal(bits(dense), bits(last["dense"]))
            last["dense"] = dense
    return a


def assert_same_bits(got, want, what):
    for s in range(STEPS):
        for name in ("numbers", "grad", "count", "dense"):
            if want[name][s] is not None:
                assert np.array_equal(bits(got[name][s]), bits(want[name][s])), (what, "step", s, name)
        if s % 2 == 0:
            count = int(want["count"][s].view(np.uint32)[0])
            assert np.array_equal(got["ids"][s][:count], want["ids"][s][:count]), (what, "step", s, "ids")
            assert np.array_equal(bits(got["rows"][s][:count]), bits(want["rows"][s][:count])), (what, "step", s, "rows")
            assert np.all(got["ids"][s][count:] == SENTINEL_ID), (what, "step", s, "ids past count")
            assert np.all(got["rows"][s][count:] == np.float32(SENTINEL_ROW)), (what, "step", s, "rows past count")


SORT_NAMES = {gs.GS_SORT_RADIX4: "radix4", gs.GS_SORT_TILE_BUCKET: "tile_bucket", gs.GS_SORT_RADIX4_SPLAT_FIRST: "radix4_splat_first",
              gs.GS_SORT_RADIX8: "radix8", gs.GS_SORT_RADIX8_SPLAT_FIRST: "radix8_splat_first"}
CONTEXTS = [pytest.param(sort, False, id=SORT_NAMES[sort] + "-no_timers") for sort in ALL_SORTS] + \
           [pytest.param(gs.GS_SORT_RADIX4, True, id="radix4-timers")]


@pytest.mark.parametrize("sort,timers", CONTEXTS)
def test_six_steps_enqueued_without_waiting(sort, timers):
    """Six steps on a caller's stream, nothing waited for between the first upload and one final synchronize -- the first
    in-place upload, the graph capture of the first frame and the scratch the first loss and the first backward allocate
    included -- give the bits of the same steps with a wait after every call: the three numbers and the image gradient of
    every step, count, ids[:count] and rows[:count] of the even steps (the sentinel untouched past count), the dense
    gradient of the odd ones.  Per step the records are records_0 + s * delta and the target a scaled image, both made by a
    torch op on that stream just before the call that reads them; the camera alternates between two poses and sh_mode
    cycles 0, 1, 2.  Every sorter without timers (the chain graph, the presort graph, the tile-bucket sorter's helper
    stream are different ways to enqueue a frame), and the default sorter with timers as make_renderer builds it."""
    pytest.importorskip("torch")
    want = answer(sort, timers)
    got = run_chain(sort, timers, "caller_stream")
    assert_same_bits(got, want, "caller's stream")


def test_six_steps_on_the_contexts_own_stream():
    """The same chain of library calls back to back on the context's own stream (no gs_set_stream), the inputs prepared and
    waited for beforehand: the same answer."""
    pytest.importorskip("torch")
    want = answer(gs.GS_SORT_RADIX4, True)
    got = run_chain(gs.GS_SORT_RADIX4, True, "own_stream")
    assert_same_bits(got, want, "own stream")
