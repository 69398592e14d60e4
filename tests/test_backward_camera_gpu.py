"""Camera gradients of an EXACT frame on the MI355X (include/gsplat.h, gs_backward_camera*): the float64 reference of
tests/test_backward_camera_cpu.py, the edges of the block sum and of the reduce, the exact zeros of the two conventions, one
set of bits whatever produced the rows, the translation identity on the GPU's own numbers, central differences of the GPU's
own forward for cam_pos, the refusals, the unsynchronised training chain and the torch bindings.  Every case is one small
frame.

view and proj get no central-difference test on purpose: on the CPU frame their h and 2h differences disagree by 2-8 %
(every splat moves, so order and tile decisions flip inside the step); for them the float64 reference and the identity are
the check."""
import ctypes as C
import functools
import itertools
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, assert_posed, camera_params, known_answer_scene, load_scene
from test_backward_cpu import batch_edge_scene, padded_cloud, truncated_scene
from test_backward_gpu import KERNELS
from test_backward_cpu import extreme_cloud
from frame64 import weights
from test_backward_camera_cpu import CAMERA_FLOATS, PROJ_CLIP_Z, VIEW_BOTTOM_ROW, camera_reference
from test_loss_cpu import BG

pytestmark = pytest.mark.gpu

# |gpu[k] - want[k]| <= TAU * S[k], S[k] = sum_g |C[g][k]| the float64 reference's sum of absolute per-splat terms: 4 x the
# worst max_k |gpu - want| / S measured over the cases of test_against_the_float64_reference on its first green run, 1.397e-6
# at ragged@pose sh 2 (profiles/camera_grad_cost.txt lists every case) -- a few float32 roundings of a sum's scale.  Far
# inside the 2e-3 of a column's scale that test_backward_gpu.compare_with_reference grants the per-splat gradients these
# sums are built from.
TAU = 5.6e-6
SENTINEL = np.float32(-12345.5)
P = lambda a: a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case_scene(oracle_mod, name):
    """(aos, w, h, cam) of a case: a scene of load_scene, or 'extreme', 'truncated', 'batch_edges', 'one_splat'."""
    if name == "extreme":
        return extreme_cloud() + ({},)
    if name == "truncated":
        return truncated_scene() + ({},)
    if name == "batch_edges":
        return batch_edge_scene(oracle_mod)[:3] + ({},)
    if name == "one_splat":
        return known_answer_scene((2.0,)) + ({},)
    return load_scene(name)


def drawn_with_backward(aos, w, h, sh_mode=0, seed=1, cam=None, **kw):
    """A context that drew the frame and ran r.backward(weights(h, w, seed)): (renderer, scene, dL/d(record))."""
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **(cam or {}))
    r = make_renderer(sc, w, h, **kw)
    r.draw(sc)
    return r, sc, r.backward(*weights(h, w, seed))


def reference_of(oracle_mod, tmp_path, name, sh_mode, seed=1):
    """want, S of a case (shared by every test that needs it, computed once)."""
    aos, w, h, cam = case_scene(oracle_mod, name)
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
    p = camera_params(oracle_mod, sc, w, h)
    if cam:
        assert_posed(p)
    wr, wd = weights(h, w, seed)
    want, S, _ = camera_reference((name, sh_mode, seed), tmp_path, p, aos, wr, wd)
    return want, S


def check_against(got, want, S, what):
    """|got - want| <= TAU * S per component, exactly 0 where S is 0; prints the worst ratio first (the figure
    profiles/camera_grad_cost.txt records)."""
    got = got.astype(np.float64)
    assert np.all(np.isfinite(got)), what
    live = S > 0
    ratio = np.abs(got[live] - want[live]) / S[live]
    print(f"camera-grad-ratio {what}: max |gpu - want| / S = {ratio.max():.3e} (component {int(np.flatnonzero(live)[ratio.argmax()])})")
    assert np.all(got[~live] == 0), (what, got[~live])
    assert np.all(ratio <= TAU), (what, np.flatnonzero(live)[ratio > TAU], ratio.max())


# ---- 1. against the float64 reference ---------------------------------------------------------------------------------------

CASES = [("ragged", 0), ("ragged", 1), ("ragged", 2), ("dense", 0), ("extreme", 0), ("extreme", 1), ("extreme", 2),
         ("ragged@pose", 0), ("ragged@pose", 1), ("ragged@pose", 2), ("ragged@garden", 0), ("truncated", 0), ("batch_edges", 0)]


@pytest.mark.parametrize("scene,sh_mode", CASES)
def test_against_the_float64_reference(oracle_mod, tmp_path, scene, sh_mode):
    """backwardCamera() behind r.backward(weights(h, w, 1)) against the column sums of the float64 per-splat contributions,
    within TAU of S per component."""
    aos, w, h, cam = case_scene(oracle_mod, scene)
    r, _, _ = drawn_with_backward(aos, w, h, sh_mode, 1, cam)
    got = r.backwardCamera()
    r.cleanup()
    want, S = reference_of(oracle_mod, tmp_path, scene, sh_mode)
    assert np.count_nonzero(S) >= 20
    check_against(got, want, S, f"{scene} sh{sh_mode}")


# ---- 2. block and reduce edges ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filler", ["behind", "outside"])
@pytest.mark.parametrize("n", [6001, 262_145, 300_000])
def test_block_and_reduce_edges(oracle_mod, tmp_path, n, filler):
    """The ragged cloud scattered over n records that emit nothing (padded_cloud: live splats on both sides of the reduce
    threads' boundaries): 24, 1025 and 1172 blocks, so k_bwd_camera_reduce gives a thread per = 1 and per = 2 blocks, a
    ragged last slice and threads with none.  The answer is the unpadded cloud's."""
    aos, w, h = SCENES["ragged"]()
    cloud, pos = padded_cloud(aos, n, seed=n, filler=filler)
    blocks = (n + 255) // 256
    assert (blocks + 1023) // 1024 == (1 if n == 6001 else 2) and blocks == {6001: 24, 262_145: 1025, 300_000: 1172}[n]
    r, _, _ = drawn_with_backward(cloud, w, h)
    got = r.backwardCamera()
    r.cleanup()
    want, S = reference_of(oracle_mod, tmp_path, "ragged", 0)
    check_against(got, want, S, f"padded {n} {filler}")


def test_one_splat(oracle_mod, tmp_path):
    """N = 1: one thread of one block holds everything, the other 255 contribute zeros."""
    aos, w, h, _ = case_scene(oracle_mod, "one_splat")
    r, _, _ = drawn_with_backward(aos, w, h)
    got = r.backwardCamera()
    r.cleanup()
    want, S = reference_of(oracle_mod, tmp_path, "one_splat", 0)
    assert np.count_nonzero(S) >= 10
    check_against(got, want, S, "one splat")


# ---- 3. exact zeros ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh_mode", [0, 2])
def test_exact_zeros(oracle_mod, sh_mode):
    """The view's bottom row and the projection's clip-z row are +0.0 (as uint32), the cam_pos block too in sh_mode 2; the
    other live entries are not."""
    aos, w, h, cam = load_scene("ragged@pose")
    r, _, _ = drawn_with_backward(aos, w, h, sh_mode, 1, cam)
    got = bits(r.backwardCamera())
    r.cleanup()
    assert np.all(got[VIEW_BOTTOM_ROW] == 0) and np.all(got[PROJ_CLIP_Z] == 0)
    assert np.all(got[32:35] == 0) == (sh_mode == 2)
    rest = np.setdiff1d(np.arange(32), VIEW_BOTTOM_ROW + PROJ_CLIP_Z)
    assert np.all(got[rest] != 0)


def test_nothing_drawn_gives_zeros():
    """A cloud entirely behind the camera: GS_OK and 35 x +0.0, from both entry points."""
    torch = pytest.importorskip("torch")
    w, h = 64, 48
    cloud = np.tile(gs.makeGaussian((0.1, -0.2, -5.0), (0.05, 0.04, 0.03), sh0=(0.3, 0.2, 0.1, 0.7)).astype(np.float32), (300, 1))
    r, _, g = drawn_with_backward(cloud, w, h)
    assert r.timings().num_sort_elements == 0 and not g.any()
    out = np.full(CAMERA_FLOATS, SENTINEL, np.float32)
    assert _lib.lib().gs_backward_camera(r._ctx.handle, P(out)) == _lib.GS_OK
    assert np.all(bits(out) == 0)
    dev = torch.full((CAMERA_FLOATS,), float(SENTINEL), device="cuda")
    torch.cuda.synchronize()
    r.backwardCameraDevice(dev.data_ptr())
    r.synchronize()
    assert np.all(bits(dev.cpu().numpy()) == 0)
    r.cleanup()


# ---- 4. one set of bits -----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pose_answer():
    """backwardCamera() of ragged@pose, sh 0, weights seed 1, on a default context."""
    aos, w, h, cam = load_scene("ragged@pose")
    r, _, _ = drawn_with_backward(aos, w, h, 0, 1, cam)
    got = r.backwardCamera()
    r.cleanup()
    assert np.count_nonzero(got) == 27
    return got


def test_every_forward_gives_the_same_bits():
    """ALL_SORTS x KERNELS, both tile orders and the three GS_COUNT_* modes: the same 35 words."""
    aos, w, h, cam = load_scene("ragged@pose")
    base = bits(pose_answer())
    variants = [dict(sort=s, kernel=k) for s, k in itertools.product(ALL_SORTS, KERNELS)] + \
               [dict(order=o) for o in (gs.GS_TILE_ORDER_LONGEST_FIRST, gs.GS_TILE_ORDER_RASTER)] + \
               [dict(count=c) for c in (gs.GS_COUNT_AUTO, gs.GS_COUNT_PER_PASS, gs.GS_COUNT_FED)]
    for kw in variants:
        r, _, _ = drawn_with_backward(aos, w, h, 0, 1, cam, **kw)
        got = r.backwardCamera()
        r.cleanup()
        assert np.array_equal(bits(got), base), kw


def test_every_backward_form_and_entry_point_gives_the_same_bits():
    """After backward, backwardVisible whole and backwardVisible with max_rows = |V| // 2 (the blend backward writes every
    row whatever max_rows is); the host and the device entry point; two calls in a row; before and after a
    gs_set_resolution away and back; a context that shares the scene."""
    torch = pytest.importorskip("torch")
    aos, w, h, cam = load_scene("ragged@pose")
    base = bits(pose_answer())
    wr, wd = weights(h, w, 1)
    r, sc, _ = drawn_with_backward(aos, w, h, 0, 1, cam)
    assert np.array_equal(bits(r.backwardCamera()), base) and np.array_equal(bits(r.backwardCamera()), base)
    dev = torch.full((CAMERA_FLOATS,), float(SENTINEL), device="cuda")
    torch.cuda.synchronize()
    r.backwardCameraDevice(dev.data_ptr())
    r.synchronize()
    assert np.array_equal(bits(dev.cpu().numpy()), base)
    r.draw(sc)
    ids, _, count = r.backwardVisible(wr, wd)
    assert count == len(ids) > 100
    assert np.array_equal(bits(r.backwardCamera()), base), "visible, whole"
    r.draw(sc)
    ids, _, count2 = r.backwardVisible(wr, wd, max_rows=count // 2)
    assert count2 == count and len(ids) == count // 2 and r.lastStatus == _lib.GS_WARN_OVERFLOW
    assert np.array_equal(bits(r.backwardCamera()), base), "visible, max_rows = |V| // 2"
    # another resolution and back: the scratch is freed and allocated again
    L = _lib.lib()
    assert L.gs_set_resolution(r._ctx.handle, 160, 96) == _lib.GS_OK
    r.width, r.height = 160, 96
    r.draw(make_scene(aos, 160, 96, **cam))
    r.backward(*weights(96, 160, 1))
    assert not np.array_equal(bits(r.backwardCamera()), base)
    assert L.gs_set_resolution(r._ctx.handle, w, h) == _lib.GS_OK
    r.width, r.height = w, h
    r.draw(sc)
    r.backward(wr, wd)
    assert np.array_equal(bits(r.backwardCamera()), base), "after gs_set_resolution away and back"
    # a context over the same uploaded scene
    other = gs.Renderer(w, h, warmup_frames=0)
    other.init(sc.getResourceManager())
    other.initForScene(share_with=r)
    other.draw(sc)
    other.backward(wr, wd)
    assert np.array_equal(bits(other.backwardCamera()), base), "gs_share_scene"
    other.cleanup()
    r.cleanup()


# ---- 5. translation identity on the GPU's own numbers -----------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["ragged@pose", "ragged@garden"])
def test_translation_identity(scene):
    """Moving camera and cloud together changes nothing: sum_g dL/dpos_g[j] + dcam[j] - sum_{r<3} dview[12 + r] view[j * 4
    + r] = 0 within TAU of the sum of the absolute terms, dL/dpos from backward() summed in float64 on the host."""
    aos, w, h, cam = load_scene(scene)
    r, sc, g = drawn_with_backward(aos, w, h, 0, 1, cam)
    c = r.backwardCamera().astype(np.float64)
    r.cleanup()
    view = sc.getCamera().getViewMatrix().astype(np.float64).reshape(16)
    g = g.astype(np.float64)
    for j in range(3):
        terms = [g[:, j].sum(), c[32 + j]] + [-c[12 + k] * view[j * 4 + k] for k in range(3)]
        scale = np.abs(g[:, j]).sum() + abs(c[32 + j]) + sum(abs(c[12 + k] * view[j * 4 + k]) for k in range(3))
        print(f"camera-grad-identity {scene} j={j}: {abs(sum(terms)) / scale:.3e} of the absolute terms")
        assert scale > 0 and abs(sum(terms)) <= TAU * scale, (j, terms, scale)


# ---- 6. central differences of the GPU's own forward, cam_pos ---------------------------------------------------------------

@pytest.mark.parametrize("scene", ["ragged@pose", "ragged@garden"])
def test_central_differences_for_cam_pos(scene):
    """dL/dcam_pos against central differences of L = sum w * RGBA32F + sum v * depth of the GPU's own EXACT frame under
    a moved cam_pos (the view matrix stays: cam_pos is the SH direction's origin alone), absolute steps h = 0.002 and 2h.
    All three entries are kept: the two differences agree to 1 % of the largest |fd|, and the gradient matches to 2 % of
    it."""
    aos, w, h, cam = load_scene(scene)
    sc = make_scene(aos, w, h, **cam)
    check_cam_pos_central_differences(make_renderer(sc, w, h), sc, w, h, scene)


def check_cam_pos_central_differences(r, sc, w, h, what):
    """The body of test_central_differences_for_cam_pos on a renderer made for the scene sc (cleaned up here)."""
    r.setOutputs(rgba32f=True, depth=True)
    camera = sc.getCamera()
    view, proj, pos = camera.getViewMatrix(), camera.getProjectionMatrix(), np.asarray(camera.getPosition(), np.float32)
    wr, wd = weights(h, w, 2)

    def loss(cam_pos):
        r.drawCamera(view, proj, cam_pos, 0)
        return float((r.readOutput(gs.GS_OUTPUT_RGBA32F).astype(np.float64) * wr).sum() +
                     (r.readOutput(gs.GS_OUTPUT_DEPTH).astype(np.float64) * wd).sum())

    r.drawCamera(view, proj, pos, 0)
    r.backward(wr, wd)
    grad = r.backwardCamera()[32:35].astype(np.float64)
    fd = np.zeros((2, 3))
    for i, step in enumerate((0.002, 0.004)):
        for k in range(3):
            hi, lo = pos.copy(), pos.copy()
            hi[k] += np.float32(step)
            lo[k] -= np.float32(step)
            fd[i, k] = (loss(hi) - loss(lo)) / (float(hi[k]) - float(lo[k]))
    r.cleanup()
    top = np.abs(fd[0]).max()
    print(f"camera-grad-fd {what}: fd(h) {fd[0]}, fd(2h) {fd[1]}, gradient {grad}")
    assert top > 0 and np.all(np.abs(fd[0] - fd[1]) <= 0.01 * top), (fd, top)
    assert np.all(np.abs(grad - fd[0]) <= 0.02 * top), (grad, fd[0], top)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------

def test_refusals():
    """Every refusal of the header, with its message behind the call's name, and nothing written to a sentinel-filled
    output: no frame; a frame but no backward; gs_visible_count alone; backwardVisibleDevice with max_rows = 0; a new frame,
    an upload, a row upload or new tile rows since the backward; a band of tile rows; a FAST context; a NULL pointer."""
    torch = pytest.importorskip("torch")
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, np.float32)
    n = len(aos)
    sc = make_scene(aos, w, h)
    L = _lib.lib()
    wr, wd = weights(h, w, 3)
    out = np.full(CAMERA_FLOATS, SENTINEL, np.float32)
    dout = torch.full((CAMERA_FLOATS,), float(SENTINEL), device="cuda")
    grad, d_aos = torch.tensor(wr, device="cuda"), torch.tensor(aos, device="cuda")
    ids = torch.zeros(n, dtype=torch.int32, device="cuda")
    rows = torch.zeros(n, 84, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def refused(r, words, what):
        calls = {"gs_backward_camera": lambda: L.gs_backward_camera(r._ctx.handle, P(out)),
                 "gs_backward_camera_device": lambda: L.gs_backward_camera_device(r._ctx.handle, C.c_void_p(dout.data_ptr()))}
        for name, call in calls.items():
            assert call() == _lib.GS_ERR_INVALID, (what, name)
            msg = L.gs_last_error(r._ctx.handle).decode()
            assert msg.startswith(name + ": ") and words in msg, (what, name, msg)

    def visible(r, max_rows=n):
        r.backwardVisibleDevice(grad.data_ptr(), None, ids.data_ptr() if max_rows else None,
                                rows.data_ptr() if max_rows else None, max_rows, count.data_ptr())

    no_frame, no_backward = "no frame since the last gs_set_resolution", "no gs_backward* on this frame"
    r = make_renderer(sc, w, h)
    refused(r, no_frame, "no frame")
    r.draw(sc)
    refused(r, no_backward, "a frame but no backward")
    assert r.visibleCount() > 0
    refused(r, no_backward, "gs_visible_count alone")
    visible(r, 0)
    refused(r, no_backward, "backwardVisibleDevice with max_rows = 0")
    visible(r)
    good = r.backwardCamera()
    assert np.count_nonzero(good) >= 20
    for name, fn in (("gs_backward_camera", L.gs_backward_camera), ("gs_backward_camera_device", L.gs_backward_camera_device)):
        assert fn(r._ctx.handle, None) == _lib.GS_ERR_INVALID
        assert L.gs_last_error(r._ctx.handle).decode() == name + ": null gradient pointer"
    r.draw(sc)
    refused(r, no_backward, "a new frame since the backward")
    visible(r)
    r.uploadDevice(d_aos.data_ptr(), n)
    refused(r, no_frame, "an upload since the backward")
    r.draw(sc); visible(r)
    r.uploadRowsDevice(d_aos.data_ptr(), n, ids.data_ptr(), count.data_ptr(), n)
    refused(r, no_frame, "a row upload since the backward")
    r.draw(sc); visible(r)
    r.setTileRows(0, 2)
    refused(r, no_frame, "new tile rows since the backward")
    r.draw(sc)
    refused(r, "the context owns a subset of the tile rows", "a band context")
    r.setTileRows(0, r.sceneInfo().tiles_y)
    refused(r, no_frame, "rows set back, no frame since")
    r.draw(sc); visible(r)
    assert np.array_equal(bits(r.backwardCamera()), bits(good))               # a refusal costs the context nothing
    r.cleanup()
    fast = make_renderer(sc, w, h, mode=gs.GS_RENDER_FAST)
    fast.draw(sc)
    refused(fast, "only GS_RENDER_EXACT frames can be differentiated", "a FAST context")
    fast.cleanup()
    torch.cuda.synchronize()
    assert np.all(out == SENTINEL) and bool((dout == float(SENTINEL)).all())


def test_sharded_context_is_refused():
    """A context whose rows gs_dist_shard_rows has dealt (world size 1: it owns every row, so this refusal and no other
    answers) is refused by both entry points; in a child process, which alone holds the communicator."""
    code = textwrap.dedent("""
        import ctypes as C
        import numpy as np
        from vk3dgaussiansplatting_amd import _lib, makeGaussian
        _lib.preload_rccl()
        L = _lib.lib()
        w, h = 33, 17
        aos = np.ascontiguousarray(makeGaussian((0.0, 0.0, 2.0), (0.1, 0.1, 0.1))[None], dtype=np.float32)
        ctx = C.c_void_p()
        assert L.gs_create(None, C.byref(ctx)) == 0
        assert L.gs_upload_gaussians(ctx, aos.ctypes.data, 1) == 0 and L.gs_set_resolution(ctx, w, h) == 0
        out = np.full(35, -7.5, np.float32)
        ident = C.create_string_buffer(_lib.DIST_UNIQUE_ID_BYTES)
        assert L.gs_dist_unique_id(ident) == 0 and L.gs_dist_init(ctx, ident, 0, 1) == 0, L.gs_last_error(ctx)
        assert L.gs_dist_shard_rows(ctx, _lib.ROWS_CONTIGUOUS) == 0, L.gs_last_error(ctx)
        for name in ("gs_backward_camera", "gs_backward_camera_device"):
            assert getattr(L, name)(ctx, out.ctypes.data) == _lib.GS_ERR_INVALID
            msg = L.gs_last_error(ctx).decode()
            assert msg.startswith(name + ": ") and "sharded context" in msg, msg
        assert np.all(out == -7.5)
        assert L.gs_destroy(ctx) == 0
        print("refused-ok")
    """)
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0 and "refused-ok" in res.stdout, (res.stdout[-500:], res.stderr[-3000:])


# ---- 8. stream discipline ---------------------------------------------------------------------------------------------------

CHAIN_STEPS = 3
CHAIN_CAMERAS = (dict(pos=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0), dict(pos=(0.2, 0.1, -0.5), yaw=0.1, pitch=-0.05))


def run_camera_chain(how):
    """Three training steps on a fresh context -- frame -> loss -> gs_backward_visible_device -> gs_backward_camera_device
    -> gs_adam_rows_raw_device -> gs_upload_rows_device -- and the 35 words of every step.  how = 'waiting': a wait after
    every call (the answer); 'own_stream': back to back on the context's stream, one wait at the end; 'caller_stream': the
    same on a torch stream handed to gs_set_stream."""
    import torch
    from vk3dgaussiansplatting_amd.renderer import default_adam_params
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, np.float32)
    n = len(aos)
    scenes = [make_scene(aos, w, h, sh_mode=s % 2, **CHAIN_CAMERAS[s % 2]) for s in range(CHAIN_STEPS)]
    r = gs.Renderer(w, h, warmup_frames=0, record_timings=False)
    r.init(scenes[0].getResourceManager())
    r.initForScene(scenes[0])
    r.setOutputs(rgba32f=True)
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(11)
    target = torch.tensor(rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32), device=dev)
    records, raw = torch.tensor(aos, device=dev), torch.zeros(n, 84, device=dev)
    m, v = torch.zeros(n, 84, device=dev), torch.zeros(n, 84, device=dev)
    numbers, grad = torch.zeros(3, device=dev), torch.zeros(h, w, 4, device=dev)
    ids, rows = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, 84, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    cams = [torch.full((CAMERA_FLOATS,), float("nan"), device=dev) for _ in range(CHAIN_STEPS)]
    params = [default_adam_params(space="raw", step=s + 1) for s in range(CHAIN_STEPS)]
    torch.cuda.synchronize()
    r.rawFromRecordsDevice(records.data_ptr(), raw.data_ptr(), n)
    r.recordsFromRawDevice(raw.data_ptr(), records.data_ptr(), n)
    r.uploadDevice(records.data_ptr(), n)
    r.synchronize()
    stream = torch.cuda.Stream(device=dev) if how == "caller_stream" else None
    if stream is not None:
        r.setStream(stream.cuda_stream)

    def wait():
        if how == "waiting":
            r.synchronize()

    for s in range(CHAIN_STEPS):
        r.drawDevice(scenes[s], None, sync=False); wait()
        r.photometricLossDevice(None, target.data_ptr(), 0.2, BG, numbers.data_ptr(), grad.data_ptr()); wait()
        r.backwardVisibleDevice(grad.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), n, count.data_ptr()); wait()
        r.backwardCameraDevice(cams[s].data_ptr()); wait()
        r.adamRowsRawDevice(raw.data_ptr(), records.data_ptr(), m.data_ptr(), v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(),
                            count.data_ptr(), n, params[s]); wait()
        r.uploadRowsDevice(records.data_ptr(), n, ids.data_ptr(), count.data_ptr(), n); wait()
    r.synchronize()
    torch.cuda.synchronize()
    words = [bits(c.cpu().numpy()) for c in cams]
    if stream is not None:
        r.setStream(None)
    r.cleanup()
    return words


@pytest.mark.parametrize("how", ["own_stream", "caller_stream"])
def test_three_steps_enqueued_without_waiting(how):
    """The camera words of three training steps enqueued back to back, one wait at the end, equal those of the same steps
    with a wait after every call -- the first call's scratch allocation included.  The steps differ (Adam moves the
    cloud, the camera alternates), so the words of a step are not those of the step before."""
    pytest.importorskip("torch")
    want = run_camera_chain("waiting")
    for s in range(CHAIN_STEPS):
        assert np.all(np.isfinite(want[s].view(np.float32))) and np.count_nonzero(want[s]) >= 20
        assert s == 0 or not np.array_equal(want[s], want[s - 1])
    got = run_camera_chain(how)
    for s in range(CHAIN_STEPS):
        assert np.array_equal(got[s], want[s]), (how, "step", s)


# ---- 9. autograd ------------------------------------------------------------------------------------------------------------

def test_torch_camera_tensors():
    """render() with tensor cameras that require grad: .grad equals backwardCamera()'s blocks reshaped -- float32 on the
    device and float64 on the host, in the tensors' own shape -- for the dense and the sparse record gradient; numpy cameras
    leave the graph as it was (the records' gradient alone, the same bits)."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    aos, w, h, cam = load_scene("ragged@pose")
    sc = make_scene(aos, w, h, **cam)
    camera = sc.getCamera()
    view, proj, pos = camera.getViewMatrix(), camera.getProjectionMatrix(), camera.getPosition()
    wr, wd = weights(h, w, 1)
    want = pose_answer()
    r0, _, want_rec = drawn_with_backward(aos, w, h, 0, 1, cam)
    r0.cleanup()
    rr = autograd.make_renderer(w, h)
    twr, twd = torch.tensor(wr, device="cuda"), torch.tensor(wd, device="cuda")

    def loss_of(records, v, p, c, **kw):
        rgba, dep = autograd.render(records, v, p, c, 0, depth=True, renderer=rr, **kw)
        return (rgba * twr).sum() + (dep * twd).sum()

    for sparse in (False, True):
        rec = torch.tensor(aos, device="cuda", requires_grad=True)
        tv = torch.tensor(np.asarray(view, np.float32).reshape(4, 4), device="cuda", requires_grad=True)
        tp = torch.tensor(np.asarray(proj, np.float64).reshape(16), requires_grad=True)             # float64, on the host
        tc = torch.tensor(np.asarray(pos, np.float64), requires_grad=True)
        loss_of(rec, tv, tp, tc, sparse_grad=sparse).backward()
        assert tv.grad.shape == (4, 4) and tv.grad.dtype == torch.float32 and tv.grad.is_cuda
        assert tp.grad.shape == (16,) and tp.grad.dtype == torch.float64 and not tp.grad.is_cuda
        assert tc.grad.shape == (3,) and tc.grad.dtype == torch.float64 and not tc.grad.is_cuda
        assert np.array_equal(bits(tv.grad.cpu().numpy().reshape(16)), bits(want[0:16])), sparse
        assert np.array_equal(tp.grad.numpy(), want[16:32].astype(np.float64)), sparse
        assert np.array_equal(tc.grad.numpy(), want[32:35].astype(np.float64)), sparse
        if sparse:                        # to_dense() adds the rows to zeros: a -0.0 becomes +0.0, so by value
            assert np.array_equal(rec.grad.to_dense().cpu().numpy(), want_rec)
        else:
            assert np.array_equal(bits(rec.grad.cpu().numpy()), bits(want_rec))
    # only the camera position asks: view and proj get none
    tc = torch.tensor(np.asarray(pos, np.float32), device="cuda", requires_grad=True)
    tv = torch.tensor(np.asarray(view, np.float32), device="cuda")
    loss_of(torch.tensor(aos, device="cuda"), tv, proj, tc).backward()
    assert tv.grad is None and np.array_equal(bits(tc.grad.cpu().numpy()), bits(want[32:35]))
    # numpy cameras: the graph of before
    rec = torch.tensor(aos, device="cuda", requires_grad=True)
    rgba = autograd.render(rec, view, proj, pos, 0, renderer=rr)
    edges = [fn for fn, _ in rgba.grad_fn.next_functions if fn is not None]
    assert len(edges) == 1 and type(edges[0]).__name__ == "AccumulateGrad"                 # the records alone
    loss_of(rec, view, proj, pos).backward()
    assert np.array_equal(bits(rec.grad.cpu().numpy()), bits(want_rec))
    rr.cleanup()


def test_visible_adam_fills_camera_grad():
    """VisibleAdam.step(camera_grad=t) fills t with the words of backwardCamera() for the same frame and loss gradient, in
    the step's own enqueue chain."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    aos, w, h, cam = load_scene("ragged@pose")
    aos = np.ascontiguousarray(aos, np.float32)
    sc = make_scene(aos, w, h, **cam)
    camera = sc.getCamera()
    view, proj, pos = camera.getViewMatrix(), camera.getProjectionMatrix(), camera.getPosition()
    rng = np.random.default_rng(5)
    target = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    # the answer: the same frame, loss and visible backward on a context of its own
    r = make_renderer(sc, w, h)
    r.setOutputs(rgba32f=True)
    r.draw(sc)
    _, grad = r.photometricLoss(None, target, 0.2, None)
    r.backwardVisible(grad)
    want = r.backwardCamera()
    r.cleanup()
    assert np.count_nonzero(want) == 27
    rr = autograd.make_renderer(w, h)
    records = torch.tensor(aos, device="cuda")
    opt = autograd.VisibleAdam(records, renderer=rr)
    t = torch.full((CAMERA_FLOATS,), float("nan"), device="cuda")
    opt.step(view, proj, pos, 0, torch.tensor(target, device="cuda"), camera_grad=t)
    opt.stream.synchronize()
    assert np.array_equal(bits(t.cpu().numpy()), bits(want))
    with pytest.raises(ValueError):
        opt.step(view, proj, pos, 0, torch.tensor(target, device="cuda"), camera_grad=torch.zeros(34, device="cuda"))
    opt.stream.synchronize()
    rr.setStream(None)
    rr.cleanup()
