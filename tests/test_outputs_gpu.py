"""The optional per-pixel outputs of a frame on the MI355X (gs_set_outputs, include/gsplat.h GS_OUTPUT_*): a known answer,
the RGBA8 frame unchanged by them in every launch shape, render mode and sorter, EXACT alpha and depth bit-identical to the C
restatement (tests/host/blend_outputs_ref.c, trusted by tests/test_outputs_cpu.py), FAST within stated tolerances, and the
C-ABI's behaviour around them."""
import ctypes as C

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import (SCENES, assert_posed, camera_params, known_answer_scene, load_scene, quantise,
                              reference_outputs)

pytestmark = pytest.mark.gpu

KERNELS = (gs.GS_RENDER_KERNEL_AUTO, gs.GS_RENDER_KERNEL_WAVE_1PX, gs.GS_RENDER_KERNEL_WAVE_2PX,
           gs.GS_RENDER_KERNEL_WAVE_4PX, gs.GS_RENDER_KERNEL_WORKGROUP, gs.GS_RENDER_KERNEL_WORKGROUP_8X8)


def outputs(r):
    return r.readOutput(gs.GS_OUTPUT_RGBA32F), r.readOutput(gs.GS_OUTPUT_DEPTH)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_known_answer():
    """Splats of opacity 0.5 on the centre pixel at view depths 2 and 4: exactly a = 0.5 and depth = 0.5 z for one, a = 0.75
    and depth = 0.5 z1 + 0.25 z2 for two, the premultiplied colour; an empty tile is (0, 0, 0, 0) / 0.  Every launch shape,
    both render modes."""
    for depths in ((2.0,), (2.0, 4.0)):
        aos, w, h = known_answer_scene(depths)
        sc = make_scene(aos, w, h)
        for mode in (gs.GS_RENDER_EXACT, gs.GS_RENDER_FAST):
            for kernel in KERNELS:
                r = make_renderer(sc, w, h, mode=mode, kernel=kernel)
                r.setOutputs(rgba32f=True, depth=True)
                r.draw(sc)
                f32, dep = outputs(r)
                col = r.debugRead(gs.BUF_COLOR)
                px = f32[h // 2, w // 2]
                if len(depths) == 1:
                    assert px[3] == np.float32(0.5) and dep[h // 2, w // 2] == np.float32(1.0), (mode, kernel, px, dep[h // 2, w // 2])
                    assert np.array_equal(px[:3], np.float32(0.5) * col[0, :3])
                else:
                    assert px[3] == np.float32(0.75) and dep[h // 2, w // 2] == np.float32(2.0), (mode, kernel, px, dep[h // 2, w // 2])
                    assert np.array_equal(px[:3], np.float32(0.5) * col[0, :3] + np.float32(0.25) * col[1, :3])
                assert not f32[:16, :16].any() and not dep[:16, :16].any()
                r.cleanup()


@pytest.mark.parametrize("sort", ALL_SORTS)
def test_rgba8_frame_is_unchanged_by_the_outputs(sort):
    """333 x 190, 6000 splats: for every launch shape and both render modes the RGBA8 frame with both outputs on is
    byte-identical to the frame without them, and quantising the float colour gives the same bytes; in EXACT mode every
    launch shape leaves the same output buffers, bit for bit."""
    aos, w, h = SCENES["ragged"]()
    sc = make_scene(aos, w, h)
    for mode in (gs.GS_RENDER_EXACT, gs.GS_RENDER_FAST):
        first = None
        for kernel in KERNELS:
            r = make_renderer(sc, w, h, mode=mode, sort=sort, kernel=kernel)
            plain = r.draw(sc).copy()
            r.setOutputs(rgba32f=True, depth=True)
            img = r.draw(sc)
            f32, dep = outputs(r)
            assert np.array_equal(img, plain), (mode, kernel)
            assert np.array_equal(quantise(f32), img), (mode, kernel)
            if mode == gs.GS_RENDER_EXACT:
                if first is None:
                    first = (f32, dep)
                else:
                    assert np.array_equal(bits(f32), bits(first[0])) and np.array_equal(bits(dep), bits(first[1])), kernel
            r.cleanup()


def _exact_against_restatement(oracle_mod, tmp_path, aos, w, h, sh_mode=0, kernels=(gs.GS_RENDER_KERNEL_AUTO,), cam=None):
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **(cam or {}))
    p = camera_params(oracle_mod, sc, w, h)
    if cam:
        assert_posed(p)
    ref = reference_outputs(tmp_path, p, aos)
    for kernel in kernels:
        r = make_renderer(sc, w, h, kernel=kernel)
        r.setOutputs(rgba32f=True, depth=True)
        img = r.draw(sc)
        f32, dep = outputs(r)
        assert np.array_equal(img, ref["rgba"]), kernel
        assert np.array_equal(bits(f32), bits(ref["rgba32f"])), kernel
        assert np.array_equal(bits(dep), bits(ref["depth"])), kernel
        r.cleanup()
    return sc, ref


@pytest.mark.parametrize("scene,sh_mode", [("ragged", 0), ("ragged", 1), ("ragged", 2), ("dense", 0), ("zero_det", 0),
                                           ("ragged@pose", 0), ("ragged@pose", 1), ("ragged@garden", 0),
                                           ("ragged@garden", 1)])
def test_exact_outputs_equal_the_restatement(oracle_mod, tmp_path, scene, sh_mode):
    """GS_RENDER_EXACT: colour, alpha and depth bit-identical to the C restatement over the oracle's intermediates -- the
    whole frame in every launch shape; all three SH modes, the dense early-out cloud, zero-determinant splats, and the
    ragged cloud in front of rotated, translated cameras (the depth row's every term counts)."""
    aos, w, h, cam = load_scene(scene)
    kernels = KERNELS if sh_mode == 0 else (gs.GS_RENDER_KERNEL_AUTO, gs.GS_RENDER_KERNEL_WAVE_2PX)
    _exact_against_restatement(oracle_mod, tmp_path, aos, w, h, sh_mode, kernels if cam or sh_mode == 0 else kernels[:1], cam)


def test_exact_outputs_bands_and_compact_rows(oracle_mod, tmp_path):
    """A band setTileRows(3, 8) writes exactly the full frame's rows 48 .. 127 and leaves the others zero; interleaved rows
    with compact output (gs_render_device) write the owned rows packed, equal to the full frame's rows."""
    import torch
    aos, w, h = SCENES["ragged"]()
    sc, ref = _exact_against_restatement(oracle_mod, tmp_path, aos, w, h)
    for kernel in (gs.GS_RENDER_KERNEL_AUTO, gs.GS_RENDER_KERNEL_WAVE_4PX):
        r = make_renderer(sc, w, h, kernel=kernel)
        r.setOutputs(rgba32f=True, depth=True)
        r.setTileRows(3, 8)
        r.draw(sc)
        f32, dep = outputs(r)
        rows = slice(48, 128)
        assert np.array_equal(bits(f32[rows]), bits(ref["rgba32f"][rows])) and np.array_equal(bits(dep[rows]), bits(ref["depth"][rows]))
        assert not f32[:48].any() and not f32[128:].any() and not dep[:48].any() and not dep[128:].any()
        # rank 1 of 3, interleaved, compact: owned tile rows 1, 4, 7, 10 packed at the top
        r.setOutputs(rgba32f=True, depth=True)          # zero-filled again
        r.setTileRowsInterleaved(1, 3, compact_output=True)
        img = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        r.drawDevice(sc, img.data_ptr())
        f32, dep = outputs(r)
        owned = [t for t in range((h + 15) // 16) if t % 3 == 1]
        for k, t in enumerate(owned):
            n = min(16, h - 16 * t)
            src, dst = slice(16 * t, 16 * t + n), slice(16 * k, 16 * k + n)
            assert np.array_equal(bits(f32[dst]), bits(ref["rgba32f"][src])), (kernel, t)
            assert np.array_equal(bits(dep[dst]), bits(ref["depth"][src])), (kernel, t)
            assert np.array_equal(img.cpu().numpy()[dst], ref["rgba"][src])
        assert not f32[16 * len(owned):].any()
        r.cleanup()


def test_exact_outputs_config_a_full_size(oracle_mod, tmp_path):
    """BASELINE config A (100k splats, 640 x 360) at full size, bit for bit."""
    aos, cfg = synth.generate_config("A")
    _exact_against_restatement(oracle_mod, tmp_path, aos, cfg["width"], cfg["height"],
                               kernels=(gs.GS_RENDER_KERNEL_AUTO, gs.GS_RENDER_KERNEL_WAVE_2PX))


@pytest.mark.parametrize("scene", ["ragged", "dense", "configA"])
def test_fast_outputs_within_tolerance(scene):
    """GS_RENDER_FAST against EXACT: alpha within 2/255 at every pixel; the expected depth (depth / alpha) within 1 %
    wherever both alphas exceed 0.05."""
    if scene == "configA":
        aos, cfg = synth.generate_config("A")
        w, h = cfg["width"], cfg["height"]
    else:
        aos, w, h = SCENES[scene]()
    sc = make_scene(aos, w, h)
    res = {}
    for mode in (gs.GS_RENDER_EXACT, gs.GS_RENDER_FAST):
        r = make_renderer(sc, w, h, mode=mode)
        r.setOutputs(rgba32f=True, depth=True)
        r.draw(sc)
        res[mode] = outputs(r)
        r.cleanup()
    (fe, de), (ff, df) = res[gs.GS_RENDER_EXACT], res[gs.GS_RENDER_FAST]
    assert np.max(np.abs(ff[..., 3] - fe[..., 3])) <= 2.0 / 255.0
    m = (fe[..., 3] > 0.05) & (ff[..., 3] > 0.05)
    assert m.any()
    ze, zf = de[m] / fe[..., 3][m], df[m] / ff[..., 3][m]
    assert np.max(np.abs(zf - ze) / ze) <= 0.01


def test_output_api_behaviour():
    """Default mask: nothing to read; unknown bits and which values, a short buffer, an output not enabled are refused;
    the buffers follow gs_set_resolution; mask 0 returns to RGBA8-only frames; gs_render_device_async + gs_synchronize
    leave the device buffer equal to gs_read_output; two contexts sharing a scene keep their own outputs; a sharded call
    with a non-zero mask is refused and enqueues nothing."""
    import torch
    L = _lib.lib()
    aos, w, h = SCENES["ragged"]()
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    ctx = r._ctx.handle
    buf = np.zeros((h, w, 4), np.float32)
    dev, size = C.c_void_p(), C.c_size_t()
    plain = r.draw(sc).copy()
    assert L.gs_read_output(ctx, gs.GS_OUTPUT_RGBA32F, buf.ctypes.data, buf.nbytes) == _lib.GS_ERR_INVALID
    assert L.gs_output_device(ctx, gs.GS_OUTPUT_DEPTH, C.byref(dev), C.byref(size)) == _lib.GS_ERR_INVALID
    assert L.gs_set_outputs(ctx, 4) == _lib.GS_ERR_INVALID and b"unknown" in L.gs_last_error(ctx)
    assert L.gs_set_outputs(ctx, gs.GS_OUTPUT_DEPTH) == _lib.GS_OK
    assert L.gs_read_output(ctx, gs.GS_OUTPUT_DEPTH, buf.ctypes.data, buf.nbytes) == _lib.GS_ERR_INVALID   # no frame yet
    r.draw(sc)
    assert L.gs_read_output(ctx, gs.GS_OUTPUT_RGBA32F, buf.ctypes.data, buf.nbytes) == _lib.GS_ERR_INVALID  # not enabled
    assert L.gs_read_output(ctx, 3, buf.ctypes.data, buf.nbytes) == _lib.GS_ERR_INVALID
    assert L.gs_read_output(ctx, 0, buf.ctypes.data, buf.nbytes) == _lib.GS_ERR_INVALID
    assert L.gs_read_output(ctx, gs.GS_OUTPUT_DEPTH, buf.ctypes.data, w * h * 4 - 1) == _lib.GS_ERR_INVALID
    assert L.gs_output_device(ctx, gs.GS_OUTPUT_DEPTH, C.byref(dev), C.byref(size)) == _lib.GS_OK and size.value == w * h * 4
    depth_only = r.readOutput(gs.GS_OUTPUT_DEPTH)
    assert depth_only.shape == (h, w) and depth_only.any()
    # resolution change: the buffers follow it (and must be rendered again before they are read)
    r.setOutputs(rgba32f=True, depth=True)
    w2, h2 = 200, 120
    r.width, r.height = w2, h2
    assert L.gs_set_resolution(ctx, w2, h2) == _lib.GS_OK
    assert L.gs_read_output(ctx, gs.GS_OUTPUT_DEPTH, buf.ctypes.data, buf.nbytes) == _lib.GS_ERR_INVALID
    sc2 = make_scene(aos, w2, h2)
    img2 = r.draw(sc2)
    f2, d2 = outputs(r)
    assert f2.shape == (h2, w2, 4) and d2.shape == (h2, w2) and np.array_equal(quantise(f2), img2)
    # async frame: the device buffers hold the frame once the stream has been waited for
    f_ptr, d_ptr = r.outputDevicePtr(gs.GS_OUTPUT_RGBA32F), r.outputDevicePtr(gs.GS_OUTPUT_DEPTH)
    out = torch.zeros((h2, w2, 4), dtype=torch.uint8, device="cuda")
    r.drawDevice(sc2, out.data_ptr(), sync=False)
    r.synchronize()
    host_f = np.zeros((h2, w2, 4), np.float32)
    host_d = np.zeros((h2, w2), np.float32)
    hip = C.CDLL("libamdhip64.so")                       # the runtime the library already runs on (by SONAME)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(host_f.ctypes.data, f_ptr, host_f.nbytes, 2) == 0     # hipMemcpyDeviceToHost
    assert hip.hipMemcpy(host_d.ctypes.data, d_ptr, host_d.nbytes, 2) == 0
    f_read, d_read = outputs(r)
    assert np.array_equal(bits(host_f), bits(f_read)) and np.array_equal(bits(host_d), bits(d_read))
    assert np.array_equal(out.cpu().numpy(), quantise(f_read))
    # a sharded call with a non-zero mask: refused before anything is enqueued
    view = np.ascontiguousarray(sc2.getCamera().getViewMatrix(), np.float32)
    proj = np.ascontiguousarray(sc2.getCamera().getProjectionMatrix(), np.float32)
    pos = np.zeros(3, np.float32)
    for call in (lambda: L.gs_render_sharded(ctx, view.ctypes.data, proj.ctypes.data, pos.ctypes.data, 0, None),
                 lambda: L.gs_render_sharded_async(ctx, view.ctypes.data, proj.ctypes.data, pos.ctypes.data, 0)):
        assert call() == _lib.GS_ERR_INVALID and b"gs_set_outputs" in L.gs_last_error(ctx)
    f_after, d_after = outputs(r)
    assert np.array_equal(bits(f_after), bits(f_read)) and np.array_equal(bits(d_after), bits(d_read))
    # mask 0: RGBA8 frames alone again, the same bytes
    r.setOutputs()
    assert L.gs_read_output(ctx, gs.GS_OUTPUT_RGBA32F, host_f.ctypes.data, host_f.nbytes) == _lib.GS_ERR_INVALID
    assert np.array_equal(r.draw(sc2), img2)
    r.cleanup()
    # two contexts sharing one scene: each keeps its own outputs
    a = make_renderer(sc, w, h)
    b = gs.Renderer(w, h, warmup_frames=0)
    b.init(sc.getResourceManager())
    b.initForScene(share_with=a)
    a.setOutputs(rgba32f=True, depth=True)
    b.setOutputs(depth=True)
    sc_b = make_scene(aos, w, h, pos=(0.3, -0.2, 0.5), yaw=4.0)
    img_a, img_b = a.draw(sc).copy(), b.draw(sc_b).copy()
    fa, da = outputs(a)
    db = b.readOutput(gs.GS_OUTPUT_DEPTH)
    assert np.array_equal(img_a, plain) and np.array_equal(quantise(fa), img_a)
    assert not np.array_equal(db, da) and db.any()
    a.draw(sc)
    assert np.array_equal(b.readOutput(gs.GS_OUTPUT_DEPTH), db)
    b.setOutputs()
    assert np.array_equal(bits(a.readOutput(gs.GS_OUTPUT_DEPTH)), bits(da))
    b.cleanup()
    a.cleanup()
