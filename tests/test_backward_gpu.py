"""Gradients of an EXACT frame on the MI355X (include/gsplat.h, gs_backward*): a known answer, the float64 reference of
tests/test_backward_cpu.py, central differences of the GPU's own forward, bitwise determinism across sorters and launch
shapes, no interference with the frames, the C-ABI's refusals, the torch autograd binding and a full-size run."""
import ctypes as C

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, known_answer_scene, oracle_params
from test_backward_cpu import frame_decisions, frozen_of, reference_gradient

pytestmark = pytest.mark.gpu

KERNELS = (gs.GS_RENDER_KERNEL_AUTO, gs.GS_RENDER_KERNEL_WAVE_1PX, gs.GS_RENDER_KERNEL_WAVE_2PX,
           gs.GS_RENDER_KERNEL_WAVE_4PX, gs.GS_RENDER_KERNEL_WORKGROUP, gs.GS_RENDER_KERNEL_WORKGROUP_8X8)
# the 59 fields a frame reads: position.xyz, scale.xyz, rot, shCoeffs[k].rgb, shCoeffs[0].a
READ_FIELDS = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 15] + [12 + 4 * k + c for k in range(16) for c in range(3)]
UNREAD = np.setdiff1d(np.arange(84), READ_FIELDS)


def weights(h, w, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((h, w, 4)).astype(np.float32), (0.1 * rng.standard_normal((h, w))).astype(np.float32)


def frame_and_grad(aos, w, h, sh_mode=0, seed=0, **kw):
    sc = make_scene(aos, w, h, sh_mode=sh_mode)
    r = make_renderer(sc, w, h, **kw)
    r.draw(sc)
    wr, wd = weights(h, w, seed)
    g = r.backward(wr, wd)
    return r, sc, g


def test_known_answer():
    """One splat of opacity 0.5 centred on pixel (w / 2, h / 2) at view depth 2 (f = 0 there, alpha = 0.5): for L = red of
    that pixel dL/dshCoeffs[k].r = 0.5 * basis_k(0, 0, 1) (SH_C0 and the three zonal terms k = 2, 6, 12), dL/dopacity = red
    colour; for L = its alpha dL/dopacity = 1; for L = its depth dL/dposition = (0, 0, 0.5), dL/dopacity = 2.  Everything
    else is zero."""
    aos, w, h = known_answer_scene((2.0,))
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    r.draw(sc)
    col = r.debugRead(gs.BUF_COLOR)[0]
    zero_rgba, zero_d = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
    cy, cx = h // 2, w // 2

    gr = zero_rgba.copy(); gr[cy, cx, 0] = 1.0
    g = r.backward(gr)[0]
    basis = np.zeros(16)
    basis[[0, 2, 6, 12]] = [0.2820947917738781, 0.4886025119029199, 0.9461746957575601 - 0.31539156525252,
                            1.865881662950577 - 1.119528997770346]
    np.testing.assert_allclose(g[12:76:4], 0.5 * basis, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(g[15], col[0], rtol=1e-6)
    assert np.all(g[13:76:4] == 0) and np.all(g[14:76:4] == 0) and np.all(g[19:76:4] == 0) and np.all(g[UNREAD] == 0)
    np.testing.assert_allclose(g[0:12], 0.0, atol=1e-6)

    ga = zero_rgba.copy(); ga[cy, cx, 3] = 1.0
    g = r.backward(ga)[0]
    np.testing.assert_allclose(g[15], 1.0, rtol=1e-6)
    assert np.all(g[12:15] == 0)

    gd = zero_d.copy(); gd[cy, cx] = 1.0
    g = r.backward(zero_rgba, gd)[0]
    np.testing.assert_allclose(g[0:3], [0.0, 0.0, 0.5], atol=1e-6)
    np.testing.assert_allclose(g[15], 2.0, rtol=1e-6)
    r.cleanup()


def extreme_cloud():
    """96 x 64, 400 splats with opacity exactly 0 and 1, zero quaternions and zero scales among them."""
    aos = synth.generate(400, 96, 64, -2.0, seed=23)
    aos[0:40, 15] = 0.0
    aos[40:80, 15] = 1.0
    aos[80:100, 8:12] = 0.0
    aos[100:120, 4:7] = 0.0
    aos[120:130, 4] = 0.0
    return aos, 96, 64


CASES = [("ragged", 0), ("ragged", 1), ("ragged", 2), ("dense", 0), ("zero_det", 0), ("extreme", 0), ("extreme", 1),
         ("extreme", 2)]


@pytest.mark.parametrize("scene,sh_mode", CASES)
def test_against_the_float64_reference(oracle_mod, tmp_path, scene, sh_mode):
    """The GPU's dL/d(record) against autograd of the float64 restatement with the same decisions.  Tolerance, per field
    (column) of the record: |gpu - ref| <= 2e-2 |ref| + 2e-3 max|ref column|.  The GPU accumulates in float32 -- sums over
    up to a few hundred list entries per pixel and over a splat's pixels, the reciprocal of a 2 x 2 determinant that can
    lose digits to cancellation -- so single entries of order 1e-5 relative error are expected and sums with cancelling
    terms lose more relative to their own size; the bound holds that to a few per mille of the column's scale.  The
    zero_det needles (a float32 determinant dominated by rounding) enter the reference as float32 constants and are not
    compared; unread fields and culled splats are exactly zero."""
    aos, w, h = extreme_cloud() if scene == "extreme" else SCENES[scene]()
    p = oracle_params(oracle_mod, w, h, sh_mode)
    ref, flags = frame_decisions(tmp_path, p, aos)
    wr, wd = weights(h, w, 1)
    fz = frozen_of(scene, aos)
    want = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64), fz if fz.any() else None)
    r, sc, got = frame_and_grad(aos, w, h, sh_mode, seed=1)
    r.cleanup()
    assert np.all(np.isfinite(got))
    assert np.all(got[:, UNREAD] == 0)
    emitting = np.zeros(len(aos), bool)
    emitting[np.asarray(ref["id"])[:ref["e"]]] = True
    assert np.all(got[~emitting] == 0)
    keep = ~fz
    bad = []
    for f in READ_FIELDS:
        a, b = got[keep, f].astype(np.float64), want[keep, f]
        scale = np.abs(b).max()
        if scale == 0:
            assert np.all(a == 0), f
            continue
        tol = 2e-2 * np.abs(b) + 2e-3 * scale
        if not np.all(np.abs(a - b) <= tol):
            i = int(np.argmax(np.abs(a - b) - tol))
            bad.append((f, i, float(a[i]), float(b[i]), float(scale)))
    assert not bad, bad[:10]


def test_central_differences_of_the_gpu_forward():
    """~200 sampled (gaussian, field) pairs of the ragged scene: the gradient against central differences of L = sum w *
    RGBA32F + sum v * depth of the GPU's own EXACT forward (records re-uploaded from the device for every evaluation).
    Steps h and 2h (h = 1e-3 of the field's scale); a pair whose two differences disagree by more than 10 % lies at a
    discontinuity of the frame (a decision flips inside the step) and is dropped.  Of the kept pairs 95 % must agree to
    5 % + 0.02 (the float32 frame's own rounding: about 1e-7 per pixel over 63 k weighted pixels, over 2h)."""
    torch = pytest.importorskip("torch")
    aos, w, h = SCENES["ragged"]()
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    r.setOutputs(rgba32f=True, depth=True)
    r.draw(sc)
    wr, wd = weights(h, w, 2)
    grad = r.backward(wr, wd)
    ids = np.unique(r.debugRead(gs.BUF_SORTED_ID))
    dev = torch.tensor(aos, device="cuda")

    def loss(rec):
        dev.copy_(torch.from_numpy(rec))
        torch.cuda.synchronize()
        r.uploadDevice(dev.data_ptr(), len(rec))
        r.draw(sc)
        return float((r.readOutput(gs.GS_OUTPUT_RGBA32F).astype(np.float64) * wr).sum() +
                     (r.readOutput(gs.GS_OUTPUT_DEPTH).astype(np.float64) * wd).sum())

    rng = np.random.default_rng(5)
    kept = agree = 0
    for _ in range(200):
        g, f = int(rng.choice(ids)), int(rng.choice(READ_FIELDS))
        hstep = 1e-3 * max(abs(float(aos[g, f])), 0.05)
        fds = []
        for s in (hstep, 2 * hstep):
            rp, rm = aos.copy(), aos.copy()
            rp[g, f] += np.float32(s)
            rm[g, f] -= np.float32(s)
            fds.append((loss(rp) - loss(rm)) / (float(rp[g, f]) - float(rm[g, f])))
        if abs(fds[0] - fds[1]) > 0.1 * max(abs(fds[0]), abs(fds[1])) + 0.02:
            continue
        kept += 1
        agree += abs(grad[g, f] - fds[0]) <= 0.05 * abs(fds[0]) + 0.02
    r.cleanup()
    assert kept >= 100, kept
    assert agree >= 0.95 * kept, (agree, kept)


def test_bitwise_determinism():
    """Two runs give identical gradients, and so do the five sorters, every launch shape of the forward, both tile orders
    and every GS_COUNT_* mode (the gradient depends on the sorted list and the pixels only)."""
    aos, w, h = SCENES["ragged"]()
    r, sc, base = frame_and_grad(aos, w, h)
    r.draw(sc)
    again = r.backward(*weights(h, w, 0))
    r.cleanup()
    assert np.array_equal(base.view(np.uint32), again.view(np.uint32))
    variants = [dict(sort=s) for s in ALL_SORTS] + [dict(kernel=k) for k in KERNELS] + \
               [dict(order=gs.GS_TILE_ORDER_RASTER)] + [dict(count=c) for c in (gs.GS_COUNT_PER_PASS, gs.GS_COUNT_FED)]
    for kw in variants:
        r, _, g = frame_and_grad(aos, w, h, **kw)
        r.cleanup()
        assert np.array_equal(base.view(np.uint32), g.view(np.uint32)), kw


def test_no_interference_and_device_entry_points():
    """RGBA8 frames and the optional outputs are byte-identical before and after a backward; gs_backward_device gives the
    bits of gs_backward; gs_upload_gaussians_device (same n: in place; another n: a new scene) gives the frames of the host
    upload."""
    torch = pytest.importorskip("torch")
    aos, w, h = SCENES["dense"]()
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    r.setOutputs(rgba32f=True, depth=True)
    img0 = r.draw(sc)
    f0, d0 = r.readOutput(gs.GS_OUTPUT_RGBA32F), r.readOutput(gs.GS_OUTPUT_DEPTH)
    wr, wd = weights(h, w, 3)
    host = r.backward(wr, wd)
    assert np.array_equal(r.draw(sc), img0)
    assert np.array_equal(r.readOutput(gs.GS_OUTPUT_RGBA32F), f0) and np.array_equal(r.readOutput(gs.GS_OUTPUT_DEPTH), d0)
    gr, gd = torch.tensor(wr, device="cuda"), torch.tensor(wd, device="cuda")
    out = torch.full((len(aos), 84), float("nan"), device="cuda")
    torch.cuda.synchronize()
    r.backwardDevice(gr.data_ptr(), gd.data_ptr(), out.data_ptr())
    r.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), host.view(np.uint32))
    # device upload, same n (in place), then a scene of another size and back
    moved = aos.copy()
    moved[:, 0] += np.float32(0.01)
    sc2 = make_scene(moved, w, h)
    ref = make_renderer(sc2, w, h)
    want = ref.draw(sc2)
    ref.cleanup()
    t = torch.tensor(moved, device="cuda")
    torch.cuda.synchronize()
    r.uploadDevice(t.data_ptr(), len(moved))
    assert np.array_equal(r.draw(sc), want)
    half = torch.tensor(aos[:3000], device="cuda")
    torch.cuda.synchronize()
    r.uploadDevice(half.data_ptr(), 3000)
    assert r.sceneInfo().num_gaussians == 3000
    r.uploadDevice(t.data_ptr(), len(moved))
    assert np.array_equal(r.draw(sc), want)
    r.cleanup()


def test_api_refusals():
    """GS_ERR_INVALID with a message, nothing enqueued: no frame since gs_set_resolution / gs_set_tile_rows / an upload /
    gs_debug_init_sort_list, a GS_RENDER_FAST context, a context that owns a subset of the tile rows, NULL buffers; short
    or mis-shaped buffers are refused by the binding."""
    aos, w, h = SCENES["ragged"]()
    sc = make_scene(aos, w, h)
    L = _lib.lib()
    wr, wd = weights(h, w)
    out = np.zeros((len(aos), 84), np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def refused(r, what):
        rc = L.gs_backward(r._ctx.handle, p(wr), p(wd), p(out))
        assert rc == _lib.GS_ERR_INVALID, what
        assert L.gs_last_error(r._ctx.handle), what

    r = make_renderer(sc, w, h)
    refused(r, "no frame after gs_set_resolution")
    r.draw(sc)
    assert L.gs_backward(r._ctx.handle, None, None, p(out)) == _lib.GS_ERR_INVALID
    assert L.gs_backward(r._ctx.handle, p(wr), None, None) == _lib.GS_ERR_INVALID
    assert L.gs_backward_device(r._ctx.handle, None, None, None) == _lib.GS_ERR_INVALID
    with pytest.raises(ValueError):
        r.backward(wr[:-1], wd)
    with pytest.raises(ValueError):
        r.backward(wr, wd[:, :-1])
    r.setTileRows(0, 2)
    refused(r, "gs_set_tile_rows")
    r.draw(sc)
    refused(r, "a subset of the tile rows")
    r.setTileRows(0, r.sceneInfo().tiles_y)
    refused(r, "rows set back, no frame since")
    r.draw(sc)
    assert L.gs_backward(r._ctx.handle, p(wr), p(wd), p(out)) == _lib.GS_OK
    r.debugInitSortList(sc)
    refused(r, "gs_debug_init_sort_list")
    r.draw(sc)
    g = np.ascontiguousarray(aos)
    assert L.gs_upload_gaussians(r._ctx.handle, p(g), len(g)) == _lib.GS_OK
    assert L.gs_set_resolution(r._ctx.handle, w, h) == _lib.GS_OK
    refused(r, "upload")
    r.cleanup()
    f = make_renderer(sc, w, h, mode=gs.GS_RENDER_FAST)
    f.draw(sc)
    refused(f, "GS_RENDER_FAST")
    f.cleanup()


def test_torch_autograd():
    """autograd.render's gradient equals Renderer.backward; a short Adam loop recovers the colours and positions of a
    16-splat scene from its target frame (loss down by at least 10x)."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    w, h = 96, 64
    rng = np.random.default_rng(7)
    recs = []
    for k in range(16):
        x, y = (k % 4 - 1.5) * 0.35, (k // 4 - 1.5) * 0.3
        recs.append(gs.makeGaussian((x, y, 2.0), (0.12, 0.12, 0.12),
                                    sh0=tuple(rng.uniform(-1.2, 1.2, 3)) + (0.8,)))
    target_aos = np.stack(recs).astype(np.float32)
    sc = make_scene(target_aos, w, h)
    cam = sc.getCamera()
    view, proj, pos = cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition()
    rr = autograd.make_renderer(w, h)
    target = torch.tensor(target_aos, device="cuda")
    with torch.no_grad():
        tgt_rgba, tgt_depth = autograd.render(target, view, proj, pos, 0, depth=True, renderer=rr)

    # the binding's gradient is Renderer.backward's
    rec = target.clone().requires_grad_(True)
    rgba, dep = autograd.render(rec, view, proj, pos, 0, depth=True, renderer=rr)
    wr, wd = weights(h, w, 4)
    (rgba * torch.tensor(wr, device="cuda")).sum().add((dep * torch.tensor(wd, device="cuda")).sum()).backward()
    r = make_renderer(sc, w, h)
    r.draw(sc)
    want = r.backward(wr, wd)
    r.cleanup()
    assert np.array_equal(rec.grad.cpu().numpy().view(np.uint32), want.view(np.uint32))

    # optimise colours and positions from a perturbed start
    start = target_aos.copy()
    start[:, 12:15] = rng.uniform(-1.2, 1.2, (16, 3))
    start[:, 0:2] += rng.uniform(-0.04, 0.04, (16, 2)).astype(np.float32)
    colour = torch.tensor(start[:, 12:15], device="cuda", requires_grad=True)
    xy = torch.tensor(start[:, 0:2], device="cuda", requires_grad=True)
    rest = torch.tensor(start, device="cuda")
    opt = torch.optim.Adam([{"params": [colour], "lr": 0.05}, {"params": [xy], "lr": 0.002}])
    losses = []
    for _ in range(150):
        opt.zero_grad()
        recs_t = torch.cat([xy, rest[:, 2:12], colour, rest[:, 15:]], 1)
        out = autograd.render(recs_t, view, proj, pos, 0, renderer=rr)
        loss = ((out - tgt_rgba) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    rr.cleanup()
    assert losses[-1] < losses[0] / 10, (losses[0], losses[-1])
    assert np.abs(colour.detach().cpu().numpy() - target_aos[:, 12:15]).mean() < \
        np.abs(start[:, 12:15] - target_aos[:, 12:15]).mean() / 3


def test_config_c_full_size():
    """Config C (1920 x 1080): the backward runs, every value is finite, unread fields and culled / non-emitting splats get
    exact zeros.  No timing assertion (tools/backward_cost.py measures)."""
    aos, cfg = synth.generate_config("C")
    w, h = cfg["width"], cfg["height"]
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    r.draw(sc)
    g = r.backward(*weights(h, w, 9))
    ids = np.unique(r.debugRead(gs.BUF_SORTED_ID))
    r.cleanup()
    assert np.all(np.isfinite(g))
    assert np.all(g[:, UNREAD] == 0)
    silent = np.ones(len(aos), bool)
    silent[ids] = False
    assert silent.any() and np.all(g[silent] == 0)
    assert np.count_nonzero(np.abs(g[ids]).sum(1)) > 10000     # the fog hides most emitting splats behind the early-out
