"""Gradients of an EXACT frame on the MI355X (include/gsplat.h, gs_backward*): a known answer, the float64 reference of
tests/test_backward_cpu.py, central differences of the GPU's own forward, bitwise determinism across sorters and launch
shapes, no interference with the frames, the C-ABI's refusals, the torch autograd binding and a full-size run.  The
values at full size (configs C, D, C-hard, a 2^32 list, a 65 k-tile grid) are checked on sampled tiles in
tests/test_backward_fullsize_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import (POSES, SCENES, assert_posed, camera, camera_params, in_front_of, known_answer_scene,
                              load_scene, oracle_params)
from test_backward_cpu import (batch_edge_scene, check_batch_edges, check_truncated, extreme_cloud, frozen_of,
                               truncated_scene)
from frame64 import frame_decisions, reference_gradient, sh_basis, weights

pytestmark = pytest.mark.gpu

KERNELS = (gs.GS_RENDER_KERNEL_AUTO, gs.GS_RENDER_KERNEL_WAVE_1PX, gs.GS_RENDER_KERNEL_WAVE_2PX,
           gs.GS_RENDER_KERNEL_WAVE_4PX, gs.GS_RENDER_KERNEL_WORKGROUP, gs.GS_RENDER_KERNEL_WORKGROUP_8X8)
# the 59 fields a frame reads: position.xyz, scale.xyz, rot, shCoeffs[k].rgb, shCoeffs[0].a
READ_FIELDS = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 15] + [12 + 4 * k + c for k in range(16) for c in range(3)]
UNREAD = np.setdiff1d(np.arange(84), READ_FIELDS)


def frame_and_grad(aos, w, h, sh_mode=0, seed=0, cam=None, **kw):
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **(cam or {}))
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


@pytest.mark.parametrize("pose", ["pose", "garden"])
def test_known_answer_posed(oracle_mod, pose):
    """One splat of opacity 0.5 on the forward axis of a rotated, translated camera, 2 in front of it: it lands on pixel
    (w / 2, h / 2) up to float32 rounding (about 2e-6 px).  For L = depth of that pixel dL/dposition = 0.5 (-V[2][0:3]) (the
    view depth row) and dL/dopacity = its depth; for L = red dL/dshCoeffs[k].r = 0.5 Y_k(dir) for all 16 k, dir the
    camera's forward axis, where no term of the basis is zero."""
    torch = pytest.importorskip("torch")
    w, h, depth = 64, 48, 2.0
    pos, yaw, pitch = POSES[pose]
    V = camera(pose, w, h).getViewMatrix().reshape(4, 4).T.astype(np.float64)      # V[r][c]
    forward = -V[2, :3]                                                               # view depth = -(V[2] . p + V[2][3])
    centre = np.asarray(pos, np.float64) + depth * forward
    aos = gs.makeGaussian(tuple(centre), (0.15 * depth,) * 3, sh0=(0.4, 0.1, 0.3, 0.5))[None].astype(np.float32)
    aos[0, 16:76] = np.linspace(-0.3, 0.3, 60, dtype=np.float32)                     # shCoeffs[1..15]
    sc = make_scene(aos, w, h, pos=pos, yaw=yaw, pitch=pitch)
    assert_posed(camera_params(oracle_mod, sc, w, h))
    r = make_renderer(sc, w, h)
    r.draw(sc)
    col = r.debugRead(gs.BUF_COLOR)[0]
    assert col[0] > 0.05                                                              # not on max(colour, 0)
    zero_rgba, zero_d = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
    cy, cx = h // 2, w // 2

    gd = zero_d.copy(); gd[cy, cx] = 1.0
    g = r.backward(zero_rgba, gd)[0]
    np.testing.assert_allclose(g[0:3], 0.5 * forward, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(g[15], depth, rtol=1e-5)
    assert np.all(g[12:15] == 0) and np.all(g[16:76] == 0) and np.all(g[UNREAD] == 0)

    gr = zero_rgba.copy(); gr[cy, cx, 0] = 1.0
    g = r.backward(gr)[0]
    basis = sh_basis(torch.tensor(forward[None] / np.linalg.norm(forward)))[0].numpy()
    assert np.all(np.abs(basis) > 1e-3), basis
    np.testing.assert_allclose(g[12:76:4], 0.5 * basis, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g[15], col[0], rtol=1e-5)
    assert np.all(g[13:76:4] == 0) and np.all(g[14:76:4] == 0) and np.all(g[19:76:4] == 0) and np.all(g[UNREAD] == 0)
    r.cleanup()


CASES = [("ragged", 0), ("ragged", 1), ("ragged", 2), ("dense", 0), ("zero_det", 0), ("extreme", 0), ("extreme", 1),
         ("extreme", 2), ("ragged@pose", 0), ("ragged@pose", 1), ("ragged@pose", 2), ("ragged@garden", 0),
         ("ragged@garden", 1), ("ragged@garden", 2)]


def compare_with_reference(got, want, keep):
    """Per read field (column): |got - want| <= 2e-2 |want| + 2e-3 max|want column| on the splats `keep`; a column that is
    zero in the reference is zero on the GPU.  Returns the offending (field, splat, got, want, scale)."""
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
    return bad


@pytest.mark.parametrize("scene,sh_mode", CASES)
def test_against_the_float64_reference(oracle_mod, tmp_path, scene, sh_mode):
    """The GPU's dL/d(record) against autograd of the float64 restatement with the same decisions.  Tolerance, per field
    (column) of the record: |gpu - ref| <= 2e-2 |ref| + 2e-3 max|ref column|.  The GPU accumulates in float32 -- sums over
    up to a few hundred list entries per pixel and over a splat's pixels, the reciprocal of a 2 x 2 determinant that can
    lose digits to cancellation -- so single entries of order 1e-5 relative error are expected and sums with cancelling
    terms lose more relative to their own size; the bound holds that to a few per mille of the column's scale.  The
    zero_det needles (a float32 determinant dominated by rounding) enter the reference as float32 constants and are not
    compared; unread fields and culled splats are exactly zero.  Posed scenes ('scene@pose'): the same cloud in front of a
    rotated, translated camera, the reference on the renderer's own camera."""
    if scene == "extreme":
        (aos, w, h), cam = extreme_cloud(), {}
    else:
        aos, w, h, cam = load_scene(scene)
    r, sc, got = frame_and_grad(aos, w, h, sh_mode, seed=1, cam=cam)
    r.cleanup()
    p = camera_params(oracle_mod, sc, w, h)
    if cam:
        assert_posed(p)
    ref, flags = frame_decisions(tmp_path, p, aos)
    wr, wd = weights(h, w, 1)
    fz = frozen_of(scene, aos)
    want = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64), fz if fz.any() else None)
    assert np.all(np.isfinite(got))
    assert np.all(got[:, UNREAD] == 0)
    emitting = np.zeros(len(aos), bool)
    emitting[np.asarray(ref["id"])[:ref["e"]]] = True
    assert np.all(got[~emitting] == 0)
    bad = compare_with_reference(got, want, ~fz)
    assert not bad, bad[:10]


def _central_differences(aos, w, h, cam):
    torch = pytest.importorskip("torch")
    sc = make_scene(aos, w, h, **cam)
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


def test_central_differences_of_the_gpu_forward():
    """~200 sampled (gaussian, field) pairs of the ragged scene: the gradient against central differences of L = sum w *
    RGBA32F + sum v * depth of the GPU's own EXACT forward (records re-uploaded from the device for every evaluation).
    Steps h and 2h (h = 1e-3 of the field's scale); a pair whose two differences disagree by more than 10 % lies at a
    discontinuity of the frame (a decision flips inside the step) and is dropped.  Of the kept pairs 95 % must agree to
    5 % + 0.02 (the float32 frame's own rounding: about 1e-7 per pixel over 63 k weighted pixels, over 2h)."""
    aos, w, h = SCENES["ragged"]()
    _central_differences(aos, w, h, {})


def test_central_differences_of_the_gpu_forward_posed(oracle_mod):
    """The same with the ragged cloud in front of a rotated, translated camera (the view block is not symmetric, the
    depth row has a translation, the SH direction starts at the camera), with the same kept / agree bars."""
    aos, w, h, cam = load_scene("ragged@pose")
    assert_posed(oracle_params(oracle_mod, w, h, **cam))
    _central_differences(aos, w, h, cam)


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
    wr, wd = weights(h, w, 0)
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


# ---- list edges ----------------------------------------------------------------------------------------------------------

def test_truncated_list(oracle_mod, tmp_path):
    """A frame whose list overflowed (GS_WARN_OVERFLOW) is differentiated as drawn, truncated: against the float64
    reference on the oracle's truncated list; the splat cut by the capacity has a gradient, the splats wholly past it
    exact zeros; every sorter gives the same bits."""
    aos, w, h = truncated_scene()
    sc = make_scene(aos, w, h)
    p = camera_params(oracle_mod, sc, w, h)
    ref, flags = frame_decisions(tmp_path, p, aos)
    across, past = check_truncated(ref, flags)
    wr, wd = weights(h, w, 6)
    want = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    first = None
    for sort in ALL_SORTS:
        r = make_renderer(sc, w, h, sort=sort)
        r.draw(sc)
        assert r.lastStatus == _lib.GS_WARN_OVERFLOW, sort
        got = r.backward(wr, wd)
        r.cleanup()
        if first is None:
            first = got
            continue
        assert np.array_equal(first.view(np.uint32), got.view(np.uint32)), sort
    got = first
    assert np.all(np.isfinite(got)) and np.all(got[:, UNREAD] == 0)
    assert np.any(got[across] != 0) and np.any(want[across] != 0)
    assert np.all(got[past] == 0)
    bad = compare_with_reference(got, want, np.ones(len(aos), bool))
    assert not bad, bad[:10]


def test_batch_edges(oracle_mod, tmp_path):
    """k_bwd_blend stages 64 entries at a time: lists of 64, 65, 128 and 129 entries, pixels that stop on in-tile
    indices 63, 64, 65, 127 and 128, a tile that blends its whole list, one whose last entries no pixel reaches, one
    that blends nothing (check_batch_edges) -- against the float64 reference; what no pixel blends gets exact zeros."""
    aos, w, h, _ = batch_edge_scene(oracle_mod)
    r, sc, got = frame_and_grad(aos, w, h, seed=7)
    r.cleanup()
    p = camera_params(oracle_mod, sc, w, h)
    ref, flags = frame_decisions(tmp_path, p, aos)
    unblended = check_batch_edges(ref, flags)
    wr, wd = weights(h, w, 7)
    want = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    assert np.all(np.isfinite(got)) and np.all(got[:, UNREAD] == 0)
    assert np.all(got[unblended] == 0) and np.all(want[unblended] == 0)
    bad = compare_with_reference(got, want, np.ones(len(aos), bool))
    assert not bad, bad[:10]


# ---- state kept between calls --------------------------------------------------------------------------------------------

def fresh_gradient(aos, w, h, wr, wd, cam=None):
    """The gradient of a context made for this one frame."""
    r, _, _ = frame_and_grad(aos, w, h, cam=cam)
    g = r.backward(wr, wd)
    r.cleanup()
    return g


def test_scratch_reuse():
    """A context's backward scratch (the rows it keeps between calls, buffers sized by pixels and by n) carries nothing
    from one call to the next: after an in-place device upload of another cloud of the same n, a larger and then a
    smaller resolution (gs_set_resolution), and a scene of another n, each gradient is that of a fresh context, bit for
    bit."""
    torch = pytest.importorskip("torch")
    L = _lib.lib()
    x, w, h = SCENES["ragged"]()
    y = synth.generate(len(x), w, h, -2.6, seed=78)
    r, sc, _ = frame_and_grad(x, w, h)
    wr, wd = weights(h, w, 11)
    r.backward(wr, wd)
    dev = torch.tensor(y, device="cuda")
    torch.cuda.synchronize()
    r.uploadDevice(dev.data_ptr(), len(y))
    r.draw(sc)
    assert np.array_equal(r.backward(wr, wd).view(np.uint32), fresh_gradient(y, w, h, wr, wd).view(np.uint32))
    for w2, h2 in ((480, 272), (160, 90)):
        r.width, r.height = w2, h2
        assert L.gs_set_resolution(r._ctx.handle, w2, h2) == _lib.GS_OK
        r.draw(make_scene(y, w2, h2))
        wr2, wd2 = weights(h2, w2, w2)
        assert np.array_equal(r.backward(wr2, wd2).view(np.uint32), fresh_gradient(y, w2, h2, wr2, wd2).view(np.uint32)), w2
    z = synth.generate(2500, w2, h2, -2.8, seed=79)
    dz = torch.tensor(z, device="cuda")
    torch.cuda.synchronize()
    r.uploadDevice(dz.data_ptr(), len(z))
    r.draw(make_scene(z, w2, h2))
    got = r.backward(wr2, wd2)
    r.cleanup()
    assert got.shape == (len(z), 84)
    assert np.array_equal(got.view(np.uint32), fresh_gradient(z, w2, h2, wr2, wd2).view(np.uint32))


def test_shared_scene_backwards(oracle_mod):
    """Three contexts over one uploaded scene (gs_share_scene), each drawn at its own camera -- the origin and two poses --
    then differentiated in another order: each gradient is that of a stand-alone context at its camera, bit for bit."""
    aos, w, h = SCENES["ragged"]()
    cams = [{}] + [dict(pos=POSES[k][0], yaw=POSES[k][1], pitch=POSES[k][2]) for k in ("pose", "garden")]
    for cam in cams[1:]:
        assert_posed(oracle_params(oracle_mod, w, h, **cam))
    scenes = [make_scene(aos, w, h, **cam) for cam in cams]
    owner = make_renderer(scenes[0], w, h)
    rs = [owner]
    for _ in cams[1:]:
        r = gs.Renderer(w, h, warmup_frames=0)
        r.init(scenes[0].getResourceManager())
        r.initForScene(share_with=owner)
        rs.append(r)
    for r, sc in zip(rs, scenes):
        r.draw(sc)
    wr, wd = weights(h, w, 12)
    got = {k: rs[k].backward(wr, wd) for k in (2, 0, 1)}
    for r in rs[::-1]:
        r.cleanup()
    for k, cam in enumerate(cams):
        want = fresh_gradient(aos, w, h, wr, wd, cam=cam)
        assert np.array_equal(got[k].view(np.uint32), want.view(np.uint32)), k
    assert not np.array_equal(got[1], got[2])


@pytest.mark.parametrize("depth_in", ["neither", "first"])
def test_torch_autograd_two_views(oracle_mod, depth_in):
    """One renderer, two posed views of one cloud in one graph, L = L_A + L_B: the records' gradient is Renderer.backward
    of view A plus that of view B, bit for bit -- view A's backward runs after view B was drawn, so _Frame.backward draws
    it again.  depth_in == 'first': view A also returns depth (the output mask changes between the frames)."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    w, h = 160, 96
    half = synth.generate(3000, w, h, -2.8, seed=81)
    cloud = np.concatenate([in_front_of(half[:1500], w, h, "pose"), in_front_of(half[1500:], w, h, "garden")])
    cams = [dict(pos=POSES[k][0], yaw=POSES[k][1], pitch=POSES[k][2]) for k in ("pose", "garden")]
    scenes = [make_scene(cloud, w, h, **cam) for cam in cams]
    for sc in scenes:
        assert_posed(camera_params(oracle_mod, sc, w, h))
    mats = [(sc.getCamera().getViewMatrix(), sc.getCamera().getProjectionMatrix(), sc.getCamera().getPosition())
            for sc in scenes]
    with_depth = (depth_in == "first", False)
    wts = [weights(h, w, 20 + k) for k in range(2)]
    rr = autograd.make_renderer(w, h)
    rec = torch.tensor(cloud, device="cuda", requires_grad=True)
    loss = 0
    for k in range(2):
        out = autograd.render(rec, *mats[k], 0, depth=with_depth[k], renderer=rr)
        if with_depth[k]:
            rgba, dep = out
            loss = loss + (rgba * torch.tensor(wts[k][0], device="cuda")).sum() + \
                (dep * torch.tensor(wts[k][1], device="cuda")).sum()
        else:
            loss = loss + (out * torch.tensor(wts[k][0], device="cuda")).sum()
    loss.backward()
    got = rec.grad.cpu().numpy()
    rr.cleanup()
    parts = []
    for k, sc in enumerate(scenes):
        r = make_renderer(sc, w, h)
        r.draw(sc)
        parts.append(r.backward(wts[k][0], wts[k][1] if with_depth[k] else None))
        r.cleanup()
    assert np.any(parts[0] != 0) and np.any(parts[1] != 0)
    assert np.array_equal(got.view(np.uint32), (parts[0] + parts[1]).view(np.uint32))
