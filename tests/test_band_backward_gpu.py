"""Gradients of a tile-row band on the MI355X (include/gsplat.h, gs_set_band_gradients): a context that owns a band of tile
rows computes the terms of its own pixels, so its gs_backward* equals the whole frame's with dL/d(outputs) zeroed outside the
band -- compared with np.array_equal against a whole-grid context of the same build, and bit for bit on the rows of V_band.
Also: the visible form and its count against the oracle's boxes, scratch left stale by k_band_cull, the camera's 35 floats,
contributions summed over a dealing, the R-rank step on one GPU (three contexts over one scene), determinism across sorters,
and what the flag admits and what stays refused."""
import ctypes as C
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, assert_posed, camera_params, load_scene
from test_backward_cpu import overflowing_scene, pick_tiles, sampled_reference_gradient, tile_weights
from test_backward_gpu import compare_with_reference
from frame64 import frame_decisions, reference_gradient, weights
from test_backward_fullsize_gpu import assert_sampled_gradient, oracle_list
from test_band_cull_cpu import C_BAND, H, W, cameras, cloud_c
from test_band_backward_cpu import DEALINGS, rows_of, v_band

pytestmark = pytest.mark.gpu

F = np.float32
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
BAND_WORDS = "the context owns a subset of the tile rows"


def set_band(r, spec):
    if spec[0] == "rows":
        r.setTileRows(spec[1], spec[2])
    else:
        r.setTileRowsInterleaved(spec[1], spec[2], bool(spec[3]))


def masked(wr, wd, rows, h):
    """The images with every value outside the pixel rows of the tile rows `rows` set to +0."""
    keep = np.zeros(h, bool)
    for row in rows:
        keep[row * 16:row * 16 + 16] = True
    return np.where(keep[:, None, None], wr, F(0)).astype(F), np.where(keep[:, None], wd, F(0)).astype(F)


def band_renderer(sc, w, h, **kw):
    r = make_renderer(sc, w, h, **kw)
    r.setBandGradients(True)
    return r


def draw_band(r, sc, spec):
    set_band(r, spec)
    r.draw(sc)
    assert r.timings().overflowed == 0, spec


def dealings_of(gh):
    return DEALINGS if gh == 12 else {"thirds": [("rows", 0, 2), ("rows", 2, 4), ("rows", 4, 6)],
                                      "stride2": [("il", 0, 2, 0), ("il", 1, 2, 0)], "empty": [("rows", 3, 3)]}


# ---- 1. a band equals the masked whole frame ----------------------------------------------------------------------------

CASES = [("ragged", 0), ("ragged", 2), ("ragged", _lib.GS_SH_DEGREE_1), ("dense", 0), ("dense", 2), ("ragged@pose", 0)]


@pytest.mark.parametrize("scene,sh_mode", CASES)
def test_band_equals_the_masked_whole_frame(oracle_mod, scene, sh_mode):
    """Every band of every dealing: gs_backward of the band context == gs_backward of a whole-grid context given the same
    images zeroed outside the band's pixel rows (np.array_equal: -0 == +0), and on the rows of V_band the same uint32 words
    -- a masked-out tile's row is +-0 and the per-splat sum starts from +0, so adding it changes no bit."""
    aos, w, h, cam = load_scene(scene)
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
    if cam:
        assert_posed(camera_params(oracle_mod, sc, w, h))
    gh = (h + 15) // 16
    whole, band = make_renderer(sc, w, h), band_renderer(sc, w, h)
    whole.draw(sc)
    assert whole.timings().overflowed == 0
    wr, wd = weights(h, w, 1)
    for name, dealing in dealings_of(gh).items():
        for spec in dealing:
            rows = rows_of(spec, gh)
            draw_band(band, sc, spec)
            got = band.backward(wr, wd)
            ids, vis_rows, count = band.backwardVisible(wr, wd)
            if not rows:
                assert count == 0 and ids.size == 0 and not got.any() and np.all(bits(got) == 0), (name, spec)
                continue
            want = whole.backward(*masked(wr, wd, rows, h))
            assert count > 0 and want.any(), (name, spec)
            assert np.all(np.isfinite(got)), (name, spec)
            assert np.array_equal(got, want), (name, spec, int(np.flatnonzero((got != want).any(1))[0]))
            assert np.array_equal(bits(got[ids]), bits(want[ids])), (name, spec)
            assert np.array_equal(bits(vis_rows), bits(got[ids])), (name, spec)
            assert not got[np.setdiff1d(np.arange(len(aos)), ids)].any(), (name, spec)
    whole.cleanup()
    band.cleanup()


# ---- 2. the visible form and the count ------------------------------------------------------------------------------------

def test_visible_form_and_count(oracle_mod):
    """ids = V_band of the oracle's whole-frame boxes clipped to the rows, ascending; every splat with a non-zero dense row
    is among them; rows = dense[ids] bit for bit; max_rows = |V_band| - 1 writes that many and nothing past them and returns
    GS_WARN_OVERFLOW; gs_visible_count agrees; the union over a dealing is V of the whole-grid context."""
    import oracle
    aos, w, h = SCENES["ragged"]()
    sc = make_scene(aos, w, h)
    gh = (h + 15) // 16
    s = oracle.full_pipeline(camera_params(oracle_mod, sc, w, h), aos)["stage1"]["splats"]
    whole, band = make_renderer(sc, w, h), band_renderer(sc, w, h)
    whole.draw(sc)
    wr, wd = weights(h, w, 2)
    v_whole = whole.backwardVisible(wr, wd)[0]
    assert np.array_equal(v_whole, np.flatnonzero(v_band(s, range(gh))))
    L, p = _lib.lib(), lambda a: a.ctypes.data_as(C.c_void_p)
    for name, dealing in DEALINGS.items():
        union = np.zeros(len(aos), bool)
        for spec in dealing:
            rows = rows_of(spec, gh)
            draw_band(band, sc, spec)
            dense = band.backward(wr, wd)
            ids, vis_rows, count = band.backwardVisible(wr, wd)
            want_ids = np.flatnonzero(v_band(s, rows))
            assert count == want_ids.size == band.visibleCount() and np.array_equal(ids, want_ids), (name, spec)
            assert np.isin(np.flatnonzero(dense.any(1)), ids).all(), (name, spec)
            assert np.array_equal(bits(vis_rows), bits(dense[ids])), (name, spec)
            union[ids] = True
            if count < 2:
                continue
            k = count - 1
            ids_k, rows_k = np.full(count + 2, 0xFFFFFFFF, np.uint32), np.full((count + 2, 84), F(-7.5))
            c = C.c_uint32()
            rc = L.gs_backward_visible(band._ctx.handle, p(wr), p(wd), p(ids_k), p(rows_k), k, C.byref(c))
            assert rc == _lib.GS_WARN_OVERFLOW and c.value == count, (name, spec, rc)
            assert np.array_equal(ids_k[:k], ids[:k]) and np.array_equal(bits(rows_k[:k]), bits(vis_rows[:k])), (name, spec)
            assert np.all(ids_k[k:] == 0xFFFFFFFF) and np.all(rows_k[k:] == F(-7.5)), (name, spec)
        if name != "empty":
            assert np.array_equal(np.flatnonzero(union), v_whole), name
    whole.cleanup()
    band.cleanup()


# ---- 3. stale scratch -----------------------------------------------------------------------------------------------------

def scene_of(aos, cam, w, h):
    rm = gs.ResourceManager()
    rm.setGaussians(aos)
    sc = gs.Scene(rm, aspect_ratio=w / h)
    sc.camera = cam
    return sc


def all_forms(r, wr, wd):
    """Dense, visible and camera results of the last frame of r."""
    dense = r.backward(wr, wd)
    cam_dense = r.backwardCamera()
    ids, rows, count = r.backwardVisible(wr, wd)
    return dict(dense=dense, cam_dense=cam_dense, ids=ids, rows=rows, count=np.uint32(count), cam_vis=r.backwardCamera())


@pytest.mark.parametrize("permuted", [False, True], ids=["designed", "permuted"])
def test_stale_scratch_of_culled_blocks(permuted):
    """cloud_c(63) under `rigid`, band (11, 12): k_band_cull rejects the blocks that hold out waves only and leaves their
    tiles_touched as an earlier frame wrote them.  After a whole-grid frame, and after a frame of band (0, 1), on the same
    context the three forms equal a fresh context's bit for bit and the masked whole frame's by value."""
    aos, _ = cloud_c(63, permuted)
    sc = scene_of(aos, cameras()["rigid"], W, H)
    wr, wd = weights(H, W, 3)
    spec = ("rows",) + C_BAND
    fresh = band_renderer(sc, W, H)
    draw_band(fresh, sc, spec)
    want = all_forms(fresh, wr, wd)
    fresh.cleanup()
    assert want["count"] > 0
    whole = make_renderer(sc, W, H)
    whole.draw(sc)
    assert whole.timings().overflowed == 0
    m_dense = whole.backward(*masked(wr, wd, rows_of(spec, 23), H))
    m_cam = whole.backwardCamera()
    whole.cleanup()
    assert m_dense.any()
    for first in (None, ("rows", 0, 1)):
        r = band_renderer(sc, W, H)
        if first:
            draw_band(r, sc, first)
        else:
            r.draw(sc)                                         # the whole grid
        draw_band(r, sc, spec)
        got = all_forms(r, wr, wd)
        r.cleanup()
        for k in want:
            assert np.array_equal(bits(got[k]), bits(want[k])), (first, k)
        assert np.array_equal(got["dense"], m_dense), first
        assert np.array_equal(got["cam_dense"], m_cam) and np.array_equal(got["cam_vis"], m_cam), first


# ---- 4. camera gradients --------------------------------------------------------------------------------------------------

CAM_ZEROS = [3, 7, 11, 15, 18, 22, 26, 30]


@pytest.mark.parametrize("scene", ["ragged", "ragged@pose"])
def test_camera_gradients_of_a_band(scene):
    """gs_backward_camera after the dense and after the visible band backward == the masked whole frame's 35 floats; the
    view's bottom row and the projection's clip-z row are exactly +0.0f."""
    aos, w, h, cam = load_scene(scene)
    sc = make_scene(aos, w, h, **cam)
    gh = (h + 15) // 16
    whole, band = make_renderer(sc, w, h), band_renderer(sc, w, h)
    whole.draw(sc)
    wr, wd = weights(h, w, 4)
    for name in ("thirds", "edges", "stride2", "stride2_compact"):
        for spec in DEALINGS[name]:
            draw_band(band, sc, spec)
            band.backward(wr, wd)
            after_dense = band.backwardCamera()
            band.backwardVisible(wr, wd)
            after_vis = band.backwardCamera()
            whole.backward(*masked(wr, wd, rows_of(spec, gh), h))
            want = whole.backwardCamera()
            assert want.any() and np.all(np.isfinite(want)), spec
            assert np.array_equal(after_dense, want) and np.array_equal(after_vis, want), spec
            assert np.array_equal(bits(after_dense), bits(after_vis)), spec
            assert np.all(bits(after_dense)[CAM_ZEROS] == 0), spec
    whole.cleanup()
    band.cleanup()


# ---- 5. contributions -----------------------------------------------------------------------------------------------------

SENT_MAX, SENT_SUM, SENT_PIX = F(-3.5), F(-7.25), np.uint32(0xDEADBEEF)


def contrib_into(torch, r, n, state):
    d = [torch.tensor(np.ascontiguousarray(a).view(np.int32), device="cuda") for a in state]
    torch.cuda.synchronize()
    r.contribDevice(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr())
    r.synchronize()
    return [t.cpu().numpy().view(a.dtype) for t, a in zip(d, state)]


@pytest.mark.parametrize("scene", ["ragged", "dense"])
def test_contributions_of_a_dealing(scene):
    """The R bands of a dealing into one set of zeroed arrays against the whole grid into another: wmax and pixels equal
    exactly (a maximum and an integer sum), wsum within 2 (T + R) 2^-24 wsum_whole (both are float32 sums of the same
    non-negative, bit-identical per-element terms, at most T + R additions each).  A splat with no pair in a band keeps the
    sentinels that band's call was given."""
    torch = pytest.importorskip("torch")
    aos, w, h = SCENES[scene]()
    n = len(aos)
    sc = make_scene(aos, w, h)
    gw, gh = (w + 15) // 16, (h + 15) // 16
    zeros = lambda: [np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32)]
    whole, band = make_renderer(sc, w, h), band_renderer(sc, w, h)
    whole.draw(sc)
    want = contrib_into(torch, whole, n, zeros())
    assert want[2].any()
    for name, dealing in dealings_of(gh).items():
        if name == "empty":
            continue
        state = zeros()
        for spec in dealing:
            draw_band(band, sc, spec)
            state = contrib_into(torch, band, n, state)
            alone = contrib_into(torch, band, n, zeros())
            kept = contrib_into(torch, band, n, [np.full(n, SENT_MAX), np.full(n, SENT_SUM), np.full(n, SENT_PIX)])
            idle = alone[2] == 0
            assert idle.any() and (~idle).any(), (name, spec)
            assert np.all(kept[0][idle] == SENT_MAX) and np.all(kept[1][idle] == SENT_SUM) and np.all(kept[2][idle] == SENT_PIX)
            assert not np.any(kept[2][~idle] == SENT_PIX), (name, spec)
        assert np.array_equal(bits(state[0]), bits(want[0])), name
        assert np.array_equal(state[2], want[2]), name
        bound = 2.0 * (gw * gh + len(dealing)) * 2.0 ** -24 * want[1].astype(np.float64)
        assert np.all(np.abs(state[1].astype(np.float64) - want[1]) <= bound), name
    draw_band(band, sc, ("rows", 1, 1))                        # the empty band touches nothing
    kept = contrib_into(torch, band, n, [np.full(n, SENT_MAX), np.full(n, SENT_SUM), np.full(n, SENT_PIX)])
    assert np.all(kept[0] == SENT_MAX) and np.all(kept[1] == SENT_SUM) and np.all(kept[2] == SENT_PIX)
    whole.cleanup()
    band.cleanup()


# ---- 6. the R-rank step on one GPU ----------------------------------------------------------------------------------------

def test_three_rank_step_on_one_gpu(oracle_mod, tmp_path):
    """Three contexts over one scene (gs_share_scene) with the bands (0, 4), (4, 8), (8, 12) of `ragged`: each calls
    gs_backward_visible_device with the same whole images, gs_rows_accumulate_device (weight 1) sums the lists and
    gs_rows_collect_device lists the union.  ids = the whole grid's V; rows against the whole grid's visible rows as float64
    under the project's gradient tolerance (the difference is float32 association across bands), and against the float64
    reference with the oracle's decisions."""
    torch = pytest.importorskip("torch")
    aos, w, h = SCENES["ragged"]()
    n = len(aos)
    sc = make_scene(aos, w, h)
    wr, wd = weights(h, w, 6)
    whole = make_renderer(sc, w, h)
    whole.draw(sc)
    want_ids, want_rows, _ = whole.backwardVisible(wr, wd)
    ranks = [whole]
    for _ in range(2):
        r = gs.Renderer(w, h, warmup_frames=0)
        r.init(sc.getResourceManager())
        r.initForScene(share_with=whole)
        ranks.append(r)
    dev = lambda a: torch.tensor(a, device="cuda")
    d_wr, d_wd = dev(wr), dev(wd)
    acc, mark = torch.zeros((n, 84), device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    ids, rows = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 84), device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for r, spec in zip(ranks, DEALINGS["thirds"]):
        r.setBandGradients(True)
        set_band(r, spec)
        r.drawDevice(sc)
        r.backwardVisibleDevice(d_wr.data_ptr(), d_wd.data_ptr(), ids.data_ptr(), rows.data_ptr(), n, count.data_ptr())
        r.rowsAccumulateDevice(acc.data_ptr(), mark.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), count.data_ptr(), n, 1.0)
        r.synchronize()
        assert 0 < int(count.item()) < len(want_ids)
    u_ids, u_rows = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 84), device="cuda")
    whole.rowsCollectDevice(acc.data_ptr(), mark.data_ptr(), n, u_ids.data_ptr(), u_rows.data_ptr(), n, count.data_ptr())
    whole.synchronize()
    k = int(count.item())
    got_ids, got_rows = u_ids.cpu().numpy().view(np.uint32)[:k], u_rows.cpu().numpy()[:k]
    for r in ranks[::-1]:
        r.cleanup()
    assert np.array_equal(got_ids, want_ids)
    bad = compare_with_reference(got_rows, want_rows.astype(np.float64), np.ones(k, bool))
    assert not bad, bad[:10]
    p = camera_params(oracle_mod, sc, w, h)
    ref, flags = frame_decisions(tmp_path, p, aos)
    want = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    dense = np.zeros((n, 84), F)
    dense[got_ids] = got_rows
    bad = compare_with_reference(dense, want, np.ones(n, bool))
    assert not bad, bad[:10]


# ---- 7. determinism and sorters -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [("rows", 4, 8), ("il", 0, 2, 0)], ids=["rows4-8", "stride2"])
def test_bitwise_determinism_of_a_band(spec):
    aos, w, h = SCENES["ragged"]()
    sc = make_scene(aos, w, h)
    wr, wd = weights(h, w, 7)
    base = None
    for sort in (ALL_SORTS[0],) + ALL_SORTS:
        r = band_renderer(sc, w, h, sort=sort)
        draw_band(r, sc, spec)
        got = all_forms(r, wr, wd)
        if base is None:
            base = got
            r.draw(sc)
            again = all_forms(r, wr, wd)
            assert all(np.array_equal(bits(again[k]), bits(base[k])) for k in base)
            assert base["dense"].any()
        r.cleanup()
        for k in base:
            assert np.array_equal(bits(got[k]), bits(base[k])), (sort, k)


# ---- 8. the flag ----------------------------------------------------------------------------------------------------------

def test_the_flag():
    """Off by default (a band is refused with today's words), on: accepted, off again: refused; enable = 2 is refused; a
    whole-grid context gives the same bits with the flag on as off; with the flag on a GS_RENDER_FAST context, a context
    without a frame since the last change, gs_densify_stats_device in a band and gs_photometric_loss* in a band keep their
    messages."""
    torch = pytest.importorskip("torch")
    aos, w, h = SCENES["ragged"]()
    n = len(aos)
    sc = make_scene(aos, w, h)
    L = _lib.lib()
    wr, wd = weights(h, w, 8)
    out = np.zeros((n, 84), F)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    r = make_renderer(sc, w, h)
    hdl = r._ctx.handle
    error = lambda: L.gs_last_error(hdl).decode()
    backward = lambda: L.gs_backward(hdl, p(wr), p(wd), p(out))
    count = C.c_uint32()

    # the whole grid, flag off and on
    def whole_forms():
        r.draw(sc)
        forms = all_forms(r, wr, wd)
        forms.update(zip(("wmax", "wsum", "pixels"), contrib_into(torch, r, n, [np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32)])))
        return forms
    off = whole_forms()
    assert L.gs_set_band_gradients(hdl, 2) == _lib.GS_ERR_INVALID and error().startswith("gs_set_band_gradients: ")
    assert L.gs_set_band_gradients(hdl, 1) == _lib.GS_OK
    on = whole_forms()
    assert all(np.array_equal(bits(on[k]), bits(off[k])) for k in off)
    assert L.gs_set_band_gradients(hdl, 0) == _lib.GS_OK

    # a band: refused, accepted, refused
    r.setTileRows(4, 8)
    r.draw(sc)
    assert backward() == _lib.GS_ERR_INVALID and error() == "gs_backward: " + BAND_WORDS
    assert L.gs_visible_count(hdl, C.byref(count)) == _lib.GS_ERR_INVALID and error() == "gs_visible_count: " + BAND_WORDS
    r.setBandGradients(True)
    assert backward() == _lib.GS_OK and out.any()
    assert L.gs_visible_count(hdl, C.byref(count)) == _lib.GS_OK and count.value > 0
    assert L.gs_set_resolution(hdl, w, h) == _lib.GS_OK       # the flag survives a resolution and new rows
    r.setTileRows(4, 8)
    assert backward() == _lib.GS_ERR_INVALID and "no frame since" in error()
    r.draw(sc)
    assert backward() == _lib.GS_OK

    # still refused in a band, flag on
    d = dict(ids=torch.zeros(n, dtype=torch.int32, device="cuda"), count=torch.zeros(1, dtype=torch.int32, device="cuda"),
             a=torch.zeros(n, device="cuda"), s=torch.zeros(n, dtype=torch.int32, device="cuda"), m=torch.zeros(n, device="cuda"),
             img=torch.zeros((h, w, 4), device="cuda"), target=torch.zeros((h, w, 3), device="cuda"), loss=torch.zeros(4, device="cuda"))
    torch.cuda.synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    rc = L.gs_densify_stats_device(hdl, vp(d["ids"]), vp(d["count"]), n, n, vp(d["a"]), vp(d["s"]), vp(d["m"]))
    assert rc == _lib.GS_ERR_INVALID and error() == "gs_densify_stats_device: " + BAND_WORDS
    rc = L.gs_photometric_loss_device(hdl, vp(d["img"]), vp(d["target"]), 0.2, None, vp(d["loss"]), None)
    assert rc == _lib.GS_ERR_INVALID and error() == "gs_photometric_loss_device: " + BAND_WORDS
    img, target, numbers = np.zeros((h, w, 4), F), np.zeros((h, w, 3), F), np.zeros(3, F)
    rc = L.gs_photometric_loss(hdl, p(img), p(target), 0.2, None, p(numbers), None)
    assert rc == _lib.GS_ERR_INVALID and error() == "gs_photometric_loss: " + BAND_WORDS

    r.setBandGradients(False)
    assert backward() == _lib.GS_ERR_INVALID and error() == "gs_backward: " + BAND_WORDS
    rc = L.gs_contrib_device(hdl, n, vp(d["a"]), None, None)
    assert rc == _lib.GS_ERR_INVALID and error() == "gs_contrib_device: " + BAND_WORDS
    assert L.gs_backward_camera(hdl, p(np.zeros(35, F))) == _lib.GS_ERR_INVALID and error() == "gs_backward_camera: " + BAND_WORDS
    r.cleanup()

    fast = make_renderer(sc, w, h, mode=gs.GS_RENDER_FAST)
    fast.setBandGradients(True)
    fast.setTileRows(4, 8)
    fast.draw(sc)
    assert L.gs_backward(fast._ctx.handle, p(wr), p(wd), p(out)) == _lib.GS_ERR_INVALID
    assert "only GS_RENDER_EXACT frames can be differentiated" in L.gs_last_error(fast._ctx.handle).decode()
    fast.cleanup()


def test_a_sharded_context_stays_refused_with_the_flag_on():
    """A context whose rows gs_dist_shard_rows has dealt (world size 1), gs_set_band_gradients on: gs_backward_device and
    gs_contrib_device keep their refusal; in a child process, which alone holds the communicator."""
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
        assert L.gs_set_band_gradients(ctx, 1) == 0
        out = np.full(84, -7.5, np.float32)
        ident = C.create_string_buffer(_lib.DIST_UNIQUE_ID_BYTES)
        assert L.gs_dist_unique_id(ident) == 0 and L.gs_dist_init(ctx, ident, 0, 1) == 0, L.gs_last_error(ctx)
        assert L.gs_dist_shard_rows(ctx, _lib.ROWS_CONTIGUOUS) == 0, L.gs_last_error(ctx)
        assert L.gs_backward_device(ctx, out.ctypes.data, None, out.ctypes.data) == _lib.GS_ERR_INVALID
        msg = L.gs_last_error(ctx).decode()
        assert msg.startswith("gs_backward_device: ") and "sharded context" in msg, msg
        assert L.gs_contrib_device(ctx, 1, out.ctypes.data, None, None) == _lib.GS_ERR_INVALID
        msg = L.gs_last_error(ctx).decode()
        assert msg.startswith("gs_contrib_device: ") and "sharded context" in msg, msg
        assert np.all(out == -7.5)
        assert L.gs_destroy(ctx) == 0
        print("refused-ok")
    """)
    from conftest import ROOT
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    assert res.returncode == 0 and "refused-ok" in res.stdout, (res.stdout[-500:], res.stderr[-3000:])


# ---- 9. overflow in a band ------------------------------------------------------------------------------------------------

OVERFLOW_BAND = (0, 34)          # the upper half of the 68 tile rows: 2.3e9 elements against a capacity of 2^24


def test_overflow_in_a_band(oracle_mod, tmp_path):
    """test_backward_cpu.overflowing_scene still overflows inside a band of its own (on the oracle: the counter of the rows
    OVERFLOW_BAND against the band context's capacity).  The band is differentiated as drawn, truncated: its sorted ids and
    ranges equal the oracle's band run, and the gradient under tile_weights on picked tiles -- some of them outside the band,
    where nothing may be read -- equals the float64 reference on the truncated band list under compare_with_reference."""
    aos, w, h = overflowing_scene()
    sc = make_scene(aos, w, h)
    p = camera_params(oracle_mod, sc, w, h, row_begin=OVERFLOW_BAND[0], row_end=OVERFLOW_BAND[1])
    gw, gh = oracle_mod.grid(w, h)
    s1, e, _, _, oi, oranges = oracle_list(oracle_mod, p, aos)
    assert s1["counter"] > s1["capacity"] == e
    tiles = pick_tiles(oranges, gw, gh, seed=3, max_entries=40_000)
    inside = tiles // gw < OVERFLOW_BAND[1]
    assert inside.sum() >= 4 and (~inside).sum() >= 2
    wr, wd = tile_weights(w, h, tiles, seed=4)
    uniq, want = sampled_reference_gradient(tmp_path, p, aos, s1, oi[:e], oranges, tiles, wr.astype(np.float64),
                                            wd.astype(np.float64))
    r = band_renderer(sc, w, h)
    r.setTileRows(*OVERFLOW_BAND)
    r.draw(sc)
    t = r.timings()
    assert r.lastStatus == gs.GS_WARN_OVERFLOW and t.overflowed == 1 and t.num_sort_elements == e
    assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), oi[:e]) and np.array_equal(r.debugRead(gs.BUF_RANGES), oranges)
    got = r.backward(wr, wd)
    r.cleanup()
    assert_sampled_gradient(got, uniq, want, 0, "overflow in a band")
