"""Anti-aliased frames on the MI355X (include/gsplat.h, gs_set_antialias).  The yardstick is the equivalence the definition
implies: the frame of records R with the flag on equals, in everything a frame produces, the frame with the flag off of R' =
R with float 15 replaced by the GS_BUF_RASTER_OPACITY read-back.  The plain frame is pinned by the oracle elsewhere; here
the flag-on frame, its gradients (record, camera, bands), its contributions and the trainer are tied to it, the read-back's
value to the float64 rho64 of tests/test_antialias_cpu.py, and the gradients to that file's composed reference."""
import ctypes as C

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, assert_posed, camera_params
from test_backward_cpu import frozen_of
from test_backward_gpu import CASES as BACKWARD_CASES, READ_FIELDS, UNREAD, compare_with_reference
from test_backward_camera_cpu import PROJ_CLIP_Z, VIEW_BOTTOM_ROW, camera_reference, masked as camera_masked
from test_backward_camera_gpu import check_against
from test_band_backward_gpu import contrib_into, set_band
from test_antialias_cpu import RHO32_DEVIATION, compared, composed_reference, load_antialias_scene, rho64_numpy
from frame64 import FLOOR, frame_decisions, weights

pytestmark = pytest.mark.gpu

F = np.float32
ALL_SCENES = ["ragged", "dense", "zero_det", "ragged@pose", "extreme", "subpixel"]
SH_ONLY = [f for f in range(12, 76) if f != 15 and f % 4 != 3]        # floats 12..75 except 15 that a frame can read
SH_BLOCK = [f for f in range(12, 76) if f != 15]
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def renderer_of(sc, w, h, antialias, **kw):
    """make_renderer with both optional outputs on and the flag set through the call under test."""
    r = make_renderer(sc, w, h, **kw)
    r.setOutputs(rgba32f=True, depth=True)
    if antialias is not None:
        r.setAntialias(antialias)
    return r


def products(r, sc):
    """Everything a frame produces."""
    out = dict(image=r.draw(sc).copy())
    out["rgba32f"], out["depth"] = r.readOutput(gs.GS_OUTPUT_RGBA32F), r.readOutput(gs.GS_OUTPUT_DEPTH)
    for name, which in (("tile", gs.BUF_SORTED_TILE), ("key", gs.BUF_SORTED_DEPTH), ("id", gs.BUF_SORTED_ID),
                        ("ranges", gs.BUF_RANGES), ("cov", gs.BUF_COV)):
        out[name] = r.debugRead(which)
    return out


def same(a, b, names=None):
    """The products that differ (bit for bit; the floats as uint32 words)."""
    return [k for k in (names or a) if not np.array_equal(bits(a[k]), bits(b[k]))]


def twin(aos, raster_opacity):
    """R': the records with float 15 replaced by the read-back."""
    out = np.array(aos, F, copy=True)
    out[:, 15] = raster_opacity
    return out


def drawn_pair(oracle_mod, scene, sh_mode=0, **kw):
    """The scene drawn with the flag on, and its twin R' drawn by a second context with the flag off: (aos, R', w, h, scene
    on, scene off, renderer on, renderer off), both with a frame behind them."""
    aos, w, h, cam = load_antialias_scene(oracle_mod, scene)
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
    on = renderer_of(sc, w, h, True, **kw)
    on.draw(sc)
    prime = twin(aos, on.debugRead(gs.BUF_RASTER_OPACITY))
    sc2 = make_scene(prime, w, h, sh_mode=sh_mode, **cam)
    off = renderer_of(sc2, w, h, None, **kw)
    off.draw(sc2)
    return aos, prime, w, h, sc, sc2, on, off


def test_extreme_scene_is_the_one_of_test_backward_gpu(oracle_mod):
    """'extreme' of load_antialias_scene is the extreme_cloud test_backward_gpu draws, bit for bit."""
    from test_backward_cpu import extreme_cloud
    aos, w, h, cam = load_antialias_scene(oracle_mod, "extreme")
    want, w2, h2 = extreme_cloud()
    assert (w, h, cam) == (w2, h2, {}) and np.array_equal(bits(aos), bits(want))


# ---- 1. equivalence of frames ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ALL_SCENES)
def test_frame_equals_the_plain_frame_of_its_twin(oracle_mod, scene):
    """Every sorter, both render modes, both outputs on: RGBA8, RGBA32F, depth, the sorted tile / depth / id words, the ranges
    and GS_BUF_COV of flag-on(R) equal those of flag-off(R') bit for bit; flag on and off give the same list and ranges for
    the same R.  The read-back: at most the scene's opacity, exactly 0 for non-emitting and det == 0 splats, and with the flag
    off exactly the scene's opacity for the emitting det != 0 ones."""
    aos, w, h, cam = load_antialias_scene(oracle_mod, scene)
    sc = make_scene(aos, w, h, **cam)
    differs = False
    for sort in ALL_SORTS:
        for mode in (gs.GS_RENDER_EXACT, gs.GS_RENDER_FAST):
            what = (scene, sort, mode)
            on, plain = renderer_of(sc, w, h, True, sort=sort, mode=mode), renderer_of(sc, w, h, None, sort=sort, mode=mode)
            a, b = products(on, sc), products(plain, sc)
            ro, ro_plain = on.debugRead(gs.BUF_RASTER_OPACITY), plain.debugRead(gs.BUF_RASTER_OPACITY)
            assert not same(a, b, ("tile", "key", "id", "ranges", "cov")), what
            differs |= bool(same(a, b, ("rgba32f",)))
            emitting = np.zeros(len(aos), bool)
            emitting[a["id"]] = True
            det = a["cov"][:, 0] * a["cov"][:, 2] - a["cov"][:, 1] * a["cov"][:, 1]
            live = emitting & (det != 0)
            assert ro.shape == (len(aos),) and np.all(np.isfinite(ro)), what
            assert np.all(bits(ro[~live]) == 0) and np.all(bits(ro_plain[~live]) == 0), what
            assert np.array_equal(bits(ro_plain[live]), bits(aos[live, 15])), what
            assert np.all(ro[aos[:, 15] >= 0] <= aos[aos[:, 15] >= 0, 15]), what
            sc2 = make_scene(twin(aos, ro), w, h, **cam)
            off = renderer_of(sc2, w, h, False, sort=sort, mode=mode)
            c = products(off, sc2)
            assert not same(a, c), (what, same(a, c))
            for r in (on, plain, off):
                r.cleanup()
    assert differs, scene                                               # the flag does something to this scene's pixels


# ---- 2. the value ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["subpixel", "ragged", "ragged@pose"])
def test_raster_opacity_against_rho64(oracle_mod, scene):
    """The read-back against opacity * rho64 on the emitting splats whose float64 r lies outside [floor / 2, 2 floor] (the
    zero_det needles would be left out as test_backward_gpu leaves them out; these scenes have none).  Bound: four times
    RHO32_DEVIATION = 3.3e-6, the largest relative deviation of a float32 NumPy restatement from rho64 on these scenes
    (tests/test_antialias_cpu.py, test_float32_restatement_deviation), i.e. 1.32e-5 relative; the GPU's own largest deviation
    was 1.8e-7 (subpixel), 3.2e-6 (ragged) and 2.8e-6 (ragged@pose) when the test first ran.  Below the floor the factor is
    sqrt(2.5e-5), exactly."""
    aos, w, h, cam = load_antialias_scene(oracle_mod, scene)
    sc = make_scene(aos, w, h, **cam)
    r = renderer_of(sc, w, h, True)
    r.draw(sc)
    ro = r.debugRead(gs.BUF_RASTER_OPACITY).astype(np.float64)
    emitting = np.zeros(len(aos), bool)
    emitting[r.debugRead(gs.BUF_SORTED_ID)] = True
    r.cleanup()
    p = camera_params(oracle_mod, sc, w, h)
    rho, r64 = rho64_numpy(p, aos)
    keep = emitting & compared(scene, aos, r64)
    assert keep.sum() >= 0.9 * emitting.sum() and keep.sum() >= 60
    want = aos[:, 15].astype(np.float64) * rho
    dev = np.abs(ro[keep] - want[keep]) / np.maximum(want[keep], 1e-300)
    print(f"{scene}: {keep.sum()} splats, largest relative deviation of the read-back from opacity * rho64 {dev.max():.3e}")
    assert np.all(np.abs(ro[keep] - want[keep]) <= 4 * RHO32_DEVIATION * want[keep]), dev.max()
    if scene == "subpixel":
        floored = keep & (r64 < FLOOR / 2)
        assert floored.sum() >= 10
        assert np.array_equal(ro[floored].astype(F), (aos[floored, 15] * np.sqrt(F(2.5e-5))).astype(F))


# ---- 3. off is off --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("timers", [False, True])
def test_off_is_off(oracle_mod, timers):
    """A context that never calls the setter, one that calls it with 0 and one that toggles 1 -> 0 (with a frame drawn while
    it was on): byte-identical frames and bit-identical gs_backward results, without timers (the frame's camera-free stages
    replay as one graph) and with them (each run of passes replays alone)."""
    for scene in ("ragged", "subpixel"):
        aos, w, h, cam = load_antialias_scene(oracle_mod, scene)
        sc = make_scene(aos, w, h, **cam)
        wr, wd = weights(h, w, 3)
        got = []
        for how in ("never", "zero", "toggled"):
            r = renderer_of(sc, w, h, {"never": None, "zero": False, "toggled": True}[how], record_timings=timers)
            if how == "toggled":
                r.draw(sc)
                r.setAntialias(False)
            r.draw(sc)                                                  # a first frame captures, the second replays
            frame = products(r, sc)
            frame["grad"] = r.backward(wr, wd)
            frame["raster_opacity"] = r.debugRead(gs.BUF_RASTER_OPACITY)
            got.append(frame)
            r.cleanup()
        assert not same(got[0], got[1]) and not same(got[0], got[2]), (scene, same(got[0], got[1]), same(got[0], got[2]))


# ---- 4. toggle and share --------------------------------------------------------------------------------------------------

def test_toggle_in_one_context(oracle_mod):
    """Off, on, off over three frames of one context: the first and third are identical, the second equals its twin's."""
    aos, prime, w, h, sc, sc2, on, off = drawn_pair(oracle_mod, "subpixel")
    want_on, want_off = products(on, sc), products(off, sc2)
    r = renderer_of(sc, w, h, None)
    first = products(r, sc)
    r.setAntialias(True)
    second = products(r, sc)
    r.setAntialias(False)
    third = products(r, sc)
    for x in (r, on, off):
        x.cleanup()
    assert not same(first, third)
    assert not same(second, want_on) and not same(second, want_off)
    assert same(first, second, ("rgba32f",))


def test_two_contexts_share_a_scene(oracle_mod):
    """Two contexts over one uploaded scene (gs_share_scene), one on and one off: each gives its own frame, in either call
    order, with both frames in flight."""
    aos, w, h, cam = load_antialias_scene(oracle_mod, "ragged@pose")
    sc = make_scene(aos, w, h, **cam)
    want = {}
    for flag in (True, False):
        r = renderer_of(sc, w, h, flag)
        want[flag] = r.draw(sc).copy()
        r.cleanup()
    assert not np.array_equal(want[True], want[False])
    owner = renderer_of(sc, w, h, True)
    other = gs.Renderer(w, h, warmup_frames=0)
    other.init(sc.getResourceManager())
    other.initForScene(share_with=owner)
    for order in ((owner, other), (other, owner), (owner, other)):
        for r in order:
            r.drawDevice(sc, None, sync=False)
        for r in order:
            r.synchronize()
        assert np.array_equal(owner.debugRead(gs.BUF_IMAGE), want[True]), order
        assert np.array_equal(other.debugRead(gs.BUF_IMAGE), want[False]), order
    other.cleanup()
    owner.cleanup()


def test_gradient_is_that_of_the_frame_as_drawn(oracle_mod):
    """The flag flipped after a frame and before gs_backward: the gradient is that of the frame as it was drawn, bit for bit,
    in both directions."""
    aos, w, h, cam = load_antialias_scene(oracle_mod, "subpixel")
    sc = make_scene(aos, w, h, **cam)
    wr, wd = weights(h, w, 5)
    want = {}
    for flag in (True, False):
        r = renderer_of(sc, w, h, flag)
        r.draw(sc)
        want[flag] = r.backward(wr, wd)
        want_camera = r.backwardCamera()
        r.draw(sc)
        r.setAntialias(not flag)
        assert np.array_equal(bits(r.backward(wr, wd)), bits(want[flag])), flag
        assert np.array_equal(bits(r.backwardCamera()), bits(want_camera)), flag
        r.cleanup()
    assert not np.array_equal(want[True], want[False])


# ---- 5. gradients against the composed reference ----------------------------------------------------------------------------

GRADIENT_CASES = [c for c in BACKWARD_CASES if c[0] in ALL_SCENES] + [("subpixel", m) for m in (0, 1, 2)]


@pytest.mark.parametrize("scene,sh_mode", GRADIENT_CASES)
def test_gradient_against_the_composed_reference(oracle_mod, tmp_path, scene, sh_mode):
    """gs_backward of flag-on(R) against the composed reference (tests/test_antialias_cpu.py) under
    test_backward_gpu.compare_with_reference, R' from the GPU's read-back, the zero_det needles left out as there.  Bit for
    bit: floats 12..75 except 15 equal those of flag-off(R'), and so do the visible ids and count; unread fields and culled
    splats are exactly zero.  The opacity column is the twin's times the factor."""
    aos, prime, w, h, sc, sc2, on, off = drawn_pair(oracle_mod, scene, sh_mode)
    wr, wd = weights(h, w, 1)
    got, got_off = on.backward(wr, wd), off.backward(wr, wd)
    ids, _, count = on.backwardVisible(wr, wd)
    ids_off, _, count_off = off.backwardVisible(wr, wd)
    emitting = np.zeros(len(aos), bool)
    emitting[on.debugRead(gs.BUF_SORTED_ID)] = True
    on.cleanup()
    off.cleanup()
    assert np.all(np.isfinite(got)) and np.all(got[:, UNREAD] == 0) and np.all(got[~emitting] == 0)
    assert np.array_equal(bits(got[:, SH_BLOCK]), bits(got_off[:, SH_BLOCK]))
    assert count == count_off and np.array_equal(ids, ids_off)
    p = camera_params(oracle_mod, sc, w, h)
    if scene.endswith("@pose"):
        assert_posed(p)
    ref, flags = frame_decisions(tmp_path, p, prime)
    fz = frozen_of(scene, aos)
    want, _, plain = composed_reference(p, aos, prime, ref, flags, wr.astype(np.float64), wd.astype(np.float64),
                                        fz if fz.any() else None)
    if scene in ("subpixel", "ragged"):                                 # the factor's own terms are not lost in the tolerance:
        assert compare_with_reference(plain, want, ~fz)                 # the twin's gradient alone does not pass
    bad = compare_with_reference(got, want, ~fz)
    assert not bad, bad[:10]


@pytest.mark.parametrize("scene", ["subpixel", "ragged@pose"])
def test_every_form_and_entry_point_gives_the_same_bits(oracle_mod, scene):
    """Flag on: the dense and the visible form, the host and the device entry points, and two runs agree bit for bit."""
    torch = pytest.importorskip("torch")
    aos, w, h, cam = load_antialias_scene(oracle_mod, scene)
    sc = make_scene(aos, w, h, **cam)
    r = renderer_of(sc, w, h, True)
    r.draw(sc)
    wr, wd = weights(h, w, 2)
    dense = r.backward(wr, wd)
    ids, rows, count = r.backwardVisible(wr, wd)
    assert count == len(ids) > 0 and np.array_equal(bits(rows), bits(dense[ids]))
    assert not dense[np.setdiff1d(np.arange(len(aos)), ids)].any()
    gr, gd = torch.tensor(wr, device="cuda"), torch.tensor(wd, device="cuda")
    out = torch.full((len(aos), 84), float("nan"), device="cuda")
    d_ids = torch.zeros(len(aos), dtype=torch.int32, device="cuda")
    d_rows = torch.full((len(aos), 84), float("nan"), device="cuda")
    d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.backwardDevice(gr.data_ptr(), gd.data_ptr(), out.data_ptr())
    r.backwardVisibleDevice(gr.data_ptr(), gd.data_ptr(), d_ids.data_ptr(), d_rows.data_ptr(), len(aos), d_count.data_ptr())
    r.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(dense))
    assert int(d_count.item()) == count
    assert np.array_equal(d_ids.cpu().numpy().view(np.uint32)[:count], ids)
    assert np.array_equal(bits(d_rows.cpu().numpy()[:count]), bits(rows))
    r.draw(sc)
    assert np.array_equal(bits(r.backward(wr, wd)), bits(dense))
    r.cleanup()
    again = renderer_of(sc, w, h, True)
    again.draw(sc)
    assert np.array_equal(bits(again.backward(wr, wd)), bits(dense))
    again.cleanup()


# ---- 6. camera gradients ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,sh_mode", [("ragged", 0), ("ragged@pose", 0), ("ragged@pose", 1), ("subpixel", 0)])
def test_camera_gradient(oracle_mod, tmp_path, scene, sh_mode):
    """gs_backward_camera of flag-on(R) against the camera reference of tests/test_backward_camera_cpu.py at R' plus sum_g
    G'[g, 15] o_g d rho64_g / dview, under the rule of tests/test_backward_camera_gpu.py (TAU of S per component, S with the
    absolute values of the added terms).  Bit for bit: the dproj and dcam_pos blocks are those of flag-off(R'); the view's bottom
    row and the projection's clip-z row are +0.0f."""
    aos, prime, w, h, sc, sc2, on, off = drawn_pair(oracle_mod, scene, sh_mode)
    wr, wd = weights(h, w, 1)
    on.backward(wr, wd)
    off.backward(wr, wd)
    got, got_off = on.backwardCamera(), off.backwardCamera()
    on.cleanup()
    off.cleanup()
    assert np.array_equal(bits(got[16:35]), bits(got_off[16:35]))
    assert np.all(bits(got[VIEW_BOTTOM_ROW + PROJ_CLIP_Z]) == 0)
    assert not np.array_equal(got[0:16], got_off[0:16])
    p = camera_params(oracle_mod, sc, w, h)
    want, S, _ = camera_reference(("antialias", scene, sh_mode), tmp_path, p, prime, wr, wd)
    ref, flags = frame_decisions(tmp_path, p, prime)
    _, view_terms, _ = composed_reference(p, aos, prime, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    want, S = want.copy(), S.copy()
    want[0:16] += camera_masked(np.concatenate([view_terms.sum(0), np.zeros(19)]))[0:16]
    S[0:16] += camera_masked(np.concatenate([np.abs(view_terms).sum(0), np.zeros(19)]))[0:16]
    check_against(got, want, S, f"antialias {scene} sh{sh_mode}")


# ---- 7. bands ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["halves", "stride2"])
def test_bands(oracle_mod, layout):
    """gs_set_band_gradients on, ragged@pose (12 tile rows) as two contiguous bands and as an interleaved dealing of stride
    2: each band's frame, its dense band gradient's SH columns and its contributions equal the flag-off(R') band's bit for
    bit, and the band gradients summed give the whole frame's under compare_with_reference (the rule of
    test_band_backward_gpu.test_three_rank_step_on_one_gpu for that sum: float32 association across bands)."""
    torch = pytest.importorskip("torch")
    aos, prime, w, h, sc, sc2, on, off = drawn_pair(oracle_mod, "ragged@pose")
    n = len(aos)
    wr, wd = weights(h, w, 4)
    whole = on.backward(wr, wd)
    zeros = lambda: [np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32)]
    total = np.zeros((n, 84), np.float64)
    for r in (on, off):
        r.setBandGradients(True)
    for spec in {"halves": [("rows", 0, 6), ("rows", 6, 12)], "stride2": [("il", 0, 2, 0), ("il", 1, 2, 0)]}[layout]:
        frames, grads, contribs = [], [], []
        for r, scene_of in ((on, sc), (off, sc2)):
            set_band(r, spec)
            frames.append(products(r, scene_of))
            assert r.timings().overflowed == 0
            grads.append(r.backward(wr, wd))
            contribs.append(contrib_into(torch, r, n, zeros()))
        assert not same(frames[0], frames[1]), (spec, same(frames[0], frames[1]))
        assert frames[0]["image"].any() and grads[0].any()
        assert np.array_equal(bits(grads[0][:, SH_BLOCK]), bits(grads[1][:, SH_BLOCK])), spec
        for a, b in zip(contribs[0], contribs[1]):
            assert np.array_equal(bits(a), bits(b)), spec
        assert contribs[0][2].any()
        total += grads[0]
    on.cleanup()
    off.cleanup()
    bad = compare_with_reference(total.astype(F), whole.astype(np.float64), np.ones(n, bool))
    assert not bad, bad[:10]


# ---- 8. contributions -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["ragged", "subpixel"])
def test_contributions(oracle_mod, scene):
    """gs_contrib_device replays with the raster opacity: flag-on(R) equals flag-off(R') bit for bit in wmax, wsum and
    pixels, and differs from the plain frame of R."""
    torch = pytest.importorskip("torch")
    aos, prime, w, h, sc, sc2, on, off = drawn_pair(oracle_mod, scene)
    n = len(aos)
    zeros = lambda: [np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32)]
    a, b = contrib_into(torch, on, n, zeros()), contrib_into(torch, off, n, zeros())
    on.setAntialias(False)
    on.draw(sc)
    plain = contrib_into(torch, on, n, zeros())
    on.cleanup()
    off.cleanup()
    assert a[2].any()
    for x, y in zip(a, b):
        assert np.array_equal(bits(x), bits(y))
    assert not np.array_equal(a[0], plain[0])


# ---- 9. the trainer ---------------------------------------------------------------------------------------------------------

def test_visible_adam_trains_antialiased():
    """autograd.VisibleAdam on an anti-aliased renderer (make_renderer(antialias=True)): the target is the truth's frame drawn
    with the flag on, the start its SH constant term moved by noise of 0.3 (the case of test_adam_gpu.test_visible_adam_trains);
    twenty steps at the default rates: the loss of step 20 is below that of step 1 and every record stays finite."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    truth, w, h = SCENES["dense"]()
    truth = np.ascontiguousarray(truth, dtype=F)
    start = truth.copy()
    start[:, 12:15] += 0.3 * np.random.default_rng(3).standard_normal((len(truth), 3)).astype(F)
    sc = make_scene(truth, w, h)
    r = renderer_of(sc, w, h, True)
    r.draw(sc)
    target = torch.tensor(np.ascontiguousarray(r.readOutput(gs.GS_OUTPUT_RGBA32F)[..., :3]), device="cuda")
    r.cleanup()
    cam = sc.getCamera()
    view, proj, pos = cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition()
    rr = autograd.make_renderer(w, h, antialias=True)
    assert rr.antialias
    records = torch.tensor(start, device="cuda")
    opt = autograd.VisibleAdam(records, renderer=rr)
    numbers = [opt.step(view, proj, pos, 0, target) for _ in range(20)]
    opt.stream.synchronize()
    losses = [float(x[0]) for x in numbers]
    final = records.cpu().numpy()
    rr.cleanup()
    print("loss per step:", losses)
    assert np.all(np.isfinite(losses)) and np.all(np.isfinite(final))
    assert losses[-1] < losses[0], losses


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------

def test_refusals(oracle_mod):
    """enable = 2 is refused with a message and leaves the flag as it was (on and off); gs_debug_read(GS_BUF_RASTER_OPACITY)
    refuses a size beyond N floats and a context without a frame, like its neighbours."""
    aos, w, h, cam = load_antialias_scene(oracle_mod, "subpixel")
    sc = make_scene(aos, w, h, **cam)
    L = _lib.lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    frames = {}
    for flag in (False, True):
        r = renderer_of(sc, w, h, flag)
        buf = np.zeros(len(aos) + 1, F)
        assert L.gs_debug_read(r._ctx.handle, gs.BUF_RASTER_OPACITY, p(buf), len(aos) * 4) == _lib.GS_ERR_NO_SCENE
        assert L.gs_debug_read(r._ctx.handle, gs.BUF_COV, p(buf), 16) == _lib.GS_ERR_NO_SCENE
        assert L.gs_set_antialias(r._ctx.handle, 2) == _lib.GS_ERR_INVALID
        assert b"enable must be 0 or 1" in L.gs_last_error(r._ctx.handle)
        assert L.gs_set_antialias(r._ctx.handle, 0xFFFFFFFF) == _lib.GS_ERR_INVALID
        frames[flag] = r.draw(sc).copy()
        assert L.gs_debug_read(r._ctx.handle, gs.BUF_RASTER_OPACITY, p(buf), buf.nbytes) == _lib.GS_ERR_INVALID
        assert b"size exceeds buffer" in L.gs_last_error(r._ctx.handle)
        assert L.gs_debug_read(r._ctx.handle, gs.BUF_RASTER_OPACITY, p(buf), len(aos) * 4) == _lib.GS_OK
        assert L.gs_debug_read(r._ctx.handle, gs.BUF_RASTER_OPACITY, p(buf), 8) == _lib.GS_OK
        assert np.array_equal(buf[:len(aos)], r.debugRead(gs.BUF_RASTER_OPACITY))
        r.cleanup()
    assert not np.array_equal(frames[False], frames[True])
