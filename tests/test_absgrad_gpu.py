"""Absolute screen gradients on the MI355X (include/gsplat.h, gs_set_abs_gradients / gs_abs_screen_gradient_device /
gs_densify_stats_abs_device): by value against the float64 reference of tests/test_absgrad_cpu.py, the designed scenes of
that file (cancellation, one pixel, the staging batch edges, the early-out over stale scratch, a truncated list), the exact
properties (the switch changes no bit of anything else, monotonicity, determinism across calls, sorters and a resolution
change, max_rows / count / foreign ids), bands, the refusals, and VisibleAdam(abs_density=True)."""
import ctypes as C

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, camera_params, load_scene
from test_backward_cpu import check_truncated, frozen_of, list_offsets, truncated_scene
from test_train_chain_gpu import LAMBDA, bits, new_renderer
from test_densify_cpu import screen_norm
from test_densify_gpu import DEV, Frame, assert_norm, down, sentinels, up, zeros
from test_band_backward_gpu import band_renderer, draw_band
from test_absgrad_cpu import (BATCH_COUNTS, STOP_FRONT, abs_screen_gradient, batch_case, cancellation_case, case_reference,
                              early_out_case, one_pixel_case)
from frame64 import frame_decisions, weights

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
NO_BACKWARD = "no gs_backward* on this frame with gs_set_abs_gradients on"


class AbsFrame(Frame):
    """Frame of tests/test_densify_gpu.py with the switch on before its backward, and the two reading calls."""

    switch = True

    def backward(self):
        self.r.setAbsGradients(self.switch)
        super().backward()

    def pairs(self, max_rows=None, ids=None, count=None, out=None):
        """gs_abs_screen_gradient_device into `out` (a fresh sentinel array of n + 8 rows by default) -> float32 [.., 2]."""
        if out is None:
            out = torch.full((self.n + 8, 2), -3.25, device=DEV)
            torch.cuda.synchronize()
        self.r.absScreenGradientDevice((ids if ids is not None else self.ids).data_ptr(),
                                       (count if count is not None else self.count).data_ptr(),
                                       self.n if max_rows is None else max_rows, out.data_ptr())
        self.r.synchronize()
        return down(out, F).reshape(-1, 2)

    def per_splat(self):
        """The pairs by splat index [n, 2] (zero outside V)."""
        V = self.visible()
        got = np.zeros((self.n, 2), F)
        got[V] = self.pairs()[:len(V)]
        return got

    def abs_stats(self, accum, max_rows=None, ids=None, count=None, n=None):
        self.r.densifyStatsAbsDevice((ids if ids is not None else self.ids).data_ptr(),
                                     (count if count is not None else self.count).data_ptr(),
                                     self.n if max_rows is None else max_rows, self.n if n is None else n, accum.data_ptr())
        self.r.synchronize()
        return down(accum, F)


class OffFrame(AbsFrame):
    switch = False


def assert_pairs(got, want, keep, what):
    """assert_norm's bound per component: |got - want| <= 2e-2 |want| + 2e-3 max|want| over the splats `keep`."""
    for k, axis in enumerate("xy"):
        assert_norm(got[:, k], want[:, k], keep, f"{what} abs_{axis}")


_REFERENCE = {}


def scene_reference(oracle_mod, tmp_path, scene, f):
    """The float64 pair of a scene of SCENES under Frame's default image gradients, computed once."""
    if scene not in _REFERENCE:
        aos, w, h, cam = load_scene(scene)
        p = camera_params(oracle_mod, f.sc, w, h)
        ref, flags = frame_decisions(tmp_path, p, aos)
        fz = frozen_of(scene.partition("@")[0], aos)
        ab, _ = abs_screen_gradient(p, aos, ref, flags, f.wr, f.wd, fz if fz.any() else None)
        ab.setflags(write=False)
        _REFERENCE[scene] = (ab, fz, list_offsets(ref)[0] != 0)
    return _REFERENCE[scene]


# ---- 1. by value --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene", ["ragged", "dense", "zero_det", "ragged@pose"])
def test_by_value(oracle_mod, tmp_path, scene):
    """grad_accum_abs after one call from zeros against screen_norm of the reference pair, within the project's gradient
    tolerance (the frozen needles of zero_det excluded), exactly 0 outside V; the pairs themselves per component; a second
    call gives fl(a + a); grad_accum_abs >= grad_accum on every splat (the same terms in the same tree, every operation of
    both norms monotone) -- the library does not return dsx, dsy themselves, so abs_x >= |dsx| is checked through the norm
    here and bit for bit in test_one_pixel."""
    aos, w, h, cam = load_scene(scene)
    f = AbsFrame(aos, w, h, cam)
    signed = f.stats(zeros(f.n))[0].copy()
    acc = zeros(f.n)[0]
    once = f.abs_stats(acc).copy()
    twice = f.abs_stats(acc).copy()
    got = f.per_splat()
    V = f.visible()
    f.r.cleanup()
    want, fz, inV = scene_reference(oracle_mod, tmp_path, scene, f)
    assert np.array_equal(V, np.flatnonzero(inV))
    assert not bits(once[~inV]).any() and np.all(np.isfinite(once[~fz])) and np.count_nonzero(once) > 20
    assert_norm(once, screen_norm(want, w, h), ~fz, scene)
    assert_pairs(got, want, ~fz, scene)
    assert np.array_equal(bits(twice), bits(once + once))
    assert np.all(once[~fz] >= signed[~fz]) and np.all(got[~fz] >= 0)
    gx, gy = got[:, 0] * F(0.5) * F(w), got[:, 1] * F(0.5) * F(h)
    assert np.array_equal(bits(once[~fz]), bits(np.sqrt(gx * gx + gy * gy)[~fz]))        # the header's expression, in float32
    more = int(np.count_nonzero(once > 2 * signed))
    print(f"{scene}: abs norm > 2 x signed norm on {more} of {len(V)} visible splats")


# ---- 2. the designed scenes ---------------------------------------------------------------------------------------------------

def designed_frame(aos, w, h, g, cls=AbsFrame):
    wd = g[1] if g[1] is not None else np.zeros((h, w), F)
    return cls(aos, w, h, grads=(g[0], wd))


def test_cancellation(oracle_mod, tmp_path):
    """One splat on the edge of two tiles under a uniform positive gradient: the signed norm is below 1e-3 of the absolute
    one, which is the reference's within the tolerance."""
    aos, w, h, g = cancellation_case()
    f = designed_frame(aos, w, h, g)
    signed = f.stats(zeros(f.n))[0].copy()
    ab = f.abs_stats(zeros(f.n)[0]).copy()
    got = f.per_splat()
    f.r.cleanup()
    _, _, _, want, _ = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    print(f"cancellation: signed {signed[0]:.3e}, absolute {ab[0]:.3e}")
    assert signed[0] < 1e-3 * ab[0]
    assert_norm(ab, screen_norm(want, w, h), np.ones(1, bool), "cancellation")
    assert_pairs(got, want, np.ones(1, bool), "cancellation")


def test_one_pixel(oracle_mod, tmp_path):
    """One (entry, pixel) pair in the whole frame: the pair is the absolute value of the one signed term, so
    grad_accum_abs has the bits of grad_accum, and the pair reproduces both through the header's expression; a second
    gs_abs_screen_gradient_device gives the same bits."""
    aos, w, h, g = one_pixel_case(oracle_mod)
    _, _, flags, want, _ = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    assert int(np.count_nonzero(flags)) == 1
    f = designed_frame(aos, w, h, g)
    signed = f.stats(zeros(f.n))[0].copy()
    ab = f.abs_stats(zeros(f.n)[0]).copy()
    got, again = f.per_splat(), f.per_splat()
    f.r.cleanup()
    assert signed[0] > 0 and np.array_equal(bits(ab), bits(signed))
    gx, gy = got[:, 0] * F(0.5) * F(w), got[:, 1] * F(0.5) * F(h)
    assert np.array_equal(bits(np.sqrt(gx * gx + gy * gy)), bits(signed)) and got.min() > 0
    assert np.array_equal(bits(got), bits(again))
    assert_pairs(got, want, np.ones(1, bool), "one pixel")


@pytest.mark.parametrize("count", BATCH_COUNTS)
def test_batch_edges(oracle_mod, tmp_path, count):
    """1, 63, 64, 65, 128 and 129 entries per tile (kBwdBatch = 64), no pixel stopping: every splat's pair."""
    aos, w, h, g = batch_case(count)
    f = designed_frame(aos, w, h, g)
    got = f.per_splat()
    f.r.cleanup()
    _, _, _, want, _ = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    assert np.all(got.min(1) > 0)
    assert_pairs(got, want, np.ones(count, bool), f"{count} entries")


def test_early_out_over_stale_scratch(oracle_mod, tmp_path):
    """The 129-entry frame first; then, in place on the same context and scratch, early_out_case: the 109 splats behind the
    front twenty are reached by no pixel -- their pairs are (0, 0) exactly (not what the first frame left in their slots)
    and grad_accum_abs keeps its sentinel bits; the front twenty are the reference's."""
    aos0, w, h, g0 = batch_case(129)
    aos, _, _, g = early_out_case()
    f = designed_frame(aos0, w, h, g0)
    first = f.per_splat()
    assert np.all(first.min(1) > 0)
    d_aos = up(aos)
    f.g_rgba, f.g_depth = up(g[0]), up(g[1])
    torch.cuda.synchronize()
    f.r.uploadDevice(d_aos.data_ptr(), len(aos))
    f.r.draw(f.sc)                      # (the scene's camera; the records are the uploaded ones)
    f.backward()
    got = f.per_splat()
    accum = f.abs_stats(sentinels(f.n)[0])
    V = f.visible()
    f.r.cleanup()
    _, _, _, want, _ = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    assert len(V) == 129 and not want[STOP_FRONT:].any()
    assert not bits(got[STOP_FRONT:]).any()
    assert np.array_equal(bits(accum[STOP_FRONT:]), bits(np.full(129 - STOP_FRONT, 7.5, F)))
    assert np.all(accum[:STOP_FRONT] > F(7.5))
    front = np.arange(129) < STOP_FRONT
    assert_pairs(got, want, front, "early out")


def test_truncated_list(oracle_mod, tmp_path):
    """truncated_scene (34207 elements against a capacity of 32768): rows at or past the capacity contribute nothing -- the
    splats wholly past it have (0, 0) exactly and are listed all the same, the straddling splat sums its surviving rows."""
    aos, w, h = truncated_scene()
    g = weights(h, w, 6)
    f = designed_frame(aos, w, h, g)
    assert f.r.lastStatus == gs.GS_WARN_OVERFLOW
    got = f.per_splat()
    V = f.visible()
    f.r.cleanup()
    _, ref, flags, want, _ = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    across, past = check_truncated(ref, flags)
    assert np.isin(np.flatnonzero(past), V).all() and not bits(got[past]).any()
    assert got[across].any()
    assert_pairs(got, want, np.ones(len(aos), bool), "truncated")


# ---- 3. exact properties ------------------------------------------------------------------------------------------------------

def everything_else(f):
    """What the calls that existed before return on f's frame: the dense form, the visible form, the camera's 35 floats
    after each, and gs_densify_stats_device's three arrays."""
    out = {"dense": f.r.backward(f.wr, f.wd), "camera_dense": f.r.backwardCamera()}
    ids, rows, count = f.r.backwardVisible(f.wr, f.wd)
    out.update(ids=ids, rows=rows, count=np.array([count]), camera_visible=f.r.backwardCamera())
    f.backward()
    for name, a in zip(("accum", "seen", "radius"), f.stats(zeros(f.n))):
        out[name] = a.copy()
    out["ids_dev"] = f.visible()
    return out


@pytest.mark.parametrize("scene", ["ragged", "dense"])
def test_the_switch_changes_nothing_else(scene):
    """ids, count, the 84-float rows, the dense records, gs_backward_camera's 35 floats and gs_densify_stats_device's
    arrays with the switch on are bit for bit those of a run with it off, in the dense and the visible form."""
    aos, w, h = SCENES[scene]()
    results = []
    for cls in (OffFrame, AbsFrame):
        f = cls(aos, w, h)
        results.append(everything_else(f))
        if cls is AbsFrame:
            assert f.per_splat().any()
        f.r.cleanup()
    off, on = results
    assert off["dense"].any() and off["camera_dense"].any() and off["count"][0] > 500
    for name in off:
        assert np.array_equal(bits(off[name]), bits(on[name])), name


def test_same_bits_from_every_call_and_sorter():
    """Two calls, every sorter, and a resolution change and back (the scratch is freed and allocated again): the same bits."""
    aos, w, h = SCENES["ragged"]()
    first = None
    for sort in ALL_SORTS:
        f = AbsFrame(aos, w, h, sort=sort)
        got = f.per_splat()
        if first is None:
            first = got
            assert first.any() and np.array_equal(bits(f.per_splat()), bits(first))
            L, hdl = _lib.lib(), f.r._ctx.handle
            assert L.gs_set_resolution(hdl, 64, 48) == _lib.GS_OK and L.gs_set_resolution(hdl, w, h) == _lib.GS_OK
            f.r.draw(f.sc)
            f.backward()
            assert np.array_equal(bits(f.per_splat()), bits(first))
        else:
            assert np.array_equal(bits(got), bits(first)), sort
        f.r.cleanup()


def test_max_rows_count_and_foreign_ids():
    """max_rows < |V|, a count below max_rows, ids >= n: rows at or past the list keep their sentinel bits, a foreign id
    writes (0, 0) into its row of abs_out and is skipped by the accumulating call; max_rows == 0 takes NULL pointers."""
    aos, w, h = SCENES["ragged"]()
    f = AbsFrame(aos, w, h)
    V = f.visible()
    full = f.pairs()[:len(V)].copy()
    acc_full = f.abs_stats(zeros(f.n)[0]).copy()
    for max_rows, count in ((100, None), (257, None), (len(V) + 50, 300), (0, None)):
        cnt = None if count is None else up(np.array([count], np.uint32))
        torch.cuda.synchronize()
        k = min(max_rows, len(V) if count is None else count)
        out = f.pairs(max_rows=max_rows, count=cnt)
        assert np.array_equal(bits(out[:k]), bits(full[:k])) and np.all(out[k:] == F(-3.25)), max_rows
        accum = f.abs_stats(sentinels(f.n + 8)[0], max_rows=max_rows, count=cnt)
        moved = np.zeros(f.n + 8, bool)
        moved[V[:k]] = True
        assert np.all(accum[~moved] == F(7.5)), max_rows
        assert np.array_equal(bits(accum[moved]), bits(F(7.5) + acc_full[V[:k]])), max_rows
    L, hdl = _lib.lib(), f.r._ctx.handle
    assert L.gs_abs_screen_gradient_device(hdl, None, None, 0, None) == _lib.GS_OK
    assert L.gs_densify_stats_abs_device(hdl, None, None, 0, f.n, None) == _lib.GS_OK
    a, b = int(V[3]), int(V[40])
    ids = up(np.array([a, f.n, b, 0xFFFFFFFF, f.n + 1, int(V[41])], np.uint32))
    cnt = up(np.array([5], np.uint32))
    torch.cuda.synchronize()
    out = f.pairs(max_rows=6, ids=ids, count=cnt)
    assert np.array_equal(bits(out[0]), bits(full[3])) and np.array_equal(bits(out[2]), bits(full[40]))
    assert not bits(out[[1, 3, 4]]).any() and np.all(out[5:] == F(-3.25))
    accum = f.abs_stats(sentinels(f.n + 8)[0], max_rows=6, ids=ids, count=cnt)
    moved = np.zeros(f.n + 8, bool)
    moved[[a, b]] = True
    assert np.all(accum[~moved] == F(7.5)) and np.all(accum[moved] > F(7.5))
    f.r.cleanup()


# ---- 4. bands -----------------------------------------------------------------------------------------------------------------

def test_two_bands_add_up(oracle_mod):
    """ragged in two bands of tile rows with gs_set_band_gradients on: a splat inside one band has the whole frame's bits
    there (and is not listed, or zero, in the other); for a splat across the edge the two partial pairs added differ from
    the whole frame's by at most 2 (k - 1) 2^-24 relative, k its tile count (non-negative floats summed in another order).
    The accumulating call stays refused on a band."""
    import oracle
    aos, w, h = SCENES["ragged"]()
    gh, cut = (h + 15) // 16, 5
    whole = AbsFrame(aos, w, h)
    want = whole.per_splat()
    sp = oracle.full_pipeline(camera_params(oracle_mod, whole.sc, w, h), aos)["stage1"]["splats"]
    touched = list_offsets(dict(stage1=dict(splats=sp)))[0]
    whole.r.cleanup()
    parts = []
    band = band_renderer(whole.sc, w, h)
    band.setAbsGradients(True)
    for spec in (("rows", 0, cut), ("rows", cut, gh)):
        draw_band(band, whole.sc, spec)
        ids = torch.full((len(aos),), -1, dtype=torch.int32, device=DEV)
        rows = torch.zeros(len(aos), 84, device=DEV)
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        out = torch.full((len(aos), 2), -3.25, device=DEV)
        torch.cuda.synchronize()
        band.backwardVisibleDevice(whole.g_rgba.data_ptr(), whole.g_depth.data_ptr(), ids.data_ptr(), rows.data_ptr(), len(aos),
                                   count.data_ptr())
        band.absScreenGradientDevice(ids.data_ptr(), count.data_ptr(), len(aos), out.data_ptr())
        rc = _lib.lib().gs_densify_stats_abs_device(band._ctx.handle, C.c_void_p(ids.data_ptr()), C.c_void_p(count.data_ptr()),
                                                    len(aos), len(aos), C.c_void_p(out.data_ptr()))
        assert rc == _lib.GS_ERR_INVALID and "subset of the tile rows" in _lib.lib().gs_last_error(band._ctx.handle).decode()
        band.synchronize()
        k = int(down(count, np.uint32)[0])
        part = np.zeros((len(aos), 2), F)
        listed = np.zeros(len(aos), bool)
        v = down(ids, np.uint32)[:k].astype(np.int64)
        part[v] = down(out, F).reshape(-1, 2)[:k]
        listed[v] = True
        parts.append((part, listed))
    band.cleanup()
    (a, in_a), (b, in_b) = parts
    vis = touched != 0
    assert np.array_equal(in_a | in_b, vis)
    both = in_a & in_b
    assert both.sum() > 50 and (in_a & ~in_b).sum() > 500 and (in_b & ~in_a).sum() > 500
    assert np.array_equal(bits(a[in_a & ~in_b]), bits(want[in_a & ~in_b]))
    assert np.array_equal(bits(b[in_b & ~in_a]), bits(want[in_b & ~in_a]))
    total = (a[both] + b[both]).astype(np.float64)
    bound = 2.0 * (touched[both] - 1)[:, None] * 2.0 ** -24 * want[both].astype(np.float64)
    err = np.abs(total - want[both])
    print(f"bands: {int(both.sum())} splats across the edge, worst error / bound "
          f"{float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
    assert np.all(err <= bound)


# ---- 5. the refusals ----------------------------------------------------------------------------------------------------------

def test_refusals():
    """Each refusal with its message and nothing enqueued (the sentinels stay): the switch off, the switch turned on after
    the backward, a new frame since the backward, NULL pointers with max_rows > 0, an n other than the scene's, a band
    without the band flag, a NULL context; and a valid call afterwards works."""
    aos, w, h = SCENES["dense"]()
    f = OffFrame(aos, w, h)
    n, L, hdl = f.n, _lib.lib(), f.r._ctx.handle
    out = torch.full((n, 2), -3.25, device=DEV)
    accum = sentinels(n)[0]
    vp = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def pairs(i=f.ids, c=f.count, max_rows=n, o=out, ctx=hdl):
        return L.gs_abs_screen_gradient_device(ctx, vp(i), vp(c), max_rows, vp(o))

    def stats(i=f.ids, c=f.count, max_rows=n, nn=n, a=accum, ctx=hdl):
        return L.gs_densify_stats_abs_device(ctx, vp(i), vp(c), max_rows, nn, vp(a))

    def refused(rc, word):
        msg = L.gs_last_error(hdl).decode()
        assert rc == _lib.GS_ERR_INVALID and word in msg, (rc, word, msg)

    for call in (pairs, stats):
        refused(call(), NO_BACKWARD)                                         # the backward ran with the switch off
        f.r.setAbsGradients(True)
        refused(call(), NO_BACKWARD)                                         # turned on after the backward
    f.switch = True
    f.backward()
    f.r.draw(f.sc)
    for call in (pairs, stats):
        refused(call(), "no gs_backward* on this frame")                     # a new frame since the backward
    assert f.r.visibleCount() > 0
    refused(pairs(), "no gs_backward* on this frame")                        # the scan alone ran no blend
    f.backward()
    for k in ("i", "c", "o"):
        refused(pairs(**{k: None}), "gs_abs_screen_gradient_device: null")
    for k in ("i", "c", "a"):
        refused(stats(**{k: None}), "gs_densify_stats_abs_device: null")
    refused(stats(nn=n - 1), "n differs from the scene's")
    refused(stats(nn=n + 1), "n differs from the scene's")
    assert pairs(ctx=None) == _lib.GS_ERR_INVALID and stats(ctx=None) == _lib.GS_ERR_INVALID
    assert L.gs_set_abs_gradients(hdl, 2) == _lib.GS_ERR_INVALID and "0 or 1" in L.gs_last_error(hdl).decode()
    f.r.setTileRows(0, 2)
    f.r.draw(f.sc)
    for call in (pairs, stats):
        refused(call(), "the context owns a subset of the tile rows")        # a band, gs_set_band_gradients off
    f.r.setTileRows(0, (h + 15) // 16)
    f.r.draw(f.sc)
    f.backward()
    f.r.synchronize()
    assert np.all(down(out, F) == F(-3.25)) and np.all(down(accum, F) == F(7.5))
    assert pairs() == _lib.GS_OK and stats() == _lib.GS_OK                   # the switch is still on: a refusal cost nothing
    f.r.synchronize()
    k = len(f.visible())
    assert down(out, F).reshape(-1, 2)[:k].any() and np.all(down(out, F).reshape(-1, 2)[k:] == F(-3.25))
    f.switch = False
    f.backward()                                                             # a blend with the switch off: the pairs no longer count
    refused(pairs(), NO_BACKWARD)
    f.r.cleanup()


# ---- 6. the trainer -----------------------------------------------------------------------------------------------------------

def striped_cloud():
    """A few large, flat splats facing the camera over a target of one-pixel stripes (the cancellation case at scale), and a
    grid of small ones beside them."""
    w, h = 96, 64
    rec = [gs.makeGaussian((x, y, 3.0), (0.5, 0.5, 1e-3), sh0=(0.0, 0.0, 0.0, 0.6)) for x in (-0.8, 0.8) for y in (-0.5, 0.5)]
    rec += [gs.makeGaussian((-1.5 + 0.2 * i, -1.0 + 0.25 * j, 2.5), (0.01, 0.01, 0.01), sh0=(0.3, -0.2, 0.1, 0.5))
            for i in range(16) for j in range(9)]
    target = np.zeros((h, w, 3), F)
    target[:, ::2] = 1.0
    return np.stack(rec).astype(F), w, h, target


def test_visible_adam_abs_density():
    """VisibleAdam(track_density=True, abs_density=True) on striped_cloud: after three steps grad_accum_abs >= grad_accum
    elementwise and seen counts the steps; with thresholds between the large splats' signed and absolute means,
    densify(abs_threshold=...) splits large splats that densify() without it leaves alone; step_batch counts views."""
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    aos, w, h, target = striped_cloud()
    sc = make_scene(aos, w, h)
    cam = gs.Renderer._camera_args(sc.getCamera())
    tgt = torch.tensor(target, device=DEV)
    results = {}
    for abs_threshold in (None, "abs"):
        r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
        opt = VisibleAdam(torch.tensor(aos, device=DEV), renderer=r, track_density=True, abs_density=True, lr=[0.0] * 6)
        for _ in range(3):
            opt.step(*cam, tgt, LAMBDA)
        opt.stream.synchronize()
        accum, ab, seen = opt.grad_accum.cpu().numpy(), opt.grad_accum_abs.cpu().numpy(), opt.seen.cpu().numpy()
        assert np.all(ab >= accum) and seen.max() == 3 and np.all(seen[:4] == 3)
        mean, mean_abs = accum[:4] / 3, ab[:4] / 3
        assert np.all(mean_abs > 4 * mean), (mean, mean_abs)
        # the signed means of the large splats lie below grad_threshold, their absolute means above abs_threshold
        params = dict(grad_threshold=float(2 * mean.max()), split_scale=0.1, prune_opacity=0.0)
        if abs_threshold is None:
            opt.abs_density = False                                          # today's rule on the same statistics
            results["signed"] = opt.densify(**params)
        else:
            results["abs"] = opt.densify(abs_threshold=float(0.5 * mean_abs.min()), **params)
            assert opt.grad_accum_abs.shape == (results["abs"][0],) and not opt.grad_accum_abs.any()
            batch = opt.step_batch([cam[:3], cam[:3]], [tgt, tgt])
            opt.stream.synchronize()
            assert np.all(np.isfinite(batch.cpu().numpy())) and int(opt.seen.max()) == 2
            assert np.all(opt.grad_accum_abs.cpu().numpy() >= opt.grad_accum.cpu().numpy())
        r.setStream(None)
        r.cleanup()
    print(f"densify: signed {results['signed']}, absolute {results['abs']}")
    assert results["signed"][2] == 0 and results["abs"][2] == 4              # split: none by the signed rule, the four large ones
    assert results["abs"][1] == results["signed"][1]                         # the small ones clone by the signed mean either way


def test_abs_density_off_is_todays_trainer():
    """abs_density=False (the default): three steps leave records, m, v and the statistics bit for bit as a trainer built
    before the option existed would -- the same calls in the same order; no grad_accum_abs, and the switch stays off."""
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    aos, w, h, target = striped_cloud()
    sc = make_scene(aos, w, h)
    cam = gs.Renderer._camera_args(sc.getCamera())
    tgt = torch.tensor(target, device=DEV)
    states = []
    for abs_density in (False, True):
        r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
        opt = VisibleAdam(torch.tensor(aos, device=DEV), renderer=r, track_density=True, abs_density=abs_density)
        for _ in range(3):
            opt.step(*cam, tgt, LAMBDA)
        opt.stream.synchronize()
        states.append([t.cpu().numpy() for t in (opt.records, opt.m, opt.v, opt.grad_accum, opt.seen, opt.max_radius, opt.rows,
                                                   opt.ids, opt.count)])
        if not abs_density:
            assert opt.grad_accum_abs is None
            out = torch.zeros(len(aos), 2, device=DEV)
            rc = _lib.lib().gs_abs_screen_gradient_device(r._ctx.handle, C.c_void_p(opt.ids.data_ptr()),
                                                          C.c_void_p(opt.count.data_ptr()), len(aos), C.c_void_p(out.data_ptr()))
            assert rc == _lib.GS_ERR_INVALID and NO_BACKWARD in _lib.lib().gs_last_error(r._ctx.handle).decode()
        r.setStream(None)
        r.cleanup()
    for a, b in zip(*states):
        assert np.array_equal(bits(a), bits(b))
    with pytest.raises(ValueError):
        VisibleAdam(torch.tensor(aos, device=DEV), renderer=None, abs_density=True)
