"""k_project stores the raster records of the chunks with an emitting splat only (a quarter wave of 16 records; a wave in the
GS_PROJECT_RECORD_CHUNK=64 build), and gs_debug_read recomputes the rest on demand.  The scenes of test_project_records_cpu.py
put whole waves and quarter waves into one class each; here the frame and every read-back of them equal the oracle's, a second
frame on the same context (the classes swapped, stored chunks gone stale) equals a fresh context's, and a band context reads
back what it always did."""
import numpy as np
import pytest
import torch

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import assert_frame_equals_oracle, make_renderer, make_scene, oracle_run
from test_densify_gpu import Frame, zeros
from test_project_records_cpu import CAMERA_1, CAMERA_2, CULLED, EMITS, FRAMES, MARGIN, N, WAVE, oracle_classes, scene

pytestmark = pytest.mark.gpu

DEG1, DEG2 = _lib.GS_SH_DEGREE_1, _lib.GS_SH_DEGREE_2
SH_RGB = np.array([12 + 4 * k + c for k in range(16) for c in range(3)])      # record floats of shCoeffs[k].rgb, k-major
READ_BACKS = (gs.BUF_COV, gs.BUF_COLOR, gs.BUF_RASTER_OPACITY)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_read_backs_equal_oracle(r, ref, aos, cls, antialias=False):
    """GS_BUF_COV and GS_BUF_COLOR: the oracle's arrays, whole -- every splat that passes the culls, zeros elsewhere.
    GS_BUF_RASTER_OPACITY: the opacity of the emitting splats (none of these has a zero determinant), zeros elsewhere."""
    cov, color = r.debugRead(gs.BUF_COV), r.debugRead(gs.BUF_COLOR)
    assert np.array_equal(bits(cov), bits(ref["stage1"]["cov"]))
    assert np.array_equal(bits(color), bits(ref["stage1"]["color"]))
    kept = cls != CULLED
    assert np.all(cov[kept, 0] != 0) and not cov[~kept].any() and not color[~kept].any() and np.all(color[kept, 3] == aos[kept, 15])
    opacity = r.debugRead(gs.BUF_RASTER_OPACITY)
    assert not opacity[cls != EMITS].any()
    if antialias:
        assert np.all((opacity[cls == EMITS] > 0) & (opacity[cls == EMITS] < aos[cls == EMITS, 15]))
    else:
        assert np.array_equal(bits(opacity[cls == EMITS]), bits(aos[cls == EMITS, 15]))


@pytest.mark.parametrize("sh_mode", [0, 1, 2])
@pytest.mark.parametrize("w,h", FRAMES)
def test_frame_and_read_backs_equal_the_oracle(oracle_mod, w, h, sh_mode):
    aos, _ = scene(w, h)
    for cam in (CAMERA_1, CAMERA_2):
        cls, _ = oracle_classes(oracle_mod, aos, w, h, cam)
        assert min(np.count_nonzero(cls == k) for k in (CULLED, MARGIN, EMITS)) > 60
        sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
        r = make_renderer(sc, w, h)
        img = r.draw(sc)
        _, ref = oracle_run(oracle_mod, sc, w, h)
        assert np.array_equal(np.unique(ref["id"][:ref["e"]]), np.nonzero(cls == EMITS)[0])
        assert_frame_equals_oracle(r, img, ref)
        assert img[..., :3].any()
        assert_read_backs_equal_oracle(r, ref, aos, cls)
        r.cleanup()


@pytest.mark.parametrize("sh_mode,K", [(DEG1, 4), (DEG2, 9)], ids=["degree1", "degree2"])
def test_read_backs_in_the_degree_modes(oracle_mod, sh_mode, K):
    """The colour of a degree mode is mode 0's on records whose coefficients K..15 are zero (test_sh_degree_gpu.py)."""
    w, h = FRAMES[0]
    aos, cls = scene(w, h)
    cut = np.array(aos, copy=True)
    cut[:, SH_RGB[3 * K:]] = 0.0
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **CAMERA_1)
    r = make_renderer(sc, w, h)
    img = r.draw(sc)
    _, ref = oracle_run(oracle_mod, make_scene(cut, w, h, sh_mode=0, **CAMERA_1), w, h)
    assert np.array_equal(img, ref["image"])
    assert_read_backs_equal_oracle(r, ref, aos, cls)
    assert not np.array_equal(ref["stage1"]["color"], oracle_run(oracle_mod, make_scene(aos, w, h, **CAMERA_1), w, h)[1]["stage1"]["color"])
    r.cleanup()


@pytest.mark.parametrize("depth,antialias", [(True, False), (False, True), (True, True)], ids=["depth", "antialias", "both"])
def test_read_backs_with_the_depth_output_and_antialiasing(oracle_mod, depth, antialias):
    """The other instantiations of k_project.  An anti-aliased frame changes the raster opacity alone: lists, covariance and
    colour stay the oracle's."""
    w, h = FRAMES[0]
    aos, cls = scene(w, h)
    sc = make_scene(aos, w, h, **CAMERA_1)
    r = make_renderer(sc, w, h)
    r.setOutputs(rgba32f=depth, depth=depth)
    r.setAntialias(antialias)
    img = r.draw(sc)
    _, ref = oracle_run(oracle_mod, sc, w, h)
    e = ref["e"]
    assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), ref["id"][:e]) and np.array_equal(r.debugRead(gs.BUF_SORTED_TILE), ref["tile"][:e])
    assert np.array_equal(r.debugRead(gs.BUF_RANGES), ref["ranges"])
    if not antialias:
        assert np.array_equal(img, ref["image"])
    assert_read_backs_equal_oracle(r, ref, aos, cls, antialias=antialias)
    r.cleanup()


def _everything(f, sc):
    """A frame of sc on f's context with its backward and densification statistics: what must not depend on the frame before."""
    f.sc = sc
    img = f.r.draw(sc).copy()
    out = {"image": img, "sorted_id": f.r.debugRead(gs.BUF_SORTED_ID), "ranges": f.r.debugRead(gs.BUF_RANGES)}
    for b in READ_BACKS:
        out[f"read_back_{b}"] = bits(f.r.debugRead(b))
    f.ids.fill_(-1); f.rows.zero_(); f.count.zero_()
    torch.cuda.synchronize()
    f.backward()
    accum, seen, radius = f.stats(zeros(f.n))
    k = len(f.visible())
    out.update(count=np.array(k), ids=f.ids.cpu().numpy()[:k], rows=bits(f.rows.cpu().numpy()[:k]), grad_accum=bits(accum), seen=seen,
               max_radius=bits(radius), dense=bits(f.r.backward(f.wr, f.wd)))
    return out


@pytest.mark.parametrize("first,second", [(CAMERA_1, CAMERA_2), (CAMERA_2, CAMERA_1)], ids=["1_then_2", "2_then_1"])
@pytest.mark.parametrize("w,h", FRAMES)
def test_second_frame_on_a_context_equals_a_fresh_context(oracle_mod, w, h, first, second):
    """The camera turns between two frames of one context: the emitting and the margin class swap, so chunks stored in the first
    frame are not stored in the second and hold the first frame's records.  Image, lists, every read-back, gs_backward (dense and
    visible) and gs_densify_stats_device of the second frame equal, bit for bit, those of a context that drew it alone."""
    aos, _ = scene(w, h)
    a, _ = oracle_classes(oracle_mod, aos, w, h, first)
    b, _ = oracle_classes(oracle_mod, aos, w, h, second)
    assert np.all(b[a == EMITS] == MARGIN) and np.all(b[a == MARGIN] == EMITS)
    sc1, sc2 = make_scene(aos, w, h, **first), make_scene(aos, w, h, **second)
    used = Frame(aos, w, h, sc=sc1)
    before = _everything(used, sc1)
    got = _everything(used, sc2)
    fresh = Frame(aos, w, h, sc=sc2)
    want = _everything(fresh, sc2)
    assert want["image"][..., :3].any() and want["count"] == np.count_nonzero(b == EMITS) and not np.array_equal(before["image"], want["image"])
    assert np.array_equal(want["seen"] != 0, b == EMITS) and np.all(want["max_radius"].view(np.float32)[b == EMITS] >= 2)
    for key in want:
        assert np.array_equal(got[key], want[key]), key
    # and back again: the first frame once more, on the context that has drawn both
    again = _everything(used, sc1)
    for key in before:
        assert np.array_equal(again[key], before[key]), key
    used.r.cleanup()
    fresh.r.cleanup()


@pytest.mark.parametrize("rows", [(0, 1), (1, 3)])
def test_band_context_reads_back_what_it_stored(oracle_mod, rows):
    """A context that owns a tile-row band stores whole waves, those with a splat that emits into the band, and reads back what it
    stored: covariance and colour of every splat that emits into the band as the oracle has them; zeros for every wave without
    such a splat and for the colour of every other splat; the covariance of another splat of a stored wave is the oracle's, or zero
    where the band's radius bound skipped the splat."""
    w, h = FRAMES[0]
    aos, _ = scene(w, h)
    for cam in (CAMERA_1, CAMERA_2):
        sc = make_scene(aos, w, h, **cam)
        r = make_renderer(sc, w, h)
        r.setTileRows(*rows)
        r.draw(sc)
        _, ref = oracle_run(oracle_mod, sc, w, h, row_begin=rows[0], row_end=rows[1])
        emits = np.zeros(N, bool)
        emits[ref["id"][:ref["e"]]] = True
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), ref["id"][:ref["e"]])
        stored = np.repeat(np.add.reduceat(emits, np.arange(0, N, WAVE)) > 0, WAVE)[:N]
        cov, color, opacity = (r.debugRead(b) for b in READ_BACKS)
        want_cov, want_color = ref["stage1"]["cov"], ref["stage1"]["color"]
        assert np.array_equal(bits(cov[emits]), bits(want_cov[emits])) and np.array_equal(bits(color[emits]), bits(want_color[emits]))
        assert np.array_equal(bits(opacity[emits]), bits(aos[emits, 15]))
        assert not cov[~stored].any() and not color[~emits].any() and not opacity[~emits].any()
        other = stored & ~emits
        assert np.all((bits(cov[other]) == bits(want_cov[other])).all(axis=1) | (cov[other] == 0).all(axis=1))
        r.cleanup()
