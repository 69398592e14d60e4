"""The visible-splat form of the backward pass on the MI355X (include/gsplat.h, gs_visible_count / gs_backward_visible /
gs_backward_visible_device): V = the splats with tiles_touched != 0, ascending, and one 84-float row for each.  Every
value check is bit equality (on .view(np.uint32)) with gs_backward, which tests/test_backward_gpu.py and
tests/test_backward_fullsize_gpu.py hold to the float64 reference; V itself is checked against the oracle's stage 1 and
the frame's own sorted list.  No tolerance anywhere."""
import ctypes as C
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, camera_params, oracle_params
from test_backward_cpu import list_offsets, padded_cloud, small_scene, truncated_scene
from frame64 import weights

pytestmark = pytest.mark.gpu

SMALL_VISIBLE = 187          # small_scene under its own camera, by the oracle
SENTINEL_ID = np.uint32(0xDEADBEEF)
SENTINEL_ROW = np.float32(-12345.5)
GUARD = 8


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def oracle_visible(oracle_mod, params, aos):
    """flatnonzero(tiles touched != 0) of the oracle's stage 1 (the tile boxes of list_offsets)."""
    s1 = oracle_mod.init_sort_list(params, aos, threads=oracle_mod.host_threads())
    touched, _ = list_offsets(dict(stage1=s1))
    return np.flatnonzero(touched != 0).astype(np.uint32), s1


def drawn(aos, w, h, sh_mode=0, **kw):
    sc = make_scene(aos, w, h, sh_mode=sh_mode)
    r = make_renderer(sc, w, h, **kw)
    r.draw(sc)
    return r, sc


@functools.lru_cache(maxsize=None)
def small_answer(sh_mode=0, with_depth=True):
    """small_scene: (ids, rows, dense) of one context -- computed once, never modified by the tests that share it."""
    aos, w, h = small_scene()
    r, _ = drawn(aos, w, h, sh_mode)
    wr, wd = weights(h, w, 3)
    ids, rows, count = r.backwardVisible(wr, wd if with_depth else None)
    dense = r.backward(wr, wd if with_depth else None)
    r.cleanup()
    assert count == len(ids)
    for a in (ids, rows, dense):
        a.setflags(write=False)
    return ids, rows, dense


def assert_equals_dense(ids, rows, count, dense, what=""):
    assert count == len(ids) == len(rows), what
    assert np.all(np.diff(ids.astype(np.int64)) > 0), what
    differ = np.flatnonzero((bits(dense[ids]) != bits(rows)).any(1))
    assert differ.size == 0, (what, len(differ), ids[differ[:10]].tolist())
    off = np.ones(len(dense), bool)
    off[ids] = False
    assert not bits(dense[off]).any(), what


# ---- 1. equals dense ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "nodepth"])
@pytest.mark.parametrize("sh_mode", [0, 1, 2])
def test_equals_dense_small(oracle_mod, sh_mode, with_depth):
    """small_scene (300 splats, 64 x 48; 187 visible): ids strictly ascending, equal to the frame's own sorted ids and to
    the oracle's splats with a non-empty tile box; count == len(ids) == visibleCount(); rows == dense[ids] bit for bit
    and dense is zero elsewhere."""
    aos, w, h = small_scene()
    r, sc = drawn(aos, w, h, sh_mode)
    assert r.lastStatus == _lib.GS_OK
    wr, wd = weights(h, w, 3)
    d = wd if with_depth else None
    assert r.visibleCount() == SMALL_VISIBLE
    ids, rows, count = r.backwardVisible(wr, d)
    assert r.lastStatus == _lib.GS_OK and r.visibleCount() == count == SMALL_VISIBLE
    assert ids.dtype == np.uint32 and rows.shape == (count, 84)
    assert np.array_equal(ids, np.unique(r.debugRead(gs.BUF_SORTED_ID)))
    want, _ = oracle_visible(oracle_mod, camera_params(oracle_mod, sc, w, h), aos)
    assert np.array_equal(ids, want)
    dense = r.backward(wr, d)
    r.cleanup()
    assert np.any(rows != 0)
    assert_equals_dense(ids, rows, count, dense)
    base = small_answer(sh_mode, with_depth)
    assert np.array_equal(ids, base[0]) and np.array_equal(bits(rows), bits(base[1]))


def test_equals_dense_ragged(oracle_mod):
    """SCENES['ragged'] (6000 splats; 3368 visible): the same checks across 24 blocks."""
    aos, w, h = SCENES["ragged"]()
    r, sc = drawn(aos, w, h)
    wr, wd = weights(h, w, 1)
    ids, rows, count = r.backwardVisible(wr, wd)
    assert count == r.visibleCount() == 3368
    assert np.array_equal(ids, np.unique(r.debugRead(gs.BUF_SORTED_ID)))
    want, _ = oracle_visible(oracle_mod, camera_params(oracle_mod, sc, w, h), aos)
    assert np.array_equal(ids, want)
    dense = r.backward(wr, wd)
    r.cleanup()
    assert_equals_dense(ids, rows, count, dense)


# ---- 2. every sorter ------------------------------------------------------------------------------------------------------

def test_every_sorter_gives_the_same_bits():
    aos, w, h = small_scene()
    wr, wd = weights(h, w, 3)
    ids0, rows0, _ = small_answer()
    for sort in ALL_SORTS:
        r, _ = drawn(aos, w, h, sort=sort)
        ids, rows, count = r.backwardVisible(wr, wd)
        r.cleanup()
        assert count == SMALL_VISIBLE, sort
        assert np.array_equal(ids, ids0) and np.array_equal(bits(rows), bits(rows0)), sort


# ---- 3. truncated list ----------------------------------------------------------------------------------------------------

def test_truncated_list(oracle_mod):
    """truncated_scene: the list overflows (GS_WARN_OVERFLOW); all 2500 splats have a tile box, 103 of them wholly past the
    capacity: they are in V (a proper superset of the sorted list's ids) with rows of exact zeros, and rows ==
    dense[ids] bit for bit."""
    aos, w, h = truncated_scene()
    r, sc = drawn(aos, w, h)
    assert r.lastStatus == _lib.GS_WARN_OVERFLOW
    want, s1 = oracle_visible(oracle_mod, camera_params(oracle_mod, sc, w, h), aos)
    touched, off = list_offsets(dict(stage1=s1))
    past = np.flatnonzero((off >= s1["capacity"]) & (touched > 0))
    assert len(want) == 2500 and len(past) == 103
    wr, wd = weights(h, w, 6)
    ids, rows, count = r.backwardVisible(wr, wd)
    assert r.lastStatus == _lib.GS_OK
    listed = np.unique(r.debugRead(gs.BUF_SORTED_ID))
    dense = r.backward(wr, wd)
    r.cleanup()
    assert count == 2500 and np.array_equal(ids, want)
    assert len(listed) < len(ids) and np.all(np.isin(listed, ids))
    assert not np.any(np.isin(past, listed))
    assert not bits(rows[np.searchsorted(ids, past)]).any()
    assert np.any(rows != 0)
    assert_equals_dense(ids, rows, count, dense)


# ---- 4. block and scan-thread edges ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("filler", ["behind", "outside"])
@pytest.mark.parametrize("n", [511, 512, 513, 262_145])
def test_padded_cloud(oracle_mod, filler, n):
    """small_scene scattered, order preserved, over n records whose others emit nothing, with live records at 0, n - 1 and
    on both sides of the 256-splat block boundaries (n = 262 145: of the two-block spans of k_splat_scan_blocks<BwdSource<true>>'
    threads): ids = the positions of the base cloud's visible splats, rows bit-equal to the unpadded scene's."""
    aos, w, h = small_scene()
    ids0, rows0, _ = small_answer()
    cloud, pos = padded_cloud(aos, n, seed=n, filler=filler)
    want, _ = oracle_visible(oracle_mod, oracle_params(oracle_mod, w, h), cloud)
    assert len(want) == SMALL_VISIBLE and np.array_equal(want, pos[ids0])
    r, _ = drawn(cloud, w, h)
    wr, wd = weights(h, w, 3)
    ids, rows, count = r.backwardVisible(wr, wd)
    r.cleanup()
    assert count == SMALL_VISIBLE
    assert np.array_equal(ids, pos[ids0].astype(np.uint32))
    differ = np.flatnonzero((bits(rows) != bits(rows0)).any(1))
    assert differ.size == 0, (len(differ), ids[differ[:10]].tolist())


@pytest.mark.parametrize("name", ["A", "B"])
def test_dense_flags_across_many_blocks(oracle_mod, name):
    """Config A (100 000 splats, 391 blocks, 52 123 visible by the oracle) and config B (559 263 splats, 2185 blocks: three
    per thread of the block scan, so a flag scan without the running carry shows here): rows == dense[ids] bit for bit,
    ids == the frame's sorted ids (no overflow)."""
    aos, cfg = synth.generate_config(name)
    w, h = cfg["width"], cfg["height"]
    blocks = (len(aos) + 255) // 256
    assert (blocks + 1023) // 1024 == {"A": 1, "B": 3}[name]
    r, sc = drawn(aos, w, h)
    assert r.lastStatus == _lib.GS_OK
    wr, wd = weights(h, w, 9)
    ids, rows, count = r.backwardVisible(wr, wd)
    assert count == r.visibleCount()
    assert np.array_equal(ids, np.unique(r.debugRead(gs.BUF_SORTED_ID)))
    dense = r.backward(wr, wd)
    r.cleanup()
    if name == "A":
        want, _ = oracle_visible(oracle_mod, camera_params(oracle_mod, sc, w, h), aos)
        assert len(want) == 52_123 and np.array_equal(ids, want)
    assert_equals_dense(ids, rows, count, dense, name)


# ---- 5. max_rows ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_rows", [0, 1, 186, 187, 188, 300])
def test_max_rows(max_rows):
    """Output arrays pre-filled with a sentinel, 8 guard rows behind them: GS_WARN_OVERFLOW iff max_rows < 187, count_out
    == 187 always, the first min(max_rows, 187) ids and rows are the head of the full answer, everything after them
    still holds the sentinel.  max_rows == 0 with NULL outputs asks for the count alone: GS_OK and the count."""
    aos, w, h = small_scene()
    ids0, rows0, _ = small_answer()
    r, _ = drawn(aos, w, h)
    wr, wd = weights(h, w, 3)
    L = _lib.lib()
    ids = np.full(max_rows + GUARD, SENTINEL_ID, np.uint32)
    rows = np.full((max_rows + GUARD, 84), SENTINEL_ROW, np.float32)
    count = C.c_uint32(77)
    rc = L.gs_backward_visible(r._ctx.handle, p(wr), p(wd), p(ids), p(rows), max_rows, C.byref(count))
    assert rc == (_lib.GS_WARN_OVERFLOW if max_rows < SMALL_VISIBLE else _lib.GS_OK)
    assert count.value == SMALL_VISIBLE
    k = min(max_rows, SMALL_VISIBLE)
    assert np.array_equal(ids[:k], ids0[:k]) and np.array_equal(bits(rows[:k]), bits(rows0[:k]))
    assert np.all(ids[k:] == SENTINEL_ID) and np.all(rows[k:] == SENTINEL_ROW)
    if max_rows == 0:
        count = C.c_uint32(77)
        assert L.gs_backward_visible(r._ctx.handle, p(wr), p(wd), None, None, 0, C.byref(count)) == _lib.GS_OK   # a count query
        assert count.value == SMALL_VISIBLE
        i, v, c = r.backwardVisible(wr, wd, max_rows=0)
        assert len(i) == 0 and v.shape == (0, 84) and c == SMALL_VISIBLE
    r.cleanup()


# ---- 6. device entry point ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_rows", [187, 100, 0])
def test_device_entry_point(max_rows):
    """torch tensors for all six pointers: after synchronize() the bits of the host call and count 187; with max_rows =
    100 the call still returns GS_OK, the count is 187, 100 are written and the rest hold the sentinel; max_rows = 0 with
    NULL outputs gives the count alone."""
    torch = pytest.importorskip("torch")
    aos, w, h = small_scene()
    ids0, rows0, _ = small_answer()
    r, _ = drawn(aos, w, h)
    wr, wd = weights(h, w, 3)
    gr, gd = torch.tensor(wr, device="cuda"), torch.tensor(wd, device="cuda")
    size = SMALL_VISIBLE + GUARD
    ids = torch.full((size,), -7, dtype=torch.int32, device="cuda")
    rows = torch.full((size, 84), float(SENTINEL_ROW), device="cuda")
    count = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = _lib.lib().gs_backward_visible_device(r._ctx.handle, C.c_void_p(gr.data_ptr()), C.c_void_p(gd.data_ptr()),
                                               C.c_void_p(ids.data_ptr()) if max_rows else None,
                                               C.c_void_p(rows.data_ptr()) if max_rows else None, max_rows,
                                               C.c_void_p(count.data_ptr()))
    assert rc == _lib.GS_OK
    r.synchronize()
    assert int(count.item()) == SMALL_VISIBLE
    got_ids, got_rows = ids.cpu().numpy(), rows.cpu().numpy()
    k = min(max_rows, SMALL_VISIBLE)
    assert np.array_equal(got_ids[:k].view(np.uint32), ids0[:k]) and np.array_equal(bits(got_rows[:k]), bits(rows0[:k]))
    assert np.all(got_ids[k:] == -7) and np.all(got_rows[k:] == SENTINEL_ROW)
    # the binding's form
    if max_rows:
        ids.fill_(-7); rows.fill_(float(SENTINEL_ROW)); count.fill_(-1)
        torch.cuda.synchronize()
        r.backwardVisibleDevice(gr.data_ptr(), gd.data_ptr(), ids.data_ptr(), rows.data_ptr(), max_rows, count.data_ptr())
        r.synchronize()
        assert int(count.item()) == SMALL_VISIBLE
        assert np.array_equal(ids.cpu().numpy()[:k].view(np.uint32), ids0[:k])
        assert np.array_equal(bits(rows.cpu().numpy()[:k]), bits(rows0[:k]))
    r.cleanup()


# ---- 7. nothing visible ---------------------------------------------------------------------------------------------------

def test_nothing_visible_then_an_ordinary_frame():
    """A cloud wholly behind the camera: GS_OK, count 0, outputs untouched (host and device form).  Then small_scene on the
    same context (an in-place upload of as many records): test 1's answer -- the scratch carries nothing over."""
    torch = pytest.importorskip("torch")
    aos, w, h = small_scene()
    ids0, rows0, _ = small_answer()
    # padded_cloud's 'behind' filler record, and nothing else
    cloud = np.tile(gs.makeGaussian((0.1, -0.2, -5.0), (0.05, 0.04, 0.03), sh0=(0.3, 0.2, 0.1, 0.7)).astype(np.float32),
                    (len(aos), 1))
    r, sc = drawn(cloud, w, h)
    assert r.timings().num_sort_elements == 0
    wr, wd = weights(h, w, 3)
    L = _lib.lib()
    ids = np.full(GUARD, SENTINEL_ID, np.uint32)
    rows = np.full((GUARD, 84), SENTINEL_ROW, np.float32)
    count = C.c_uint32(77)
    assert L.gs_backward_visible(r._ctx.handle, p(wr), p(wd), p(ids), p(rows), GUARD, C.byref(count)) == _lib.GS_OK
    assert count.value == 0 and r.visibleCount() == 0
    assert np.all(ids == SENTINEL_ID) and np.all(rows == SENTINEL_ROW)
    gr, gd = torch.tensor(wr, device="cuda"), torch.tensor(wd, device="cuda")
    dids = torch.full((GUARD,), -7, dtype=torch.int32, device="cuda")
    drows = torch.full((GUARD, 84), float(SENTINEL_ROW), device="cuda")
    dcount = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    r.backwardVisibleDevice(gr.data_ptr(), gd.data_ptr(), dids.data_ptr(), drows.data_ptr(), GUARD, dcount.data_ptr())
    r.synchronize()
    assert int(dcount.item()) == 0 and bool((dids == -7).all()) and bool((drows == float(SENTINEL_ROW)).all())
    i, v, c = r.backwardVisible(wr, wd)
    assert c == 0 and len(i) == 0 and v.shape == (0, 84)
    assert not r.backward(wr, wd).any()
    # the ordinary frame on the same context
    dev = torch.tensor(aos, device="cuda")
    torch.cuda.synchronize()
    r.uploadDevice(dev.data_ptr(), len(aos))
    r.draw(make_scene(aos, w, h))
    ids, rows, count = r.backwardVisible(wr, wd)
    r.cleanup()
    assert count == SMALL_VISIBLE and np.array_equal(ids, ids0) and np.array_equal(bits(rows), bits(rows0))


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------

def test_refusals():
    """GS_ERR_INVALID with a message that names the function, nothing enqueued: no frame yet, after gs_set_resolution, a
    GS_RENDER_FAST context, a gs_set_tile_rows band context, NULL grad_rgba32f, NULL count_out, NULL ids_out with max_rows
    > 0.  A valid call afterwards works."""
    aos, w, h = small_scene()
    ids0, rows0, _ = small_answer()
    sc = make_scene(aos, w, h)
    L = _lib.lib()
    wr, wd = weights(h, w, 3)
    ids = np.zeros(300, np.uint32)
    rows = np.zeros((300, 84), np.float32)
    count = C.c_uint32()
    torch = pytest.importorskip("torch")
    dbuf = torch.zeros(300 * 84 + h * w * 5, device="cuda")
    dp = C.c_void_p(dbuf.data_ptr())

    def refused(r, what):
        cases = {"gs_visible_count": lambda: L.gs_visible_count(r._ctx.handle, C.byref(count)),
                 "gs_backward_visible": lambda: L.gs_backward_visible(r._ctx.handle, p(wr), p(wd), p(ids), p(rows), 300,
                                                                      C.byref(count)),
                 "gs_backward_visible_device": lambda: L.gs_backward_visible_device(r._ctx.handle, dp, None, dp, dp, 300, dp)}
        for name, call in cases.items():
            assert call() == _lib.GS_ERR_INVALID, (what, name)
            assert name.encode() + b":" in L.gs_last_error(r._ctx.handle), (what, name, L.gs_last_error(r._ctx.handle))

    def null_argument(r, call, name, what):
        assert call() == _lib.GS_ERR_INVALID, what
        assert name.encode() + b":" in L.gs_last_error(r._ctx.handle), (what, L.gs_last_error(r._ctx.handle))

    r = make_renderer(sc, w, h)
    refused(r, "no frame yet")
    r.draw(sc)
    hd = r._ctx.handle
    null_argument(r, lambda: L.gs_backward_visible(hd, None, p(wd), p(ids), p(rows), 300, C.byref(count)),
                  "gs_backward_visible", "NULL grad_rgba32f")
    null_argument(r, lambda: L.gs_backward_visible_device(hd, None, None, dp, dp, 300, dp),
                  "gs_backward_visible_device", "NULL grad_rgba32f")
    null_argument(r, lambda: L.gs_backward_visible(hd, p(wr), p(wd), p(ids), p(rows), 300, None),
                  "gs_backward_visible", "NULL count_out")
    null_argument(r, lambda: L.gs_backward_visible_device(hd, dp, None, dp, dp, 300, None),
                  "gs_backward_visible_device", "NULL count_out")
    null_argument(r, lambda: L.gs_visible_count(hd, None), "gs_visible_count", "NULL count_out")
    null_argument(r, lambda: L.gs_backward_visible(hd, p(wr), p(wd), None, p(rows), 300, C.byref(count)),
                  "gs_backward_visible", "NULL ids_out")
    null_argument(r, lambda: L.gs_backward_visible(hd, p(wr), p(wd), p(ids), None, 1, C.byref(count)),
                  "gs_backward_visible", "NULL grad_rows_out")
    null_argument(r, lambda: L.gs_backward_visible_device(hd, dp, None, None, dp, 300, dp),
                  "gs_backward_visible_device", "NULL ids_out")
    with pytest.raises(ValueError):
        r.backwardVisible(wr[:-1], wd)
    assert L.gs_set_resolution(hd, w, h) == _lib.GS_OK
    refused(r, "after gs_set_resolution")
    r.draw(sc)
    r.setTileRows(0, 2)
    r.draw(sc)
    refused(r, "a band of tile rows")
    r.setTileRows(0, r.sceneInfo().tiles_y)
    refused(r, "rows set back, no frame since")
    r.draw(sc)
    got_ids, got_rows, c = r.backwardVisible(wr, wd)
    r.cleanup()
    assert c == SMALL_VISIBLE and np.array_equal(got_ids, ids0) and np.array_equal(bits(got_rows), bits(rows0))
    f = make_renderer(sc, w, h, mode=gs.GS_RENDER_FAST)
    f.draw(sc)
    refused(f, "GS_RENDER_FAST")
    f.cleanup()


# ---- 9. no interference ---------------------------------------------------------------------------------------------------

def test_no_interference():
    """The RGBA8 frame and gs_backward's bits are identical before and after a visible backward on the same context."""
    aos, w, h = SCENES["ragged"]()
    r, sc = drawn(aos, w, h)
    img0 = r.draw(sc)
    wr, wd = weights(h, w, 3)
    before = r.backward(wr, wd)
    ids, rows, count = r.backwardVisible(wr, wd)
    after = r.backward(wr, wd)
    assert np.array_equal(bits(before), bits(after))
    assert np.array_equal(r.draw(sc), img0)
    again = r.backward(wr, wd)
    ids2, rows2, _ = r.backwardVisible(wr, wd)
    r.cleanup()
    assert np.array_equal(bits(before), bits(again))
    assert np.array_equal(ids, ids2) and np.array_equal(bits(rows), bits(rows2))
    assert_equals_dense(ids, rows, count, before)


# ---- 10. torch ------------------------------------------------------------------------------------------------------------

def torch_scene():
    """The 16-splat 96 x 64 scene of test_backward_gpu.test_torch_autograd."""
    w, h = 96, 64
    rng = np.random.default_rng(7)
    recs = []
    for k in range(16):
        x, y = (k % 4 - 1.5) * 0.35, (k // 4 - 1.5) * 0.3
        recs.append(gs.makeGaussian((x, y, 2.0), (0.12, 0.12, 0.12), sh0=tuple(rng.uniform(-1.2, 1.2, 3)) + (0.8,)))
    return np.stack(recs).astype(np.float32), w, h, rng


def camera_of(aos, w, h, **kw):
    cam = make_scene(aos, w, h, **kw).getCamera()
    return cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition()


def test_torch_sparse_grad_equals_dense():
    """sparse_grad=True: rec.grad is sparse and to_dense() has the bits of the dense path's rec.grad; two views
    accumulated into one leaf give the sum of the two dense gradients bit for bit (two operands: order-free)."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    aos, w, h, _ = torch_scene()
    cams = [camera_of(aos, w, h), camera_of(aos, w, h, pos=(0.1, -0.05, -0.2), yaw=0.05, pitch=-0.03)]
    wts = [weights(h, w, 4), weights(h, w, 5)]
    rr = autograd.make_renderer(w, h)

    def grad_of(views, sparse):
        rec = torch.tensor(aos, device="cuda", requires_grad=True)
        loss = 0
        for k in views:
            rgba, dep = autograd.render(rec, *cams[k], 0, depth=True, renderer=rr, sparse_grad=sparse)
            loss = loss + (rgba * torch.tensor(wts[k][0], device="cuda")).sum() + \
                (dep * torch.tensor(wts[k][1], device="cuda")).sum()
        loss.backward()
        return rec.grad

    dense = [grad_of([k], False) for k in range(2)]
    for k in range(2):
        g = grad_of([k], True)
        assert g.is_sparse and not dense[k].is_sparse and tuple(g.shape) == (16, 84)
        assert np.any(dense[k].cpu().numpy() != 0)
        assert np.array_equal(bits(g.to_dense().cpu().numpy()), bits(dense[k].cpu().numpy())), k
    both = grad_of([0, 1], True)
    rr.cleanup()
    assert both.is_sparse
    assert np.array_equal(bits(both.to_dense().cpu().numpy()), bits((dense[0] + dense[1]).cpu().numpy()))


def test_torch_sparse_adam_moves_the_listed_rows_alone():
    """A torch.optim.SparseAdam step on the sparse gradient changes exactly the rows in ids: on the 16-splat scene (all
    listed) and on the same scene with 8 records behind the camera mixed in (never listed, never moved)."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    aos, w, h, _ = torch_scene()
    padded, pos = padded_cloud(aos, 24, seed=3, filler="behind")
    view, proj, cpos = camera_of(aos, w, h)
    rr = autograd.make_renderer(w, h)
    for cloud, live in ((aos, np.arange(16)), (padded, pos)):
        rec = torch.tensor(cloud, device="cuda", requires_grad=True)
        opt = torch.optim.SparseAdam([rec], lr=0.01)
        out = autograd.render(rec, view, proj, cpos, 0, renderer=rr, sparse_grad=True)
        (out * torch.tensor(weights(h, w, 4)[0], device="cuda")).sum().backward()
        ids = rec.grad.coalesce().indices()[0].cpu().numpy()
        assert np.array_equal(ids, live)
        assert bool((rec.grad.to_dense()[ids] != 0).any(1).all())
        opt.step()
        moved = np.flatnonzero((bits(rec.detach().cpu().numpy()) != bits(cloud)).any(1))
        assert np.array_equal(moved, ids), (moved, ids)
    rr.cleanup()


def test_torch_optimisation_loop_with_sparse_grad():
    """The loop of test_torch_autograd (colours and xy as separate leaves feeding torch.cat, torch.optim.Adam: the leaves
    receive dense gradients through cat) with sparse_grad=True: 150 steps still bring the loss down 10x."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    target_aos, w, h, rng = torch_scene()
    view, proj, pos = camera_of(target_aos, w, h)
    rr = autograd.make_renderer(w, h)
    target = torch.tensor(target_aos, device="cuda")
    with torch.no_grad():
        tgt_rgba = autograd.render(target, view, proj, pos, 0, renderer=rr)
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
        out = autograd.render(recs_t, view, proj, pos, 0, renderer=rr, sparse_grad=True)
        loss = ((out - tgt_rgba) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    rr.cleanup()
    assert losses[-1] < losses[0] / 10, (losses[0], losses[-1])
