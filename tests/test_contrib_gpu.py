"""gs_contrib_device and gs_prune_below_device on the MI355X (include/gsplat.h) against the CPU reference of
tests/test_contrib_cpu.py (tests/host/contrib_ref.c and a NumPy mask), bit for bit: the per-splat largest blend weight, the
fixed-order sum and the pair count on the designed scenes, their accumulation over frames, their independence of sorter,
launch shape, tile order and count mode, the backward's scratch left alone, the stable compaction at the block edges of
the scan, the invariant that ties both calls together (pruning what no view shows leaves the frames byte for byte), the
refusals of both, and autograd.VisibleAdam.prune_by_contribution end to end."""
import ctypes as C
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
from test_outputs_cpu import SCENES, camera_params, load_scene
from test_backward_cpu import batch_edge_scene, check_batch_edges, check_truncated, padded_cloud, small_scene, truncated_scene
from frame64 import weights
from test_train_chain_gpu import LAMBDA, new_renderer
from test_contrib_cpu import bits, contrib_reference, prune_mask, prune_ref, scene_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F = np.float32
DEV = "cuda:0"
# what a splat the frame never blends must keep: no value the call could have computed (weights lie in [0, 1])
SENT_MAX, SENT_SUM, SENT_PIX = F(-3.5), F(-7.25), np.uint32(0xDEADBEEF)
TINY = np.nextafter(F(0), F(1))


def up(a):
    """A host array on the device, bits kept whatever they spell (uint32 / float32 as int32 storage)."""
    a = np.ascontiguousarray(a)
    return torch.tensor(a.view(np.int32) if a.dtype.itemsize == 4 else a, device=DEV)


def down(t, dtype):
    return t.cpu().numpy().view(dtype)


def sentinel_state(n, zero=None):
    """The three arrays of n, sentinels everywhere but zeros on the splats `zero` (a mask)."""
    z = np.zeros(n, bool) if zero is None else zero
    return (np.where(z, F(0), SENT_MAX).astype(F), np.where(z, F(0), SENT_SUM).astype(F),
            np.where(z, np.uint32(0), SENT_PIX).astype(np.uint32))


def contrib(r, n, state, want_sum=True, want_pixels=True):
    """One gs_contrib_device on the last frame of r into device copies of `state` -> (wmax, wsum, pixels) on the host."""
    d = [up(a) for a in state]
    torch.cuda.synchronize()
    r.contribDevice(n, d[0].data_ptr(), d[1].data_ptr() if want_sum else None, d[2].data_ptr() if want_pixels else None)
    r.synchronize()
    return down(d[0], F), down(d[1], F), down(d[2], np.uint32)


def assert_same(got, want, what=""):
    for name, a, b in zip(("wmax", "wsum", "pixels"), got, want):
        assert np.array_equal(bits(a), bits(b)), (what, name, int(np.flatnonzero(bits(a) != bits(b))[0]))


def ref_arrays(c):
    return c["wmax"], c["wsum"], c["pixels"]


# ---- 1. bit for bit against the reference -----------------------------------------------------------------------------------

def designed(oracle_mod, tmp_path, name):
    """(aos, w, h, cam) of a case of test 1 and a check of what it is there for (given the reference)."""
    if name in ("ragged", "dense", "zero_det", "ragged@pose"):
        aos, w, h, cam = load_scene(name)
        return aos, w, h, cam, None
    if name == "truncated":
        aos, w, h = truncated_scene()
        return aos, w, h, {}, lambda c: check_truncated(c["ref"], c["flags"])
    if name == "batch_edges":
        aos, w, h, _ = batch_edge_scene(oracle_mod)
        return aos, w, h, {}, lambda c: check_batch_edges(c["ref"], c["flags"])
    n = int(name.partition("_")[2])                    # padded_<n>: live splats at 0 and n - 1, the rest behind the camera
    aos, w, h = small_scene()
    cloud, _ = padded_cloud(aos[:200], n, seed=n, filler="behind")
    return cloud, w, h, {}, None


@pytest.mark.parametrize("scene", ["ragged", "dense", "zero_det", "ragged@pose", "truncated", "batch_edges", "padded_257",
                                   "padded_513"])
def test_contributions_equal_the_reference(oracle_mod, tmp_path, scene):
    """wmax, wsum and pixels bit for bit, from arrays that hold zeros on the splats the reference touches and sentinels on
    all others: a splat without a pair is neither read nor written.  Per scene: image edges inside tiles (ragged), stops
    that count and entries behind them that do not (dense), det == 0 entries (zero_det), a posed camera, an overflowed
    list (the straddling splat's surviving elements count, splats past the capacity stay untouched), lists of 64 / 65 /
    128 / 129 entries with stops at 63, 64, 65, 127 and 128, a silent tile and an unreached tail (batch_edges), and the
    grid edges of the per-splat kernel (n = 257, 513 with a live last splat)."""
    aos, w, h, cam, check = designed(oracle_mod, tmp_path, scene)
    aos = np.ascontiguousarray(aos, F)
    n = len(aos)
    sc = make_scene(aos, w, h, **cam)
    r = make_renderer(sc, w, h)
    r.draw(sc)
    if scene in ("ragged", "dense", "zero_det", "ragged@pose"):
        c = scene_reference(oracle_mod, tmp_path, scene)[5]
    else:
        c = contrib_reference(tmp_path, camera_params(oracle_mod, sc, w, h), aos)
    if check is not None:
        check(c)
    assert (r.lastStatus == gs.GS_WARN_OVERFLOW) == (scene == "truncated")
    hit = c["touched"]
    assert 0 < hit.sum() < n and np.all(c["wmax"][hit] > 0) and np.all(c["pixels"][hit] > 0)
    if scene.startswith("padded"):
        assert hit[n - 1] or c["emitting"][n - 1]
    start = sentinel_state(n, zero=hit)
    got = contrib(r, n, start)
    want = tuple(np.where(hit, a, s) for a, s in zip(ref_arrays(c), start))
    assert_same(got, want, scene)
    print(f"{scene}: n {n}, {int(c['emitting'].sum())} emitting, {int(hit.sum())} blended, {int(c['pixels'].sum())} pairs")
    r.cleanup()


# ---- 2. accumulation --------------------------------------------------------------------------------------------------------

MOVED = dict(pos=(0.05, -0.03, -0.1), yaw=0.04, pitch=-0.02)


def test_two_frames_accumulate(oracle_mod, tmp_path):
    """Two frames of the ragged cloud, under the origin camera and a slightly moved one: the arrays equal the reference's
    two-step accumulation bit for bit; without wsum or pixels the other arrays are the same and the missing one is not
    touched; a pixels of 2^32 - 2 saturates at 2^32 - 1."""
    aos, w, h, cam, p0, c0 = scene_reference(oracle_mod, tmp_path, "ragged")
    n = len(aos)
    sc0, sc1 = make_scene(aos, w, h), make_scene(aos, w, h, **MOVED)
    p1 = camera_params(oracle_mod, sc1, w, h)
    c1 = contrib_reference(tmp_path, p1, aos, state=ref_arrays(c0))
    assert (c1["touched"] & ~c0["touched"]).sum() > 0 and (c0["touched"] & ~c1["touched"]).sum() > 0     # the views differ
    both = c0["touched"] & c1["touched"]
    assert np.any(c1["wmax"][both] > c0["wmax"][both]) and np.any(c1["wmax"][both] == c0["wmax"][both])
    r = make_renderer(sc0, w, h)
    forms = {}
    for want_sum, want_pixels in ((True, True), (False, True), (True, False), (False, False)):
        r.draw(sc0)
        first = contrib(r, n, (np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32)), want_sum, want_pixels)
        r.draw(sc1)
        forms[want_sum, want_pixels] = contrib(r, n, first, want_sum, want_pixels)
    assert_same(forms[True, True], ref_arrays(c1), "two frames")
    for (want_sum, want_pixels), got in forms.items():
        assert np.array_equal(bits(got[0]), bits(c1["wmax"]))
        assert np.array_equal(bits(got[1]), bits(c1["wsum"])) if want_sum else not got[1].any()
        assert np.array_equal(got[2], c1["pixels"]) if want_pixels else not got[2].any()
    # saturation: the frame under the moved camera onto counts of 2^32 - 2
    near = (np.zeros(n, F), np.zeros(n, F), np.full(n, 0xFFFFFFFE, np.uint32))
    got = contrib(r, n, near)
    alone = contrib_reference(tmp_path, p1, aos, ref=c1["ref"], state=near)
    assert_same(got, ref_arrays(alone), "saturation")
    pairs = np.zeros(n, np.int64)                              # of this frame alone, per splat
    np.add.at(pairs, np.asarray(c1["ref"]["id"])[:c1["ref"]["e"]], alone["entry_count"])
    assert (pairs >= 2).sum() > 100 and np.array_equal(pairs > 0, c1["touched"])
    assert np.all(got[2][pairs >= 1] == 0xFFFFFFFF) and np.all(got[2][pairs == 0] == 0xFFFFFFFE)
    r.cleanup()


# ---- 3. independence --------------------------------------------------------------------------------------------------------

def test_bits_do_not_depend_on_how_the_frame_was_made(oracle_mod, tmp_path):
    """The same three arrays -- the reference's -- from all five sorters, every render launch shape, both tile orders, every
    count mode, and from call to call on one frame."""
    aos, w, h, cam, p, c = scene_reference(oracle_mod, tmp_path, "ragged")
    n = len(aos)
    sc = make_scene(aos, w, h)
    zeros = (np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32))
    kernels = (gs.GS_RENDER_KERNEL_WAVE_1PX, gs.GS_RENDER_KERNEL_WAVE_2PX, gs.GS_RENDER_KERNEL_WAVE_4PX,
               gs.GS_RENDER_KERNEL_WORKGROUP, gs.GS_RENDER_KERNEL_WORKGROUP_8X8)
    configs = ([dict(sort=s) for s in ALL_SORTS] + [dict(kernel=k) for k in kernels] +
               [dict(order=gs.GS_TILE_ORDER_RASTER)] + [dict(count=k) for k in (gs.GS_COUNT_PER_PASS, gs.GS_COUNT_FED)])
    for cfg in configs:
        r = make_renderer(sc, w, h, **cfg)
        r.draw(sc)
        assert_same(contrib(r, n, zeros), ref_arrays(c), cfg)
        assert_same(contrib(r, n, zeros), ref_arrays(c), ("again", cfg))
        r.cleanup()


# ---- 4. neighbours ----------------------------------------------------------------------------------------------------------

def test_the_backward_is_left_alone(oracle_mod, tmp_path):
    """gs_backward_visible_device, gs_contrib_device, then gs_backward_camera_device and gs_densify_stats_device give the
    bits they give without the contrib call -- also when the first contrib call came before any backward (slot offsets of
    its own) and the second after it (the backward's scan); both contrib calls give the reference."""
    aos, w, h, cam, p, c = scene_reference(oracle_mod, tmp_path, "ragged")
    n = len(aos)
    sc = make_scene(aos, w, h)
    wr, wd = weights(h, w, 5)
    zeros = (np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32))

    def run(with_contrib):
        r = make_renderer(sc, w, h)
        r.draw(sc)
        if with_contrib:
            assert_same(contrib(r, n, zeros), ref_arrays(c), "before any backward")
        g_rgba, g_depth = up(wr), up(wd)
        ids = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        rows = torch.zeros(n, 84, device=DEV)
        count = torch.zeros(1, dtype=torch.int32, device=DEV)
        cam_grad = torch.zeros(_lib.CAMERA_GRAD_FLOATS, device=DEV)
        stats = (torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV), torch.zeros(n, device=DEV))
        torch.cuda.synchronize()
        r.backwardVisibleDevice(g_rgba.data_ptr(), g_depth.data_ptr(), ids.data_ptr(), rows.data_ptr(), n, count.data_ptr())
        if with_contrib:
            assert_same(contrib(r, n, zeros), ref_arrays(c), "between the backward and its readers")
        r.backwardCameraDevice(cam_grad.data_ptr())
        r.densifyStatsDevice(ids.data_ptr(), count.data_ptr(), n, n, *(t.data_ptr() for t in stats))
        r.synchronize()
        out = [down(t, np.uint32).copy() for t in (ids, rows, count, cam_grad, *stats)]
        r.cleanup()
        return out

    plain, mixed = run(False), run(True)
    assert plain[3].any() and plain[4].any() and int(plain[2][0]) > 500
    for a, b in zip(plain, mixed):
        assert np.array_equal(a, b)


# ---- 5. the prune -----------------------------------------------------------------------------------------------------------

GUARD = 3                      # sentinel rows behind max_out
SENT_ROW = F(-12345.5)


@pytest.fixture(scope="module")
def bare():
    """A context without a scene and without a resolution: all gs_prune_below_device needs."""
    r = gs.Renderer(64, 64, record_timings=False)
    r.init(gs.ResourceManager())
    yield r
    r.cleanup()


def prune_inputs(n):
    """Four arrays of n rows of random BITS (NaN payloads, infinities, denormals and -0.0f among them; float 83 of a records
    row carries the row's index) and a score in [0, 1) with NaNs, -0.0f and ties at 0.5."""
    rng = np.random.default_rng(1000 + n)
    arrays = [rng.integers(0, 1 << 32, (n, 84), dtype=np.uint64).astype(np.uint32) for _ in range(4)]
    for a in arrays:
        a[:, 7] = np.array([0x7FC12345, 0xFFC00001, 0x80000000, 0x7F800000], np.uint32)[np.arange(n) % 4]
    arrays[0][:, 83] = np.arange(n)
    score = rng.uniform(0, 1, n).astype(F)
    score[rng.random(n) < 0.1] = F("nan")
    score[rng.random(n) < 0.1] = F(0.5)
    score[rng.random(n) < 0.05] = -F(0.0)
    if n >= 255:
        score[[0, 254, n - 1]] = F(0.75)                      # kept at the edges of the first block and of the cloud
    return [a.view(F) for a in arrays], score


def run_prune(r, score, threshold, arrays, max_out, given=(True, True, True)):
    """gs_prune_below_device on device copies (records and those of raw, m, v that `given` names) -> the outputs
    [max_out + GUARD, 84] (None where not given) and counts [2]."""
    n = len(score)
    use = [True, *given]
    d = [up(a) if u else None for a, u in zip(arrays, use)]
    d_score = up(score)
    outs = [torch.full((max_out + GUARD, 84), float(SENT_ROW), device=DEV) if u else None for u in use]
    counts = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    r.pruneBelowDevice(d_score.data_ptr(), threshold, n, *(ptr(t) for t in d), *(ptr(t) for t in outs), max_out, counts.data_ptr())
    r.synchronize()
    for t, a in zip(d + [d_score], list(arrays) + [score]):
        if t is not None:
            assert np.array_equal(down(t, np.uint32).reshape(-1), bits(a).reshape(-1))      # the inputs are only read
    return [None if o is None else down(o, F) for o in outs], down(counts, np.uint32)


def assert_pruned(got, counts, score, threshold, arrays, max_out, given=(True, True, True)):
    use = [True, *given]
    want_counts, want = prune_ref(score, threshold, [a if u else None for a, u in zip(arrays, use)], max_out)
    assert tuple(int(c) for c in counts) == want_counts
    k = min(want_counts[0], max_out)
    for o, b in zip(got, want):
        assert (o is None) == (b is None)
        if o is not None:
            assert len(b) == k and np.array_equal(bits(o[:k]), bits(b)) and np.all(o[k:] == SENT_ROW)
    return want_counts


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_prune_against_the_mask(bare, n):
    """Order and bits equal the NumPy mask at one splat, one block of 256 part and full, two blocks and four: thresholds that
    keep every finite score, none (count 0, outputs untouched) and about half (ties at the threshold kept, NaN scores
    dropped, rows with NaN payloads and -0.0f copied as they are); max_out below the kept count leaves everything from
    max_out on untouched and the count unclamped; every NULL combination of raw / m / v."""
    arrays, score = prune_inputs(n)
    nans = int(np.isnan(score).sum())
    for threshold in (-np.inf, 0.5, 2.0, np.inf):
        got, counts = run_prune(bare, score, threshold, arrays, n)
        kept, dropped = assert_pruned(got, counts, score, threshold, arrays, n)
        assert kept + dropped == n
        if threshold == -np.inf:
            assert dropped == nans
        if threshold >= 2.0:
            assert kept == 0 and all(np.all(o == SENT_ROW) for o in got)
    if n > 1:
        kept = int(prune_mask(score, 0.5).sum())
        assert 0.3 * n < kept < 0.8 * n and nans > 0
        for max_out in (kept - 1, kept, 1, 0):
            got, counts = run_prune(bare, score, 0.5, arrays, max_out)
            assert assert_pruned(got, counts, score, 0.5, arrays, max_out)[0] == kept
    for given in itertools.product((False, True), repeat=3):
        got, counts = run_prune(bare, score, 0.5, arrays, n, given)
        assert_pruned(got, counts, score, 0.5, arrays, n, given)
    none = run_prune(bare, np.full(n, F("nan")), -np.inf, arrays, n)
    assert tuple(none[1]) == (0, n) and all(np.all(o == SENT_ROW) for o in none[0])


# ---- 6. the invariant that ties both calls together -------------------------------------------------------------------------

def test_pruning_what_no_view_shows_keeps_the_frames(oracle_mod, tmp_path):
    """wmax over two cameras on ragged, pruned at the smallest positive float: the kept cloud, uploaded, renders both
    cameras' RGBA8 and RGBA32F frames byte for byte as before.  The condition -- no frame overflowed -- is asserted."""
    aos, w, h, cam, p, c = scene_reference(oracle_mod, tmp_path, "ragged")
    aos = np.ascontiguousarray(aos, F)
    n = len(aos)
    scenes = (make_scene(aos, w, h), make_scene(aos, w, h, **MOVED))
    r = make_renderer(scenes[0], w, h)
    r.setOutputs(rgba32f=True)
    wmax = torch.zeros(n, device=DEV)
    torch.cuda.synchronize()
    before = []
    for sc in scenes:
        img = r.draw(sc).copy()
        assert r.lastStatus == _lib.GS_OK
        before.append((img, r.readOutput(gs.GS_OUTPUT_RGBA32F).copy()))
        r.contribDevice(n, wmax.data_ptr(), None, None)
    d_aos, out = up(aos), torch.zeros(n, 84, device=DEV)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    r.pruneBelowDevice(wmax.data_ptr(), float(TINY), n, d_aos.data_ptr(), None, None, None, out.data_ptr(), None, None, None, n,
                       counts.data_ptr())
    r.synchronize()
    kept, dropped = (int(x) for x in down(counts, np.uint32))
    score = down(wmax, F)
    assert kept == int((score > 0).sum()) and kept + dropped == n and dropped > 2000 and kept > 2000
    assert np.array_equal(bits(down(out, F)[:kept]), bits(aos[score > 0]))
    r.uploadDevice(out.data_ptr(), kept)
    assert r.sceneInfo().num_gaussians == kept
    for sc, (img, f32) in zip(scenes, before):
        again = r.draw(sc)
        assert r.lastStatus == _lib.GS_OK
        assert again.tobytes() == img.tobytes() and r.readOutput(gs.GS_OUTPUT_RGBA32F).tobytes() == f32.tobytes()
    r.cleanup()


# ---- 7. VisibleAdam.prune_by_contribution -----------------------------------------------------------------------------------

@pytest.mark.parametrize("space", ["raw", "records"])
def test_visible_adam_prunes_by_contribution(oracle_mod, tmp_path, space):
    """After three steps on the dense scene: wmax is the reference's on the optimiser's current records; the kept rows of
    records, raw, m and v are the old rows bit for bit, in order (raw without a log/exp round trip); sizes, max_rows and
    the statistics follow the new n, t stays; the next step runs on a full upload of the new cloud; a threshold above
    every weight raises and leaves the optimiser as it was."""
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, F)
    n = len(aos)
    sc = make_scene(aos, w, h)
    cam = gs.Renderer._camera_args(sc.getCamera())
    target = torch.full((h, w, 3), 0.4, device=DEV)
    r = new_renderer(sc, w, h, gs.GS_SORT_RADIX4, False)
    opt = VisibleAdam(torch.tensor(aos, device=DEV), renderer=r, track_density=True, space=space)
    for _ in range(3):
        opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    names = ("records", "m", "v") + (("raw",) if space == "raw" else ())
    old = {k: getattr(opt, k).cpu().numpy().copy() for k in names}
    assert old["m"].any() and opt.seen.any()
    with pytest.raises(RuntimeError, match="every gaussian"):
        opt.prune_by_contribution([cam[:3]], 2.0)
    assert opt.records.shape[0] == n and np.array_equal(bits(opt.records.cpu().numpy()), bits(old["records"]))
    n_out, dropped = opt.prune_by_contribution([cam[:3]], float(TINY))
    score = opt.wmax.cpu().numpy()
    keep = prune_mask(score, TINY)
    assert (n_out, dropped) == (int(keep.sum()), n - int(keep.sum())) and 50 < n_out < n - 1000
    assert opt.wmax.shape == opt.wsum.shape == opt.pixels.shape == (n,)
    if space == "records":
        c = contrib_reference(tmp_path, camera_params(oracle_mod, sc, w, h), old["records"])
        assert_same((score, opt.wsum.cpu().numpy(), opt.pixels.cpu().numpy().view(np.uint32)), ref_arrays(c), "opt")
    for k in names:
        t = getattr(opt, k)
        assert t.shape == (n_out, 84) and t.is_contiguous() and np.array_equal(bits(t.cpu().numpy()), bits(old[k][keep])), k
    assert opt.t == 3 and opt.max_rows == n_out and opt.ids.shape == (n_out,) and opt.rows.shape == (n_out, 84)
    assert opt.grad_accum.shape == opt.seen.shape == opt.max_radius.shape == (n_out,)
    assert not opt.grad_accum.any() and not opt.seen.any() and not opt.max_radius.any()
    assert opt._full_upload
    numbers = opt.step(*cam, target, LAMBDA)
    opt.stream.synchronize()
    assert np.all(np.isfinite(numbers.cpu().numpy())) and opt.t == 4 and not opt._full_upload
    assert r.sceneInfo().num_gaussians == n_out and 0 < int(opt.count.cpu()[0]) <= n_out
    assert not np.array_equal(bits(opt.records.cpu().numpy()), bits(old["records"][keep]))
    r.setStream(None)
    r.cleanup()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------

def test_contrib_refusals():
    """Every refusal of the header returns GS_ERR_INVALID with a message that names the call, and writes nothing."""
    aos, w, h = SCENES["dense"]()
    aos = np.ascontiguousarray(aos, F)
    n, L = len(aos), _lib.lib()
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h)
    hdl = r._ctx.handle
    state = [up(a) for a in sentinel_state(n)]
    d_aos = up(aos)
    one = up(np.zeros(1, np.uint32))
    torch.cuda.synchronize()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())

    def call(h_=None, nn=n, a=state[0], s=state[1], p=state[2]):
        return L.gs_contrib_device(hdl if h_ is None else h_, nn, vp(a), vp(s), vp(p))

    def refused(rc, word, h_=None):
        msg = L.gs_last_error(hdl if h_ is None else h_).decode()
        assert rc == _lib.GS_ERR_INVALID and msg.startswith("gs_contrib_device: ") and word in msg, (rc, word, msg)

    assert L.gs_contrib_device(None, n, vp(state[0]), None, None) == _lib.GS_ERR_INVALID
    refused(call(), "no frame since")                                        # a resolution, no frame
    r.draw(sc)
    refused(call(a=None), "null wmax")
    refused(call(nn=n - 1), "n differs from the scene's")
    refused(call(nn=n + 1), "n differs from the scene's")
    r.setTileRows(0, 2)
    refused(call(), "no frame since")                                        # new tile rows
    r.draw(sc)
    refused(call(), "a subset of the tile rows")
    r.setTileRows(0, (h + 15) // 16)
    r.draw(sc)
    r.uploadDevice(d_aos.data_ptr(), n)
    refused(call(), "no frame since")                                        # an upload in place
    r.draw(sc)
    r.uploadRowsDevice(d_aos.data_ptr(), n, one.data_ptr(), one.data_ptr(), 1)
    refused(call(), "no frame since")                                        # an upload of rows
    r.draw(sc)
    r.debugInitSortList(sc)
    refused(call(), "no frame since")                                        # an unsorted list in the buffers
    r.synchronize()
    fast = make_renderer(sc, w, h, mode=gs.GS_RENDER_FAST)
    fast.draw(sc)
    refused(call(h_=fast._ctx.handle), "only GS_RENDER_EXACT frames can be differentiated", fast._ctx.handle)
    fast.cleanup()
    torch.cuda.synchronize()
    for t, a in zip(state, sentinel_state(n)):
        assert np.array_equal(down(t, np.uint32), bits(a))
    r.draw(sc)
    assert call() == _lib.GS_OK                                              # a refusal costs the context nothing
    r.synchronize()
    assert (down(state[2], np.uint32) != SENT_PIX).sum() > 50
    r.cleanup()


def test_contrib_refuses_a_sharded_context():
    """A context whose rows gs_dist_shard_rows has dealt (world size 1: it owns every row, so this refusal and no other
    answers); in a child process, which alone holds the communicator."""
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
        out = np.full(1, -7.5, np.float32)
        ident = C.create_string_buffer(_lib.DIST_UNIQUE_ID_BYTES)
        assert L.gs_dist_unique_id(ident) == 0 and L.gs_dist_init(ctx, ident, 0, 1) == 0, L.gs_last_error(ctx)
        assert L.gs_dist_shard_rows(ctx, _lib.ROWS_CONTIGUOUS) == 0, L.gs_last_error(ctx)
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


def test_prune_refusals(bare):
    """Every refusal of the header returns GS_ERR_INVALID with a message that names the call and enqueues nothing; a valid
    call afterwards works."""
    n = 40
    arrays, score = prune_inputs(n)
    L, hdl = _lib.lib(), bare._ctx.handle
    d = dict(score=up(score), rec=up(arrays[0]), raw=up(arrays[1]), m=up(arrays[2]), v=up(arrays[3]),
             c=torch.full((2,), -1, dtype=torch.int32, device=DEV))
    for k in ("rec_o", "raw_o", "m_o", "v_o"):
        d[k] = torch.full((n, 84), float(SENT_ROW), device=DEV)
    torch.cuda.synchronize()
    vp = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())

    def call(threshold=0.5, n_=n, max_out=n, h_=hdl, **swap):
        a = dict(d, **swap)
        return L.gs_prune_below_device(h_, vp(a["score"]), threshold, n_, vp(a["rec"]), vp(a["raw"]), vp(a["m"]), vp(a["v"]),
                                       vp(a["rec_o"]), vp(a["raw_o"]), vp(a["m_o"]), vp(a["v_o"]), max_out, vp(a["c"]))

    def refused(rc, word):
        msg = L.gs_last_error(hdl).decode()
        assert rc == _lib.GS_ERR_INVALID and msg.startswith("gs_prune_below_device: ") and word in msg, (rc, word, msg)

    assert call(h_=None) == _lib.GS_ERR_INVALID
    for k in ("score", "rec", "c"):
        refused(call(**{k: None}), "null")
    refused(call(rec_o=None), "null records_out")
    refused(call(n_=0), "n is 0")
    refused(call(n_=1 << 31), "below 2^31")
    refused(call(threshold=float("nan")), "threshold is a NaN")
    for k in ("raw", "m", "v", "raw_o", "m_o", "v_o"):
        refused(call(**{k: None}), "together with their own output")
    refused(call(rec_o=d["rec"]), "aliases an input")
    refused(call(raw_o=d["raw"]), "aliases an input")
    refused(call(m_o=d["v"]), "aliases an input")
    refused(call(v_o=d["score"]), "aliases an input")
    refused(call(rec_o=d["rec"].data_ptr() + 336 * (n - 1)), "aliases an input")           # the last input row only
    refused(call(rec_o=d["rec"].data_ptr() - 336 * n + 4), "aliases an input")             # the first input float only
    refused(call(c=d["score"]), "aliases an input")
    refused(call(c=d["rec_o"]), "alias each other")
    refused(call(m_o=d["v_o"]), "alias each other")
    refused(call(raw_o=d["rec_o"]), "alias each other")
    bare.synchronize()
    for k in ("rec_o", "raw_o", "m_o", "v_o"):
        assert np.all(down(d[k], F) == SENT_ROW)
    assert np.all(down(d["c"], np.int32) == -1)
    # adjacent is not aliased; max_out == 0 needs no output rows; infinite thresholds are thresholds, not errors
    assert call(rec_o=d["rec"].data_ptr() + 336 * n, raw=None, raw_o=None, m=None, m_o=None, v=None, v_o=None, max_out=0) == _lib.GS_OK
    assert call(rec_o=None, raw_o=None, m_o=None, v_o=None, max_out=0) == _lib.GS_OK
    assert call(threshold=float("inf")) == _lib.GS_OK and call(threshold=float("-inf")) == _lib.GS_OK
    assert call() == _lib.GS_OK
    bare.synchronize()
    want_counts, want = prune_ref(score, 0.5, arrays, n)
    assert tuple(down(d["c"], np.uint32).tolist()) == want_counts
    for k, b in zip(("rec_o", "raw_o", "m_o", "v_o"), want):
        assert np.array_equal(bits(down(d[k], F)[:want_counts[0]]), bits(b))
