"""The backward's two stages on the MI355X, each against its own float64 reference and on each splat's own scale
(tests/test_backward_split_cpu.py has the references, the calibration of the tiers and the proof that the criterion rejects
wrong-term chains today's by-value tests accept).

  rows    gs_debug_read(GS_BUF_BACKWARD_ROWS) -- what k_bwd_blend left, summed per splat as k_bwd_rowsum_chain sums it --
          against rows_reference: |gpu - signed| <= ROWS_TIER * absolute per entry, exactly 0 where absolute == 0.
  chain   the record gradient of the same call against chain64 of the GPU's OWN rows (as float64): only bwd_chain's
          arithmetic differs.  Every entry within CHAIN_TIER * S, at most 0.1 % above CHAIN_P999_TIER * S, exactly 0 where
          S == 0 (unread fields, unlisted splats, a zero row).
  camera  gs_backward_camera against the camera twin on the same rows, on the splat-summed scale.

The branches bwd_chain holds fixed are the float32 frame's: the clamp as clamp_masks restates it in float32, max(colour, 0)
from the colour the frame stored (GS_BUF_COLOR), the anti-aliasing floor from float64 with the splats within a factor 2 of
it left out (test_antialias_cpu.compared).  Each test prints its worst |err| / scale."""
import ctypes as C

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from vk3dgaussiansplatting_amd.renderer import GsplatError
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import camera_params
from test_camera_constants_cpu import clamp_masks, with_constants
from test_backward_split_cpu import (CAMERA_REF32_MAX, CAMERA_UNWRITTEN, CHAIN_P999_TIER, CHAIN_TIER, ROWS_TIER, chain64,
                                     chain_scale, decisions64, load_split_scene, read_fields, split_frame)
from frame64 import FLOOR, live_of, splat_values, weights

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
BAND = (3, 8)                                # tile rows of the band case: `ragged` has 12


def drawn(oracle, name, sh_mode=0, antialias=False, band=None, seed=1, with_depth=True, **kw):
    """A designed scene drawn on a fresh context and differentiated once: dict(r, sc, aos, w, h, p, wr, wd, grad, rows)."""
    aos, w, h, cam, constants = load_split_scene(oracle, name)
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
    r = make_renderer(sc, w, h, **constants, **kw)
    if antialias:
        r.setAntialias(True)
    if band is not None:
        r.setBandGradients(True)
        r.setTileRows(*band)
    r.draw(sc)
    wr, wd = weights(h, w, seed)
    wd = wd if with_depth else None
    grad = r.backward(wr, wd)
    rows = r.debugRead(gs.BUF_BACKWARD_ROWS)
    p = with_constants(camera_params(oracle, sc, w, h), constants)
    return dict(r=r, sc=sc, aos=aos, w=w, h=h, p=p, wr=wr, wd=wd, grad=grad, rows=rows)


# ---- rows --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "no_depth"])
@pytest.mark.parametrize("scene", ["ragged", "dense", "ragged@pose", "truncated", "batch_edges"])
def test_rows(oracle_mod, tmp_path, scene, with_depth):
    """The summed rows of the blend against rows_reference on the float32 frame's own values: per entry within ROWS_TIER
    (16 x the float32 reference's own worst error) of `absolute`, the sum of the absolute per-pixel terms of that entry;
    exactly 0 where no term exists (unlisted splats, splats no pixel blends, the depth column without a depth gradient).
    16 x: the kernel adds the pixels in a tree and the four waves after it where the reference adds in sequence, rebuilds T
    on the walk back with one division per entry, and uses its pinned exp."""
    f = split_frame(oracle_mod, tmp_path, scene, with_depth=with_depth)
    d = drawn(oracle_mod, scene, with_depth=with_depth)
    d["r"].cleanup()
    rows = d["rows"].astype(np.float64)
    assert rows.shape == (len(f["aos"]), 10) and np.all(np.isfinite(rows))
    absolute, signed = f["absolute"], f["signed"]
    assert not rows[absolute == 0].any()
    assert np.count_nonzero(absolute.any(1)) >= (100 if scene != "batch_edges" else 50)
    if not with_depth:
        assert not absolute[:, 9].any()
    ratio = np.abs(rows - signed)[absolute > 0] / absolute[absolute > 0]
    print(f"rows {scene} {'with' if with_depth else 'without'} depth: median {np.median(ratio):.1e} max {ratio.max():.1e} "
          f"of the tier {ROWS_TIER:.1e}")
    assert ratio.max() <= ROWS_TIER


# ---- chain -------------------------------------------------------------------------------------------------------------------

def frame_decisions_of(d, ref, antialias):
    """dec of splat_values as the float32 frame decided: the clamp restated in float32, max(colour, 0) from the stored
    colour, the anti-aliasing branches from float64; and the splats to compare (not within a factor 2 of the floor)."""
    p, aos = d["p"], d["aos"]
    dec = decisions64(p, aos, ref, antialias)
    dec["clamp_x"], dec["clamp_y"] = clamp_masks(p, aos)
    dec["colour"] = d["r"].debugRead(gs.BUF_COLOR)[:, :3] > 0
    keep = np.ones(len(aos), bool)
    if antialias:
        with torch.no_grad():
            _, aux = splat_values(p, torch.tensor(aos.astype(np.float64)), live_of(ref), antialias=True)
        with np.errstate(invalid="ignore"):
            keep = ~((aux["ratio"] >= FLOOR / 2) & (aux["ratio"] <= 2 * FLOOR))
    return dec, keep


def check_chain(oracle, d, antialias=False, what=""):
    """The record gradient d['grad'] against chain64 of d['rows'].  Returns (dec, keep, ref) for a camera check behind it."""
    p, aos, rows = d["p"], d["aos"], d["rows"].astype(np.float64)
    ref = dict(stage1=oracle.init_sort_list(p, aos))
    dec, keep = frame_decisions_of(d, ref, antialias)
    want = chain64(p, aos, ref, rows, antialias=antialias, dec=dec)
    S = chain_scale(p, aos, ref, rows, antialias=antialias, dec=dec)
    got = d["grad"].astype(np.float64)
    assert np.all(np.isfinite(got))
    unread = np.setdiff1d(np.arange(84), read_fields(p.sh_mode))
    assert not S[:, unread].any() and not S[~rows.any(1)].any()
    assert not got[keep][S[keep] == 0].any()
    compared = (S > 0) & keep[:, None]
    assert compared.sum() >= 1000
    ratio = np.abs(got - want)[compared] / S[compared]
    share = float(np.mean(ratio > CHAIN_P999_TIER))
    print(f"chain {what}: {int(compared.sum())} entries, median {np.median(ratio):.1e} 99.9th {np.percentile(ratio, 99.9):.1e} "
          f"max {ratio.max():.1e} of the tier {CHAIN_TIER:.1e}; share above {CHAIN_P999_TIER:.1e}: {share:.1e}")
    assert ratio.max() <= CHAIN_TIER
    assert share <= 1e-3
    return dec, keep, ref


CHAIN_CASES = [("ragged", m, False) for m in (0, 1, 2, 4, 5)] + \
    [("ragged@pose", 0, False), ("ragged@garden", 0, False), ("extreme", 0, False), ("clamp", 0, False),
     ("ragged", 0, True), ("subpixel", 0, True)]


@pytest.mark.parametrize("scene,sh_mode,antialias", CHAIN_CASES,
                         ids=[f"{s}-sh{m}{'-antialias' if a else ''}" for s, m, a in CHAIN_CASES])
def test_chain(oracle_mod, scene, sh_mode, antialias):
    """bwd_chain against chain64 on the GPU's own rows: all five GS_SH_* modes, posed cameras, the extreme cloud, both
    clamps of getCovarianceMatrix (clamp_scene) and the anti-aliasing factor on either side of its floor."""
    d = drawn(oracle_mod, scene, sh_mode, antialias)
    try:
        check_chain(oracle_mod, d, antialias, f"{scene} sh_mode {sh_mode}{' antialias' if antialias else ''}")
    finally:
        d["r"].cleanup()


def test_chain_of_a_band(oracle_mod):
    """A contiguous band of tile rows with gs_set_band_gradients on: the read-back holds the band's partial sums -- the
    splats of blocks the band cull rejected are all zero whatever their stale counts say -- and the band's gradient is the
    chain of them."""
    whole = drawn(oracle_mod, "ragged")
    whole["r"].cleanup()
    d = drawn(oracle_mod, "ragged", band=BAND)
    try:
        listed = np.zeros(len(d["aos"]), bool)
        listed[np.unique(d["r"].debugRead(gs.BUF_SORTED_ID))] = True
        assert not d["rows"][~listed].any() and not d["grad"][~listed].any()
        assert 100 < np.count_nonzero(d["rows"].any(1)) < np.count_nonzero(whole["rows"].any(1))
        check_chain(oracle_mod, d, what="ragged, tile rows %d..%d" % BAND)
    finally:
        d["r"].cleanup()


def test_visible_form_is_the_dense_one(oracle_mod):
    """gs_backward_visible on the same frame: row i is the dense record gradient of splat ids[i] bit for bit, so the chain
    is compared once (test_chain); the read-back after it has the bits it had after gs_backward."""
    d = drawn(oracle_mod, "ragged")
    r = d["r"]
    ids, vis, count = r.backwardVisible(d["wr"], d["wd"])
    rows_after = r.debugRead(gs.BUF_BACKWARD_ROWS)
    r.cleanup()
    assert count == len(ids) > 1000
    assert np.array_equal(bits(vis), bits(d["grad"][ids]))
    silent = np.ones(len(d["aos"]), bool)
    silent[ids] = False
    assert not d["grad"][silent].any() and not d["rows"][silent].any()
    assert np.array_equal(bits(rows_after), bits(d["rows"]))


# ---- camera ------------------------------------------------------------------------------------------------------------------

CAMERA_CASES = [("ragged@pose", False), ("clamp", False), ("ragged@pose", True)]


@pytest.mark.parametrize("scene,antialias", CAMERA_CASES, ids=[f"{s}{'-antialias' if a else ''}" for s, a in CAMERA_CASES])
def test_camera_chain(oracle_mod, scene, antialias):
    """gs_backward_camera after the same backward against the camera twin on the GPU's rows, both summed over the compared
    splats, on the splat-summed scale.  Tier: 8 x the float32 reference's own worst error on that scale (CAMERA_REF32_MAX),
    times 1 + log2(listed splats) for the reduction -- gs_camera.hip adds a block's 256 splats in a float32 tree of eight
    levels and the blocks in double, each level at most 2^-24 of the summed scale, which the factor covers with room.  The
    entries gs_camera.hip never writes are exactly 0."""
    d = drawn(oracle_mod, scene, antialias=antialias)
    try:
        got = d["r"].backwardCamera().astype(np.float64)
        dec, keep, ref = check_chain(oracle_mod, d, antialias, f"{scene} before its camera")
    finally:
        d["r"].cleanup()
    p, aos, rows = d["p"], d["aos"], d["rows"].astype(np.float64)
    assert keep.all() or not rows[~keep].any(), "a splat within a factor 2 of the floor is listed: its term cannot be left out"
    _, per_splat = chain64(p, aos, ref, rows, antialias=antialias, dec=dec, camera=True)
    _, scale = chain_scale(p, aos, ref, rows, antialias=antialias, dec=dec, camera=True)
    want, S = per_splat.sum(0), scale.sum(0)
    listed = int(np.count_nonzero(rows.any(1)))
    tier = 8.0 * CAMERA_REF32_MAX * (1.0 + np.log2(listed))
    assert not got[CAMERA_UNWRITTEN].any() and not got[S == 0].any()
    assert np.count_nonzero(S) >= 20
    ratio = np.abs(got - want)[S > 0] / S[S > 0]
    print(f"camera {scene}{' antialias' if antialias else ''}: {listed} listed splats, max {ratio.max():.1e} of the tier {tier:.1e}")
    assert ratio.max() <= tier


# ---- the read-back itself ----------------------------------------------------------------------------------------------------

def test_read_back_behaviour(oracle_mod):
    """GS_BUF_BACKWARD_ROWS is refused ("no gs_backward* on this frame") before any backward and again after a new frame; a
    request larger than float[N][10] is refused, a shorter one served; the words behind the destination keep their value;
    reading changes nothing: a second gs_backward returns the bits of the first."""
    aos, w, h, cam, _ = load_split_scene(oracle_mod, "ragged")
    sc = make_scene(aos, w, h, **cam)
    r = make_renderer(sc, w, h)
    L = _lib.lib()
    n = len(aos)
    guard = np.float32(-777.25)
    buf = np.full(n * 10 + 64, guard, np.float32)
    ptr = buf.ctypes.data_as(C.c_void_p)

    def refused():
        assert L.gs_debug_read(r._ctx.handle, gs.BUF_BACKWARD_ROWS, ptr, n * 40) == _lib.GS_ERR_INVALID
        assert b"no gs_backward* on this frame" in L.gs_last_error(r._ctx.handle)
        assert np.all(buf == guard)

    r.draw(sc)
    refused()
    with pytest.raises(GsplatError):
        r.debugRead(gs.BUF_BACKWARD_ROWS)
    wr, wd = weights(h, w, 1)
    first = r.backward(wr, wd)
    assert L.gs_debug_read(r._ctx.handle, gs.BUF_BACKWARD_ROWS, ptr, n * 40 + 4) == _lib.GS_ERR_INVALID
    assert np.all(buf == guard)
    assert L.gs_debug_read(r._ctx.handle, gs.BUF_BACKWARD_ROWS, ptr, n * 40) == _lib.GS_OK
    assert np.all(buf[n * 10:] == guard) and np.count_nonzero(buf[:n * 10]) > 1000
    whole = buf[:n * 10].copy()
    assert np.array_equal(bits(whole.reshape(n, 10)), bits(r.debugRead(gs.BUF_BACKWARD_ROWS)))
    buf[:] = guard
    assert L.gs_debug_read(r._ctx.handle, gs.BUF_BACKWARD_ROWS, ptr, 1000 * 40) == _lib.GS_OK
    assert np.array_equal(bits(buf[:10000]), bits(whole[:10000])) and np.all(buf[10000:] == guard)
    assert np.array_equal(bits(r.backward(wr, wd)), bits(first))
    assert np.array_equal(bits(r.backwardCamera()), bits(r.backwardCamera()))
    r.draw(sc)
    buf[:] = guard
    refused()
    r.cleanup()


def test_read_back_under_every_sorter(oracle_mod):
    """The read-back's bits are those of the default sorter under every sorter (the rows depend on the sorted list and the
    pixels only)."""
    base = None
    for sort in ALL_SORTS:
        d = drawn(oracle_mod, "ragged", sort=sort)
        d["r"].cleanup()
        if base is None:
            base = d["rows"]
            assert np.count_nonzero(base.any(1)) > 1000
        assert np.array_equal(bits(d["rows"]), bits(base)), sort
