"""The work a frame skips, read back on the MI355X: GS_BUF_WAVE_WROTE (the quarter waves whose raster records k_project stored),
GS_BUF_BAND_BLOCKS (the blocks and waves k_band_cull kept for a band of tile rows) and GS_BUF_TILE_ORDER (RenderGaussians'
dispatch order), against the designs tests/test_skipped_work_cpu.py proves on the oracle.  No test here compares times, and none
of these decisions changes a pixel: a library that stores every record, culls nothing or dispatches in any order passes every
other file of the suite.

On the default library the 52 tests of this file pass.  What a library that skips less turns red (each edit made alone on a copy of
the sources outside the tree, built for gfx950 -- the three macros as tools/build_variants.sh passes them --, loaded through
GS_LIB_OVERRIDE and run against this file alone; every other test of the file stayed green in each run):
  -DGS_PROJECT_WRITE_ALL=1, -DGS_PROJECT_WRITE_KEPT=1, -DGS_PROJECT_RECORD_CHUNK=64, each: the same 21 tests, all on a mask
      assertion -- test_masks_equal_the_design (e.g. layout B read back 15, 0, 15, 15, 15 from the whole-wave build and 15 five times
      from the other two, for the designed 15, 0, 1, 2, 4), test_second_frame_..., test_masks_of_the_other_instantiations, the masks
      after gs_debug_init_sort_list in test_read_backs_are_refused_..., and the whole-grid masks that end
      test_band_context_stores_whole_waves (its band masks passed: a band stores whole waves in every build);
  k_band_cull with `skip = false`: test_band_blocks_of_cloud_c_as_designed (read back blocks 0, 1, 2, ... with mask 0),
      test_band_blocks_of_cloud_c_permuted for the tails 0, 1 and 65 (a survivor the float64 restatement rejects; with tail 63 it
      keeps all 17 blocks) and the masks of the clean waves in test_poisoned_blocks_survive;
  `band_skip = false` in k_project: test_out_splats_of_stored_waves_are_skipped, all four tails ("2016 out splats of stored waves
      were projected"), nothing else;
  k_tile_scatter reading s_total[t] for s_total[32 - t] (the store index held inside the table, since a wrong base leaves it
      otherwise): "not a permutation of the owned tiles" at 1025, 2049, 16 384 and 16 385 tiles, the two 1440-tile row subsets, all
      five sorters and test_raster_order_and_the_largest_frame; 1, 1023 and 1024 tiles and the 480-tile band passed;
  the same edit in k_tile_order_small: "not a permutation" at 1023 and 1024 tiles and the 480-tile band, and -- a table that is no
      permutation leaves tiles undrawn -- the pixel assertions of the small frames of this file (test_masks_of_the_other_
      instantiations, test_layout_b_..., assert_band in test_band_blocks_of_cloud_c_as_designed); every shape above 1024 tiles passed;
  and the tables that ARE permutations in the wrong order, shortest class first (the reads and the writes of s_base both
      un-reversed, in k_tile_scatter and in k_tile_order_small): every pixel assertion of the file passed, and exactly the order
      assertions failed -- the twelve tests above 1024 tiles for the first, 1023 and 1024 tiles and the 480-tile band for the second
      ("class 1 (tile 0) dispatched behind class 0 (tile 895) at position 1015" at 1023 tiles)"""
import ctypes as C

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, dist as gsdist
from test_parity_gpu import ALL_SORTS, assert_frame_equals_oracle, make_renderer, make_scene, oracle_run
from test_band_cull_cpu import C_BAND, C_TAILS, GH, H, W, cameras, cloud_c, cloud_e, oracle_run as band_oracle_run
from test_band_cull_gpu import assert_band, scene_of
from test_project_records_cpu import CAMERA_1, CAMERA_2, EMITS, FRAMES, oracle_classes
from test_project_records_gpu import assert_read_backs_equal_oracle, bits
from test_skipped_work_cpu import (CAMERAS, LAYOUTS, band_classes, blocks_the_restatement_keeps, designed_stacks, expected_band_records,
                                   expected_masks, stack_cloud, tile_order_faults, ROWS, SHAPES)

pytestmark = pytest.mark.gpu

SKIPPED = (gs.BUF_WAVE_WROTE, gs.BUF_BAND_BLOCKS, gs.BUF_TILE_ORDER)


def raw_read(r, which, nbytes):
    """gs_debug_read into a buffer of nbytes -> (status, buffer)."""
    buf = np.zeros(max(nbytes, 1), np.uint8)
    return _lib.lib().gs_debug_read(r._ctx.handle, which, buf.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes)), buf


# ---- the read-backs themselves --------------------------------------------------------------------------------------------------

def test_read_backs_are_refused_before_a_frame_and_beyond_their_size(oracle_mod):
    w, h = FRAMES[0]
    aos, _ = LAYOUTS["B"](w, h)
    n = aos.shape[0]
    sc = make_scene(aos, w, h, **CAMERA_1)
    r = make_renderer(sc, w, h)
    for which in SKIPPED:
        with pytest.raises(gs.GsplatError):
            r.debugRead(which)
        assert raw_read(r, which, 4)[0] < 0
    # a list without a frame: the masks and the blocks are its own, no tile has been dispatched
    r.debugInitSortList(sc)
    cls, _ = oracle_classes(oracle_mod, aos, w, h, CAMERA_1)
    assert np.array_equal(r.debugRead(gs.BUF_WAVE_WROTE), expected_masks(cls))
    assert np.array_equal(r.debugRead(gs.BUF_BAND_BLOCKS), np.arange((n + 255) // 256, dtype=np.uint32))
    with pytest.raises(gs.GsplatError):
        r.debugRead(gs.BUF_TILE_ORDER)
    r.draw(sc)
    tiles, waves, blocks = 4 * 3, (n + 63) // 64, (n + 255) // 256
    for which, size in ((gs.BUF_WAVE_WROTE, waves), (gs.BUF_BAND_BLOCKS, 4 * (1 + blocks)), (gs.BUF_TILE_ORDER, 4 * tiles)):
        assert raw_read(r, which, size)[0] == 0 and raw_read(r, which, 0)[0] == 0 and raw_read(r, which, size + 1)[0] < 0
        assert b"size" in _lib.lib().gs_last_error(r._ctx.handle)
    rc, first = raw_read(r, gs.BUF_BAND_BLOCKS, 4)                      # the first word is the count
    assert rc == 0 and first[:4].view(np.uint32)[0] == blocks
    # a prefix is a prefix
    whole = r.debugRead(gs.BUF_TILE_ORDER)
    assert np.array_equal(raw_read(r, gs.BUF_TILE_ORDER, 20)[1][:20].view(np.uint32), whole[:5])
    r.cleanup()


# ---- stored raster records ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w,h", FRAMES)
@pytest.mark.parametrize("layout", ["A", "B"])
def test_masks_equal_the_design(oracle_mod, layout, w, h):
    """Both layouts, both frame sizes, both cameras: GS_BUF_WAVE_WROTE is expected_masks(oracle classes), byte for byte."""
    aos, _ = LAYOUTS[layout](w, h)
    for cam in CAMERAS.values():
        cls, _ = oracle_classes(oracle_mod, aos, w, h, cam)
        sc = make_scene(aos, w, h, **cam)
        r = make_renderer(sc, w, h)
        r.draw(sc)
        got = r.debugRead(gs.BUF_WAVE_WROTE)
        assert got.dtype == np.uint8 and np.array_equal(got, expected_masks(cls)), (got.tolist(), expected_masks(cls).tolist())
        r.cleanup()


@pytest.mark.parametrize("first,second", [("camera_1", "camera_2"), ("camera_2", "camera_1")])
@pytest.mark.parametrize("layout", ["A", "B"])
def test_second_frame_reads_back_the_second_cameras_masks(oracle_mod, layout, first, second):
    """One context, the camera turned between two frames: quarters stored in the first frame and not in the second read back 0."""
    w, h = FRAMES[0]
    aos, _ = LAYOUTS[layout](w, h)
    a, b = (expected_masks(oracle_classes(oracle_mod, aos, w, h, CAMERAS[c])[0]) for c in (first, second))
    assert np.any(a & ~b) and np.any(b & ~a)
    sc1, sc2 = make_scene(aos, w, h, **CAMERAS[first]), make_scene(aos, w, h, **CAMERAS[second])
    r = make_renderer(sc1, w, h)
    r.draw(sc1)
    assert np.array_equal(r.debugRead(gs.BUF_WAVE_WROTE), a)
    r.draw(sc2)
    assert np.array_equal(r.debugRead(gs.BUF_WAVE_WROTE), b)
    r.draw(sc1)
    assert np.array_equal(r.debugRead(gs.BUF_WAVE_WROTE), a)
    r.cleanup()


@pytest.mark.parametrize("family", ["depth", "antialias", "degree1", "degree2"])
@pytest.mark.parametrize("layout", ["A", "B"])
def test_masks_of_the_other_instantiations(oracle_mod, layout, family):
    """k_project<NT_SH, VIEW_Z, SH_K, AA>: the depth output, anti-aliasing and the degree modes are instantiations of their own and
    store the same quarters."""
    w, h = FRAMES[1]
    aos, _ = LAYOUTS[layout](w, h)
    sh_mode = {"degree1": _lib.GS_SH_DEGREE_1, "degree2": _lib.GS_SH_DEGREE_2}.get(family, 0)
    for cam in CAMERAS.values():
        cls, _ = oracle_classes(oracle_mod, aos, w, h, cam)
        sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
        r = make_renderer(sc, w, h)
        if family == "depth":
            r.setOutputs(rgba32f=True, depth=True)
        r.setAntialias(family == "antialias")
        img = r.draw(sc)
        assert img[..., :3].any() and np.array_equal(r.debugRead(gs.BUF_WAVE_WROTE), expected_masks(cls))
        r.cleanup()


@pytest.mark.parametrize("rows", [(0, 1), (1, 3)])
@pytest.mark.parametrize("layout", ["A", "B"])
def test_band_context_stores_whole_waves(oracle_mod, layout, rows):
    """A contiguous band: 0xF for a wave with a splat that emits into the band, else 0 -- for the waves of a block k_band_cull
    rejected too; then the whole grid again on the same context."""
    w, h = FRAMES[0]
    aos, _ = LAYOUTS[layout](w, h)
    for cam in CAMERAS.values():
        sc = make_scene(aos, w, h, **cam)
        r = make_renderer(sc, w, h)
        r.draw(sc)                                                        # whole-grid masks first: the band must replace them
        r.setTileRows(*rows)
        r.draw(sc)
        want = expected_masks(band_classes(oracle_mod, aos, w, h, cam, *rows), band=True)
        got = r.debugRead(gs.BUF_WAVE_WROTE)
        assert np.array_equal(got, want), (got.tolist(), want.tolist())
        blocks = r.debugRead(gs.BUF_BAND_BLOCKS)
        listed = np.zeros((len(want) + 3) // 4 * 4, bool)                 # the waves the band list hands to k_project
        for rec in blocks:
            listed[4 * (int(rec) & 0x0FFFFFFF):][:4] = [not (int(rec) >> 28) >> k & 1 for k in range(4)]
        assert np.all(listed[:len(want)][want != 0])                      # nothing that emits was culled
        r.setTileRows(0, 3)
        r.draw(sc)
        assert np.array_equal(r.debugRead(gs.BUF_WAVE_WROTE), expected_masks(oracle_classes(oracle_mod, aos, w, h, cam)[0]))
        r.cleanup()


@pytest.mark.parametrize("w,h", FRAMES)
def test_layout_b_frame_lists_and_read_backs_equal_the_oracle(oracle_mod, w, h):
    """The layout with a partial last quarter that is stored: frame, lists and the three older read-backs."""
    aos, _ = LAYOUTS["B"](w, h)
    for cam in CAMERAS.values():
        cls, _ = oracle_classes(oracle_mod, aos, w, h, cam)
        sc = make_scene(aos, w, h, **cam)
        r = make_renderer(sc, w, h)
        img = r.draw(sc)
        _, ref = oracle_run(oracle_mod, sc, w, h)
        assert np.array_equal(np.unique(ref["id"][:ref["e"]]), np.nonzero(cls == EMITS)[0])
        assert_frame_equals_oracle(r, img, ref)
        assert img[..., :3].any()
        assert_read_backs_equal_oracle(r, ref, aos, cls)
        r.cleanup()


# ---- band culls -----------------------------------------------------------------------------------------------------------------

def band_context(aos, band=C_BAND):
    sc = scene_of(aos, cameras()["rigid"], W, H)
    r = make_renderer(sc, W, H)
    r.setTileRows(*band)
    return r, sc


@pytest.mark.parametrize("tail", C_TAILS)
def test_band_blocks_of_cloud_c_as_designed(oracle_mod, tail):
    """Block b survives with the waves of ~b skipped, block 0 is rejected, the tail block skips its waves past the last splat."""
    aos, _ = cloud_c(tail)
    r, sc = band_context(aos)
    assert_band(r, sc, band_oracle_run(("C", tail, False), aos, cameras()["rigid"], W, H, C_BAND), C_BAND[0], C_BAND[1], H, tail)
    got = r.debugRead(gs.BUF_BAND_BLOCKS)
    assert np.array_equal(got, expected_band_records(tail)), ([hex(v) for v in got], [hex(v) for v in expected_band_records(tail)])
    r.draw(sc)                                                            # the other parity slot of the counter
    assert np.array_equal(r.debugRead(gs.BUF_BAND_BLOCKS), expected_band_records(tail))
    # where k_band_cull does not run: every block, no wave skipped
    identity = np.arange((aos.shape[0] + 255) // 256, dtype=np.uint32)
    r.setTileRowsInterleaved(1, 3)
    r.draw(sc)
    assert np.array_equal(r.debugRead(gs.BUF_BAND_BLOCKS), identity)
    r.setTileRows(0, GH)
    r.draw(sc)
    assert np.array_equal(r.debugRead(gs.BUF_BAND_BLOCKS), identity)
    r.cleanup()


@pytest.mark.parametrize("tail", C_TAILS)
def test_band_blocks_of_cloud_c_permuted(oracle_mod, tail):
    """Nothing is designed: the survivors hold every block with an emitting splat and no block the float64 restatement rejects."""
    aos, in_mask = cloud_c(tail, permuted=True)
    r, sc = band_context(aos)
    r.draw(sc)
    survivors = r.debugRead(gs.BUF_BAND_BLOCKS) & 0x0FFFFFFF
    assert np.all(np.diff(survivors.astype(np.int64)) > 0)
    assert np.isin(np.unique(np.nonzero(in_mask)[0] // 256), survivors).all()
    assert np.isin(survivors, blocks_the_restatement_keeps(aos, cameras()["rigid"], W, H, *C_BAND)).all()
    r.cleanup()


@pytest.mark.parametrize("tail", C_TAILS)
def test_out_splats_of_stored_waves_are_skipped(oracle_mod, tail):
    """GS_BUF_COV of the band context: the oracle's for every in splat, exactly zero for every out splat of a stored wave (band_skip
    skipped it: the CPU file shows it passes both culls and lies 93 px clear of the band) and for every wave that is not stored."""
    aos, in_mask = cloud_c(tail)
    r, sc = band_context(aos)
    r.draw(sc)
    want = band_oracle_run(("C", tail, False), aos, cameras()["rigid"], W, H)["cov"]
    cov = r.debugRead(gs.BUF_COV)
    assert np.array_equal(bits(cov[in_mask]), bits(want[in_mask])) and np.all(want[~in_mask, 0] != 0)
    n = aos.shape[0]
    stored = np.repeat([in_mask[k:k + 64].any() for k in range(0, n, 64)], 64)[:n]
    assert np.array_equal(r.debugRead(gs.BUF_WAVE_WROTE), np.where(stored[::64], 0xF, 0))
    skipped = np.nonzero(cov[stored & ~in_mask].any(axis=1))[0]
    assert skipped.size == 0, f"{skipped.size} out splats of stored waves were projected"
    assert not cov[~stored].any()
    r.cleanup()


def test_poisoned_blocks_survive(oracle_mod):
    """Cloud E: a NaN or an infinity in a position, a scale or a quaternion must fail the box test towards keeping the wave."""
    aos, poisoned = cloud_e()
    r, sc = band_context(aos)
    r.draw(sc)
    rec = {int(v) & 0x0FFFFFFF: int(v) >> 28 for v in r.debugRead(gs.BUF_BAND_BLOCKS)}
    for g, col, val in poisoned:
        assert g // 256 in rec and not (rec[g // 256] >> (g % 256) // 64) & 1, (g, col, val)
    # the clean waves are skipped as in cloud C
    clean = {int(v) & 0x0FFFFFFF: int(v) >> 28 for v in expected_band_records(63)}
    dirty = {(g // 256, (g % 256) // 64) for g, _, _ in poisoned}
    for b in range(17):
        want = clean.get(b, 0xF)
        for w in range(4):
            if (b, w) in dirty:
                want &= ~(1 << w)
        assert rec.get(b, 0xF) == want, (b, rec.get(b), want)
    r.cleanup()


# ---- tile dispatch order --------------------------------------------------------------------------------------------------------

def assert_order(r, owned, stacks, grid_tiles):
    """The ranges have the designed lengths and GS_BUF_TILE_ORDER meets its specification on them."""
    rg = r.debugRead(gs.BUF_RANGES).astype(np.int64)
    lens = rg[:, 1] - rg[:, 0]
    want = np.zeros(grid_tiles, np.int64)
    for t, k in stacks.items():
        want[t] = k
    assert np.array_equal(lens, want)
    order = r.debugRead(gs.BUF_TILE_ORDER)
    assert order.dtype == np.uint32 and tile_order_faults(order, owned, lens) == []
    return order


@pytest.mark.parametrize("tiles", sorted(SHAPES))
def test_tile_order_is_longest_class_first(tiles):
    w, h, first = SHAPES[tiles]
    gw, gh = (w + 15) // 16, (h + 15) // 16
    assert gw * gh == tiles
    owned = np.arange(tiles)
    stacks = designed_stacks(owned, first)
    aos, cam = stack_cloud(w, h, stacks)
    sc = scene_of(aos, cam, w, h)
    r = make_renderer(sc, w, h)
    img = r.draw(sc)
    assert img[..., :3].any() and r.timings().num_sort_elements == aos.shape[0]
    order = assert_order(r, owned, stacks, tiles)
    r.draw(sc)                                                            # the replayed graph writes the table again
    assert_order(r, owned, stacks, tiles)
    if tiles > 1:
        assert not np.array_equal(order, owned)
    r.cleanup()


@pytest.mark.parametrize("rows", sorted(ROWS))
def test_tile_order_of_a_subset_of_the_rows(rows):
    w, h, gw, gh = 768, 960, 48, 60
    own = ROWS[rows]
    owned = np.array([y * gw + x for y in own for x in range(gw)])
    stacks = designed_stacks(owned, {"band 3..32": 3, "interleaved 1/2": 8, "band 50..59": 5}[rows])
    aos, cam = stack_cloud(w, h, stacks)
    sc = scene_of(aos, cam, w, h)
    r = make_renderer(sc, w, h)
    r.draw(sc)                                                            # the whole grid first: 2880 tiles in the table
    if rows.startswith("band"):
        r.setTileRows(own[0], own[-1] + 1)
    else:
        r.setTileRowsInterleaved(1, 2)
        assert list(gsdist.interleaved_rows(gh, 1, 2)) == own
    img = r.draw(sc)
    assert img[..., :3].any() and r.sceneInfo().rows_owned == len(own)
    order = assert_order(r, owned, stacks, gw * gh)
    assert order.min() == owned[0] and order.max() == owned[-1]
    r.cleanup()


@pytest.mark.parametrize("sort", ALL_SORTS)
def test_tile_order_under_every_sorter(sort):
    tiles = 1025
    w, h, first = SHAPES[tiles]
    owned = np.arange(tiles)
    stacks = designed_stacks(owned, first + sort)
    aos, cam = stack_cloud(w, h, stacks)
    sc = scene_of(aos, cam, w, h)
    r = make_renderer(sc, w, h, sort=sort)
    r.draw(sc)
    assert_order(r, owned, stacks, tiles)
    r.cleanup()


def test_raster_order_and_the_largest_frame():
    """GS_TILE_ORDER_RASTER reads back the owned tiles ascending -- whole grid, band, interleaved rows -- and the frame of the largest
    shape is the same bytes in either order."""
    tiles = 16385
    w, h, first = SHAPES[tiles]
    gw, gh = (w + 15) // 16, (h + 15) // 16
    stacks = designed_stacks(np.arange(tiles), first)
    aos, cam = stack_cloud(w, h, stacks)
    sc = scene_of(aos, cam, w, h)
    a = make_renderer(sc, w, h)
    img = a.draw(sc).copy()
    assert_order(a, np.arange(tiles), stacks, tiles)
    a.cleanup()
    b = make_renderer(sc, w, h, order=gs.GS_TILE_ORDER_RASTER)
    assert np.array_equal(b.draw(sc), img) and img[..., :3].any()
    assert np.array_equal(b.debugRead(gs.BUF_TILE_ORDER), np.arange(tiles, dtype=np.uint32))
    b.setTileRows(5, 9)
    b.draw(sc)
    assert np.array_equal(b.debugRead(gs.BUF_TILE_ORDER), np.arange(5 * gw, 9 * gw, dtype=np.uint32))
    b.setTileRowsInterleaved(2, 7)
    b.draw(sc)
    want = np.array([y * gw + x for y in gsdist.interleaved_rows(gh, 2, 7) for x in range(gw)], np.uint32)
    assert np.array_equal(b.debugRead(gs.BUF_TILE_ORDER), want)
    b.cleanup()
