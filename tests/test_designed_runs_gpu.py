"""The sorters on the designed runs of tests/test_designed_runs_cpu.py: every size class of GS_SORT_TILE_BUCKET on both sides of
each of its edges, under keys whose passes move or stand still by design (that file's docstring has the lengths per class and the
moving passes per pattern).  Every frame against the CPU oracle bit for bit: sorted tile, depth and id words, ranges, covariance,
colour and pixels."""
import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from test_parity_gpu import ALL_SORTS, assert_frame_equals_oracle, make_renderer, make_scene
from test_designed_runs_cpu import (BIG_CLASSES, GRID_H, GRID_W, OVERFLOW_PADS, PATTERNS, overflow_runs, range_lengths,
                                    size_class, sorted_list)

pytestmark = pytest.mark.gpu

_FRAMES = {}


def oracle_frame(oracle, pattern, **rows):
    """(scene, w, h, oracle frame) of a pattern, once per module; rows = row_begin / row_end of a band (a run of its own)."""
    key = (pattern,) + tuple(sorted(rows.items()))
    if key not in _FRAMES:
        aos, w, h, _, ref = sorted_list(oracle, pattern)
        sc = make_scene(aos, w, h)
        cam = sc.getCamera()
        p = oracle.make_params(w, h, cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition(), **rows)
        if rows:
            ref = oracle.full_pipeline(p, aos, threads=oracle.host_threads(16))
        else:
            s1 = ref["stage1"]
            ref = dict(ref, image=oracle.render(p, aos, s1["color"], s1["cov"], ref["id"], ref["ranges"],
                                                threads=oracle.host_threads(16)))
        _FRAMES[key] = (sc, w, h, ref)
    return _FRAMES[key]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("sort", ALL_SORTS)
def test_every_sorter_on_every_pattern(oracle_mod, sort, pattern):
    """Runs of 1 ... 13001 elements at every class, lane, wave-stride and chunk edge, under each key pattern: all equal (every
    pass stands still, ties keep ascending splat index), dense low bytes under a constant top byte, a constant low byte, an odd
    number of moving 4-bit passes, a long tie of saturated keys (0xFFFFFFFF, the value of the kernels' padding lanes), the whole
    range, back to front, and all of these in one frame.  Two frames on one renderer: the in-place sort must not read what the
    frame before left in either half.  GS_SORT_TILE_BUCKET is the subject; the radix variants meet the same ties, saturated keys
    and constant digits."""
    sc, w, h, ref = oracle_frame(oracle_mod, pattern)
    r = make_renderer(sc, w, h, sort=sort)
    for _ in range(2):
        img = r.draw(sc)
        assert_frame_equals_oracle(r, img, ref)
    r.cleanup()


def test_one_context_changing_patterns(oracle_mod):
    """One GS_SORT_TILE_BUCKET renderer, the records rewritten in place between frames: wide, equal, far_odd, wide.  The run
    lengths stay, so every run meets, in the alternate half (global class) and in its own, the sorted data of another frame: a
    run without a moving pass, or with an odd number of them, must not pick any of it up."""
    import torch
    sc, w, h, _ = oracle_frame(oracle_mod, "wide")
    r = make_renderer(sc, w, h, sort=gs.GS_SORT_TILE_BUCKET)
    n = r.sceneInfo().num_gaussians
    for pattern in ("wide", "equal", "far_odd", "wide"):
        sc_p, _, _, ref = oracle_frame(oracle_mod, pattern)
        dev = torch.tensor(sc_p.getResourceManager().getGaussians(), device="cuda")
        torch.cuda.synchronize()
        r.uploadDevice(dev.data_ptr(), n)
        assert r.sceneInfo().num_gaussians == n == dev.shape[0]
        img = r.draw(sc_p)
        assert_frame_equals_oracle(r, img, ref)
    r.cleanup()


def test_band_of_tile_rows_on_the_big_classes(oracle_mod):
    """setTileRows for a band that starts past row 0 (ts_tile: first_row > 0) on the mixed pattern: S3, chunked and global runs
    inside the band, and a context that goes from the whole frame to the band and back."""
    sc, w, h, ref = oracle_frame(oracle_mod, "mixed")
    rb, re = 1, 3
    _, _, _, band = oracle_frame(oracle_mod, "mixed", row_begin=rb, row_end=re)
    lens = range_lengths(ref)
    in_band = lens[rb * GRID_W:re * GRID_W]
    assert {size_class(v) for v in in_band if v} >= set(BIG_CLASSES)
    assert np.array_equal(range_lengths(band)[rb * GRID_W:re * GRID_W], in_band) and range_lengths(band).sum() == in_band.sum()
    r = make_renderer(sc, w, h, sort=gs.GS_SORT_TILE_BUCKET)
    assert_frame_equals_oracle(r, r.draw(sc), ref)
    r.setTileRows(rb, re)
    e = band["e"]
    for _ in range(2):
        img = r.draw(sc)
        assert r.timings().num_sort_elements == e
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_TILE), band["tile"][:e])
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_DEPTH), band["depth"][:e])
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), band["id"][:e])
        assert np.array_equal(r.debugRead(gs.BUF_RANGES), band["ranges"])
        assert np.array_equal(img[rb * 16:re * 16], band["image"][rb * 16:re * 16])
        assert np.array_equal(img[rb * 16:re * 16], ref["image"][rb * 16:re * 16])
    r.setTileRows(0, GRID_H)
    assert_frame_equals_oracle(r, r.draw(sc), ref)
    r.cleanup()


@pytest.mark.parametrize("world", [2, 3])
def test_interleaved_rows_on_the_big_classes(oracle_mod, world):
    """setTileRowsInterleaved(rank, world) on the mixed pattern, every rank on one context: its list is the frame's restricted
    to its tiles, its ranges their lengths, its image rows the frame's -- and every rank owns a row with an S3, a chunked and a
    global run (ts_tile: row_stride > 1 on the classes that sort outside the small kernels)."""
    from vk3dgaussiansplatting_amd import dist as gsdist
    sc, w, h, ref = oracle_frame(oracle_mod, "mixed")
    e, lens = ref["e"], range_lengths(ref)
    r = make_renderer(sc, w, h, sort=gs.GS_SORT_TILE_BUCKET)
    for rank in range(world):
        rows = gsdist.interleaved_rows(GRID_H, rank, world)
        own_tiles = np.isin(np.arange(GRID_W * GRID_H) // GRID_W, rows)
        assert {size_class(v) for v in lens[own_tiles] if v} >= set(BIG_CLASSES), (rank, world)
        r.setTileRowsInterleaved(rank, world)
        info = r.sceneInfo()
        assert (info.row_stride, info.first_row, info.rows_owned) == (world, rank, len(rows))
        mine = np.isin(ref["tile"][:e] // GRID_W, rows)
        for _ in range(2):
            img = r.draw(sc)
            assert r.timings().num_sort_elements == mine.sum()
            assert np.array_equal(r.debugRead(gs.BUF_SORTED_TILE), ref["tile"][:e][mine])
            assert np.array_equal(r.debugRead(gs.BUF_SORTED_DEPTH), ref["depth"][:e][mine])
            assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), ref["id"][:e][mine])
            rg = r.debugRead(gs.BUF_RANGES).astype(np.int64)
            assert np.array_equal((rg[:, 1] - rg[:, 0])[own_tiles], lens[own_tiles])
            for row in rows:
                assert np.array_equal(img[row * 16:row * 16 + 16], ref["image"][row * 16:row * 16 + 16])
    r.setTileRows(0, GRID_H)
    assert_frame_equals_oracle(r, r.draw(sc), ref)
    r.cleanup()


def test_overflow_cuts_inside_a_chunked_and_a_global_run(oracle_mod):
    """E > C with the cut inside two designed runs (test_designed_runs_cpu.overflow_runs): the truncated list, whose cut runs
    are still a chunked and a global one, against the oracle, as test_overflow_truncates_like_reference does for small runs."""
    aos, w, h, whole, cut = overflow_runs(oracle_mod)
    sc = make_scene(aos, w, h)
    cam = sc.getCamera()
    p = oracle_mod.make_params(w, h, cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition())
    ref = oracle_mod.full_pipeline(p, aos, threads=oracle_mod.host_threads(16))
    lens = range_lengths(ref)
    for tile, (cls, uncut) in cut.items():
        assert size_class(lens[tile]) == cls and OVERFLOW_PADS < lens[tile] < uncut
    r = make_renderer(sc, w, h, sort=gs.GS_SORT_TILE_BUCKET)
    cap = r.sceneInfo().capacity
    assert cap == oracle_mod.capacity(aos.shape[0], GRID_W * GRID_H)
    assert ref["stage1"]["counter"] > cap, "the scene does not overflow"
    for _ in range(2):
        img = r.draw(sc)
        t = r.timings()
        assert r.lastStatus == gs.GS_WARN_OVERFLOW and t.overflowed == 1
        assert t.num_sort_elements == cap == ref["e"]
        assert_frame_equals_oracle(r, img, ref)
    r.cleanup()
