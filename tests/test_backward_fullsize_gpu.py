"""Gradients of an EXACT frame (gs_backward*) checked BY VALUE at the sizes the project is built for, on the MI355X.

The float64 reference of tests/test_backward_cpu.py walks every tile of a frame in torch and cannot run on a 13 M-element
frame.  Here the loss weights are zero outside a few sampled tiles (pick_tiles: the corners, the partial last tile row,
the last column, the longest / median / a short / the shortest list, an empty tile, seeded random ones), so the loss
depends on the lists of those tiles only and the reference is evaluated on the frame's own full-size sorted list
restricted to them (sampled_reference_gradient; test_sampled_reference_equals_the_full_one shows it equals the full
reference).  Every splat outside the union of those lists must get exactly zero.  What this reaches that the small
scenes of test_backward_gpu.py do not: k_splat_scan_blocks with several blocks per thread, offsets saturated at 2^32 - 1,
slots up to 2^24 / 2^26, tile lists of up to 24 063 entries (376 batches of k_bwd_blend), boxes of thousands of rows in
k_bwd_rowsum_chain, the half tile row of 1080 lines, the 4K grid, a grid of more than 65 535 tiles and the tiles_touched /
extents the splat-first sorters leave.  The tolerance is compare_with_reference's, unchanged.

Measured on an MI355X, worst |gpu - ref| / tolerance over the read fields (the bound is 1): C 0.003, C under the garden
pose 0.006 (sh_mode 1: 0.002), D 0.015, Chard 0.020, Train-7k@900p 0.002 (sh_mode 2: 0.0004), the list past 2^32 0.0006,
the 65 792-tile grid 0.012; both sorters and all eight padded clouds bit-identical.  Tiles, entries and union splats per
case: profiles/backward_fullsize.txt."""
import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import SCENES, assert_posed, camera_params
from test_backward_cpu import (check_overflowing, overflow_tiles, overflowing_scene, padded_cloud, pick_tiles,
                               read_fields_of, sampled_decisions, sampled_reference_gradient, tile_lengths, tile_weights)
from test_backward_gpu import READ_FIELDS, UNREAD, compare_with_reference, frame_and_grad
from frame64 import frame_decisions, reference_gradient, weights

pytestmark = pytest.mark.gpu

SORTS = (gs.GS_SORT_RADIX4, gs.GS_SORT_RADIX8_SPLAT_FIRST)


def worst_ratio(got, want):
    """max over the read fields and splats of |got - want| / (2e-2 |want| + 2e-3 max|want column|): what
    compare_with_reference bounds by 1, as a figure to print."""
    worst = 0.0
    for f in READ_FIELDS:
        b = want[:, f]
        scale = np.abs(b).max()
        if scale:
            worst = max(worst, float((np.abs(got[:, f].astype(np.float64) - b) / (2e-2 * np.abs(b) + 2e-3 * scale)).max()))
    return worst


def oracle_list(oracle_mod, p, aos, want_splats=False):
    """The oracle's stage 1 and sorted list of a full-size frame, as test_parity_gpu.full_size_parity builds them (the
    threaded stage functions): (stage 1, e, sorted tile, depth, id, ranges)."""
    threads = oracle_mod.host_threads()
    gw, gh = oracle_mod.grid(p.width, p.height)
    s1 = oracle_mod.init_sort_list(p, aos, threads=threads, want_splats=want_splats)
    e = min(s1["counter"], s1["capacity"])
    ot, od, oi = oracle_mod.sort_stable(s1["tile"], s1["depth"], s1["id"], e, threads=threads, inplace=True)
    return s1, e, ot, od, oi, oracle_mod.find_ranges(ot, e, gw * gh)


def assert_sampled_gradient(got, uniq, want, sh_mode, what):
    """got [N, 84] of the GPU against the sampled reference (uniq, want): finite, unread fields exactly zero, every
    splat outside the union exactly zero, compare_with_reference on the union.  The reference must not be empty: at
    least 500 non-zero rows and a non-zero scale in every column the SH mode reads."""
    assert np.count_nonzero(np.abs(want).sum(1)) >= 500, what
    for f in read_fields_of(sh_mode):
        assert np.abs(want[:, f]).max() > 0, (what, f)
    assert np.all(np.isfinite(got)), what
    assert np.all(got[:, UNREAD] == 0), what
    touched_rows = np.flatnonzero(got.any(1))
    assert np.all(np.isin(touched_rows, uniq)), (what, np.setdiff1d(touched_rows, uniq)[:10])
    sub = got[uniq]
    print(f"{what}: worst |gpu - ref| / tolerance {worst_ratio(sub, want):.4f}")
    bad = compare_with_reference(sub, want, np.ones(len(uniq), bool))
    assert not bad, (what, bad[:10])


def full_size_cloud(name):
    """(aos, w, h, camera) of a BASELINE config ('C', 'D', 'Chard'), of it under a benchmark pose ('C@garden') or of a
    README shape ('Train-7k@900p')."""
    if name in synth.README_SHAPES:
        shp = synth.README_SHAPES[name]
        aos = synth.generate(shp["n"], shp["width"], shp["height"], shp["mu"], shp["seed"])
        return aos, shp["width"], shp["height"], ((0.0, 0.0, 0.0), 0.0, 0.0)
    base, _, pose = name.partition("@")
    aos, cfg = synth.generate_config(base, pose=pose or None)
    return aos, cfg["width"], cfg["height"], cfg["camera"]


@pytest.mark.parametrize("name,sh_mode", [("C", 0), ("C@garden", 0), ("C@garden", 1), ("D", 0), ("Chard", 0),
                                          ("Train-7k@900p", 0), ("Train-7k@900p", 2)])
def test_by_value_at_full_size(oracle_mod, tmp_path, name, sh_mode):
    """Config C (5.8 M splats, 1920 x 1080, E = 13.1 M), the same under the garden benchmark pose (also with the SH modes'
    direction-dependent colour, sh_mode 1), config D (3840 x 2160, 32 400 tiles, E = 33 M), Chard (tile lists of 29 to
    24 063 entries) and the README shape Train-7k@900p (100 x 57 tiles, a 4-pixel last tile row; also sh_mode 2): the
    frame's sorted ids and ranges equal the oracle's, so the reference uses the decisions of the frame that is
    differentiated; the gradient under tile_weights on the picked tiles (the frame's longest list and a tile of the
    last, at 1080 and 900 lines partial, tile row among them) against sampled_reference_gradient within
    compare_with_reference's bound, exact zeros outside the union and in the unread fields, and the same bits after
    GS_SORT_RADIX4 and GS_SORT_RADIX8_SPLAT_FIRST."""
    aos, w, h, (pos, yaw, pitch) = full_size_cloud(name)
    sc = make_scene(aos, w, h, pos=pos, yaw=yaw, pitch=pitch, sh_mode=sh_mode)
    p = camera_params(oracle_mod, sc, w, h)
    assert p.sh_mode == sh_mode
    if "@garden" in name:
        assert_posed(p)
    gw, gh = oracle_mod.grid(w, h)
    s1, e, _, _, oi, oranges = oracle_list(oracle_mod, p, aos)
    assert s1["counter"] <= s1["capacity"] and len(aos) > 262_144 * 2          # several blocks per scan thread
    tiles = pick_tiles(oranges, gw, gh, seed=len(name) + sh_mode)
    lens = tile_lengths(oranges)
    assert lens[tiles].max() == lens.max()
    assert np.any(tiles // gw == gh - 1) and (h % 16 != 0) == (h in (1080, 900))   # a tile of the partial bottom row
    assert np.any(lens[tiles] == 0) or not np.any(lens == 0)
    wr, wd = tile_weights(w, h, tiles, seed=17)
    uniq, want = sampled_reference_gradient(tmp_path, p, aos, s1, oi[:e], oranges, tiles, wr.astype(np.float64),
                                            wd.astype(np.float64))
    print(f"{name} sh_mode {sh_mode}: E {e}, {len(tiles)} tiles {tiles.tolist()}, lists {int(lens[tiles].min())} .. "
          f"{int(lens[tiles].max())}, {int(lens[tiles].sum())} entries, {len(uniq)} union splats, "
          f"{np.count_nonzero(np.abs(want).sum(1))} non-zero reference rows")
    first = None
    for sort in SORTS:
        r = make_renderer(sc, w, h, sort=sort)
        r.draw(sc)
        assert r.lastStatus == _lib.GS_OK
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), oi[:e]), sort
        assert np.array_equal(r.debugRead(gs.BUF_RANGES), oranges), sort
        got = r.backward(wr, wd)
        r.cleanup()
        if first is None:
            first = got
        else:
            assert np.array_equal(first.view(np.uint32), got.view(np.uint32)), sort
        del got
    assert_sampled_gradient(first, uniq, want, sh_mode, f"{name} sh_mode {sh_mode}")


@pytest.mark.parametrize("filler", ["behind", "outside"])
@pytest.mark.parametrize("n", [262_144, 262_145, 524_545, 1_048_577])
def test_compaction_invariance(filler, n):
    """Slot offsets across the thread boundaries of k_splat_scan_blocks: the 6000 splats of the ragged scene (compared
    with the float64 reference in test_backward_gpu.py) scattered, order preserved, over n records whose others emit
    nothing (padded_cloud; n = 262 144: 1024 blocks, one per thread; 262 145: two; 524 545: three, the last block
    partial; 1 048 577: five) with live splats at 0, n - 1 and on both sides of thread and wave boundaries.  The sort is
    stable and the index map monotone, so the sorted list is the compact cloud's list (on the oracle:
    test_padded_cloud_has_the_compact_list); rows are summed in slot order and the chain is per splat: the live
    splats' gradient equals the compact cloud's BIT FOR BIT and every filler row is exactly zero."""
    aos, w, h = SCENES["ragged"]()
    r, sc, base = frame_and_grad(aos, w, h, seed=1)
    compact_ids, compact_ranges = r.debugRead(gs.BUF_SORTED_ID), r.debugRead(gs.BUF_RANGES)
    r.cleanup()
    assert np.count_nonzero(base.any(1)) > 1000
    cloud, pos = padded_cloud(aos, n, seed=n, filler=filler)
    r, sc, got = frame_and_grad(cloud, w, h, seed=1)
    ids, ranges = r.debugRead(gs.BUF_SORTED_ID), r.debugRead(gs.BUF_RANGES)
    r.cleanup()
    assert np.array_equal(ids, pos[compact_ids]) and np.array_equal(ranges, compact_ranges)
    assert got.shape == (n, 84)
    live = np.zeros(n, bool)
    live[pos] = True
    assert not got[~live].any()
    differ = np.flatnonzero((got[pos].view(np.uint32) != base.view(np.uint32)).any(1))
    assert differ.size == 0, (len(differ), pos[differ[:10]].tolist())


def test_list_past_2_to_32(oracle_mod, tmp_path):
    """A frame whose element counter passes 2^32 (overflowing_scene: 800 000 frame-filling splats at 1920 x 1080, counter
    4.5e9, capacity 2^24; the conditions are checked on the oracle by check_overflowing).
    Forward: GS_WARN_OVERFLOW, emitted_elements is the 64-bit counter, num_sort_elements the capacity, sorted tiles,
    depths, ids and ranges equal the oracle's with every sorter, pixels bit-exact on three tile rows.
    Backward under whole-frame weights: every splat wholly past the capacity gets exact zeros -- in particular the
    'victims', whose true offset is past 2^32 and would wrap below the capacity if block_offsets / offsets did not
    saturate, so that they would sum other splats' rows -- and the splat the capacity cuts has a gradient.
    Backward under tile weights: by value against the sampled reference, as test_by_value_at_full_size."""
    aos, w, h = overflowing_scene()
    sc = make_scene(aos, w, h)
    p = camera_params(oracle_mod, sc, w, h)
    gw, gh = oracle_mod.grid(w, h)
    s1, e, ot, od, oi, oranges = oracle_list(oracle_mod, p, aos, want_splats=True)
    across, past, victims = check_overflowing(s1)
    cap = s1["capacity"]
    assert e == cap and not np.any(past[oi[:e]]) and np.all(past[victims])
    rows = (0, 33, gh - 1)
    cam = sc.getCamera()
    ref_img = np.zeros((h, w, 4), np.uint8)
    for tr in rows:
        pb = oracle_mod.make_params(w, h, cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition(),
                                    row_begin=tr, row_end=tr + 1)
        oracle_mod.render(pb, aos, s1["color"], s1["cov"], oi, oranges, out=ref_img, threads=oracle_mod.host_threads())
    row_sel = np.concatenate([np.arange(tr * 16, min(tr * 16 + 16, h)) for tr in rows])
    tiles = overflow_tiles(oranges, gw, gh, ot[:e], oi[:e], across)
    lens = tile_lengths(oranges)
    dec = sampled_decisions(tmp_path, p, aos, s1, oi[:e], oranges, tiles)
    assert np.any(dec[2][dec[0] == across])                                   # some pixel blends the cut splat
    twr, twd = tile_weights(w, h, tiles, seed=4)
    uniq, want = sampled_reference_gradient(tmp_path, p, aos, s1, oi[:e], oranges, tiles, twr.astype(np.float64),
                                            twd.astype(np.float64), decisions=dec)
    assert np.any(want[np.searchsorted(uniq, across)] != 0)
    print(f"past 2^32: counter {s1['counter']}, {int(victims.sum())} victims, {len(tiles)} tiles {tiles.tolist()}, "
          f"{int(lens[tiles].sum())} entries, {len(uniq)} union splats, "
          f"{np.count_nonzero(np.abs(want).sum(1))} non-zero reference rows")
    wr, wd = weights(h, w, 13)
    whole = sampled = None
    for sort in ALL_SORTS:
        r = make_renderer(sc, w, h, sort=sort)
        img = r.draw(sc)
        t = r.timings()
        assert r.lastStatus == gs.GS_WARN_OVERFLOW and t.overflowed == 1, sort
        assert t.emitted_elements == s1["counter"] and t.num_sort_elements == cap == r.sceneInfo().capacity, sort
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_TILE), ot[:e]), sort
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_DEPTH), od[:e]), sort
        assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), oi[:e]), sort
        assert np.array_equal(r.debugRead(gs.BUF_RANGES), oranges), sort
        assert np.array_equal(img[row_sel], ref_img[row_sel]), sort
        if sort in SORTS:
            g_whole, g_sampled = r.backward(wr, wd), r.backward(twr, twd)
            if whole is None:
                whole, sampled = g_whole, g_sampled
            else:
                assert np.array_equal(whole.view(np.uint32), g_whole.view(np.uint32)), sort
                assert np.array_equal(sampled.view(np.uint32), g_sampled.view(np.uint32)), sort
        r.cleanup()
    assert np.all(np.isfinite(whole)) and np.all(whole[:, UNREAD] == 0)
    assert not whole[victims].any()
    assert not whole[past].any()
    assert np.any(whole[across] != 0)
    assert np.count_nonzero(whole.any(1)) >= 500
    assert_sampled_gradient(sampled, uniq, want, 0, "past 2^32")


@pytest.mark.parametrize("sort", [gs.GS_SORT_RADIX4, gs.GS_SORT_RADIX4_SPLAT_FIRST])
def test_grid_beyond_16_bit_tile_ids(oracle_mod, tmp_path, sort):
    """More than 65 535 tiles (4096 x 4112: 256 x 257 = 65 792, 32-bit tile words, the grid of
    test_parity_gpu.test_grid_beyond_16_bit_tile_ids with its 600 splats): the gradient under whole-frame weights
    against the full float64 reference_gradient (the cloud is small), exact zeros in the unread fields and on the splats
    that emit nothing."""
    w, h = 4096, 4112
    aos = synth.generate(600, w, h, -3.5, seed=5)
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h, sort=sort)
    assert r.sceneInfo().tile_word_bytes == 4 and r.sceneInfo().tiles_x * r.sceneInfo().tiles_y > 65535
    r.draw(sc)
    ids, ranges = r.debugRead(gs.BUF_SORTED_ID), r.debugRead(gs.BUF_RANGES)
    wr, wd = weights(h, w, 14)
    got = r.backward(wr, wd)
    r.cleanup()
    p = camera_params(oracle_mod, sc, w, h)
    ref, flags = frame_decisions(tmp_path, p, aos)
    e = int(ref["e"])
    assert e > 30000 and np.array_equal(ids, ref["id"][:e]) and np.array_equal(ranges, ref["ranges"])
    assert np.count_nonzero(tile_lengths(ref["ranges"])[65536:]) > 0          # lists on tiles past the 16-bit ids
    want = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    assert np.count_nonzero(np.abs(want).sum(1)) >= 200
    assert np.all(np.isfinite(got)) and np.all(got[:, UNREAD] == 0)
    emitting = np.zeros(len(aos), bool)
    emitting[ref["id"][:e]] = True
    assert np.all(got[~emitting] == 0)
    print(f"65 792 tiles, sorter {sort}: worst |gpu - ref| / tolerance {worst_ratio(got, want):.4f}")
    bad = compare_with_reference(got, want, np.ones(len(aos), bool))
    assert not bad, bad[:10]
