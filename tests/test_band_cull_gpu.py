"""A context that owns a subset of the tile rows against the oracle, on the inputs of tests/test_band_cull_cpu.py: the
designed clouds put splats where only the conservative culls of such a context decide (sig2 and the wave boxes of
gs_upload.hip, w_norm2 of make_frame_params, radius_bound / misses_owned_rows / box_misses_owned_rows / k_band_cull and
k_project's band_skip in gs_project.hip).  Every list is compared in full: element count, sorted tile / depth / id words,
tile ranges, and the pixels of the owned rows.  A contiguous band against the oracle's band run; interleaved rows against
the oracle's whole-frame list restricted to the owned rows."""
import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import dist as gsdist
from test_parity_gpu import make_renderer
from test_band_cull_cpu import (BANDS, C_TAILS, D_SIZE, GH, GW, H, VIEWS, W, cameras, cloud_a, cloud_b, cloud_c, cloud_d, cloud_e,
                                default_camera, oracle_rows, oracle_run)

pytestmark = pytest.mark.gpu


def scene_of(aos, cam, w, h):
    rm = gs.ResourceManager()
    rm.setGaussians(aos)
    sc = gs.Scene(rm, aspect_ratio=w / h)
    sc.camera = cam
    return sc


def read_list(r):
    return r.debugRead(gs.BUF_SORTED_TILE), r.debugRead(gs.BUF_SORTED_DEPTH), r.debugRead(gs.BUF_SORTED_ID)


def assert_band(r, sc, ref, rb, re, h, what):
    """The context's rows [rb, re) against the oracle's band run `ref`."""
    r.setTileRows(rb, re)
    img = r.draw(sc)
    e = ref["e"]
    assert r.timings().num_sort_elements == e, what
    tile, depth, ident = read_list(r)
    assert np.array_equal(tile, ref["tile"]), what
    assert np.array_equal(depth, ref["depth"]), what
    assert np.array_equal(ident, ref["id"]), what
    assert np.array_equal(r.debugRead(gs.BUF_RANGES), ref["ranges"]), what
    rows = slice(rb * 16, min(re * 16, h))
    assert np.array_equal(img[rows], ref["image"][rows]), what


def restricted(full, rows, gw, gh):
    """A whole-frame list read back from a context (tile, depth, id, ranges, image) restricted to the tile rows `rows`, in
    the form of test_band_cull_cpu.oracle_rows."""
    mine = np.isin(full["tile"] // gw, rows)
    lens = full["ranges"][:, 1].astype(np.int64) - full["ranges"][:, 0]
    lens[~np.isin(np.arange(gw * gh) // gw, rows)] = 0
    return dict(e=int(mine.sum()), tile=full["tile"][mine], depth=full["depth"][mine], id=full["id"][mine], lens=lens,
                image=full["image"], rows=list(rows))


def assert_rows(r, img, want, gw, h, what):
    """The context's list and pixels against `want` (oracle_rows, or restricted): the words, the lengths of the owned
    tiles' ranges, the pixels of the owned rows."""
    assert r.timings().num_sort_elements == want["e"], what
    tile, depth, ident = read_list(r)
    assert np.array_equal(tile, want["tile"]), what
    assert np.array_equal(depth, want["depth"]), what
    assert np.array_equal(ident, want["id"]), what
    rg = r.debugRead(gs.BUF_RANGES).astype(np.int64)
    own_tiles = np.isin(np.arange(rg.shape[0]) // gw, want["rows"])
    assert np.array_equal((rg[:, 1] - rg[:, 0])[own_tiles], want["lens"][own_tiles]), what
    for row in want["rows"]:
        px = slice(row * 16, min(row * 16 + 16, h))
        assert np.array_equal(img[px], want["image"][px]), what


def assert_interleaved(r, sc, key, aos, cam, w, h, phase, stride, what):
    gw, gh = (w + 15) // 16, (h + 15) // 16
    r.setTileRowsInterleaved(phase, stride)
    img = r.draw(sc)
    assert_rows(r, img, oracle_rows(key, aos, cam, w, h, gsdist.interleaved_rows(gh, phase, stride)), gw, h, what)


A_CASES = [(view, gs.GS_SORT_RADIX4) for view in VIEWS] \
    + [(view, sort) for view in ("roll37", "scale2.5") for sort in (gs.GS_SORT_RADIX4_SPLAT_FIRST, gs.GS_SORT_TILE_BUCKET)]


@pytest.mark.parametrize("view,sort", A_CASES, ids=[f"{v}-sort{s}" for v, s in A_CASES])
def test_cloud_a_bands(oracle_mod, view, sort):
    """Cloud A under every view: the first, a middle and the ragged last row, and interleaved rows 1, 4, 7, ...  The views
    with a scale are the only inputs of the suite whose w_norm2 is not 1; the rolls turn the wave boxes on the screen."""
    cam, aos = cameras()[view], cloud_a()
    sc = scene_of(aos, cam, W, H)
    r = make_renderer(sc, W, H, sort=sort)
    for band in BANDS:
        assert_band(r, sc, oracle_run(("A", view), aos, cam, W, H, band), band[0], band[1], H, (view, band))
    assert_interleaved(r, sc, ("A", view), aos, cam, W, H, 1, 3, (view, "interleaved 1/3"))
    r.cleanup()


@pytest.mark.parametrize("view", ["rigid", "scale2.5"])
def test_cloud_b_edges(oracle_mod, view):
    """The designed edges: splats wholly above the frame that the reference's truncation puts in row 0, the ragged last
    row, the near plane running through a wave, boxes that straddle the camera plane, quaternions of norm 0 .. 1e3, needles,
    negative / zero / tiny scales."""
    cam, (aos, _, _) = cameras()[view], cloud_b()
    sc = scene_of(aos, cam, W, H)
    r = make_renderer(sc, W, H)
    for band in ((0, 1), (22, 23), (10, 13)):
        ref = oracle_run(("B", view), aos, cam, W, H, band)
        assert ref["e"] > 0
        assert_band(r, sc, ref, band[0], band[1], H, (view, band))
    assert_interleaved(r, sc, ("B", view), aos, cam, W, H, 0, 2, (view, "interleaved 0/2"))
    r.cleanup()


@pytest.mark.parametrize("permuted", [False, True], ids=["designed", "permuted"])
@pytest.mark.parametrize("tail", C_TAILS)
def test_cloud_c_wave_masks(oracle_mod, tail, permuted):
    """Every four-bit mask of skipped waves in a 256-splat block, in waves whose one emitting splat sits at lane 0 or 63,
    and a partial last wave of emitting splats (1, 63, 64 + 1 of them, or none); the same records in a random order."""
    cam, (aos, _) = cameras()["rigid"], cloud_c(tail, permuted)
    sc = scene_of(aos, cam, W, H)
    r = make_renderer(sc, W, H)
    for band in ((11, 12), (0, 1)):
        ref = oracle_run(("C", tail, permuted), aos, cam, W, H, band)
        assert ref["e"] > 0
        assert_band(r, sc, ref, band[0], band[1], H, (tail, permuted, band))
    r.cleanup()


def test_cloud_d_extreme(oracle_mod):
    """conftest.extreme_cloud: saturating footprints, splats on the cull planes, zero quaternions and scales."""
    w, h = D_SIZE
    cam, aos = default_camera(w, h), cloud_d()
    sc = scene_of(aos, cam, w, h)
    r = make_renderer(sc, w, h)
    for band in ((0, 1), (3, 5), (7, 8)):
        assert_band(r, sc, oracle_run(("D", "default"), aos, cam, w, h, band), band[0], band[1], h, band)
    assert_interleaved(r, sc, ("D", "default"), aos, cam, w, h, 1, 2, "interleaved 1/2")
    r.cleanup()


def test_cloud_e_nan_and_infinity(oracle_mod):
    """A NaN or an infinity in one splat of a wave.  The oracle restates a reference whose int(NaN) is undefined, so the
    reference here is the library's own whole-frame context, which runs none of the band culls: its sorted list restricted
    to the band rows must be the band context's list.  Where the whole-frame list equals the oracle's anyway, the band is
    compared with the oracle's band run too.  (Such a splat's covariance is NaN and the frame puts it into tile 0.  This
    test found store_record_planes losing a NaN scale in fmaxf and an infinite quaternion component in the Gershgorin
    maximum: sig2 came out finite and the rows (0, 1) lost those splats.)"""
    cam, (aos, poisoned) = cameras()["rigid"], cloud_e()
    sc = scene_of(aos, cam, W, H)
    r = make_renderer(sc, W, H)
    whole = r.draw(sc).copy()
    tile, depth, ident = read_list(r)
    full = dict(tile=tile, depth=depth, id=ident, ranges=r.debugRead(gs.BUF_RANGES), image=whole)
    assert tile.size == r.timings().num_sort_elements > 0
    bad = np.array(sorted(g for g, _, _ in poisoned))
    o = oracle_run(("E", "rigid"), aos, cam, W, H)
    same_as_oracle = o["e"] == tile.size and np.array_equal(o["tile"], tile) and np.array_equal(o["depth"], depth) \
        and np.array_equal(o["id"], ident)
    print(f"cloud E: whole-frame list {'equals' if same_as_oracle else 'differs from'} the oracle's; "
          f"{np.isin(ident, bad).sum()} elements of {np.isin(bad, ident).sum()} poisoned splats")
    b = gs.Renderer(W, H, warmup_frames=0)
    b.init(sc.getResourceManager())
    b.initForScene(sc)
    for band in ((11, 12), (0, 1), (22, 23), (5, 17)):
        b.setTileRows(*band)
        img = b.draw(sc)
        assert_rows(b, img, restricted(full, list(range(*band)), GW, GH), GW, H, band)
        if same_as_oracle:
            assert_band(b, sc, oracle_run(("E", "rigid"), aos, cam, W, H, band), band[0], band[1], H, (band, "oracle"))
    b.setTileRowsInterleaved(0, 3)
    assert_rows(b, b.draw(sc), restricted(full, gsdist.interleaved_rows(GH, 0, 3), GW, GH), GW, H, "interleaved 0/3")
    b.cleanup()
    r.cleanup()


@pytest.mark.parametrize("sort", [gs.GS_SORT_RADIX4, gs.GS_SORT_RADIX4_SPLAT_FIRST])
def test_one_context_through_a_sequence(oracle_mod, sort):
    """One context: rows (0, 1) -> (11, 12) -> interleaved 1/3 -> (22, 23) -> the whole frame, another view at every step
    and two frames per step, each equal to its oracle run: the frame parity of the helper and band-list counters, a band
    list left by the step before, wave_wrote flags left by another band."""
    aos = cloud_a()
    cams = cameras()
    sc = scene_of(aos, cams["rigid"], W, H)
    r = make_renderer(sc, W, H, sort=sort)
    steps = [((0, 1), "roll37"), ((11, 12), "scale2.5"), ("interleaved", "aniso"), ((22, 23), "mirror"), ("whole", "roll90")]
    for rows, view in steps:
        sc.camera = cams[view]
        for frame in range(2):
            what = (rows, view, frame)
            if rows == "interleaved":
                assert_interleaved(r, sc, ("A", view), aos, cams[view], W, H, 1, 3, what)
            elif rows == "whole":
                ref = oracle_run(("A", view), aos, cams[view], W, H)
                assert_band(r, sc, ref, 0, GH, H, what)
                assert r.timings().emitted_elements == ref["counter"]
            else:
                assert_band(r, sc, oracle_run(("A", view), aos, cams[view], W, H, rows), rows[0], rows[1], H, what)
    r.cleanup()
