"""The sorters in a frame on the designed list lengths of tests/test_designed_lengths_cpu.py: every word layout a frame uses
(16-bit compact and 32-bit tile words, depth words shrinking from 4 to 2 to 0 bytes, Count on runs of equal digits, fed counts,
the splat-first list whose payload is a tile count) at the group, wave, segment and block edges the radix kernels and the
splat-first chain branch on -- that file's docstring has the lengths.  Every frame against the CPU oracle bit for bit."""
import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from test_parity_gpu import ALL_SORTS, assert_frame_equals_oracle, make_renderer, make_scene
from test_designed_lengths_cpu import (AUTO_CAPACITY, AUTO_FRAMES, AUTO_N, BIG_CAPACITY, GROUPS_CULLED, GROUPS_N,
                                       SHORT_CAPACITY, SHORT_N, SORT8_SMALL_BELOW, WIDE_BAND, WIDE_CAPACITY, WIDE_GH, WIDE_GW,
                                       auto_frames, auto_modes, big_frames, big_scene, groups_frames, groups_scene,
                                       short_frames, wide_frame, wide_scene)

pytestmark = pytest.mark.gpu

SPLAT_FIRST = (gs.GS_SORT_RADIX4_SPLAT_FIRST, gs.GS_SORT_RADIX8_SPLAT_FIRST)


def renderer(sc, w, h, sort, record_timings=1, count=gs.GS_COUNT_AUTO):
    r = gs.Renderer(w, h, warmup_frames=0, sort_algorithm=sort, record_timings=record_timings, count_launches=count)
    r.init(sc.getResourceManager())
    r.initForScene(sc)
    return r


def upload(r, records):
    """The scene's records rewritten in place from a device tensor (same N: resolution, buffers and captured graphs stay)."""
    import torch
    dev = records if isinstance(records, torch.Tensor) else torch.tensor(records, device="cuda")
    torch.cuda.synchronize()
    n = r.sceneInfo().num_gaussians
    assert dev.shape == (n, 84) and dev.dtype == torch.float32 and dev.is_contiguous()
    r.uploadDevice(dev.data_ptr(), n)
    assert r.sceneInfo().num_gaussians == n
    return dev


def assert_lists_equal_oracle(r, ref):
    e = ref["e"]
    assert r.timings().num_sort_elements == e
    assert np.array_equal(r.debugRead(gs.BUF_SORTED_TILE), ref["tile"][:e])
    assert np.array_equal(r.debugRead(gs.BUF_SORTED_DEPTH), ref["depth"][:e])
    assert np.array_equal(r.debugRead(gs.BUF_SORTED_ID), ref["id"][:e])
    assert np.array_equal(r.debugRead(gs.BUF_RANGES), ref["ranges"])


@pytest.mark.parametrize("sort,record_timings", [(s, 1) for s in ALL_SORTS] + [(s, 0) for s in SPLAT_FIRST])
def test_short_lists_on_one_context(oracle_mod, sort, record_timings):
    """28 frames of 0 ... 6145 elements through one context, N fixed, the records rewritten in place: E = M on every lane, block,
    emit-round and group edge (a last group of one key, M mod 4 = 1, 2, 3), and M on an edge with E off it and the other way
    round.  Every short frame follows a longer one -- the ping-pong halves hold sorted data of another frame beyond E -- the
    empty frame follows the longest and a long one follows it.  record_timings = 0: the splat-first chain as ONE graph."""
    frames = short_frames(oracle_mod)
    w, h = 160, 64
    r = renderer(make_scene(frames[0][2], w, h), w, h, sort, record_timings)
    info = r.sceneInfo()
    assert (info.num_gaussians, info.capacity, info.tile_word_bytes) == (SHORT_N, SHORT_CAPACITY, 2)
    for k, (s, p, aos, ref) in enumerate(frames):
        sc = make_scene(aos, w, h)
        if k:
            dev = upload(r, aos)
        img = r.draw(sc)
        assert ref["e"] == s + 40 * p
        assert_frame_equals_oracle(r, img, ref)
        if ref["e"] == 0:
            assert np.all(img[..., :3] == 0) and np.all(img[..., 3] == 255)
            assert np.all(r.debugRead(gs.BUF_RANGES) == 0)
    r.cleanup()


@pytest.mark.parametrize("sort,count", [(s, gs.GS_COUNT_AUTO) for s in ALL_SORTS] +
                         [(gs.GS_SORT_RADIX4, gs.GS_COUNT_PER_PASS), (gs.GS_SORT_RADIX4, gs.GS_COUNT_FED)])
def test_512_and_513_groups_in_a_frame(oracle_mod, sort, count):
    """E = 512 * 2048 (every reduce segment exactly one group, no ragged group) and one element more (groups_per_seg 2, a last
    group of one key, a second batch of row loads in the fed prologue) in the frame layouts: lists, ranges and pixels.  The
    longer frame first, then the shorter, then the longer again on the same context."""
    aos, w, h = groups_scene(oracle_mod)
    frames = groups_frames(oracle_mod)
    r = renderer(make_scene(aos, w, h), w, h, sort, count=count)
    assert r.sceneInfo().capacity == 1 << 21
    sc = make_scene(aos[:1], w, h)                                    # the camera only
    dev = upload(r, aos)
    z = float(aos[GROUPS_CULLED, 2])
    for e in (GROUPS_N, GROUPS_N - 1, GROUPS_N):
        dev[GROUPS_CULLED, 2] = z if e == GROUPS_N else -z
        upload(r, dev)
        img = r.draw(sc)
        assert_frame_equals_oracle(r, img, frames[e])
    r.cleanup()


@pytest.mark.parametrize("sort", [gs.GS_SORT_RADIX8, gs.GS_SORT_RADIX8_SPLAT_FIRST, gs.GS_SORT_RADIX4])
def test_4096_key_groups_in_a_frame(oracle_mod, sort):
    """A capacity of 2^24 selects the 4096-key groups of the 8-bit sorter: E = 9 * 4096, + 1, - 1 by value (tile, depth and id
    words, ranges, pixels), one context, the longest frame not last.  GS_SORT_RADIX4 on the same frames is the control."""
    aos, w, h = big_scene(oracle_mod)
    r = renderer(make_scene(aos, w, h), w, h, sort)
    assert r.sceneInfo().capacity == BIG_CAPACITY >= SORT8_SMALL_BELOW
    sc = make_scene(aos[:1], w, h)
    for e, ids, ref in big_frames(oracle_mod):
        culled = aos.copy()
        culled[ids, 2] = -culled[ids, 2]
        dev = upload(r, culled)
        img = r.draw(sc)
        assert ref["e"] == e
        assert_frame_equals_oracle(r, img, ref)
    r.cleanup()


@pytest.mark.parametrize("sort", ALL_SORTS)
def test_more_than_65535_tiles_every_sorter(oracle_mod, sort):
    """256 x 257 tiles, 52 sort bits, 32-bit tile words: designed runs in tiles t, t + 32,768 and t + 65,536 (a tile word cut to
    16 bits merges them) and two splats of 65,792 tiles each (a tile count cut to 16 bits is 256), under every sorter; then the
    band of rows 100 - 200 in 16-bit words on the same context, and the whole frame again."""
    aos, w, h, _ = wide_scene(oracle_mod)
    ref = wide_frame(oracle_mod)
    rb, re_ = WIDE_BAND
    band = wide_frame(oracle_mod, row_begin=rb, row_end=re_)
    sc = make_scene(aos, w, h)
    r = make_renderer(sc, w, h, sort=sort)
    info = r.sceneInfo()
    assert (info.tiles_x, info.tiles_y, info.capacity, info.num_sort_bits) == (WIDE_GW, WIDE_GH, WIDE_CAPACITY, 52)
    assert info.tile_word_bytes == 4
    assert_frame_equals_oracle(r, r.draw(sc), ref)
    r.setTileRows(rb, re_)
    assert r.sceneInfo().tile_word_bytes == 2
    img = r.draw(sc)
    assert_lists_equal_oracle(r, band)
    assert np.array_equal(img[rb * 16:re_ * 16], band["image"][rb * 16:re_ * 16])
    assert np.array_equal(img[rb * 16:re_ * 16], ref["image"][rb * 16:re_ * 16])
    r.setTileRows(0, WIDE_GH)
    assert r.sceneInfo().tile_word_bytes == 4
    assert_frame_equals_oracle(r, r.draw(sc), ref)
    r.cleanup()


@pytest.mark.parametrize("record_timings", [1, 0])
def test_count_auto_changes_its_mind(oracle_mod, record_timings):
    """GS_COUNT_AUTO on one context over the lengths of AUTO_FRAMES: a Count per pass, the hysteresis band entered from above
    (stays per pass), the first switch to fed counts, the band from below (stays fed, 1024 whole groups), 1025 groups fed, the
    switch back.  draw waits for its frame, so the length a frame goes by is the previous frame's; the expected mode of every
    frame comes from the rule restated in test_designed_lengths_cpu.auto_modes, the library is not asked.  Every frame: sorted
    tile, depth and id words and ranges; pixels on the frames on both sides of each switch.  With and without timers: different graphs are dropped and captured again."""
    import torch
    aos, w, h, frames = auto_frames(oracle_mod)
    modes = auto_modes(AUTO_FRAMES)
    assert {"fed", "per pass"} == set(modes) and modes[4:6] == ["per pass", "fed"] and modes[8:10] == ["fed", "per pass"]
    assert all(frames[e]["image"] is not None for e in AUTO_FRAMES[4:6] + AUTO_FRAMES[8:10])
    r = renderer(make_scene(aos, w, h), w, h, gs.GS_SORT_RADIX4, record_timings, gs.GS_COUNT_AUTO)
    assert (r.sceneInfo().num_gaussians, r.sceneInfo().capacity) == (AUTO_N, AUTO_CAPACITY)
    sc = make_scene(aos[:1], w, h)
    dev = torch.tensor(aos, device="cuda")
    z = dev[:, 2].clone()
    index = torch.arange(AUTO_N, device="cuda")
    for k, e in enumerate(AUTO_FRAMES):
        dev[:, 2] = torch.where(index < e, z, -z)
        upload(r, dev)
        img = r.draw(sc)
        ref = frames[e]
        assert ref["e"] == e, (k, modes[k])
        assert_lists_equal_oracle(r, ref)
        if ref["image"] is not None:                              # frames 5, 6 and 9, 10: both modes at either length
            assert np.array_equal(img, ref["image"]), (k, e, modes[k])
    r.cleanup()
