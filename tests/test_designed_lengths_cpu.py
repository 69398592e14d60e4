"""Designed list lengths: scenes whose WHOLE sort list has a chosen length E, and whose list of emitting splats has a chosen
length M, so that the radix kernels (vk3dgaussiansplatting_amd/csrc/gs_sort.hip, gs_sort8.hip) and the splat-first chain
(k_splat_list, k_sorted_sums, k_emit<true>) meet their group, wave, segment and block edges on purpose, in the narrow word
layouts only a frame uses.  tests/test_designed_runs_cpu.py designs the per-tile runs; this file designs the length of the list.
It owns the scenes and proves on the CPU oracle that they are what they claim; tests/test_designed_lengths_gpu.py runs the
sorters on them.

The building blocks (the tests below prove each on the oracle):
  single   a splat of about 0.3 px on a tile centre, position and scale multiplied by its view depth: exactly one element
  pad      a splat of 100 px (3000 px on the 4096 x 4112 frame) on the frame centre: one element in every tile
  culled   any record with z moved behind the camera: none
so s singles, p pads and c culled records give M = s + p emitting splats and E = s + tiles * p elements while N = s + p + c stays.

What the oracle found (the test prints it):
  short frames   160 x 64, N 6,200, capacity 65,536, 28 frames; E (M where it differs), in the order they are drawn:
                 6145 0 6144 1025 4097 1024 4096 1023 4096(3706) 491(257) 4095 490(256) 2438(2048) 257 2051 256 2050 255 2049 65
                 2049(1854) 64 2048 63 2048(1853) 2 2047 1
  512 | 513      160 x 64, N 1,048,577, capacity 2^21: E 1,048,576 (one record culled) and 1,048,577; runs 25,888 - 26,480 per tile
  4096-key       1920 x 1080, N 36,868 on 300 tiles, capacity 2^24: E 36,864, 36,865, 36,863 (9 groups of 4096 -1, +0, +1)
  > 65,535 tiles 4096 x 4112 (256 x 257 tiles, 52 sort bits), N 18,661, capacity 2^27: E 150,243 = 18,659 singles + 2 * 65,792;
                 17 designed runs (+ 2 each from the pads); the band of tile rows 100 - 200 has 25,600 tiles and 6 of the runs
                 (65,791 = 65,536 + 255 is one tile, so 32,767 is added to the tiles of the issue for the 17th run)
  AUTO           160 x 64, N 2,100,000, capacity 2^22, runs 51,990 - 53,080 per tile: records E and later culled, E as
                 AUTO_FRAMES has it"""
import os
import re

import numpy as np

from conftest import ROOT, default_camera
from test_backward_cpu import screen_splat
from test_designed_runs_cpu import range_lengths

# ---- the kernel constants the lengths are designed around, restated (csrc/gs_internal.h) ---------------------------------
K_SORT_TILE = 2048                  # kSortTile: keys per group of the 4-bit sorter
K_SORT8_TILE_SMALL = 2048           # kSort8TileSmall: keys per group of the 8-bit sorter below ...
K_SORT8_TILE = 4096                 # kSort8Tile: ... and from ...
SORT8_SMALL_BELOW = 12_000_000      # GS_SORT8_SMALL_BELOW: ... this capacity
K_SEGMENTS = 512                    # kSegments: reduce segments; groups_per_seg = ceil(groups / kSegments)
FED_MAX_GROUPS = 1024               # GS_FED_MAX_GROUPS: GS_COUNT_AUTO feeds counts up to this many groups
K_PROJ_THREADS = 256                # kProjThreads: splats per project / emit workgroup
EMIT_SLICE = 4096                   # GS_EMIT_SLICE: output elements per k_emit workgroup (rounds of 1024)
RESTATED = dict(kSortTile=K_SORT_TILE, kSort8TileSmall=K_SORT8_TILE_SMALL, kSort8Tile=K_SORT8_TILE,
                GS_SORT8_SMALL_BELOW=SORT8_SMALL_BELOW, kSegments=K_SEGMENTS, GS_FED_MAX_GROUPS=FED_MAX_GROUPS,
                kProjThreads=K_PROJ_THREADS, GS_EMIT_SLICE=EMIT_SLICE)

OPACITY = 0.05
SMALL_W, SMALL_H, SMALL_TILES = 160, 64, 40


def header_constants():
    """Every `constexpr <type> name = expr[, name = expr];` and `#define NAME value` of gs_internal.h whose value is a product,
    shift or sum of integers and of names defined before it."""
    text = open(os.path.join(ROOT, "vk3dgaussiansplatting_amd", "csrc", "gs_internal.h")).read()
    found = []
    for m in re.finditer(r"^#define[ \t]+(\w+)[ \t]+(\d+)|^constexpr[ \t]+\w+[ \t]+([^;]+);", text, re.M):
        if m.group(1):
            found.append((m.start(), m.group(1), m.group(2)))
        else:
            for part in m.group(3).split(","):
                name, _, expr = part.partition("=")
                found.append((m.start(), name.strip(), expr.strip()))
    values = {}
    for _, name, expr in sorted(found):
        expr = re.sub(r"\b(\d+)[uU]?[lL]*\b", r"\1", expr)
        expr = re.sub(r"\([a-z0-9_]+\)", "", expr)                                   # casts
        expr = re.sub(r"[A-Za-z_]\w*", lambda t: str(values.get(t.group(0), "?")), expr)
        if expr and re.fullmatch(r"[0-9 *+()<-]+", expr):
            try:
                values[name] = int(eval(expr))                                       # digits and operators only
            except SyntaxError:
                pass
    return values


def test_restated_constants_agree_with_the_header():
    """A retune of a group size, the segment count or a threshold fails here instead of moving the scenes off their edges."""
    values = header_constants()
    for name, want in RESTATED.items():
        assert values.get(name) == want, (name, values.get(name), want)
    assert values["kFedMaxGroups"] == FED_MAX_GROUPS and values["kSort8SmallBelow"] == SORT8_SMALL_BELOW
    assert values["kEmitSlice"] == EMIT_SLICE and EMIT_SLICE % 1024 == 0


# ---- the building blocks --------------------------------------------------------------------------------------------------
def ceil_pow2(x):
    return 1 << (int(x) - 1).bit_length()


def tile_units(oracle, w, h, tiles):
    """One unit record (view depth 1) per tile: a 0.3 px splat on the tile's centre."""
    gw = (w + 15) // 16
    return np.stack([screen_splat(oracle, w, h, (t % gw) * 16 + 8.0, (t // gw) * 16 + 8.0, 1.0, 0.3, OPACITY)
                     for t in tiles]).astype(np.float32)


def at_depths(units, z, rng):
    """The unit records moved to view depths z (float32): position and scale multiplied, colours drawn."""
    z = np.asarray(z, np.float32).astype(np.float64)[:, None]
    rec = np.array(units, np.float32)
    rec[:, 0:3] = units[:, 0:3].astype(np.float64) * z
    rec[:, 4:7] = units[:, 4:7].astype(np.float64) * z
    rec[:, 12:15] = rng.uniform(-1.0, 1.0, (rec.shape[0], 3))
    return rec


def wide_depths(rng, k):
    return np.exp(rng.uniform(np.log(0.1001), np.log(99.99), k)).astype(np.float32)


def cull(aos, ids):
    """The records `ids` moved behind the camera (a copy)."""
    out = aos.copy()
    out[ids, 2] = -out[ids, 2]
    return out


def oracle_frame(oracle, aos, w, h, image=True, **rows):
    """The oracle's frame as tests/test_parity_gpu.py::assert_frame_equals_oracle takes it; only the E listed elements are
    sorted (a capacity of 2^27 is not copied), image = False stops after the ranges."""
    view, proj, pos = default_camera(oracle, w, h)
    p = oracle.make_params(w, h, view, proj, pos, **rows)
    th = oracle.host_threads(16)
    s1 = oracle.init_sort_list(p, aos, threads=th)
    e = min(s1["counter"], s1["capacity"])
    t, d, i = oracle.sort_stable(s1["tile"][:e], s1["depth"][:e], s1["id"][:e], e, threads=th)
    gw, gh = oracle.grid(w, h)
    ranges = oracle.find_ranges(t, e, gw * gh)
    img = oracle.render(p, aos, s1["color"], s1["cov"], i, ranges, threads=th) if image else None
    return dict(stage1=s1, e=e, tile=t, depth=d, id=i, ranges=ranges, image=img)


def emitting(ref):
    """M: the splats with at least one element."""
    return int(np.unique(ref["id"][:ref["e"]]).size)


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- A: short lists on one context ------------------------------------------------------------------------------------------
SHORT_N = 6200
SHORT_SINGLES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 2050, 2051, 4095, 4096, 4097, 6144, 6145)
# (singles, pads): M = s + p, E = s + 40 p
SHORT_PADDED = ((2038, 10),          # M = 2048 (eight whole project blocks), E = 2438
                (3696, 10),          # E = 4096 (two whole groups, four whole emit rounds), M = 3706
                (250, 6), (251, 6),  # M = 256 | 257 (one project block | one splat more), E = 490 | 491 inside a group
                (1848, 5), (1849, 5))  # E = 2048 | 2049 (one whole group | a group of one key), M = 1853 | 1854 off every edge
SHORT_CAPACITY = 65536


def short_specs():
    return [(s, 0) for s in SHORT_SINGLES] + list(SHORT_PADDED)


def short_sequence():
    """The frames in the order one context draws them: the longer half descending, the shorter half descending between its frames,
    the empty frame second -- every short frame directly behind a longer one, 0 behind the longest and in front of the next."""
    spec = sorted((sp for sp in short_specs() if sp != (0, 0)), key=lambda sp: (-(sp[0] + SMALL_TILES * sp[1]), sp[1]))
    half = (len(spec) + 1) // 2
    long_, short = spec[:half], spec[half:]
    seq = [long_[0], (0, 0)]
    for k in range(1, half):
        seq.append(long_[k])
        if k - 1 < len(short):
            seq.append(short[k - 1])
    return seq


def short_scene(oracle, s, p):
    """(aos, w, h): s singles, p pads and SHORT_N - s - p culled records, shuffled in record order."""
    rng = np.random.default_rng(1000 * s + p)
    units = cached("small_units", lambda: tile_units(oracle, SMALL_W, SMALL_H, range(SMALL_TILES)))
    pad = screen_splat(oracle, SMALL_W, SMALL_H, SMALL_W / 2, SMALL_H / 2, 1.0, 100.0, 0.01).astype(np.float32)
    n = SHORT_N
    rec = at_depths(units[rng.integers(0, SMALL_TILES, n)], wide_depths(rng, n), rng)
    slots = rng.permutation(n)
    pads = slots[s:s + p]
    rec[pads] = at_depths(np.tile(pad, (p, 1)), wide_depths(rng, p), rng)
    return cull(rec, slots[s + p:]), SMALL_W, SMALL_H


def short_frames(oracle):
    """[(s, p, aos, oracle frame)] in short_sequence() order, once per session."""
    def make():
        out = []
        for s, p in short_sequence():
            aos, w, h = short_scene(oracle, s, p)
            out.append((s, p, aos, oracle_frame(oracle, aos, w, h)))
        return out
    return cached("short", make)


# ---- B: 512 | 513 groups ----------------------------------------------------------------------------------------------------
GROUPS_N = K_SEGMENTS * K_SORT_TILE + 1          # 1,048,577
GROUPS_CULLED = 777_777                          # the record the shorter frame culls


def groups_scene(oracle):
    def make():
        rng = np.random.default_rng(512)
        units = cached("small_units", lambda: tile_units(oracle, SMALL_W, SMALL_H, range(SMALL_TILES)))
        return at_depths(units[rng.integers(0, SMALL_TILES, GROUPS_N)], wide_depths(rng, GROUPS_N), rng)
    return cached("groups_aos", make), SMALL_W, SMALL_H


def groups_frames(oracle, image=True):
    """{E: oracle frame} for E = 512 * 2048 (GROUPS_CULLED behind the camera) and 512 * 2048 + 1."""
    def make():
        aos, w, h = groups_scene(oracle)
        return {GROUPS_N - 1: oracle_frame(oracle, cull(aos, [GROUPS_CULLED]), w, h, image),
                GROUPS_N: oracle_frame(oracle, aos, w, h, image)}
    return cached(("groups", image), make)


# ---- C: the 4096-key groups of the 8-bit sorter, in a frame ---------------------------------------------------------------------
BIG_W, BIG_H = 1920, 1080
BIG_N = 36_868
BIG_GROUPS = 9
BIG_LENGTHS = (BIG_GROUPS * K_SORT8_TILE, BIG_GROUPS * K_SORT8_TILE + 1, BIG_GROUPS * K_SORT8_TILE - 1)   # the longest is not last
BIG_CULL_ORDER = (31_000, 7, 20_481, 4_096, 36_867)      # a frame of E elements culls the first BIG_N - E of these
BIG_CAPACITY = 1 << 24


def big_scene(oracle):
    def make():
        rng = np.random.default_rng(4096)
        gw = BIG_W // 16
        tiles = rng.choice(gw * (BIG_H // 16), 300, replace=False)           # whole tile rows only
        units = tile_units(oracle, BIG_W, BIG_H, tiles)
        return at_depths(units[rng.integers(0, 300, BIG_N)], wide_depths(rng, BIG_N), rng)
    return cached("big_aos", make), BIG_W, BIG_H


def big_frames(oracle, image=True):
    """[(E, culled ids, oracle frame)] in BIG_LENGTHS order."""
    def make():
        aos, w, h = big_scene(oracle)
        out = []
        for e in BIG_LENGTHS:
            ids = list(BIG_CULL_ORDER[:BIG_N - e])
            out.append((e, ids, oracle_frame(oracle, cull(aos, ids), w, h, image)))
        return out
    return cached(("big", image), make)


# ---- D: more than 65,535 tiles --------------------------------------------------------------------------------------------------
WIDE_W, WIDE_H, WIDE_GW, WIDE_GH = 4096, 4112, 256, 257
WIDE_RUNS = (1, 2, 63, 64, 65, 255, 256, 257, 300, 4095, 4096, 4097, 1000, 5, 7, 2049, 2047)
WIDE_COLUMNS = (0, 1, 63, 128, 255)
WIDE_BAND = (100, 200)
WIDE_PADS = 2
WIDE_CAPACITY = 1 << 27


def wide_tiles():
    """Tiles c, 32,768 + c and 65,536 + c (a tile word cut to 16 bits merges the first and the last, one cut to 15 all three),
    and tiles 32,767 and 65,535, whose successors they are.  65,791, the last tile, is 65,536 + 255."""
    tiles = [base + c for c in WIDE_COLUMNS for base in (0, 32768, 65536)] + [65535, 32767]
    assert len(set(tiles)) == len(tiles) == len(WIDE_RUNS) and 65791 in tiles
    return tiles


def wide_scene(oracle):
    """(aos, w, h, lengths): the designed runs of singles and two pads that touch all 65,792 tiles, shuffled."""
    def make():
        rng = np.random.default_rng(65536)
        tiles = wide_tiles()
        units = tile_units(oracle, WIDE_W, WIDE_H, tiles)
        which = np.repeat(np.arange(len(tiles)), WIDE_RUNS)
        rec = at_depths(units[which], wide_depths(rng, which.size), rng)
        pad = screen_splat(oracle, WIDE_W, WIDE_H, WIDE_W / 2, WIDE_H / 2, 1.0, 3000.0, 0.01).astype(np.float32)
        pads = at_depths(np.tile(pad, (WIDE_PADS, 1)), np.float32([3.0, 41.0]), rng)
        aos = np.concatenate([rec, pads])[rng.permutation(which.size + WIDE_PADS)]
        lengths = np.full(WIDE_GW * WIDE_GH, WIDE_PADS, np.int64)
        lengths[tiles] += WIDE_RUNS
        return aos, lengths
    aos, lengths = cached("wide_aos", make)
    return aos, WIDE_W, WIDE_H, lengths


def wide_frame(oracle, image=True, **rows):
    aos, w, h, _ = wide_scene(oracle)
    return cached(("wide", image) + tuple(sorted(rows.items())), lambda: oracle_frame(oracle, aos, w, h, image, **rows))


# ---- E: GS_COUNT_AUTO changing its mind ---------------------------------------------------------------------------------------
AUTO_N = 2_100_000
AUTO_CAPACITY = 1 << 22
FED_STAYS_UP_TO = FED_MAX_GROUPS * K_SORT_TILE                     # 2,097,152
FED_STARTS_UP_TO = FED_STAYS_UP_TO - FED_STAYS_UP_TO // 16         # 1,966,080
AUTO_FRAMES = (2_100_000, 2_100_000, 2_000_000, 2_000_000, FED_STARTS_UP_TO, FED_STARTS_UP_TO, FED_STAYS_UP_TO, FED_STAYS_UP_TO,
               FED_STAYS_UP_TO + 1, FED_STAYS_UP_TO + 1, FED_STARTS_UP_TO + 1, FED_STARTS_UP_TO + 1)


AUTO_PIXELS = (FED_STARTS_UP_TO, FED_STAYS_UP_TO + 1)      # the lengths on both sides of each switch: pixels too (6 s of oracle each)


def auto_modes(lengths):
    """enqueue_frame's rule, restated: a frame sorts with fed counts iff a previous frame's length is known and is at most
    FED_STAYS_UP_TO when the last frame was fed, at most FED_STARTS_UP_TO when it was not."""
    modes, fed, prev = [], False, None
    for e in lengths:
        fed = prev is not None and prev <= (FED_STAYS_UP_TO if fed else FED_STARTS_UP_TO)
        modes.append("fed" if fed else "per pass")
        prev = e
    return modes


def auto_scene(oracle, n=AUTO_N):
    def make():
        rng = np.random.default_rng(n)
        units = cached("small_units", lambda: tile_units(oracle, SMALL_W, SMALL_H, range(SMALL_TILES)))
        return at_depths(units[rng.integers(0, SMALL_TILES, n)], wide_depths(rng, n), rng)
    return cached(("auto_aos", n), make), SMALL_W, SMALL_H


def tail_culled(full, aos, e, oracle, w, h, image=True):
    """The frame of `aos` with the records e and later behind the camera, from the whole frame's sorted list: an element's key
    does not depend on the other records and the sort is stable in record order, so the shorter frame's list is the whole one
    without the culled ids (test_removing_culled_ids_gives_the_shorter_frame proves it on the oracle)."""
    keep = full["id"][:full["e"]] < e
    t, d, i = full["tile"][:full["e"]][keep], full["depth"][:full["e"]][keep], full["id"][:full["e"]][keep]
    gw, gh = oracle.grid(w, h)
    ranges = oracle.find_ranges(t, t.size, gw * gh)
    img = None
    if image:
        view, proj, pos = default_camera(oracle, w, h)
        p = oracle.make_params(w, h, view, proj, pos)
        s1 = full["stage1"]
        img = oracle.render(p, aos, s1["color"], s1["cov"], i, ranges, threads=oracle.host_threads(16))
    return dict(e=int(t.size), tile=t, depth=d, id=i, ranges=ranges, image=img)


def auto_frames(oracle):
    """(aos, w, h, {E: frame}) for the lengths of AUTO_FRAMES; one run of the oracle, the shorter frames by tail_culled; image
    None but at the lengths of AUTO_PIXELS."""
    def make():
        aos, w, h = auto_scene(oracle)
        full = oracle_frame(oracle, aos, w, h, image=False)
        return {e: tail_culled(full, aos, e, oracle, w, h, image=e in AUTO_PIXELS) for e in sorted(set(AUTO_FRAMES))}
    aos, w, h = auto_scene(oracle)
    return aos, w, h, cached("auto", make)


# ---- the proofs ---------------------------------------------------------------------------------------------------------------
def check_lengths(ref, e, m, capacity):
    s1 = ref["stage1"]
    assert s1["counter"] == ref["e"] == e < capacity == s1["capacity"], (s1["counter"], ref["e"], e, s1["capacity"])
    assert emitting(ref) == m, (emitting(ref), m)
    assert range_lengths(ref).sum() == e


def groups(e, tile=K_SORT_TILE):
    return -(-e // tile)


def test_short_frames_have_the_claimed_lengths_and_order(oracle_mod):
    """Section A: E, M, counter and capacity of every short frame on the oracle; the lengths cover the lanes, the 256-splat
    blocks, the 1024-element emit round, one to three whole groups, a group of one key and every M mod 4; M differs from E with
    either on an edge and the other off it; and the order of the frames is the designed one."""
    frames = short_frames(oracle_mod)
    assert [(s, p) for s, p, _, _ in frames] == short_sequence() and len(frames) == len(short_specs()) == len(set(short_specs()))
    lens = []
    for s, p, aos, ref in frames:
        assert aos.shape[0] == SHORT_N
        check_lengths(ref, s + SMALL_TILES * p, s + p, SHORT_CAPACITY)
        assert ref["stage1"]["capacity"] == ceil_pow2(SHORT_N + 1024 * SMALL_TILES)
        if p:
            assert range_lengths(ref).min() >= p                                 # a pad is in every tile
        lens.append((ref["e"], emitting(ref)))
    print("\nshort frames, E(M):", " ".join(f"{e}({m})" if m != e else str(e) for e, m in lens))
    es = [e for e, _ in lens]
    have = {e for e, m in lens if e == m}
    for edge in (64, 256, 1024, 2048, 4096):                                       # lanes, project block, emit round, groups
        assert {edge - 1, edge, edge + 1} <= have, edge
    assert {0, 1, 2, 3 * K_SORT_TILE, 3 * K_SORT_TILE + 1} <= have and {m % 4 for m in have if m > 2048} == {0, 1, 2, 3}
    assert all(groups(e) <= 4 for e in es) and {groups(e) for e in es} == {0, 1, 2, 3, 4}
    off_edge = lambda v: all(v % q not in (0, 1, q - 1) for q in (64, 256, 1024, 2048))
    by_m = {m: e for e, m in lens if m != e}
    by_e = {e: m for e, m in lens if m != e}
    assert by_m[2048] == 2438 and by_e[4096] == 3706                               # the two rows measured in the issue
    assert off_edge(by_m[256]) and off_edge(by_m[257]) and groups(by_m[256]) == groups(by_m[257]) == 1
    assert off_edge(by_e[2048]) and off_edge(by_e[2049]) and by_e[2048] % 4 and by_e[2049] % 4
    # the order: not ascending; the empty frame directly behind a long one and in front of one; every frame but the first has
    # a longer one somewhere before it (stale sorted data beyond its E in both halves); every short one directly before it
    assert es[1] == 0 and es[0] >= 3 * K_SORT_TILE and es[2] >= 3 * K_SORT_TILE
    assert all(max(es[:k]) > es[k] for k in range(1, len(es)))
    assert all(es[k - 1] > es[k] for k in range(1, len(es)) if es[k] < 2047)
    assert sum(es[k] > es[k - 1] for k in range(1, len(es))) >= 12
    empty = frames[1][3]
    assert np.all(empty["image"][..., :3] == 0) and np.all(empty["image"][..., 3] == 255) and np.all(empty["ranges"] == 0)


def test_group_edge_frames_have_the_claimed_lengths(oracle_mod):
    """Sections B and C: 512 whole groups of 2048 and one key more (groups_per_seg 1 -> 2) under a capacity of 2^21; nine
    groups of 4096 keys minus one, exactly, plus one, under a capacity that selects the 4096-key groups of the 8-bit sorter."""
    frames = groups_frames(oracle_mod, image=False)
    assert sorted(frames) == [K_SEGMENTS * K_SORT_TILE, K_SEGMENTS * K_SORT_TILE + 1]
    for e, ref in frames.items():
        check_lengths(ref, e, e, 1 << 21)
        assert ref["stage1"]["capacity"] < SORT8_SMALL_BELOW
        lens = range_lengths(ref)
        print(f"\n{groups(e)} groups: E {e}, runs {lens.min()} - {lens.max()} per tile")
        assert lens.min() > 20_000
    assert [-(-groups(e) // K_SEGMENTS) for e in sorted(frames)] == [1, 2]
    assert GROUPS_CULLED not in frames[GROUPS_N - 1]["id"] and GROUPS_CULLED in frames[GROUPS_N]["id"]
    big = big_frames(oracle_mod, image=False)
    assert [e for e, _, _ in big] == [36864, 36865, 36863] and max(BIG_LENGTHS) != BIG_LENGTHS[-1]
    for e, ids, ref in big:
        check_lengths(ref, e, e, BIG_CAPACITY)
        assert len(ids) == BIG_N - e and not np.isin(ids, ref["id"]).any()
        assert ref["stage1"]["capacity"] == ceil_pow2(BIG_N + 1024 * 8160) >= SORT8_SMALL_BELOW
        lens = range_lengths(ref)
        print(f"4096-key groups: E {e} = {BIG_GROUPS} * {K_SORT8_TILE} {e - BIG_GROUPS * K_SORT8_TILE:+d}, "
              f"{(lens > 0).sum()} tiles, runs up to {lens.max()}")
        assert (lens > 0).sum() == 300
    assert [groups(e, K_SORT8_TILE) for e, _, _ in big] == [BIG_GROUPS, BIG_GROUPS + 1, BIG_GROUPS]
    assert BIG_N >= 36_865                                                          # below, the capacity is 2^23


def test_wide_grid_scene_is_what_it_claims(oracle_mod):
    """Section D: more than 65,535 tiles (32-bit tile words in a frame, 52 sort bits); every designed tile holds its run plus the
    two pads, every other tile the two pads; tiles that differ by 32,768 or 65,536 hold runs of different lengths, so a tile
    word cut to 16 bits merges runs; each pad has more tiles than 16 bits count.  The band of rows 100 - 200 fits 16 bits."""
    aos, w, h, lengths = wide_scene(oracle_mod)
    ref = wide_frame(oracle_mod, image=False)
    tiles = WIDE_GW * WIDE_GH
    assert oracle_mod.grid(w, h) == (WIDE_GW, WIDE_GH) and tiles == 65792 > 65535 and oracle_mod.num_sort_bits(tiles) == 52
    singles = sum(WIDE_RUNS)
    check_lengths(ref, singles + WIDE_PADS * tiles, singles + WIDE_PADS, WIDE_CAPACITY)
    assert aos.shape[0] == singles + WIDE_PADS and ref["stage1"]["capacity"] == ceil_pow2(aos.shape[0] + 1024 * tiles)
    assert np.array_equal(range_lengths(ref), lengths)
    per_splat = np.bincount(ref["id"], minlength=aos.shape[0])
    assert sorted(per_splat)[-WIDE_PADS:] == [tiles] * WIDE_PADS and tiles & 0xFFFF == 256
    for c in WIDE_COLUMNS:
        assert len({int(lengths[c]), int(lengths[32768 + c]), int(lengths[65536 + c])}) == 3
    assert lengths[65535] > WIDE_PADS and lengths[65791] > WIDE_PADS and lengths[32767] > WIDE_PADS
    assert ref["tile"].max() == 65791
    # what a sorter that kept 16 (or 15) bits of the tile word would leave: another order of the ids
    s1, e = ref["stage1"], ref["e"]
    for bits in (16, 15):
        cut = ((s1["tile"][:e].astype(np.uint64) & np.uint64((1 << bits) - 1)) << np.uint64(32)) | s1["depth"][:e]
        assert not np.array_equal(s1["id"][:e][np.argsort(cut, kind="stable")], ref["id"]), bits
    rb, re_ = WIDE_BAND
    band = wide_frame(oracle_mod, image=False, row_begin=rb, row_end=re_)
    in_band = lengths[rb * WIDE_GW:re_ * WIDE_GW]
    assert (re_ - rb) * WIDE_GW == 25600 <= 65535
    assert band["e"] == in_band.sum() and np.array_equal(range_lengths(band)[rb * WIDE_GW:re_ * WIDE_GW], in_band)
    print(f"\n{tiles} tiles: N {aos.shape[0]}, E {ref['e']} = {singles} + {WIDE_PADS} * {tiles}; runs",
          *[int(lengths[t]) for t in wide_tiles()], f"; band E {band['e']}, {(in_band > WIDE_PADS).sum()} designed runs in it")
    assert (in_band > WIDE_PADS).sum() >= 5


def test_auto_sequence_is_what_it_claims(oracle_mod):
    """Section E: the restated rule gives the designed mode for every frame -- both modes, both switches, the hysteresis band
    entered from above (per pass) and from below (fed), a fed frame of exactly 1024 groups and one of 1025; every record of the
    scene emits exactly one element, and none once it is behind the camera, so culling the records E and later gives E."""
    modes = auto_modes(AUTO_FRAMES)
    pp, fed = "per pass", "fed"
    assert modes == [pp, pp, pp, pp, pp, fed, fed, fed, fed, pp, pp, pp]
    switches = [(a, b) for a, b in zip(modes, modes[1:]) if a != b]
    assert switches == [(pp, fed), (fed, pp)]
    assert (FED_STAYS_UP_TO, FED_STARTS_UP_TO) == (2_097_152, 1_966_080)
    assert all(FED_STARTS_UP_TO < e <= FED_STAYS_UP_TO and m == pp for e, m in zip(AUTO_FRAMES[2:4], modes[2:4]))
    assert all(FED_STARTS_UP_TO < e <= FED_STAYS_UP_TO and m == fed for e, m in zip(AUTO_FRAMES[6:8], modes[6:8]))
    assert (groups(AUTO_FRAMES[7]), groups(AUTO_FRAMES[8]), modes[8]) == (FED_MAX_GROUPS, FED_MAX_GROUPS + 1, fed)
    aos, w, h = auto_scene(oracle_mod)
    view, proj, pos = default_camera(oracle_mod, w, h)
    p = oracle_mod.make_params(w, h, view, proj, pos)
    th = oracle_mod.host_threads(16)
    s1 = oracle_mod.init_sort_list(p, aos, threads=th, want_splats=False)
    assert s1["counter"] == AUTO_N == max(AUTO_FRAMES) < s1["capacity"] == AUTO_CAPACITY == ceil_pow2(AUTO_N + 1024 * SMALL_TILES)
    assert np.array_equal(s1["id"][:AUTO_N], np.arange(AUTO_N))                     # one element each, in record order
    lens = np.bincount(s1["tile"][:AUTO_N], minlength=SMALL_TILES)
    print(f"\nAUTO: N {AUTO_N}, runs {lens.min()} - {lens.max()} per tile; modes", list(zip(AUTO_FRAMES, modes)))
    gone = oracle_mod.init_sort_list(p, cull(aos, np.arange(AUTO_N)), threads=th, want_splats=False)
    assert gone["counter"] == 0


def test_removing_culled_ids_gives_the_shorter_frame(oracle_mod):
    """tail_culled against the oracle run on the culled records themselves, on the AUTO scene's generator at 1/35 of its size
    and the AUTO lengths scaled alike: sorted list, ranges and pixels."""
    n = 60_000
    aos, w, h = auto_scene(oracle_mod, n)
    full = oracle_frame(oracle_mod, aos, w, h, image=False)
    assert full["e"] == n
    for e in sorted({n * v // AUTO_N for v in AUTO_FRAMES} | {0, 1, n}):
        culled = cull(aos, np.arange(e, n))
        want = oracle_frame(oracle_mod, culled, w, h)
        got = tail_culled(full, aos, e, oracle_mod, w, h)
        assert want["e"] == got["e"] == e
        for key in ("tile", "depth", "id", "ranges", "image"):
            assert np.array_equal(want[key][:e] if key in ("tile", "depth", "id") else want[key], got[key]), (e, key)
        # and the pixels do not depend on which of the two record arrays the oracle blends from
        assert np.array_equal(tail_culled(full, culled, e, oracle_mod, w, h)["image"], want["image"])
