"""Designed tile runs: scenes whose per-tile list lengths and depth-key statistics are chosen, not drawn, so that every
size class of GS_SORT_TILE_BUCKET (vk3dgaussiansplatting_amd/csrc/gs_tilesort.hip) is met on both sides of each of its
edges, with keys that make its passes move or stand still by design.  This file owns the scenes and proves on the CPU
oracle that they are what they claim; tests/test_designed_runs_gpu.py runs the sorters on them.

A splat of about 0.3 px on a tile centre has a 3-sigma radius of 2 px and touches that tile only, so k of them give the
tile a run of exactly k, and the view depth of each chooses its key (a float32 in [0, 1] times 2^32: 24 significant bits).

What the oracle found for these scenes (test_designed_scenes_are_what_they_claim prints it; 35 runs on a 160 x 64 frame of
10 x 4 tiles, 131,641 splats, capacity 262,144, 5 tiles empty):
  class       runs  designed lengths
  untouched      1  1 (and the empty tiles)
  S1            14  2 3 63 64 65 255 256 257 512 513 768 769 1023 1024
  S2             5  1025 1536 1537 2047 2048
  S3             5  2049 2560 2561 4095 4096
  chunked        6  4097 8191 8192 8193 9983 9984
  global         4  9985 12288 12289 13001
Non-constant 4-bit digits of the depth keys, the number of moving passes of a chunked or global run (odd: the result ends in
the alternate image / half), per pattern over the six chunked and the four global runs:
  equal 0 | near 6 | far 6 | far_odd 7 | beyond 8 | wide 8 | descending 8 | mixed: chunked 8 8 8 0 6 6, global 7 8 8 8
so far_odd (and one global run of mixed) gives the odd outcome and every other pattern the even one.  Non-constant bytes
(the moving 8-bit passes of S1-S3) of the S3 runs: equal 0, near 3, far 3, far_odd 4, beyond 4, wide 4, descending 4."""
import numpy as np

from conftest import default_camera
from test_backward_cpu import screen_splat

# ---- the routing of gs_tilesort.hip, restated (TS_KERNELS and k_tile_sort_global there) ------------------------------
# a kernel takes the runs with NMIN < n <= NMAX; nothing takes n <= 1; k_tile_sort_global takes n > kTsBigMax
CLASSES = (("untouched", 0, 1), ("S1", 2, 1024), ("S2", 1025, 2048), ("S3", 2049, 4096), ("chunked", 4097, 9984),
           ("global", 9985, 1 << 31))
BIG_CLASSES = ("S3", "chunked", "global")
# the edges inside the classes: 64 lanes; the keys one wave holds in a single-chunk pass (ROUNDS * 64: 256 in S1, 512 in S2
# and S3); the 4096-key chunk of the chunked passes (1024 threads * kTsRounds)
LENGTHS = (1, 2, 3, 63, 64, 65,
           255, 256, 257, 512, 513, 768, 769,
           1023, 1024, 1025, 1536, 1537,
           2047, 2048, 2049, 2560, 2561, 4095, 4096, 4097,
           8191, 8192, 8193,
           9983, 9984, 9985,
           12288, 12289, 13001)
BASE_PATTERNS = ("equal", "near", "far", "far_odd", "beyond", "wide", "descending")
PATTERNS = BASE_PATTERNS + ("mixed",)
GRID_W, GRID_H = 10, 4                      # 40 tiles for 35 runs: five stay empty
OPACITY = 0.05


def size_class(n):
    return next(name for name, lo, hi in CLASSES if lo <= n <= hi) if n else "untouched"


def run_tiles():
    """Tile of the j-th run (LENGTHS is ascending): down the columns, so consecutive lengths lie in consecutive tile rows and
    each of S3, chunked and global has a run in every one of the four rows."""
    return [(j % GRID_H) * GRID_W + j // GRID_H for j in range(len(LENGTHS))]


def run_patterns(pattern):
    """Base pattern of the j-th run: the frame's own, or in `mixed` the base patterns dealt round-robin over the runs."""
    return [BASE_PATTERNS[j % len(BASE_PATTERNS)] if pattern == "mixed" else pattern for j in range(len(LENGTHS))]


def _depths(base, j, k, rng):
    """View depths of a run of k splats in ascending record index; key = (z - 0.1) / 99.9 * 2^32, saturating at z >= 100."""
    if base == "equal":
        return np.full(k, 3.0 + 0.37 * j)
    if base == "near":                       # (z - 0.1) / 99.9 < 2^-9: keys below 2^23, every bit below that in use
        return rng.uniform(0.1001, 0.29, k)
    if base == "far":                        # normalised depth in [0.5, 1): a float32 there is a multiple of 2^-24, low byte 0
        return rng.uniform(50.1, 99.99, k)
    if base == "far_odd":                    # also [0.25, 0.5): multiples of 2^-25, the low byte is 0x00 or 0x80
        return rng.uniform(30.0, 99.99, k)
    if base == "beyond":                     # half past the far plane (no far cull: the key saturates), half in front
        z = rng.uniform(0.2, 99.0, k)
        z[rng.permutation(k)[:(k + 1) // 2]] = rng.uniform(100.5, 5000.0, (k + 1) // 2)
        return z
    if base == "wide":
        return np.exp(rng.uniform(np.log(0.1001), np.log(99.99), k))
    if base == "descending":                 # emission order is ascending record index: the run arrives back to front
        return np.linspace(99.0, 0.2, k)
    raise ValueError(base)


def designed_runs(oracle, pattern, seed=20):
    """(aos, w, h, lengths): lengths[t] small splats on the centre of tile t (0 for the tiles left empty), records shuffled, so
    a tile's splat indices are neither contiguous nor in any order but the ascending one the emission gives them."""
    w, h = GRID_W * 16, GRID_H * 16
    rng = np.random.default_rng(seed)
    n = sum(LENGTHS)
    slots = rng.permutation(n)
    aos = np.zeros((n, 84), np.float32)
    lengths = np.zeros(GRID_W * GRID_H, np.int64)
    off = 0
    for j, (k, tile, base) in enumerate(zip(LENGTHS, run_tiles(), run_patterns(pattern))):
        ids = np.sort(slots[off:off + k])
        off += k
        lengths[tile] = k
        unit = screen_splat(oracle, w, h, (tile % GRID_W) * 16 + 8.0, (tile // GRID_W) * 16 + 8.0, 1.0, 0.3, OPACITY)
        z = _depths(base, j, k, rng).astype(np.float32).astype(np.float64)
        rec = np.tile(unit, (k, 1))
        rec[:, 0:3] = unit[0:3].astype(np.float64) * z[:, None]         # position and size scale with the view depth
        rec[:, 4:7] = unit[4:7].astype(np.float64) * z[:, None]
        rec[:, 12:15] = rng.uniform(-1.0, 1.0, (k, 3))                  # colours: the pixels depend on the order
        aos[ids] = rec
    return aos, w, h, lengths


_SORTED = {}


def sorted_list(oracle, pattern):
    """The oracle's stage 1, stable sort and ranges of a pattern's frame, once per session: (aos, w, h, lengths, dict)."""
    if pattern not in _SORTED:
        aos, w, h, lengths = designed_runs(oracle, pattern)
        view, proj, pos = default_camera(oracle, w, h)
        p = oracle.make_params(w, h, view, proj, pos)
        s1 = oracle.init_sort_list(p, aos)
        e = min(s1["counter"], s1["capacity"])
        t, d, i = oracle.sort_stable(s1["tile"], s1["depth"], s1["id"], e)
        ranges = oracle.find_ranges(t, e, GRID_W * GRID_H)
        _SORTED[pattern] = (aos, w, h, lengths, dict(stage1=s1, e=e, tile=t, depth=d, id=i, ranges=ranges))
    return _SORTED[pattern]


def range_lengths(ref):
    return ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]


def varying_digits(keys, bits):
    """How many of the 32 / bits digits of the keys take more than one value: the passes of an LSD sort that move anything."""
    keys = np.asarray(keys, np.uint32)
    return sum(int(np.unique((keys >> np.uint32(s)) & np.uint32((1 << bits) - 1)).size > 1) for s in range(0, 32, bits))


def check_run_keys(base, keys, ids):
    """The claims of a base pattern on one run's keys (sorted) and splat indices (in sorted order)."""
    k = keys.size
    byte = [np.unique((keys >> np.uint32(s)) & np.uint32(255)).size for s in (0, 8, 16, 24)]
    if base == "equal":
        assert np.unique(keys).size == 1
        assert np.all(np.diff(ids.astype(np.int64)) > 0), "ties keep ascending splat index"
    elif base == "near":
        assert keys.max() < 1 << 23 and byte[3] == 1
        if k >= 64:
            assert min(byte[:3]) >= 2, byte
    elif base == "far":
        assert byte[0] == 1 and keys.min() >= 1 << 31 and keys.max() < 0xFFFFFFFF
    elif base == "far_odd":
        assert set(np.unique(keys & np.uint32(255)).tolist()) <= {0, 0x80}
        if k >= 64:
            assert byte[0] == 2 and varying_digits(keys, 4) == 7
    elif base == "beyond":
        assert 4 * int((keys == 0xFFFFFFFF).sum()) >= k
        if k >= 2:
            assert keys.min() < 0xFFFFFFFF
            far = ids[keys == 0xFFFFFFFF].astype(np.int64)
            assert np.all(np.diff(far) > 0), "the saturated keys are one long tie"
    elif base == "wide":
        if k >= 64:
            assert keys.min() < 1 << 24 and keys.max() >= 1 << 31 and min(byte) >= 2
    elif base == "descending":
        assert np.all(np.diff(keys.astype(np.int64)) > 0)
        assert np.all(np.diff(ids.astype(np.int64)) < 0), "sorting reverses the whole run"


def test_designed_scenes_are_what_they_claim(oracle_mod):
    """Nothing about the designed scenes is assumed: on the oracle, for every pattern, the range of every tile has the designed
    length and the other tiles are empty; the list stays below its capacity; every class of gs_tilesort.hip's routing holds a run
    on each side of each of its edges, and the 64-lane, wave-stride and chunk edges inside it; the keys of every run have the
    byte and digit statistics its pattern names; and both ping-pong outcomes (an even and an odd number of moving 4-bit passes)
    occur in the chunked and in the global class.  The counts are in the module docstring."""
    tiles = run_tiles()
    assert len(set(tiles)) == len(LENGTHS) < GRID_W * GRID_H and GRID_H >= 4
    parities = {c: set() for c in ("chunked", "global")}
    for pattern in PATTERNS:
        aos, w, h, lengths, ref = sorted_list(oracle_mod, pattern)
        s1, e = ref["stage1"], ref["e"]
        assert aos.shape[0] == lengths.sum() == sum(LENGTHS)
        lens = range_lengths(ref)
        assert np.array_equal(lens, lengths), "a tile's range is not the designed run"
        assert int((lens == 0).sum()) == GRID_W * GRID_H - len(LENGTHS) >= 4
        assert e == s1["counter"] == lengths.sum() < s1["capacity"]
        # one element per splat, none culled, and no tile's splat indices contiguous
        assert np.array_equal(np.sort(ref["id"][:e]), np.arange(e))
        # the edges of the routing table, from the oracle's lengths and the restated constants
        have = set(lens.tolist())
        per_class = {name: sorted(int(v) for v in lens if v and size_class(v) == name) for name, _, _ in CLASSES}
        for name, lo, hi in CLASSES[1:]:
            assert lo in have and lo - 1 in have, (name, lo)            # first of the class, last of the one below
            if name != "global":
                assert hi in have and hi + 1 in have, (name, hi)
            assert size_class(lo) == name != size_class(lo - 1)
        assert 0 in have and 1 in have
        for edge in (64, 256, 512, 768, 1536, 2560, 8192, 12288):      # lanes, wave strides of S1 / S2 / S3, 4096-key chunks
            assert {edge - 1, edge, edge + 1} & have >= {edge, edge + 1}, edge
        assert max(have) % 4096 not in (0, 1) and max(have) > 12289     # a partial last chunk well inside the global class
        if pattern == PATTERNS[0]:
            print()
            for name, _, _ in CLASSES:
                print(f"{name:10s} {len(per_class[name]):2d} runs:", *per_class[name])
        # the keys, run by run
        digits = {c: [] for c in parities}
        bytes_s3 = []
        for j, (tile, base) in enumerate(zip(tiles, run_patterns(pattern))):
            b, en = (int(v) for v in ref["ranges"][tile])
            assert np.all(ref["tile"][b:en] == tile)
            keys, ids = ref["depth"][b:en], ref["id"][b:en]
            assert np.all(np.diff(keys.astype(np.int64)) >= 0)
            if en - b >= 3:
                assert int(ids.max()) - int(ids.min()) + 1 > en - b, "the run's splat indices are contiguous"
            check_run_keys(base, keys, ids)
            cls = size_class(en - b)
            if cls in digits:
                digits[cls].append(varying_digits(keys, 4))
                parities[cls].add(digits[cls][-1] % 2)
            if cls == "S3":
                bytes_s3.append(varying_digits(keys, 8))
        print(f"{pattern:10s} moving 4-bit passes: chunked {digits['chunked']} global {digits['global']}; "
              f"moving 8-bit passes of the S3 runs {bytes_s3}")
        if pattern == "mixed":
            for cls in BIG_CLASSES:
                rows = {t // GRID_W for t in tiles if size_class(lens[t]) == cls}
                assert rows == set(range(GRID_H)), (cls, rows)
    assert parities == {"chunked": {0, 1}, "global": {0, 1}}, parities


# ---- a list that overflows its capacity inside a chunked and a global run ---------------------------------------------
# The capacity is ceilPow2(N + 1024 * tiles) (Renderer.cpp:725; gs_set_resolution), and the elements past it are dropped by
# their offset in record order.  Small splats give one element each, so a frame of them can never overflow; OVERFLOW_PADS splats
# that cover the whole frame add one element to every tile each.  Record order: the designed runs, shuffled; then the pads;
# then the shuffled tails of two runs, into which the capacity cuts.
OVERFLOW_PADS = 1300
OVERFLOW_FINAL = (2048, 2049, 4096, 4097, 8192, 8193, 9984, 9985, 12289, 13001)    # whole runs: pads + small splats
OVERFLOW_CUT = (("chunked", 5000, 3000), ("global", 9000, 3000))                   # class after the cut, splats before the pads, behind them


def overflow_runs(oracle, seed=21):
    """(aos, w, h, whole, cut): whole = {tile: length} of the runs the cut leaves alone, cut = {tile: (class, uncut length)}."""
    w, h = GRID_W * 16, GRID_H * 16
    rng = np.random.default_rng(seed)
    tile_of = lambda j: (j % GRID_H) * GRID_W + j // GRID_H
    head = [(tile_of(j), f - OVERFLOW_PADS) for j, f in enumerate(OVERFLOW_FINAL)]
    cut_tiles = [tile_of(len(OVERFLOW_FINAL) + j) for j in range(len(OVERFLOW_CUT))]
    head += [(t, c[1]) for t, c in zip(cut_tiles, OVERFLOW_CUT)]
    tail = [(t, c[2]) for t, c in zip(cut_tiles, OVERFLOW_CUT)]
    n_head, n_tail = sum(k for _, k in head), sum(k for _, k in tail)
    aos = np.zeros((n_head + OVERFLOW_PADS + n_tail, 84), np.float32)

    def place(runs, first, count):
        slots, off = first + rng.permutation(count), 0
        for j, (tile, k) in enumerate(runs):
            ids = np.sort(slots[off:off + k])
            off += k
            unit = screen_splat(oracle, w, h, (tile % GRID_W) * 16 + 8.0, (tile // GRID_W) * 16 + 8.0, 1.0, 0.3, OPACITY)
            z = _depths(BASE_PATTERNS[j % len(BASE_PATTERNS)], j, k, rng).astype(np.float32).astype(np.float64)
            rec = np.tile(unit, (k, 1))
            rec[:, 0:3] = unit[0:3].astype(np.float64) * z[:, None]
            rec[:, 4:7] = unit[4:7].astype(np.float64) * z[:, None]
            rec[:, 12:15] = rng.uniform(-1.0, 1.0, (k, 3))
            aos[ids] = rec

    place(head, 0, n_head)
    unit = screen_splat(oracle, w, h, w / 2, h / 2, 1.0, 100.0, 0.01)               # 3-sigma radius of 300 px: every tile
    z = _depths("wide", 0, OVERFLOW_PADS, rng).astype(np.float32).astype(np.float64)
    pads = np.tile(unit, (OVERFLOW_PADS, 1))
    pads[:, 0:3] = unit[0:3].astype(np.float64) * z[:, None]
    pads[:, 4:7] = unit[4:7].astype(np.float64) * z[:, None]
    pads[:, 12:15] = rng.uniform(-1.0, 1.0, (OVERFLOW_PADS, 3))
    aos[n_head:n_head + OVERFLOW_PADS] = pads
    place(tail, n_head + OVERFLOW_PADS, n_tail)
    whole = {tile_of(j): f for j, f in enumerate(OVERFLOW_FINAL)}
    cut = {t: (c[0], c[1] + OVERFLOW_PADS + c[2]) for t, c in zip(cut_tiles, OVERFLOW_CUT)}
    return aos, w, h, whole, cut


def test_overflow_scene_cuts_inside_big_runs(oracle_mod):
    """The overflowing scene on the oracle: the list is longer than its capacity; the runs in front of the cut have their designed
    lengths on both sides of the edges of S2 | S3 | chunked | global; the two runs the capacity cuts into lost some but not all of
    their tail and are still a chunked and a global run; every other tile holds the pads only."""
    aos, w, h, whole, cut = overflow_runs(oracle_mod)
    assert aos.shape[0] < 300_000
    view, proj, pos = default_camera(oracle_mod, w, h)
    p = oracle_mod.make_params(w, h, view, proj, pos)
    s1 = oracle_mod.init_sort_list(p, aos)
    cap = s1["capacity"]
    assert cap == oracle_mod.capacity(aos.shape[0], GRID_W * GRID_H) == 131072
    n_tail = sum(c[2] for c in OVERFLOW_CUT)
    assert s1["counter"] == aos.shape[0] + (GRID_W * GRID_H - 1) * OVERFLOW_PADS
    assert cap < s1["counter"] < cap + n_tail // 2, "the cut does not fall inside the tails"
    t, d, i = oracle_mod.sort_stable(s1["tile"], s1["depth"], s1["id"], cap)
    lens = range_lengths(dict(ranges=oracle_mod.find_ranges(t, cap, GRID_W * GRID_H)))
    assert lens.sum() == cap
    for tile in range(GRID_W * GRID_H):
        if tile in whole:
            assert lens[tile] == whole[tile]
        elif tile in cut:
            cls, uncut = cut[tile]
            tail = dict(zip(cut, OVERFLOW_CUT))[tile][2]
            assert uncut - tail + tail // 4 < lens[tile] < uncut - tail // 4 and size_class(lens[tile]) == cls, (tile, lens[tile])
        else:
            assert lens[tile] == OVERFLOW_PADS
    have = set(lens.tolist())
    for edge in (2048, 4096, 9984):
        assert edge in have and edge + 1 in have
    print("\ncut runs:", {tile: int(lens[tile]) for tile in cut}, "of", {tile: c[1] for tile, c in cut.items()},
          "emitted", s1["counter"], "capacity", cap)
