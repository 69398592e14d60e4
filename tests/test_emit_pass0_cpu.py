"""Pass 0 of a frame's depth sort inside InitSortList, on the CPU: the scenes of tests/test_emit_pass0_gpu.py, proven, and a numpy
model of what the three kernels compute.

A frame of the contractual sorter with a Count launch per pass stores its list where pass 0 -- a stable counting sort on
depth_key & 15 -- would put it (k_emit<false, true>, gs_project.hip).  Every element of a splat shares that digit, so the place of
element j of splat s is  P(s, j) = D[d_s] + (elements of digit d_s emitted by the splats before s) + j,  D[d] = the elements of
smaller digits.  k_project leaves a row of sixteen element counts per block of 256 splats, k_scan_blocks scans the sixteen columns
over the blocks, k_emit adds the part inside its block.  pass0_table() is that table as gs_debug_read(GS_BUF_PASS0_OFFSETS) returns
it, pass0_positions() the formula; the tests compare them with np.argsort(key & 15, kind="stable") of the oracle's own list and
assert that every scene still has the property it is designed for (a scene that loses it fails here, it does not pass empty).

The reference's key is uint(nd * 2^32) of a float32 nd: its low four bits are zero unless nd < 2^-4, and odd only below 2^-8.  The
scenes that need all sixteen values therefore sit at view depths 0.12 - 0.45 (default planes) or use far_plane = 10000."""
import numpy as np
import pytest

from conftest import default_camera
from test_backward_cpu import screen_splat
from test_designed_lengths_cpu import cached, cull

BLOCK = 256                 # kProjThreads
EMIT_SLICE = 4096           # GS_EMIT_SLICE
W, H = 256, 208             # 16 x 13 = 208 tiles
OW, OH = 320, 180           # the overflow recipe of tests/test_parity_gpu.py::test_overflow_truncates_like_reference
FAR = dict(far_plane=10000.0)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def pass0_table(keys, counts):
    """uint32 [blocks + 1][16]: row b = the elements of each digit that the splats before block b emit, the last row = the digit
    bases.  keys, counts: depth key and element count per splat (count 0: the key does not matter)."""
    n = len(counts)
    blocks = (n + BLOCK - 1) // BLOCK
    hist = np.zeros((blocks, 16), np.int64)
    np.add.at(hist, (np.arange(n) // BLOCK, (keys & 15).astype(np.int64)), counts.astype(np.int64))
    table = np.zeros((blocks + 1, 16), np.int64)
    table[1:blocks] = np.cumsum(hist, axis=0)[:-1]
    totals = hist.sum(axis=0)
    table[blocks] = np.cumsum(totals) - totals
    return table.astype(np.uint32)


def pass0_positions(keys, counts):
    """P(s, 0) per splat, by the formula, from the table and the splats of the same digit before s inside its block."""
    table = pass0_table(keys, counts).astype(np.int64)
    n = len(counts)
    blocks = (n + BLOCK - 1) // BLOCK
    pos = np.zeros(n, np.int64)
    for b in range(blocks):
        inside = np.zeros(16, np.int64)
        for s in range(b * BLOCK, min(n, (b + 1) * BLOCK)):
            d = int(keys[s] & 15)
            pos[s] = table[blocks][d] + table[b][d] + inside[d]
            inside[d] += int(counts[s])
    return pos


def stage1(oracle, aos, w, h, constants=None):
    """The oracle's unsorted list and per-splat records of the frame (default camera), uncut: keys, counts, counter, capacity."""
    view, proj, pos = default_camera(oracle, w, h)
    p = oracle.make_params(w, h, view, proj, pos)
    for k, v in (constants or {}).items():
        setattr(p, k, v)
    gw, gh = oracle.grid(w, h)
    cap = oracle.capacity(len(aos), gw * gh)
    counter = oracle.init_sort_list(p, aos, cap=16)["counter"]
    s1 = oracle.init_sort_list(p, aos, cap=max(counter, 16))
    sp = s1["splats"]
    counts = np.where(sp["visible"] != 0, (sp["max_x"] - sp["min_x"]).astype(np.int64) * (sp["max_y"] - sp["min_y"]).astype(np.int64), 0)
    assert counts.sum() == s1["counter"] == counter
    return dict(keys=sp["depth_key"].copy(), counts=counts, counter=int(s1["counter"]), capacity=cap, ids=s1["id"][:s1["counter"]].copy())


# ---- the scenes ---------------------------------------------------------------------------------------------------------------
def _splats(oracle, w, h, z, sigma, rng):
    z = np.asarray(z, np.float32)
    sx, sy = rng.uniform(4.0, w - 4.0, z.size), rng.uniform(4.0, h - 4.0, z.size)
    sig = np.broadcast_to(np.asarray(sigma, np.float64), z.shape)
    return np.stack([screen_splat(oracle, w, h, float(sx[i]), float(sy[i]), float(z[i]), float(sig[i]), 0.3,
                                  tuple(rng.uniform(-1.0, 1.0, 3))) for i in range(z.size)]).astype(np.float32)


def _behind(aos):
    return cull(aos, np.arange(len(aos)))


def scene(oracle, name):
    """(aos, w, h, constants) of a designed scene; cached, do not write to the arrays."""
    def make():
        rng = np.random.default_rng(sum(map(ord, name)))
        if name in ("mixed", "n257"):                 # all sixteen digits inside every block; three full blocks and a ragged one
            aos = _splats(oracle, W, H, rng.uniform(0.12, 0.45, 1000), rng.uniform(1.0, 14.0, 1000), rng)
            return (aos if name == "mixed" else aos[:257].copy()), W, H, {}
        if name == "mixed_far":                       # the same under far_plane = 10000: nd < 2^-8 up to z = 39
            return _splats(oracle, W, H, rng.uniform(0.5, 30.0, 1000), rng.uniform(1.0, 14.0, 1000), rng), W, H, dict(FAR)
        if name == "one_digit":                       # every splat at one view depth
            return _splats(oracle, W, H, np.full(600, 1.0), rng.uniform(1.0, 14.0, 600), rng), W, H, {}
        if name == "alternating":                     # two depths by splat index: the maximal interleave inside a block
            z = np.where(np.arange(700) % 2 == 0, 0.2, 0.31)
            return _splats(oracle, W, H, z, rng.uniform(1.0, 14.0, 700), rng), W, H, {}
        if name == "heavy":                           # light block, a block of 48 whole-frame splats (9984 elements), light block
            light = lambda: _splats(oracle, W, H, rng.uniform(0.12, 0.45, BLOCK), 1.0, rng)
            big = _splats(oracle, W, H, rng.uniform(0.12, 0.45, 48), 3000.0, rng)
            mid = _behind(_splats(oracle, W, H, np.full(BLOCK, 1.0), 1.0, rng))
            mid[rng.choice(BLOCK, 48, replace=False)] = big
            return np.concatenate([light(), mid, light()[:100]]), W, H, {}
        if name == "holes":                           # emitting, all culled, emitting, all culled, a ragged emitting block
            part = lambda k: _splats(oracle, W, H, rng.uniform(0.12, 0.45, k), rng.uniform(1.0, 14.0, k), rng)
            return np.concatenate([part(BLOCK), _behind(part(BLOCK)), part(BLOCK), _behind(part(BLOCK)), part(40)]), W, H, {}
        if name == "nothing":
            return _behind(_splats(oracle, W, H, np.full(300, 1.0), 4.0, rng)), W, H, {}
        raise KeyError(name)
    return cached(("pass0", name), make)


SCENES = ("mixed", "mixed_far", "n257", "one_digit", "alternating", "heavy", "holes", "nothing")


def overflow_scene(oracle, delta):
    """The overflow recipe (320 x 180, n = 4000, mu = 2.0), n kept.  delta None: as it is.  Else the cloud trimmed -- a suffix moved
    behind the camera, then single-tile splats of odd digits and, for 'straddle', one whole-frame splat put in its place -- so that the
    counter is capacity + delta (delta = -1, 0, 1), or capacity + 300 with the whole-frame splat across the capacity and singles of
    other digits behind it ('straddle')."""
    def make():
        from vk3dgaussiansplatting_amd import synth
        aos = np.array(synth.generate(4000, OW, OH, 2.0, seed=9), np.float32)
        if delta is None:
            return aos
        s = stage1_of_overflow(oracle, aos)
        cap = s["capacity"]
        target = cap + (300 if delta == "straddle" else delta)
        cum = np.cumsum(s["counts"])
        keep = int(np.searchsorted(cum, target - 1500))              # the first `keep` splats stay: at least 1500 elements short
        rng = np.random.default_rng(7)
        out = cull(aos, np.arange(keep, 4000))
        missing = target - int(cum[keep - 1])
        pool = _splats(oracle, OW, OH, rng.uniform(0.12, 0.45, 3 * missing + 600), 0.3, rng)
        pool = pool[stage1_of_overflow(oracle, pool)["counts"] == 1]  # a 0.3 px splat touches one tile unless it sits near a tile edge
        if delta == "straddle":                                      # 240 elements across the capacity: 180 below it, 60 beyond
            before = missing - 480
            big = _splats(oracle, OW, OH, [0.3], 3000.0, rng)
            assert stage1_of_overflow(oracle, big)["counts"][0] == 240
            tail = np.concatenate([pool[:before], big, pool[before:before + 240]])
        else:
            tail = pool[:missing]
        k = len(tail)
        assert k == (missing - 239 if delta == "straddle" else missing)
        assert keep + k <= 4000
        out[keep:keep + k] = tail
        return out
    return cached(("pass0_overflow", delta), make)


def stage1_of_overflow(oracle, aos):
    return stage1(oracle, aos, OW, OH)


OVERFLOWS = (None, -1, 0, 1, "straddle")


# ---- the tests ----------------------------------------------------------------------------------------------------------------
def check_model(s):
    """The formula against a stable argsort of the list's digits: element i of the list lands at inverse_perm[i]."""
    keys, counts = s["keys"], s["counts"]
    digits = (keys[s["ids"]] & 15).astype(np.int64)
    perm = np.argsort(digits, kind="stable")
    where = np.empty(len(perm), np.int64)
    where[perm] = np.arange(len(perm))
    first = np.cumsum(counts) - counts                                # list index of a splat's first element
    pos = pass0_positions(keys, counts)
    emit = np.flatnonzero(counts)
    assert np.array_equal(pos[emit], where[first[emit]])
    last = first[emit] + counts[emit] - 1
    assert np.array_equal(pos[emit] + counts[emit] - 1, where[last])   # ... and its elements stay together, in order
    table = pass0_table(keys, counts)
    assert int(table[-1][15]) + int((counts * ((keys & 15) == 15)).sum()) == s["counter"]


def block_digits(s):
    """Distinct digits among the emitting splats of every block."""
    keys, counts = s["keys"], s["counts"]
    return [len(set((keys[b:b + BLOCK][counts[b:b + BLOCK] > 0] & 15).tolist())) for b in range(0, len(counts), BLOCK)]


def block_elements(s):
    return [int(s["counts"][b:b + BLOCK].sum()) for b in range(0, len(s["counts"]), BLOCK)]


@pytest.mark.parametrize("name", SCENES)
def test_scene_has_its_property_and_the_model_sorts_it(oracle_mod, name):
    aos, w, h, constants = scene(oracle_mod, name)
    s = stage1(oracle_mod, aos, w, h, constants)
    assert s["counter"] < s["capacity"]
    present = set((s["keys"][s["counts"] > 0] & 15).tolist())
    per_block, elems = block_digits(s), block_elements(s)
    print(name, "n", len(aos), "E", s["counter"], "digits", sorted(present), "per block", per_block, "elements", elems)
    if name in ("mixed", "mixed_far"):
        assert len(aos) == 1000 and present == set(range(16)) and min(per_block) == 16
    elif name == "n257":
        assert len(aos) == 257 and s["counts"][256] > 0 and per_block[0] >= 4
    elif name == "one_digit":
        assert len(present) == 1 and s["counter"] > 600
        assert np.count_nonzero(pass0_table(s["keys"], s["counts"])[-1]) <= 15 and len(set(pass0_table(s["keys"], s["counts"])[-1].tolist())) <= 2
    elif name == "alternating":
        d = s["keys"] & 15
        assert len(present) == 2 and (s["counts"] > 0).all() and (d[0::2] == d[0]).all() and (d[1::2] == d[1]).all() and d[0] != d[1]
    elif name == "heavy":
        assert max(elems) == elems[1] == 48 * 208 == 9984 and (9984 - 1) // EMIT_SLICE == 2          # three slices: two helper records
        assert len(set((s["keys"][BLOCK:2 * BLOCK][s["counts"][BLOCK:2 * BLOCK] > 0] & 15).tolist())) >= 3
        assert 0 < elems[0] <= EMIT_SLICE and 0 < elems[2] <= EMIT_SLICE
    elif name == "holes":
        assert [e > 0 for e in elems] == [True, False, True, False, True] and min(per_block[0], per_block[2]) >= 4
    elif name == "nothing":
        assert s["counter"] == 0
    if s["counter"]:
        check_model(s)
    else:
        assert not pass0_table(s["keys"], s["counts"]).any()


@pytest.mark.parametrize("delta", OVERFLOWS, ids=[str(d) for d in OVERFLOWS])
def test_overflow_scene_has_its_counter(oracle_mod, delta):
    aos = overflow_scene(oracle_mod, delta)
    s = stage1_of_overflow(oracle_mod, aos)
    cap = s["capacity"]
    print("overflow", delta, "counter", s["counter"], "capacity", cap)
    assert len(aos) == 4000
    if delta is None:
        assert s["counter"] > cap + 10000
    elif delta == "straddle":
        assert s["counter"] == cap + 300
        first = np.cumsum(s["counts"]) - s["counts"]
        k = int(np.flatnonzero((first < cap) & (first + s["counts"] > cap) & (s["counts"] == 240))[0])      # the splat across the capacity
        d = s["keys"] & 15
        assert ((d[:k] != d[k]) & (s["counts"][:k] > 0)).any() and ((d[k + 1:] != d[k]) & (s["counts"][k + 1:] > 0)).any()
    else:
        assert s["counter"] == cap + delta
    check_model(s)          # the formula itself knows no capacity: an overflowing frame writes the plain list (gs_project.hip)
