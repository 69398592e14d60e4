"""The packed payload of a frame's depth passes (vk3dgaussiansplatting_amd/csrc/gs_sort_words.h: pk32 = tile16 << 16 | id & 0xFFFF,
pk8 = id >> 16 in a byte plane or in a consumed byte of the depth word): the pass table as gs_internal.h derives it, and the
scenes tests/test_packed_words_gpu.py renders, proven on the CPU oracle to be what they claim.

  pass table   tests/host/sort_pass_table.cpp over gs_internal.h (host code): forms chain from pass to pass, the last depth pass
               unpacks, bytes per element and side as the design states them; N = 2^24 packs, 2^24 + 1 does not, and neither
               does a frame with per-pass timers (record_timings = 2), whose reported bytes stay those of the word layouts
  high ids     HIGH_K visible splats at chosen indices of a cloud of N = 2^24 or 2^24 + 256 whose other records lie behind the
               camera; the same records as a compact cloud are the reference (ids through the index map)
  nibbles      N = 3 * 65,536 + 500: per nibble k of the depth key one tile with those of the 15 keys B_k | j << 4 k that some
               float32 depth produces (at least NIB_MIN_KEYS of them), two splats per key, at ids spread over all three
               65,536-blocks and shuffled against the key order; two runs of 40 equal (tile, depth)
               elements over ids 65,516 - 65,555 and 131,052 - 131,091; six equal pads (an element in every tile) over ids
               196,605 - 196,610
  low ids      N = 70,000, the 6,200 records of a short frame in front: every emitting id below 65,536 (pk8 = 0 throughout)"""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, default_camera
from test_backward_cpu import screen_splat
from test_designed_lengths_cpu import (SMALL_H, SMALL_TILES, SMALL_W, at_depths, cached, cull, oracle_frame, short_scene,
                                       tile_units, wide_depths)

CSRC = os.path.join(ROOT, "vk3dgaussiansplatting_amd", "csrc")
PACK_MAX_N = 1 << 24                     # kPackedMaxSplats
PK_NONE, PK_PLANE, PK_WORD = 0, 1, 2     # kPkNone, kPkPlane, kPkWord

# bytes per element read -> written by the eight depth passes of a 16-bit-tile frame: packed, and the layouts before
PACKED_BYTES = ((9, 9), (9, 8), (8, 8), (8, 7), (7, 7), (7, 6), (6, 6), (6, 6))
UNPACKED_BYTES = ((10, 10), (10, 10), (10, 10), (10, 8), (8, 8), (8, 8), (8, 8), (8, 6))
# a fed run (short lists) keeps the unpacked element out of passes 3 and 4: no byte plane beside a 16-bit depth word
PACKED_FED_BYTES = ((9, 9), (9, 8), (8, 8), (8, 8), (8, 8), (8, 6), (6, 6), (6, 6))
PACKED_MEAN = sum(a + b for a, b in PACKED_BYTES) / 8        # 14.625, what gs_timings.scatter_bytes_per_elem reports
PACKED_FED_MEAN = sum(a + b for a, b in PACKED_FED_BYTES) / 8    # 15.125
UNPACKED_MEAN = sum(a + b for a, b in UNPACKED_BYTES) / 8    # 17.5
assert (PACKED_MEAN, UNPACKED_MEAN) == (117 / 8, 140 / 8)


# ---- the pass table ---------------------------------------------------------------------------------------------------------
def pass_table(tmp, hi16, n, sort_bits, digit_bits=4, fed=False, record_timings=1):
    """[(pass, shift, lo_in, lo_out, pk_in, pk_out, word16, word_shift, bytes)] of a frame's run, from the header itself."""
    exe = os.path.join(str(tmp), "sort_pass_table")
    if not os.path.exists(exe):
        rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
        subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"), "-I", CSRC,
                        "-o", exe, os.path.join(ROOT, "tests", "host", "sort_pass_table.cpp")], check=True)
    out = subprocess.run([exe, str(int(hi16)), str(n), str(sort_bits), str(digit_bits), str(int(fed)), str(record_timings)], check=True, capture_output=True, text=True)
    return [tuple(int(v) for v in ln.split()) for ln in out.stdout.splitlines()]


def side_bytes(lo, pk, hi16):
    return lo + {PK_NONE: (2 if hi16 else 4) + 4, PK_PLANE: 1 + 4, PK_WORD: 4}[pk]


@pytest.mark.parametrize("fed", [False, True])
@pytest.mark.parametrize("n", [PACK_MAX_N, PACK_MAX_N + 1])
def test_pass_table_of_a_16_bit_tile_frame(tmp_path_factory, n, fed):
    """hi16, 40 sort bits (144 tiles): with N = 2^24 every depth pass reads the form the pass before wrote, starting from what
    k_emit writes (depth u32, pk32, byte plane), the last depth pass writes tile u16 + id u32, the bytes are the design's and
    Count's word and shift are those of the unpacked run; with one splat more nothing packs.  A fed run differs in the element
    between passes 3 and 5, which stays unpacked."""
    tmp = tmp_path_factory.getbasetemp()
    rows = pass_table(tmp, True, n, 40, fed=fed)
    plain = pass_table(tmp, True, PACK_MAX_N + 1, 40, fed=fed)
    assert len(rows) == len(plain) == 10
    packs = n <= PACK_MAX_N
    want = (PACKED_FED_BYTES if fed else PACKED_BYTES) if packs else UNPACKED_BYTES
    prev_lo, prev_pk = 4, PK_PLANE if packs else PK_NONE              # what k_emit wrote
    for (k, shift, lo_in, lo_out, pk_in, pk_out, w16, wshift, nbytes), ref in zip(rows, plain):
        assert shift == 4 * k and (w16, wshift) == (ref[6], ref[7]) and (lo_in, lo_out) == (ref[2], ref[3])
        if k < 8:
            assert (lo_in, pk_in) == (prev_lo, prev_pk), k
            assert (side_bytes(lo_in, pk_in, True), side_bytes(lo_out, pk_out, True)) == want[k], k
            assert (pk_in != PK_NONE) == (packs and not (fed and k in (4, 5)))
            # pk8 rides in the word exactly when the byte it replaces is consumed: key bits 0-7 of a 32-bit word, 16-23 of the upper half
            if pk_in != PK_NONE:
                assert pk_in == (PK_WORD if (shift % 16) >= 8 else PK_PLANE), k
        else:
            assert (lo_in, lo_out, pk_in, pk_out) == (0, 0, PK_NONE, PK_NONE), k
        assert nbytes == side_bytes(lo_in, pk_in, True) + side_bytes(lo_out, pk_out, True)
        prev_lo, prev_pk = lo_out, pk_out
    assert rows[7][5] == PK_NONE and rows[7][3] == 0                  # the last depth pass unpacks
    assert sum(r[8] for r in rows[:8]) == ((121 if fed else 117) if packs else 140)


@pytest.mark.parametrize("hi16,n,sort_bits,digit_bits,record_timings",
                         [(False, 1000, 52, 4, 1), (True, 1000, 40, 8, 1), (True, 1 << 25, 40, 4, 1), (True, 1000, 40, 4, 2)])
def test_pass_table_of_everything_else_is_unpacked(tmp_path_factory, hi16, n, sort_bits, digit_bits, record_timings):
    """32-bit tile words, 8-bit digits, more than 2^24 splats and frames with per-pass timers: no pass packs, the bytes are
    depth + tile + id on both sides."""
    for k, shift, lo_in, lo_out, pk_in, pk_out, w16, wshift, nbytes in pass_table(tmp_path_factory.getbasetemp(), hi16, n, sort_bits,
                                                                                 digit_bits, record_timings=record_timings):
        assert (pk_in, pk_out) == (PK_NONE, PK_NONE)
        assert nbytes == lo_in + lo_out + 2 * ((2 if hi16 else 4) + 4)


# ---- high ids ------------------------------------------------------------------------------------------------------------------
HIGH_NS = (PACK_MAX_N, PACK_MAX_N + 256)
HIGH_RANDOM = 3000
HIGH_PADS = 4


def high_specials(n):
    return [0, 65535, 65536, 65537, (1 << 23) - 1, 1 << 23, n - 1]


HIGH_K = HIGH_RANDOM + len(high_specials(PACK_MAX_N))


def high_indices(n):
    """The HIGH_K indices of the visible splats in a cloud of n, ascending: the specials and seeded random ones."""
    rng = np.random.default_rng(n)
    sp = high_specials(n)
    picks = rng.choice(n, HIGH_RANDOM + 64, replace=False)
    picks = picks[~np.isin(picks, sp)][:HIGH_RANDOM]
    idx = np.sort(np.concatenate([np.asarray(sp, np.int64), picks.astype(np.int64)]))
    assert idx.size == HIGH_K and np.unique(idx).size == HIGH_K
    return idx


def high_scene(oracle):
    """(visible records [HIGH_K, 84], one culled record [84], w, h): singles at wide depths and HIGH_PADS pads."""
    def make():
        rng = np.random.default_rng(24)
        units = cached("small_units", lambda: tile_units(oracle, SMALL_W, SMALL_H, range(SMALL_TILES)))
        rec = at_depths(units[rng.integers(0, SMALL_TILES, HIGH_K)], wide_depths(rng, HIGH_K), rng)
        pad = screen_splat(oracle, SMALL_W, SMALL_H, SMALL_W / 2, SMALL_H / 2, 1.0, 100.0, 0.01).astype(np.float32)
        at = rng.choice(HIGH_K, HIGH_PADS, replace=False)
        rec[at] = at_depths(np.tile(pad, (HIGH_PADS, 1)), wide_depths(rng, HIGH_PADS), rng)
        return rec, cull(rec[:1], [0])[0].copy()
    rec, culled = cached("high_scene", make)
    return rec, culled, SMALL_W, SMALL_H


def high_frame(oracle):
    rec, _, w, h = high_scene(oracle)
    return cached("high_frame", lambda: oracle_frame(oracle, rec, w, h))


def test_high_id_scene_is_what_it_claims(oracle_mod):
    rec, culled, w, h = high_scene(oracle_mod)
    ref = high_frame(oracle_mod)
    assert ref["e"] == HIGH_K - HIGH_PADS + SMALL_TILES * HIGH_PADS == ref["stage1"]["counter"]
    assert np.unique(ref["id"][:ref["e"]]).size == HIGH_K                        # every visible record emits
    assert oracle_frame(oracle_mod, culled[None, :], w, h, image=False)["e"] == 0   # the filler emits nothing
    for n in HIGH_NS:
        idx = high_indices(n)
        assert set(high_specials(n)) <= set(idx.tolist()) and idx[-1] == n - 1 and idx[0] == 0
        assert np.unique(idx >> 16).size > 200                                   # the high index byte takes most of its values
    assert HIGH_NS[0] <= PACK_MAX_N < HIGH_NS[1]


# ---- nibbles and equal runs ---------------------------------------------------------------------------------------------------
NIB_N = 3 * 65536 + 500
NIB_RUNS = ((8, 65536 - 20), (9, 2 * 65536 - 20))        # (tile, first id) of the runs of 40 equal (tile, depth) elements
NIB_RUN_LEN = 40
NIB_PADS = tuple(range(3 * 65536 - 3, 3 * 65536 + 3))    # six equal pads: equal (tile, depth) in every tile, ids around 196,608


NIB_MIN_KEYS = 4


def nibble_keys(k):
    """The 15 candidate keys of nibble k: the bits above the nibble fixed, those below zero (a key is a float32 times 2^32: 24
    bits).  Not every key has a float32 depth (near the camera one step of the depth moves the key by 2 - 3): depths_of_keys keeps
    those that have one."""
    base = (0xA5C3F << (4 * k + 4)) & 0xFFFFFFFF
    return [base | (j << (4 * k)) for j in range(1, 16)]


def depths_of_keys(oracle, keys):
    """(keys, depths): those of `keys` that some float32 view depth produces exactly, and such a depth for each: candidates
    around the inverse of InitSortList.comp:70-80, judged by the oracle's own keys."""
    view, proj, pos = default_camera(oracle, SMALL_W, SMALL_H)
    p = oracle.make_params(SMALL_W, SMALL_H, view, proj, pos)
    near, far = float(p.near_plane), float(p.far_plane)
    unit = cached("small_units", lambda: tile_units(oracle, SMALL_W, SMALL_H, range(SMALL_TILES)))[:1]
    span = 9
    cand = []
    for key in keys:
        z = np.float32(near + key / 4294967296.0 * (far - near))
        lo = z
        for _ in range(span // 2):
            lo = np.nextafter(lo, np.float32(0))
        zs = [lo]
        for _ in range(span - 1):
            zs.append(np.nextafter(zs[-1], np.float32(np.inf)))
        cand.extend(zs)
    cand = np.asarray(cand, np.float32)
    rec = at_depths(np.repeat(unit, cand.size, axis=0), cand, np.random.default_rng(0))
    s1 = oracle.init_sort_list(p, rec, threads=oracle.host_threads(16))
    assert s1["counter"] == cand.size                                            # every candidate is a single
    got = np.empty(cand.size, np.uint32)
    got[s1["id"][:cand.size]] = s1["depth"][:cand.size]
    hits, out = [], []
    for i, key in enumerate(keys):
        hit = np.flatnonzero(got[i * span:(i + 1) * span] == np.uint32(key))
        if hit.size:
            hits.append(key)
            out.append(cand[i * span + hit[0]])
    return hits, np.asarray(out, np.float32)


def nibble_scene(oracle):
    """(aos [NIB_N, 84], w, h, {k: (keys of nibble k, ids of its splats in key order, two per key)})."""
    def make():
        rng = np.random.default_rng(4)
        units = cached("small_units", lambda: tile_units(oracle, SMALL_W, SMALL_H, range(SMALL_TILES)))
        filler = cull(at_depths(units[:1], [3.0], rng), [0])[0]
        aos = np.tile(filler, (NIB_N, 1)).astype(np.float32)
        reserved = set(NIB_PADS)
        for _, first in NIB_RUNS:
            reserved |= set(range(first, first + NIB_RUN_LEN))
        free = rng.permutation(np.setdiff1d(np.arange(NIB_N), np.fromiter(reserved, np.int64)))
        blocks = [free[(free >> 16) == b][:8] for b in range(3)]
        free = free[~np.isin(free, np.concatenate(blocks))]
        by_nibble, used = {}, 0
        for k in range(8):
            keys, z = depths_of_keys(oracle, nibble_keys(k))
            m = 2 * len(keys)
            ids = free[used:used + m].copy()
            used += m
            for b in range(3):                                                    # every nibble has ids in all three blocks
                ids[b] = blocks[b][k]
            aos[ids] = at_depths(np.repeat(units[k:k + 1], m, axis=0), np.repeat(z, 2), rng)
            by_nibble[k] = (keys, ids)
        every = np.concatenate([ids for _, ids in by_nibble.values()])
        assert np.unique(every).size == every.size and not (set(every.tolist()) & reserved)
        for (tile, first), z in zip(NIB_RUNS, (1.7, 23.0)):
            one = at_depths(units[tile:tile + 1], [z], rng)
            aos[first:first + NIB_RUN_LEN] = one
        pad = screen_splat(oracle, SMALL_W, SMALL_H, SMALL_W / 2, SMALL_H / 2, 1.0, 100.0, 0.01).astype(np.float32)
        aos[list(NIB_PADS)] = at_depths(pad[None, :], [5.0], rng)
        return aos, by_nibble
    aos, by_nibble = cached("nibble_scene", make)
    return aos, SMALL_W, SMALL_H, by_nibble


def nibble_frame(oracle):
    aos, w, h, _ = nibble_scene(oracle)
    return cached("nibble_frame", lambda: oracle_frame(oracle, aos, w, h))


def test_nibble_scene_is_what_it_claims(oracle_mod):
    aos, w, h, by_nibble = nibble_scene(oracle_mod)
    ref = nibble_frame(oracle_mod)
    e = ref["e"]
    assert e == sum(ids.size for _, ids in by_nibble.values()) + 2 * NIB_RUN_LEN + SMALL_TILES * len(NIB_PADS)
    print("keys per nibble:", [len(by_nibble[k][0]) for k in range(8)])
    tile, depth, ident = ref["tile"][:e], ref["depth"][:e], ref["id"][:e]
    pads = np.isin(ident, NIB_PADS)
    for k in range(8):
        sel = (tile == k) & ~pads
        keys = depth[sel]
        assert len(by_nibble[k][0]) >= NIB_MIN_KEYS, (k, by_nibble[k][0])
        want = np.repeat(np.asarray(by_nibble[k][0], np.uint32), 2)
        assert np.array_equal(keys, want), k                                      # keys that differ in nibble k alone, twice each
        assert np.unique(keys ^ keys[0]).max() < (16 << (4 * k)) and np.all((keys ^ keys[0]) % (1 << (4 * k)) == 0)
        got = ident[sel]
        assert sorted(got.tolist()) == sorted(by_nibble[k][1].tolist())
        assert np.unique(got >> 16).size >= 3                                     # the high index byte differs inside the tile
        assert not np.array_equal(got, np.sort(got))                              # ... and the key order is not the id order
        assert np.all(got.reshape(-1, 2)[:, 0] < got.reshape(-1, 2)[:, 1])        # equal keys: stable, ascending ids
    for t, first in NIB_RUNS:
        sel = (tile == t) & ~pads
        assert np.unique(depth[sel]).size == 1
        assert np.array_equal(ident[sel], np.arange(first, first + NIB_RUN_LEN))  # the run straddles a multiple of 65,536
        assert (first >> 16) != ((first + NIB_RUN_LEN - 1) >> 16)
    assert np.unique(depth[pads]).size == 1
    for t in range(SMALL_TILES):
        assert np.array_equal(ident[pads & (tile == t)], np.asarray(NIB_PADS))
    assert min(NIB_PADS) < 3 * 65536 <= max(NIB_PADS) < NIB_N


# ---- low ids -------------------------------------------------------------------------------------------------------------------
LOW_N = 70_000


def low_scene(oracle):
    def make():
        front, w, h = short_scene(oracle, 4097, 0)
        filler = front[0].copy()
        filler[2] = -abs(filler[2])                                               # behind the camera
        return np.concatenate([front, np.tile(filler, (LOW_N - front.shape[0], 1))]).astype(np.float32)
    return cached("low_scene", make), SMALL_W, SMALL_H


def low_frame(oracle):
    aos, w, h = low_scene(oracle)
    return cached("low_frame", lambda: oracle_frame(oracle, aos, w, h))


def test_low_id_scene_is_what_it_claims(oracle_mod):
    aos, w, h = low_scene(oracle_mod)
    ref = low_frame(oracle_mod)
    assert aos.shape[0] == LOW_N > 65536 and ref["e"] == 4097
    assert ref["id"][:ref["e"]].max() < 6200
