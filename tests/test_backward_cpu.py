"""The float64 reference of the frame's gradients (include/gsplat.h, gs_backward), on the CPU: what makes tests/frame64.py
trusted, and the scenes of the gradient tests.  frame64.forward64 is the EXACT frame restated in torch with the float32
frame's decisions held fixed; two checks here stand behind it: its RGBA32F and depth match the float32 C restatement to
1e-5, and its gradients match its own central differences.  tests/test_backward_gpu.py compares the GPU's gradients with it.
Helpers are shared with that file.

At full size (13 M to 33 M list elements) the reference is evaluated on sampled tiles: with loss weights that are zero
outside a set of tiles the gradient follows from those tiles' lists alone, so sampled_reference_gradient runs forward64
on the frame's own sorted list restricted to them and on the splats that appear in it.  It is trusted by a third check
here: on the small scenes it equals the full reference to 1e-12, and the full reference is exactly zero outside the
union.  tests/test_backward_fullsize_gpu.py compares the GPU's gradients with it at configs C, D, C-hard and the
1600 x 900 README shape; its scenes (a padded cloud, a list whose counter passes 2^32) are checked on the oracle here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

from test_outputs_cpu import SCENES, POSES, assert_posed, in_front_of, load_scene, oracle_params, reference_outputs
from frame64 import forward64, frame_decisions, ptr, raster32, reference_gradient, trace_lib

torch = pytest.importorskip("torch")


def frozen_of(scene, aos):
    """The splats forward64 takes as float32 constants in a scene of SCENES: the zero_det needles."""
    fz = np.zeros(len(aos), bool)
    if scene == "zero_det":
        fz[:600] = True
    return fz


def small_scene():
    from vk3dgaussiansplatting_amd import synth
    aos = synth.generate(300, 64, 48, -2.5, seed=11)
    return aos, 64, 48


def extreme_cloud():
    """96 x 64, 400 splats with opacity exactly 0 and 1, zero quaternions and zero scales among them."""
    from vk3dgaussiansplatting_amd import synth
    aos = synth.generate(400, 96, 64, -2.0, seed=23)
    aos[0:40, 15] = 0.0
    aos[40:80, 15] = 1.0
    aos[80:100, 8:12] = 0.0
    aos[100:120, 4:7] = 0.0
    aos[120:130, 4] = 0.0
    return aos, 96, 64


def screen_splat(oracle, w, h, sx, sy, z, sigma_px, opacity, colour=(0.3, -0.2, 0.5)):
    """A round splat of the origin camera centred on screen point (sx, sy) at view depth z, of about sigma_px pixels
    before the 0.3 blur (the inverse of the projection, in float64); flat along the view axis, whose extent would
    stretch it off the image centre."""
    _, proj = oracle.camera_matrices(np.zeros(3, np.float32), 0.0, 0.0, w / h)
    p00, p11 = float(proj[0]), float(proj[5])
    x = -(2.0 * sx / w - 1.0) * z / p00                     # view (-x, y, -z); ndc = (p00 vx, p11 vy) / z
    y = (1.0 - 2.0 * sy / h) * z / p11
    s = sigma_px * z / (0.5 * p00 * w)
    from vk3dgaussiansplatting_amd import makeGaussian
    return makeGaussian((x, y, z), (s, s, 1e-3 * s), sh0=tuple(colour) + (opacity,))


def truncated_scene():
    """64 x 64 (16 tiles, list capacity ceilPow2(2500 + 16384) = 32768), 2500 rotated, anisotropic splats of 4 to 16
    tiles whose list overflows: 34207 elements, the last 103 splats wholly past the capacity and splat 2396 (offset
    32762, 16 tiles) cut after its first six.  Depth falls with the record index, so what survives of the late splats is
    in front."""
    from vk3dgaussiansplatting_amd import makeGaussian
    n, w, h = 2500, 64, 64
    rng = np.random.default_rng(41)
    z = np.linspace(4.0, 2.0, n)
    xy = rng.uniform(-0.45, 0.45, (n, 2)) * z[:, None]
    s = np.exp(rng.uniform(np.log(0.1), np.log(1.2), n))[:, None] * z[:, None] * np.exp(rng.uniform(-0.3, 0.3, (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    rec = [makeGaussian((float(xy[i, 0]), float(xy[i, 1]), float(z[i])), tuple(s[i]), rot=tuple(q[i]),
                        sh0=tuple(rng.uniform(-1, 1, 3)) + (float(rng.uniform(0.2, 0.8)),)) for i in range(n)]
    return np.stack(rec).astype(np.float32), w, h


def list_offsets(ref):
    """Per splat of the oracle's frame: tiles touched (its tile box) and the splat-order offset of its first element --
    the position the list's capacity cuts by."""
    sp = ref["stage1"]["splats"]
    touched = (sp["max_x"].astype(np.int64) - sp["min_x"]) * (sp["max_y"].astype(np.int64) - sp["min_y"])
    touched = np.where(sp["visible"] != 0, touched, 0)
    return touched, np.concatenate([[0], np.cumsum(touched)[:-1]])


# the stacks of batch_edge_scene: tile -> (list length, {in-tile index: local pixel (x, y) of an opaque splat on it}, opacity
# of the others); the others are round splats centred in the tile, of that opacity
BATCH_STACKS = {0: (64, {63: (5, 8)}, 0.06), 1: (65, {63: (5, 8), 64: (11, 8)}, 0.06),
                2: (128, {65: (5, 8), 127: (11, 8)}, 0.06), 3: (129, {64: (5, 8), 128: (11, 8)}, 0.06),
                4: (100, {}, 0.06),                  # no pixel stops: the whole list is blended
                5: (130, {}, None),                  # entries 0 .. 69 blended, 70 .. 129 (opacity 0.003) by no pixel
                7: (3, {}, 0.003)}                   # opacity below 1/255: no pixel of the tile blends anything


def batch_edge_scene(oracle):
    """96 x 32 (6 x 2 tiles), stacks of splats that each stay inside one tile (BATCH_STACKS), depth rising with the
    in-tile index: lists of 64, 65, 128, 129 entries on k_bwd_blend's 64-entry batches, pixels that stop (an opacity-1
    splat centred on them) at in-tile indices 63, 64, 65, 127 and 128, a tile that blends its whole list, one whose last
    60 entries no pixel reaches, and a tile whose entries no pixel blends.  Returns aos, w, h, and the tile of every
    record."""
    w, h, gw = 96, 32, 6
    rec, tile_of = [], []
    for t, (length, opaque, op) in BATCH_STACKS.items():
        ty, tx = divmod(t, gw)
        for k in range(length):
            z = 2.0 + 0.01 * k
            if k in opaque:
                lx, ly = opaque[k]
                rec.append(screen_splat(oracle, w, h, 16 * tx + lx, 16 * ty + ly, z, 1.0, 1.0))
            else:
                o = op if op is not None else (0.06 if k < 70 else 0.003)
                rec.append(screen_splat(oracle, w, h, 16 * tx + 7.5, 16 * ty + 7.5, z, 1.8, o,
                                        colour=(0.5 - 0.004 * k, 0.1 + 0.003 * k, -0.3)))
            tile_of.append(t)
    return np.stack(rec).astype(np.float32), w, h, np.array(tile_of)


def check_truncated(ref, flags):
    """The oracle's list of truncated_scene overflowed, with a splat across the capacity that the frame blends.  Returns
    (straddling splat, mask of the splats wholly past the capacity)."""
    cap = ref["stage1"]["capacity"]
    assert ref["stage1"]["counter"] > cap and ref["e"] == cap, (ref["stage1"]["counter"], cap)
    touched, off = list_offsets(ref)
    across = np.flatnonzero((off < cap) & (off + touched > cap))
    assert len(across) == 1, across
    g = int(across[0])
    blended = np.asarray(ref["id"])[:ref["e"]][flags.any(1)]
    assert g in blended                                          # its surviving elements are in front
    past = (off >= cap) & (touched > 0)
    assert past.sum() > 10
    return g, past


def check_batch_edges(ref, flags):
    """batch_edge_scene as intended: its list lengths, the in-tile indices pixels stop on, a tile that blends its whole
    list without a stop, one whose tail no pixel reaches and one that blends nothing.  Returns the mask of the records no
    pixel blends."""
    ranges = np.asarray(ref["ranges"]).reshape(-1, 2).astype(np.int64)
    lengths = ranges[:, 1] - ranges[:, 0]
    assert {64, 65, 128, 129} <= set(lengths.tolist()), lengths
    stops, whole, tail, silent = set(), False, False, False
    for s, e in ranges:
        if e <= s:
            continue
        f = flags[s:e]
        stops |= set(np.nonzero(f == 2)[0].tolist())
        blended = np.flatnonzero(f.any(1))
        whole |= e - s > 64 and not (f == 2).any() and bool(np.all(f != 0, axis=0).any())
        tail |= len(blended) > 0 and e - s - (blended[-1] + 1) > 1
        silent |= not len(blended)
    assert {63, 64, 65, 127, 128} <= stops, sorted(stops)
    assert whole and tail and silent
    ids = np.asarray(ref["id"])[:ref["e"]]
    unblended = np.ones(len(ref["stage1"]["color"]), bool)
    unblended[ids[flags.any(1)]] = False
    return unblended


# ---- the reference on sampled tiles ---------------------------------------------------------------------------------------
# forward64 walks every tile of the frame in torch and keeps [E, 256] decisions: fine for a few thousand splats, out of
# reach for a 13 M-element frame.  But where the loss weights are zero outside a set of tiles T, L depends on the lists of
# the tiles of T only, and its whole gradient follows from those lists alone: a splat that also touches other tiles gets
# exactly nothing from them.  So the reference of a full-size frame is forward64 on the frame's OWN sorted list restricted
# to T and on the splats that appear in it (test_sampled_reference_equals_the_full_one: the same numbers as the full one).

def tile_lengths(ranges):
    r = np.asarray(ranges).reshape(-1, 2).astype(np.int64)
    return np.maximum(r[:, 1] - r[:, 0], 0)


def pick_tiles(ranges, gw, gh, seed, max_entries=100_000, n_random=24):
    """Tiles to put the loss on, from the frame's ranges: the longest list (always kept), the four corner tiles, a tile of
    the last (possibly partial) tile row and of the last tile column, the median, a low-percentile and the shortest
    non-empty list, an empty tile if there is one, and n_random seeded random tiles -- in that order of preference, as
    long as their lists together stay within max_entries.  Returns the sorted tile indices."""
    lens = tile_lengths(ranges)
    assert len(lens) == gw * gh
    filled = np.flatnonzero(lens > 0)
    by_len = filled[np.argsort(lens[filled], kind="stable")]
    want = [int(by_len[-1])] if len(by_len) else []
    want += [0, gw - 1, (gh - 1) * gw, gh * gw - 1, (gh - 1) * gw + gw // 2, (gh // 2) * gw + gw - 1]
    if len(by_len):
        want += [int(by_len[len(by_len) // 2]), int(by_len[len(by_len) // 20]), int(by_len[0])]
    empty = np.flatnonzero(lens == 0)
    if len(empty):
        want.append(int(empty[len(empty) // 2]))
    rng = np.random.default_rng(seed)
    want += [int(t) for t in rng.choice(gw * gh, min(n_random, gw * gh), replace=False)]
    picked, total = [], 0
    for t in want:
        if t in picked or (picked and total + lens[t] > max_entries):
            continue
        picked.append(t)
        total += int(lens[t])
    return np.array(sorted(picked), np.int64)


def tile_weights(w, h, tiles, seed):
    """Loss weights (dL/dRGBA32F [h, w, 4], dL/ddepth [h, w], float32) that are zero outside the tiles `tiles` and
    standard normal (x 0.1 for the depth) inside, clipped to the frame on the ragged tiles."""
    rng = np.random.default_rng(seed)
    gw = (w + 15) // 16
    wr, wd = np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.float32)
    for t in sorted(int(t) for t in tiles):
        ty, tx = divmod(t, gw)
        ys, xs = slice(ty * 16, min(ty * 16 + 16, h)), slice(tx * 16, min(tx * 16 + 16, w))
        a = rng.standard_normal((16, 16, 4)).astype(np.float32)
        d = (0.1 * rng.standard_normal((16, 16))).astype(np.float32)
        wr[ys, xs] = a[:ys.stop - ys.start, :xs.stop - xs.start]
        wd[ys, xs] = d[:ys.stop - ys.start, :xs.stop - xs.start]
    return wr, wd


def sampled_list(ids, ranges, tiles):
    """The sorted list restricted to the tiles `tiles`: (their entries concatenated in tile order, a full-length ranges
    array re-based on them and (0, 0) everywhere else)."""
    ids = np.asarray(ids)
    r = np.asarray(ranges).reshape(-1, 2).astype(np.int64)
    sub_ranges = np.zeros((len(r), 2), np.uint32)
    parts, at = [], 0
    for t in sorted(int(t) for t in tiles):
        s, e = int(r[t, 0]), int(r[t, 1])
        if e <= s:
            continue
        parts.append(ids[s:e])
        sub_ranges[t] = (at, at + e - s)
        at += e - s
    sub_ids = np.concatenate(parts).astype(np.uint32) if parts else np.zeros(0, np.uint32)
    return sub_ids, sub_ranges


def sampled_decisions(tmp_dir, p, aos, stage1, ids, ranges, tiles):
    """frame_decisions on the list restricted to `tiles`: (entries, re-based ranges, flags [entries, 256]).
    blend_trace_ref.c indexes the whole cloud (records, colour, covariance) by the global id and takes the pixel
    position from the tile index, so it runs on the restricted list as it is."""
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    sub_ids, sub_ranges = sampled_list(ids, ranges, tiles)
    flags = np.zeros((max(len(sub_ids), 1), 256), np.uint8)
    trace_lib(tmp_dir).gsb_blend_trace(C.byref(p), ptr(aos), ptr(np.ascontiguousarray(stage1["color"])),
                                       ptr(np.ascontiguousarray(stage1["cov"])), ptr(sub_ids), ptr(sub_ranges),
                                       ptr(flags))
    return sub_ids, sub_ranges, flags[:len(sub_ids)]


def sampled_reference_gradient(tmp_dir, p, aos, stage1, ids, ranges, tiles, w_rgba, w_depth, frozen=None, decisions=None):
    """reference_gradient of a frame whose loss weights are zero outside `tiles`, from the frame's own sorted list (ids,
    ranges; stage1: the oracle's per-splat colour and covariance of the whole cloud) restricted to those tiles
    (sampled_decisions, or `decisions` if given), with forward64 on the splats that appear in it, their ids remapped.
    Returns (the indices of those splats, ascending; dL/d(record) [len, 84] of them, float64); every other splat's
    gradient is zero."""
    aos = np.ascontiguousarray(aos, dtype=np.float32)
    sub_ids, sub_ranges, flags = decisions or sampled_decisions(tmp_dir, p, aos, stage1, ids, ranges, tiles)
    uniq, inverse = np.unique(sub_ids, return_inverse=True)
    sub = dict(stage1=dict(color=np.asarray(stage1["color"])[uniq], cov=np.asarray(stage1["cov"])[uniq]),
               id=inverse.reshape(-1), ranges=sub_ranges, e=len(sub_ids))
    fz = np.asarray(frozen, bool)[uniq] if frozen is not None else None
    return uniq.astype(np.int64), reference_gradient(p, aos[uniq], sub, flags, w_rgba, w_depth, fz)


def padded_cloud(aos, n, seed, filler):
    """The records `aos` scattered, order preserved, over a cloud of n records whose other records emit nothing (filler
    'behind': behind the origin camera; 'outside': in front of it, far outside the +-1.3 NDC cull).  Returns (cloud, the
    ascending positions of the live records).  k_splat_scan_blocks gives each of its 1024 threads per = ceil(ceil(n / 256)
    / 1024) consecutive 256-splat blocks: live records sit at 0 and n - 1 and on both sides of the 256 * per boundaries
    of threads 1, 63, 64 (the first of the second wave), 65, 512 and the last thread with data, the others at seeded
    positions."""
    from vk3dgaussiansplatting_amd import makeGaussian
    m = len(aos)
    per = ((n + 255) // 256 + 1023) // 1024
    step = 256 * per
    fixed = {0, n - 1}
    for k in (1, 63, 64, 65, 512, (n - 1) // step):
        if 0 < k * step < n:
            fixed |= {k * step - 1, k * step}
    assert len(fixed) <= m <= n
    rng = np.random.default_rng(seed)
    rest = np.setdiff1d(np.arange(n), np.array(sorted(fixed)))
    pos = np.sort(np.concatenate([np.array(sorted(fixed)), rng.choice(rest, m - len(fixed), replace=False)])).astype(np.int64)
    centre = {"behind": (0.1, -0.2, -5.0), "outside": (400.0, 0.0, 2.0)}[filler]
    cloud = np.tile(makeGaussian(centre, (0.05, 0.04, 0.03), sh0=(0.3, 0.2, 0.1, 0.7)).astype(np.float32), (n, 1))
    cloud[pos] = aos
    return cloud, pos


OVERFLOW_CUT = 2878


def overflowing_scene():
    """1920 x 1080, 800 000 splats that each cover the whole frame (mu = 2: scales of about 7 units), opacity 0.01 so
    that several hundred entries of every pixel blend before the early-out: the element counter is 4.5e9, past 2^32,
    against a capacity of 2^24 -- the first 2 879 records (2 057 of them emit) reach the list, the true offset of every splat from 746 052 on is at or
    beyond 2^32, and 2 370 of them have an offset that, taken modulo 2^32, falls below the capacity again (the splats
    that would collect other splats' rows if an offset wrapped instead of saturating).  Splat OVERFLOW_CUT is the one the
    capacity cuts (its first 256 of 8160 tiles survive); the cloud is stored in Morton order, so it would be the
    deepest of the surviving ones, behind every pixel's early-out: it is moved along its ray in front of the others."""
    from vk3dgaussiansplatting_amd import synth
    w, h = 1920, 1080
    aos = synth.generate(800_000, w, h, 2.0, seed=9)
    aos[:, 15] = 0.01
    aos[OVERFLOW_CUT, 0:3] *= np.float32(0.45 / aos[OVERFLOW_CUT, 2])
    return aos, w, h


def check_overflowing(s1):
    """overflowing_scene on the oracle (stage 1 with the per-splat boxes): counter past 2^32, at least 1000 'victims'
    (offset at or beyond 2^32 whose low 32 bits fall below the capacity), one splat cut by the capacity.  Returns (cut
    splat, mask of the emitting splats wholly past the capacity, mask of the victims)."""
    cap = s1["capacity"]
    assert s1["counter"] > 2**32 and cap == 2**24, (s1["counter"], cap)
    touched, off = list_offsets(dict(stage1=s1))
    assert int(touched.sum()) == s1["counter"]
    across = np.flatnonzero((off < cap) & (off + touched > cap))
    assert across.tolist() == [OVERFLOW_CUT], across
    past = (off >= cap) & (touched > 0)
    victims = past & (off >= 2**32) & ((off % 2**32) < cap)
    assert victims.sum() >= 1000, victims.sum()
    return int(across[0]), past, victims


def overflow_tiles(ranges, gw, gh, sorted_tile, sorted_id, across):
    """The tiles the by-value check of overflowing_scene puts its loss on: pick_tiles within 40 000 entries; the corner
    tile 0 among them is one of the tiles the cut splat survives in."""
    tiles = pick_tiles(ranges, gw, gh, seed=3, max_entries=40_000)
    assert 0 in tiles and 0 in sorted_tile[sorted_id == across]
    return tiles


def read_fields_of(sh_mode):
    """The record fields a frame of this SH mode reads: position, scale, rotation, opacity and the rgb of the SH
    coefficients it evaluates (0: all 16, 1: 1 .. 15, 2: the first)."""
    ks = {0: range(16), 1: range(1, 16), 2: range(1)}[sh_mode]
    return [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 15] + [12 + 4 * k + c for k in ks for c in range(3)]


# ---- tests ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scene,sh_mode", [("ragged", 0), ("ragged", 1), ("ragged", 2), ("dense", 0), ("zero_det", 0),
                                           ("ragged@pose", 0), ("ragged@pose", 1), ("ragged@garden", 0)])
def test_reference_forward_matches_the_restatement(oracle_mod, tmp_path, scene, sh_mode):
    """The float64 frame with the float32 decisions equals the C restatement's RGBA32F and depth to 1e-5 relative + 2e-5
    absolute (the absolute part is the float32 restatement's own rounding on pixels that blend a few hundred entries: one
    pixel of the ragged scene is 1.5e-5 off): the restatement and the float64 one describe the same function -- also at
    posed cameras, where the view block is not symmetric and the depth row and camera position are not trivial."""
    aos, w, h, cam = load_scene(scene)
    p = oracle_params(oracle_mod, w, h, sh_mode, **cam)
    if cam:
        assert_posed(p)
    ref, flags = frame_decisions(tmp_path, p, aos)
    c = reference_outputs(tmp_path, p, aos, ref=ref)
    fz = frozen_of(scene, aos)
    with torch.no_grad():
        rgba, dep = forward64(p, torch.tensor(aos.astype(np.float64)), ref, flags, fz, raster32(p, aos, ref))
    rgba, dep = rgba.numpy(), dep.numpy()
    assert np.count_nonzero(flags) > 1000
    np.testing.assert_allclose(rgba, c["rgba32f"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(dep, c["depth"], rtol=1e-5, atol=2e-5 * max(1.0, float(np.abs(c["depth"]).max())))


def _check_central_differences(tmp_path, p, aos, rng, pairs):
    """autograd of forward64 against its own central differences on `pairs` sampled (gaussian, field) pairs, plus the
    exact zeros of the fields and splats the frame does not read."""
    w, h = p.width, p.height
    ref, flags = frame_decisions(tmp_path, p, aos)
    wr, wd = rng.standard_normal((h, w, 4)), rng.standard_normal((h, w)) * 0.1
    grad = reference_gradient(p, aos, ref, flags, wr, wd)
    emitting = np.unique(np.asarray(ref["id"])[:ref["e"]])
    fields = [0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 15] + [12 + 4 * k + c for k in range(16) for c in range(3)]
    base = torch.tensor(aos.astype(np.float64))

    def loss(r):
        with torch.no_grad():
            a, d = forward64(p, r, ref, flags)
        return float((a.numpy() * wr).sum() + (d.numpy() * wd).sum())

    checked = 0
    for f in pairs:
        g, f = int(rng.choice(emitting)), int(rng.choice(fields) if f is None else f)
        step = 1e-6 * max(1.0, abs(float(aos[g, f])))
        rp, rm = base.clone(), base.clone()
        rp[g, f] += step
        rm[g, f] -= step
        fd = (loss(rp) - loss(rm)) / (2 * step)
        assert abs(fd - grad[g, f]) <= 1e-5 + 1e-4 * abs(fd), (g, f, fd, grad[g, f])
        checked += 1
    assert checked == len(pairs)
    assert np.all(grad[:, [3, 7]] == 0) and np.all(grad[:, 76:] == 0)
    assert np.all(grad[:, 19:76:4] == 0)                    # shCoeffs[1..15].a
    culled = np.setdiff1d(np.arange(len(aos)), emitting)
    assert np.all(grad[culled] == 0)
    return grad


@pytest.mark.parametrize("sh_mode", [0, 1, 2])
def test_reference_gradient_matches_central_differences(oracle_mod, tmp_path, sh_mode):
    """autograd of the float64 frame against its own central differences (decisions held fixed) on 40 sampled
    (gaussian, field) pairs of the 59 fields a frame reads, L = sum w * RGBA32F + sum v * depth with random w, v."""
    aos, w, h = small_scene()
    p = oracle_params(oracle_mod, w, h, sh_mode)
    _check_central_differences(tmp_path, p, aos, np.random.default_rng(3 + sh_mode), [None] * 40)


@pytest.mark.parametrize("pose,sh_mode", [("pose", 0), ("pose", 1), ("garden", 0), ("garden", 1)])
def test_reference_gradient_matches_central_differences_posed(oracle_mod, tmp_path, pose, sh_mode):
    """The same at posed cameras (rotated and translated: the view block is not symmetric, the SH direction is taken
    from the camera position), in the SH modes whose colour depends on the direction: 40 sampled pairs and 15 more on
    the position, whose derivative carries the view block, the depth row and p - cam_pos."""
    aos, w, h = small_scene()
    aos = in_front_of(aos, w, h, pose)
    pos, yaw, pitch = POSES[pose]
    p = oracle_params(oracle_mod, w, h, sh_mode, pos=pos, yaw=yaw, pitch=pitch)
    assert_posed(p)
    _check_central_differences(tmp_path, p, aos, np.random.default_rng(13 + sh_mode), [None] * 40 + [0, 1, 2] * 5)


@pytest.mark.parametrize("scene", ["truncated", "batch_edges"])
def test_reference_forward_on_list_edges(oracle_mod, tmp_path, scene):
    """The scenes of the list-edge GPU tests are what they claim (check_truncated, check_batch_edges), and the float64
    frame matches the C restatement on them as on the others: on an overflowed, truncated list, and on stacks whose
    lengths and stops sit on the edges of k_bwd_blend's 64-entry batches."""
    if scene == "truncated":
        aos, w, h = truncated_scene()
    else:
        aos, w, h, _ = batch_edge_scene(oracle_mod)
    p = oracle_params(oracle_mod, w, h)
    ref, flags = frame_decisions(tmp_path, p, aos)
    if scene == "truncated":
        check_truncated(ref, flags)
    else:
        check_batch_edges(ref, flags)
    c = reference_outputs(tmp_path, p, aos, ref=ref)
    assert np.array_equal(c["rgba"], ref["image"])
    with torch.no_grad():
        rgba, dep = forward64(p, torch.tensor(aos.astype(np.float64)), ref, flags)
    np.testing.assert_allclose(rgba.numpy(), c["rgba32f"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(dep.numpy(), c["depth"], rtol=1e-5, atol=2e-5 * max(1.0, float(np.abs(c["depth"]).max())))


def _list_edge_or_loaded(oracle_mod, scene):
    if scene == "truncated":
        return truncated_scene() + ({},)
    if scene == "batch_edges":
        return batch_edge_scene(oracle_mod)[:3] + ({},)
    return load_scene(scene)


@pytest.mark.parametrize("scene", ["ragged", "ragged@pose", "dense", "truncated", "batch_edges"])
def test_sampled_reference_equals_the_full_one(oracle_mod, tmp_path, scene):
    """What lets the full-size GPU tests trust sampled_reference_gradient: with loss weights that are zero outside the
    picked tiles, the gradient from the restricted list and the sub-cloud equals the full reference_gradient of the same
    weights to 1e-12 of each column's maximum (the same float64 arithmetic on the same entries), and the full one is
    exactly zero on every splat outside the union of the picked lists."""
    aos, w, h, cam = _list_edge_or_loaded(oracle_mod, scene)
    p = oracle_params(oracle_mod, w, h, **cam)
    ref, flags = frame_decisions(tmp_path, p, aos)
    e, (gw, gh) = int(ref["e"]), oracle_mod.grid(w, h)
    tiles = pick_tiles(ref["ranges"], gw, gh, seed=5, n_random=3)
    lens = tile_lengths(ref["ranges"])
    assert lens[tiles].max() == lens.max() and 0 < lens[tiles].sum() < e          # the longest list; a strict subset
    assert {0, gw - 1, (gh - 1) * gw, gh * gw - 1} <= set(tiles.tolist())
    wr, wd = tile_weights(w, h, tiles, seed=8)
    inside = np.zeros((gh * 16, gw * 16), bool)
    for t in tiles:
        inside[t // gw * 16:t // gw * 16 + 16, t % gw * 16:t % gw * 16 + 16] = True
    assert np.all(wr[~inside[:h, :w]] == 0) and np.all(wd[~inside[:h, :w]] == 0) and np.all(wr[inside[:h, :w]] != 0)
    full = reference_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64))
    uniq, got = sampled_reference_gradient(tmp_path, p, aos, ref["stage1"], ref["id"][:e], ref["ranges"], tiles,
                                           wr.astype(np.float64), wd.astype(np.float64))
    assert got.shape == (len(uniq), 84) and np.count_nonzero(np.abs(got).sum(1)) > 20
    outside = np.ones(len(aos), bool)
    outside[uniq] = False
    assert np.all(full[outside] == 0)
    if scene != "truncated":                                                       # its splats cover 4 to 16 of 16 tiles
        assert np.any(outside[np.asarray(ref["id"])[:e]])                          # some emitting splat is outside
    scale = np.abs(full).max(0)
    assert np.all(np.abs(got - full[uniq]) <= 1e-12 * scale), np.abs(got - full[uniq]).max(0) / np.maximum(scale, 1e-300)


@pytest.mark.parametrize("filler", ["behind", "outside"])
@pytest.mark.parametrize("n", [262_144, 262_145, 524_545, 1_048_577])
def test_padded_cloud_has_the_compact_list(oracle_mod, filler, n):
    """The scene of the compaction-invariance GPU test: the ragged cloud scattered, order preserved, over n records that
    emit nothing (padded_cloud).  The oracle's sorted list of the padded cloud, its ids mapped back, is the compact
    cloud's list, and the ranges are equal -- the sort is stable and the index map monotone."""
    aos, w, h = SCENES["ragged"]()
    p = oracle_params(oracle_mod, w, h)
    cloud, pos = padded_cloud(aos, n, seed=n, filler=filler)
    per = ((n + 255) // 256 + 1023) // 1024
    assert per == {262_144: 1, 262_145: 2, 524_545: 3, 1_048_577: 5}[n]
    assert pos[0] == 0 and pos[-1] == n - 1 and len(pos) == len(aos) and np.all(np.diff(pos) > 0)
    for k in (1, 64):
        assert {k * 256 * per - 1, k * 256 * per} <= set(pos.tolist())
    threads = oracle_mod.host_threads()
    compact = oracle_mod.full_pipeline(p, aos)
    s1 = oracle_mod.init_sort_list(p, cloud, threads=threads)
    e = min(s1["counter"], s1["capacity"])
    assert e == compact["e"] == s1["counter"]
    emitting = np.flatnonzero(s1["splats"]["visible"] != 0)
    assert np.all(np.isin(emitting, pos))                                          # the filler emits nothing
    t, d, i = oracle_mod.sort_stable(s1["tile"], s1["depth"], s1["id"], e, threads=threads)
    back = np.searchsorted(pos, i[:e])
    assert np.array_equal(pos[back], i[:e]) and np.array_equal(back, compact["id"][:e])
    assert np.array_equal(t[:e], compact["tile"][:e]) and np.array_equal(d[:e], compact["depth"][:e])
    assert np.array_equal(oracle_mod.find_ranges(t, e, len(compact["ranges"])), compact["ranges"])


def test_overflowing_scene_is_what_it_claims(oracle_mod, tmp_path):
    """The scene of the GPU test of a list past 2^32 (overflowing_scene, check_overflowing), on the oracle: the 64-bit
    counter passes 2^32, at least 1000 splats have an offset that wraps below the capacity, one splat is cut by the
    capacity and the frame blends it; and on sampled tiles the float64 reference has at least 500 non-zero rows."""
    aos, w, h = overflowing_scene()
    p = oracle_params(oracle_mod, w, h)
    threads = oracle_mod.host_threads()
    s1 = oracle_mod.init_sort_list(p, aos, threads=threads)
    across, past, victims = check_overflowing(s1)
    e, (gw, gh) = s1["capacity"], oracle_mod.grid(w, h)
    t, _, ids = oracle_mod.sort_stable(s1["tile"], s1["depth"], s1["id"], e, threads=threads, inplace=True)
    ranges = oracle_mod.find_ranges(t, e, gw * gh)
    assert not np.any(past[ids[:e]])
    tiles = overflow_tiles(ranges, gw, gh, t[:e], ids[:e], across)
    dec = sampled_decisions(tmp_path, p, aos, s1, ids[:e], ranges, tiles)
    assert np.any(dec[2][dec[0] == across])                                        # some pixel blends the cut splat
    wr, wd = tile_weights(w, h, tiles, seed=4)
    uniq, want = sampled_reference_gradient(tmp_path, p, aos, s1, ids[:e], ranges, tiles, wr.astype(np.float64),
                                            wd.astype(np.float64), decisions=dec)
    assert np.count_nonzero(np.abs(want).sum(1)) >= 500
    assert np.any(want[np.searchsorted(uniq, across)] != 0)


def test_backward_entry_points_refuse_a_null_context():
    """gs_backward / gs_backward_device / gs_upload_gaussians_device: GS_ERR_INVALID on a NULL context, no crash."""
    from vk3dgaussiansplatting_amd import _lib
    L = _lib.lib()
    buf = np.zeros(84, np.float32)
    assert L.gs_backward(None, ptr(buf), None, ptr(buf)) == _lib.GS_ERR_INVALID
    assert L.gs_backward_device(None, ptr(buf), None, ptr(buf)) == _lib.GS_ERR_INVALID
    assert L.gs_upload_gaussians_device(None, ptr(buf), 1) == _lib.GS_ERR_INVALID
    assert _lib.API_VERSION == 7


def test_autograd_module_is_not_imported_by_the_package():
    """import vk3dgaussiansplatting_amd does not import torch (the autograd module does, on its own)."""
    code = ("import sys; import vk3dgaussiansplatting_amd as gs; "
            "assert 'torch' not in sys.modules and 'vk3dgaussiansplatting_amd.autograd' not in sys.modules")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True,
                       env={**os.environ, "GS_HIP_RUNTIME": "system"})
    assert r.returncode == 0, r.stderr[-2000:]
