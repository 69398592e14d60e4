"""The CPU reference of gs_contrib_device and gs_prune_below_device (include/gsplat.h): tests/host/contrib_ref.c -- the loop of
blend_outputs_ref.c with the blend weight w = T * alpha written out per (entry, tile pixel), and the header's fixed-order
reduction per entry and per splat -- trusted before it is used: its weights are non-zero exactly where blend_trace_ref.c
flags, and the colour re-accumulated from them is the restatement's RGBA32F bit for bit.  The designed scenes are checked
on the oracle alone: each has splats that emit elements and are never blended, and deleting them leaves the oracle's frame
byte for byte the same.  A NumPy mask restates the prune.  tests/test_contrib_gpu.py compares the GPU with all of it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_outputs_cpu import known_answer_scene, load_scene, oracle_params, reference_outputs, assert_posed
from test_backward_cpu import batch_edge_scene, check_batch_edges, check_truncated, list_offsets, truncated_scene
from frame64 import frame_decisions

F = np.float32
_CONTRIB = {}


def contrib_lib(tmp_dir):
    """tests/host/contrib_ref.c as a shared library: -O2 -ffp-contract=off, gso_exp from oracle/libgs_oracle.so."""
    if "lib" not in _CONTRIB:
        import oracle
        oracle.lib()
        so = os.path.join(str(tmp_dir), "libcontrib_ref.so")
        odir = os.path.join(ROOT, "oracle")
        build = subprocess.run(["gcc", "-std=c11", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-I", odir, "-o", so,
                                os.path.join(ROOT, "tests", "host", "contrib_ref.c"), "-L", odir, "-lgs_oracle",
                                f"-Wl,-rpath,{odir}", "-lm"], capture_output=True, text=True)
        assert build.returncode == 0, build.stderr[-2000:]
        R = C.CDLL(so)
        R.gsb_contrib_weights.restype = None
        R.gsb_contrib_reduce.restype = None
        _CONTRIB["lib"] = R
    return _CONTRIB["lib"]


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def entry_slots(p, ref):
    """The slot of every list entry of the oracle's frame: the splat's offset (list_offsets) + the raster index of the
    entry's tile inside the splat's tile box."""
    e = int(ref["e"])
    gw, _ = gs_grid(p)
    ids = np.asarray(ref["id"])[:e].astype(np.int64)
    tile = np.asarray(ref["tile"])[:e].astype(np.int64)
    sp = ref["stage1"]["splats"]
    _, off = list_offsets(ref)
    tx, ty = tile % gw, tile // gw
    min_x, max_x, min_y = (sp[k].astype(np.int64)[ids] for k in ("min_x", "max_x", "min_y"))
    assert np.all((tx >= min_x) & (tx < max_x) & (ty >= min_y))
    return off[ids] + (ty - min_y) * (max_x - min_x) + (tx - min_x)


def gs_grid(p):
    return (p.width + 15) // 16, (p.height + 15) // 16


def contrib_reference(tmp_dir, p, aos, ref=None, state=None, want_sum=True, want_pixels=True):
    """The reference of one gs_contrib_device call on the oracle's frame of (p, aos).  state: (wmax, wsum, pixels) to
    accumulate into (copied; zeros by default).  Returns dict(ref, flags, w [E, 256], e / max / count per entry, slot,
    wmax, wsum, pixels [n], touched [n]: the splats with at least one pair)."""
    R = contrib_lib(tmp_dir)
    aos = np.ascontiguousarray(aos, dtype=F)
    ref, flags = frame_decisions(tmp_dir, p, aos, ref)
    e, n = int(ref["e"]), len(aos)
    w = np.zeros((max(e, 1), 256), F)
    R.gsb_contrib_weights(C.byref(p), _ptr(aos), _ptr(np.ascontiguousarray(ref["stage1"]["color"])),
                          _ptr(np.ascontiguousarray(ref["stage1"]["cov"])), _ptr(np.ascontiguousarray(ref["id"], dtype=np.uint32)),
                          _ptr(np.ascontiguousarray(ref["ranges"], dtype=np.uint32)), _ptr(w))
    w = w[:e]
    slot = entry_slots(p, ref)
    cap = int(ref["stage1"]["capacity"])
    assert len(np.unique(slot)) == e and (e == 0 or slot.max() < cap)     # every entry has a slot of its own below the capacity
    assert np.array_equal(np.sort(slot), np.arange(e))                     # ... and every slot below the list's end is an entry
    touched, off = list_offsets(ref)
    if state is None:
        state = (np.zeros(n, F), np.zeros(n, F), np.zeros(n, np.uint32))
    wmax, wsum, pixels = (np.ascontiguousarray(a).copy() for a in state)
    ee, em, ec = np.zeros(max(e, 1), F), np.zeros(max(e, 1), F), np.zeros(max(e, 1), np.uint32)
    fl = np.ascontiguousarray(flags) if e else np.zeros((1, 256), np.uint8)
    R.gsb_contrib_reduce(_ptr(np.ascontiguousarray(w) if e else np.zeros((1, 256), F)), _ptr(fl), C.c_uint32(e),
                         _ptr(np.ascontiguousarray(slot.astype(np.uint32))), C.c_uint32(cap), C.c_uint32(n),
                         _ptr(np.ascontiguousarray(touched.astype(np.uint32))), _ptr(np.ascontiguousarray(off.astype(np.uint64))),
                         _ptr(ee), _ptr(em), _ptr(ec), _ptr(wmax), _ptr(wsum) if want_sum else None,
                         _ptr(pixels) if want_pixels else None)
    hit = np.zeros(n, bool)
    hit[np.asarray(ref["id"])[:e][flags.any(1)]] = True
    return dict(ref=ref, flags=flags, w=w, entry_e=ee[:e], entry_max=em[:e], entry_count=ec[:e], slot=slot, wmax=wmax, wsum=wsum,
                pixels=pixels, touched=hit, emitting=touched > 0)


def prune_mask(score, threshold):
    """keep(g) = score[g] >= threshold in float32, exactly as the header writes it: a NaN score compares false."""
    with np.errstate(invalid="ignore"):
        return np.asarray(score, F) >= F(threshold)


def prune_ref(score, threshold, arrays, max_out):
    """The NumPy restatement of gs_prune_below_device: (kept, dropped) and, per given array, the rows written (the first
    min(kept, max_out) kept rows in ascending g)."""
    keep = prune_mask(score, threshold)
    kept = int(keep.sum())
    return (kept, len(keep) - kept), [None if a is None else a[keep][:max_out] for a in arrays]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


SCENE_NAMES = ["ragged", "dense", "zero_det", "ragged@pose"]


def scene_reference(oracle_mod, tmp_dir, name, cache={}):
    """(aos, w, h, cam, p, reference) of a scene of SCENE_NAMES, computed once per session and never modified."""
    if name not in cache:
        aos, w, h, cam = load_scene(name)
        p = oracle_params(oracle_mod, w, h, 0, **cam)
        c = contrib_reference(tmp_dir, p, aos)
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        cache[name] = (aos, w, h, cam, p, c)
    return cache[name]


@pytest.mark.parametrize("scene", SCENE_NAMES)
def test_weights_are_the_frames_own(oracle_mod, tmp_path, scene):
    """w != 0 exactly where gsb_blend_trace flags, and col = col + w * c in entry order is gsb_render_outputs' RGBA32F rgb
    bit for bit: the weights are the ones the frame blended with."""
    aos, w, h, cam, p, c = scene_reference(oracle_mod, tmp_path, scene)
    if cam:
        assert_posed(p)
    ref, flags, wts = c["ref"], c["flags"], c["w"]
    assert np.array_equal(wts != 0, flags != 0) and np.all(wts >= 0) and np.all(np.isfinite(wts))
    out = reference_outputs(tmp_path, p, aos, ref=ref)
    col = np.asarray(ref["stage1"]["color"], F)
    ids = np.asarray(ref["id"])[:ref["e"]]
    ranges = np.asarray(ref["ranges"]).reshape(-1, 2).astype(np.int64)
    gw, gh = gs_grid(p)
    img = np.zeros((gh * 16, gw * 16, 3), F)
    for t, (s, e) in enumerate(ranges):
        acc = np.zeros((256, 3), F)
        for k in range(s, e):
            wk = wts[k]
            if wk.any():
                acc = np.where(wk[:, None] != 0, acc + wk[:, None] * col[ids[k], :3][None, :], acc)
        ty, tx = divmod(t, gw)
        img[16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = acc.reshape(16, 16, 3)
    assert np.array_equal(bits(img[:h, :w]), bits(out["rgba32f"][..., :3]))
    # the per-entry reduction against plain NumPy: the count, the maximum, and the sum up to association
    assert np.array_equal(c["entry_count"], (flags != 0).sum(1)) and np.array_equal(c["entry_max"], wts.max(1))
    assert np.allclose(c["entry_e"], wts.astype(np.float64).sum(1), rtol=1e-5, atol=0)
    # ... and per splat, by id alone (no slot arithmetic): the same count and maximum
    n = len(aos)
    cnt, top = np.zeros(n, np.int64), np.zeros(n, F)
    np.add.at(cnt, ids, (flags != 0).sum(1))
    np.maximum.at(top, ids, wts.max(1))
    s64 = np.zeros(n)
    np.add.at(s64, ids, wts.astype(np.float64).sum(1))
    assert np.array_equal(c["pixels"], cnt.astype(np.uint32)) and np.array_equal(bits(c["wmax"]), bits(top))
    assert np.allclose(c["wsum"], s64, rtol=1e-5, atol=0) and np.array_equal(c["touched"], cnt > 0)


def test_known_answer(oracle_mod, tmp_path):
    """Two splats of opacity 0.5 on the camera axis at depths 2 and 4: the centre pixel blends the first with w = 0.5 and
    the second with T = 0.5, w = 0.25, each splat's largest weight, exactly."""
    aos, w, h = known_answer_scene((2.0, 4.0))
    c = contrib_reference(tmp_path, oracle_params(oracle_mod, w, h), aos)
    assert c["wmax"][0] == F(0.5) and c["wmax"][1] == F(0.25)
    assert c["pixels"][0] > 0 and c["pixels"][1] > 0 and c["wsum"][0] > c["wmax"][0]


@pytest.mark.parametrize("scene", ["ragged", "dense", "zero_det"])
def test_never_blended_splats_can_go(oracle_mod, tmp_path, scene):
    """Each designed scene has emitting splats no pixel ever blends (and blended ones), and the oracle's frame without every
    splat of reference wmax == 0 is byte for byte the frame with them."""
    aos, w, h, cam, p, c = scene_reference(oracle_mod, tmp_path, scene)
    silent = c["emitting"] & ~c["touched"]
    print(f"{scene}: {int(c['emitting'].sum())} emitting splats, {int(silent.sum())} never add colour to any pixel")
    assert silent.sum() >= 1 and c["touched"].sum() >= 1
    assert np.array_equal(c["wmax"] > 0, c["touched"])
    keep = prune_mask(c["wmax"], np.nextafter(F(0), F(1)))
    assert np.array_equal(keep, c["touched"])
    pruned = oracle_mod.full_pipeline(p, np.ascontiguousarray(aos[keep]))
    assert pruned["stage1"]["counter"] <= pruned["stage1"]["capacity"]
    assert np.array_equal(pruned["image"], c["ref"]["image"])


def test_list_edge_scenes_hold(oracle_mod, tmp_path):
    """truncated_scene and batch_edge_scene are what tests/test_backward_cpu.py designed, and the reference treats them as
    the header says: splats wholly past the capacity stay untouched, the straddling splat counts its surviving elements,
    records no pixel blends stay untouched."""
    aos, w, h = truncated_scene()
    c = contrib_reference(tmp_path, oracle_params(oracle_mod, w, h), aos)
    g, past = check_truncated(c["ref"], c["flags"])
    assert c["pixels"][g] > 0 and c["wmax"][g] > 0 and not c["pixels"][past].any() and not c["wmax"][past].any()
    aos, w, h, _ = batch_edge_scene(oracle_mod)
    c = contrib_reference(tmp_path, oracle_params(oracle_mod, w, h), aos)
    unblended = check_batch_edges(c["ref"], c["flags"])
    assert unblended.sum() > 60 and not c["pixels"][unblended].any() and np.all(c["pixels"][~unblended] > 0)


def test_accumulation_and_saturation_of_the_reference(oracle_mod, tmp_path):
    """A second call on the same frame: wmax stays, wsum = fl(S + S), pixels doubles; a count near 2^32 saturates."""
    aos, w, h, cam, p, c = scene_reference(oracle_mod, tmp_path, "ragged")
    start = (c["wmax"], c["wsum"], np.where(c["touched"], np.uint32(0xFFFFFFFE), c["pixels"]).astype(np.uint32))
    twice = contrib_reference(tmp_path, p, aos, ref=c["ref"], state=start)
    assert np.array_equal(bits(twice["wmax"]), bits(c["wmax"])) and np.array_equal(bits(twice["wsum"]), bits(c["wsum"] + c["wsum"]))
    assert np.all(twice["pixels"][c["touched"]] == 0xFFFFFFFF) and not twice["pixels"][~c["touched"]].any()
    alone = contrib_reference(tmp_path, p, aos, ref=c["ref"], want_sum=False, want_pixels=False)
    assert np.array_equal(bits(alone["wmax"]), bits(c["wmax"])) and not alone["wsum"].any() and not alone["pixels"].any()


def test_prune_mask_restates_the_comparison():
    score = np.array([0.0, -0.0, 1e-45, 0.5, np.nan, np.inf, -np.inf, 0.25], F)
    assert prune_mask(score, 0.25).tolist() == [False, False, False, True, False, True, False, True]
    assert prune_mask(score, np.nextafter(F(0), F(1))).tolist() == [False, False, True, True, False, True, False, True]
    assert prune_mask(score, -np.inf).tolist() == [True, True, True, True, False, True, True, True]
    rows = np.arange(8 * 84, dtype=F).reshape(8, 84)
    (kept, dropped), (out, none) = prune_ref(score, 0.25, [rows, None], 2)
    assert (kept, dropped) == (3, 5) and none is None and np.array_equal(out, rows[[3, 5]])


def test_contrib_entry_points_refuse_a_null_context():
    """gs_contrib_device / gs_prune_below_device: GS_ERR_INVALID on a NULL context, no crash, without a GPU; the binding
    lists both."""
    L = _lib.lib()
    buf = np.zeros(84, F)
    cnt = np.zeros(2, np.uint32)
    assert L.gs_contrib_device(None, 1, _ptr(buf), None, None) == _lib.GS_ERR_INVALID
    assert L.gs_prune_below_device(None, _ptr(buf), 0.5, 1, _ptr(buf), None, None, None, _ptr(buf), None, None, None, 1,
                                   _ptr(cnt)) == _lib.GS_ERR_INVALID
    assert {"gs_contrib_device", "gs_prune_below_device"} <= set(_lib.EXPORTS)
    assert hasattr(gs.Renderer, "contribDevice") and hasattr(gs.Renderer, "pruneBelowDevice")
