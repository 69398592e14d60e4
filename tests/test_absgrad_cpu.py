"""Absolute screen gradients (include/gsplat.h, gs_set_abs_gradients), on the CPU: the float64 reference of the AbsGS pair
-- the tile walk and blend of tests/frame64.py with one zero offset per (list element, pixel) instead of test_densify_cpu's
one per splat, so that the gradient of the offsets holds the per-pixel terms -- the proof that this reference may be trusted,
and the designed scenes tests/test_absgrad_gpu.py runs on the MI355X (cancellation, one pixel, the staging batch edges, the
early-out over stale scratch, a truncated list), each checked here for being what it claims."""
import ctypes as C
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from test_outputs_cpu import known_answer_scene, load_scene, oracle_params
from test_backward_cpu import check_truncated, frozen_of, list_offsets, screen_splat, truncated_scene
from frame64 import frame_decisions, live_of, pair_terms, raster32, splat_values, weights
from test_densify_cpu import screen_gradient, screen_norm

torch = pytest.importorskip("torch")

F = np.float32
BATCH_COUNTS = (1, 63, 64, 65, 128, 129)          # kBwdBatch = 64: one batch part and full, two and three with a rest of 1


# ---- the reference ----------------------------------------------------------------------------------------------------------

def splat_values64(p, rec, ref, frozen=None, r32=None):
    """The per-splat part of forward64: (sx, sy, ix, iy, iz, col [N, 3], opac, zview) in float64, the columns of
    frame64.splat_values (frozen splats: the float32 frame's values)."""
    v, _ = splat_values(p, rec, live_of(ref), frozen=frozen, r32=r32)
    return v[:, 0], v[:, 1], v[:, 2], v[:, 3], v[:, 4], v[:, 5:8], v[:, 8], v[:, 9]


def abs_screen_gradient(p, aos, ref, flags, w_rgba, w_depth=None, frozen=None):
    """(abs [N, 2], signed [N, 2]) in float64 of L = sum w_rgba * RGBA32F + sum w_depth * depth: frame64.pair_terms of width
    2, a zero offset per (list element, pixel) added to (sx, sy) of that element at that pixel only.  Its gradient holds the
    per-pixel terms of dL/d(sx, sy); abs() of it, or the terms as they are, summed over the 256 pixels and then over the
    elements of each splat."""
    n = len(aos)
    with torch.no_grad():
        vals, _ = splat_values(p, torch.tensor(np.asarray(aos, np.float64)), live_of(ref), frozen=frozen,
                               r32=raster32(p, aos, ref) if frozen is not None else None)
    absum = torch.zeros(n, 2, dtype=torch.float64)
    signed = torch.zeros(n, 2, dtype=torch.float64)
    for g, grad in pair_terms(p, vals, ref, flags, w_rgba, w_depth, width=2):
        absum.index_add_(0, g, grad.abs().sum(1))
        signed.index_add_(0, g, grad.sum(1))
    return absum.numpy(), signed.numpy()


@functools.lru_cache(maxsize=None)
def _scene_reference(scene):
    import oracle
    aos, w, h, cam = load_scene(scene)
    p = oracle_params(oracle, w, h, **cam)
    return aos, w, h, p


@pytest.mark.parametrize("scene", ["ragged", "dense", "ragged@pose"])
def test_the_reference_is_trusted(oracle_mod, tmp_path, scene):
    """The signed sum of the per-pixel terms is screen_gradient's dL/d(sx, sy) within 1e-10 max|ds| (both float64, the same
    expressions); the absolute pair is >= |signed pair| for every splat and exactly 0 outside the emitting splats; on `dense`
    it exceeds twice the signed norm for more than 100 splats: the statistic is not the old one in disguise."""
    aos, w, h, p = _scene_reference(scene)
    ref, flags = frame_decisions(tmp_path, p, aos)
    wr, wd = weights(h, w, 1)
    fz = frozen_of(scene.partition("@")[0], aos)
    frozen = fz if fz.any() else None
    ab, sg = abs_screen_gradient(p, aos, ref, flags, wr, wd, frozen)
    ds, _ = screen_gradient(p, aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64), frozen)
    scale = np.abs(ds).max()
    assert scale > 0 and np.abs(sg - ds).max() <= 1e-10 * scale, (np.abs(sg - ds).max(), scale)
    assert np.all(ab >= np.abs(sg))
    emitting = np.unique(np.asarray(ref["id"])[:ref["e"]])
    assert not ab[np.setdiff1d(np.arange(len(aos)), emitting)].any() and np.count_nonzero(ab.any(1)) > 100
    more = int(np.count_nonzero(screen_norm(ab, w, h) > 2.0 * screen_norm(sg, w, h)))
    print(f"{scene}: the absolute norm exceeds twice the signed one for {more} of {len(emitting)} emitting splats")
    if scene == "dense":
        assert more > 100, more


# ---- the designed scenes (shared with tests/test_absgrad_gpu.py) ------------------------------------------------------------

def cancellation_case():
    """One splat centred on pixel (32, 24) of 64 x 48 -- on the edge between tiles (1, 1) and (2, 1), the middle of tile row 1,
    so its two list elements hold half of the pixels each -- under a uniform positive dL/dRGBA32F and no depth gradient: the
    per-pixel terms of opposite pixels cancel."""
    aos, w, h = known_answer_scene([2.0])
    return aos, w, h, (np.full((h, w, 4), 0.25, F), None)


ONE_PIXEL_AT = (20.2, 13.85)                       # 0.2 px right of and 0.15 px above the centre of pixel (20, 14)


def one_pixel_case(oracle):
    """One splat of opacity 0.008 and 0.3 px (0.62 px with the dilation) centred at ONE_PIXEL_AT: alpha reaches 1 / 255 at
    pixel (20, 14) alone (0.0077 there, 0.0036 at the nearest neighbour)."""
    w, h = 64, 48
    aos = np.stack([screen_splat(oracle, w, h, ONE_PIXEL_AT[0], ONE_PIXEL_AT[1], 2.0, 0.3, 0.008)]).astype(F)
    return aos, w, h, weights(h, w, 3)


def batch_case(count):
    """`count` splats of opacity 0.02 on the camera axis, front to back: the two tiles along the centre's edge hold `count`
    entries each and no pixel stops early (0.98^129 = 0.074)."""
    aos, w, h = known_answer_scene([2.0 + 0.02 * k for k in range(count)], opacity=0.02)
    return aos, w, h, weights(h, w, 4)


STOP_FRONT = 20


def early_out_case():
    """The cloud drawn second on the context of batch_case(129), in place: as many records on the same axis, opacity 0.5;
    the front STOP_FRONT eight times as wide, the 109 behind them a quarter as wide -- wherever one of those reaches
    alpha >= 1 / 255 the front ones have taken T below 1e-4 (the centre stops after about 14 entries)."""
    aos, w, h = known_answer_scene([2.0 + 0.02 * k for k in range(129)], opacity=0.5)
    aos[:STOP_FRONT, 4:7] *= F(8.0)
    aos[STOP_FRONT:, 4:7] *= F(0.25)
    return aos, w, h, weights(h, w, 5)


def case_reference(oracle, tmp_dir, aos, w, h, g):
    """(p, ref, flags, abs [N, 2], signed [N, 2]) of a designed case under the origin camera."""
    p = oracle_params(oracle, w, h)
    ref, flags = frame_decisions(tmp_dir, p, aos)
    ab, sg = abs_screen_gradient(p, aos, ref, flags, g[0], g[1])
    return p, ref, flags, ab, sg


def test_cancellation_case(oracle_mod, tmp_path):
    aos, w, h, g = cancellation_case()
    p, ref, flags, ab, sg = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    assert ref["e"] == 2 and flags.any(1).all()                       # the two tiles along the edge, both blended
    assert screen_norm(sg, w, h)[0] < 1e-3 * screen_norm(ab, w, h)[0] and ab[0].min() > 0


def test_one_pixel_case(oracle_mod, tmp_path):
    aos, w, h, g = one_pixel_case(oracle_mod)
    p, ref, flags, ab, sg = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    assert int(np.count_nonzero(flags)) == 1                          # one (entry, pixel) pair blends in the whole frame
    e, px = (int(x[0]) for x in np.nonzero(flags))
    tile = next(t for t, (a, b) in enumerate(np.asarray(ref["ranges"]).reshape(-1, 2)) if a <= e < b)
    assert (tile % 4 * 16 + px % 16, tile // 4 * 16 + px // 16) == (20, 14)
    assert np.array_equal(ab, np.abs(sg)) and ab[0].min() > 0         # one term: its absolute value, exactly


@pytest.mark.parametrize("count", BATCH_COUNTS)
def test_batch_cases(oracle_mod, tmp_path, count):
    aos, w, h, g = batch_case(count)
    p, ref, flags, ab, sg = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    lengths = np.diff(np.asarray(ref["ranges"]).reshape(-1, 2), axis=1).ravel()
    assert sorted(lengths[lengths > 0].tolist()) == [count] * 2 and ref["e"] == 2 * count
    assert not (flags == 2).any() and flags.any(1).all()              # no pixel stops, every entry is blended
    assert np.all(ab.min(1) > 0) and np.all(ab >= np.abs(sg))


def test_early_out_case(oracle_mod, tmp_path):
    aos, w, h, g = early_out_case()
    p, ref, flags, ab, sg = case_reference(oracle_mod, tmp_path, aos, w, h, g)
    touched, _ = list_offsets(ref)
    assert np.all(touched > 0) and (flags == 2).any()
    reached = np.zeros(len(aos), bool)
    reached[np.asarray(ref["id"])[:ref["e"]][flags.any(1)]] = True
    assert reached[:STOP_FRONT].all() and not reached[STOP_FRONT:].any()
    assert np.all(ab[:STOP_FRONT].min(1) > 0) and not ab[STOP_FRONT:].any()
    a, b = np.asarray(ref["ranges"]).reshape(-1, 2)[1 * 4 + 2]        # tile (2, 1): its pixel (0, 8) is the centre (32, 24)
    assert 10 <= int(np.count_nonzero(flags[a:b, 8 * 16])) <= 16      # it stops after about 14 entries


def test_truncated_case(oracle_mod, tmp_path):
    """truncated_scene of tests/test_backward_cpu.py (64 x 64, 2500 splats, 34207 elements against a capacity of 32768): the
    splats wholly past the capacity have a zero pair in the reference, the straddling one a non-zero pair."""
    aos, w, h = truncated_scene()
    p, ref, flags, ab, sg = case_reference(oracle_mod, tmp_path, aos, w, h, weights(h, w, 6))
    across, past = check_truncated(ref, flags)
    assert not ab[past].any() and ab[across].any() and np.count_nonzero(ab.any(1)) > 100


# ---- the entry points ---------------------------------------------------------------------------------------------------------

def test_absgrad_entry_points_refuse_a_null_context():
    """GS_ERR_INVALID on a NULL context, no crash; the API version is unchanged (callers detect the calls by symbol)."""
    from vk3dgaussiansplatting_amd import _lib
    L = _lib.lib()
    buf = np.zeros(8, F)
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert L.gs_set_abs_gradients(None, 1) == _lib.GS_ERR_INVALID
    assert L.gs_abs_screen_gradient_device(None, ptr, ptr, 1, ptr) == _lib.GS_ERR_INVALID
    assert L.gs_densify_stats_abs_device(None, ptr, ptr, 1, 1, ptr) == _lib.GS_ERR_INVALID
    assert not buf.any() and _lib.API_VERSION == 7 and L.gs_api_version() == 7
    for name in ("setAbsGradients", "absScreenGradientDevice", "densifyStatsAbsDevice"):
        assert callable(getattr(gs.Renderer, name))
