"""Frames and gradients on the MI355X under camera constants other than the defaults: the four configurations of
tests/test_camera_constants_cpu.py (pinhole, split, off_centre, tight -- each isolates some readers of near_plane, far_plane,
ndc_cull, in_view_limit and fov_y, and that file shows on the oracle alone that they decide) through Renderer(..., **constants).
Frames against the oracle with the same params, the float outputs against the C restatement, tile-row bands against the
oracle's band runs, the gaussians' and the camera's gradients against the float64 references, the densification statistics,
and one trainer step.  Every helper and tolerance is the existing test files' own.

What a wrong constant breaks here (each edit made alone on a copy of the sources, built for gfx950 and run against this file):
  k_project's near cull with a literal 0.1f, or its NDC cull with 1.3f: every tight frame, band, gradient and statistic
      (the CPU file counts 163 and 477 splats that only those constants cull);
  k_project's depth key with a literal 100.0f: the depth words of every pinhole and tight list (frames, outputs, bands);
  bwd_chain's clamp limit with a literal 0.8f: the gaussians' and the camera's gradients under pinhole (nothing clamps at
      1.3) and tight (two thirds of the visible splats clamp at 0.3);
  radius_bound's tan_fov_y replaced by 1.0f: the bands of pinhole, split and off_centre lose the splats the CPU file counts
      as "accepted only here" that emit (at the defaults the factor is 0.99995, inside the bound's 2 % widening);
  a screen y taken from tan_fov_y instead of proj in k_project: every frame of split and off_centre, by whole tiles;
  get_covariance's tan_fov_y replaced by 1.0f: the covariance bits of every frame."""
import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_parity_gpu import assert_frame_equals_oracle, assert_within_one_step, make_renderer
from test_outputs_cpu import reference_outputs
from test_outputs_gpu import bits, outputs
from test_band_cull_cpu import GW, H, W
from test_band_cull_gpu import assert_band, assert_rows, scene_of
from test_backward_cpu import list_offsets
from test_backward_gpu import UNREAD, compare_with_reference
from frame64 import frame_decisions, reference_gradient, weights
from test_backward_camera_cpu import PROJ_CLIP_Z, VIEW_BOTTOM_ROW, camera_reference
from test_backward_camera_gpu import check_against, check_cam_pos_central_differences
from test_camera_constants_cpu import (BAND_ROWS, BAND_RUNS, CONFIGS, CONSTANTS, DEFAULTS, FRAME_CASES, GRAD_CASES, band_cloud,
                                       band_references, case, case_id, oracle_frame)

pytestmark = pytest.mark.gpu

F = np.float32
SORTS = {"radix4": gs.GS_SORT_RADIX4, "splat_first": gs.GS_SORT_RADIX4_SPLAT_FIRST, "bucket": gs.GS_SORT_TILE_BUCKET,
         "radix8": gs.GS_SORT_RADIX8}
# GS_SORT_RADIX4 for every frame; tight and off_centre also with the sorters whose depth key is made in another kernel order
FRAME_SORTS = [(c, "radix4") for c in FRAME_CASES] + \
    [(c, s) for c in FRAME_CASES if c[0] in ("tight", "off_centre") and c[1:] == ("ragged", None) for s in ("splat_first", "bucket", "radix8")]


def drawn(c, **kw):
    """(renderer, scene) of a case of test_camera_constants_cpu.case, the context made with the configuration's constants."""
    sc = scene_of(c["aos"], c["cam"], c["w"], c["h"])
    r = make_renderer(sc, c["w"], c["h"], **kw, **c["constants"])
    for k in CONSTANTS:
        assert getattr(r.cfg, k) == F(c["constants"].get(k, DEFAULTS[k])), k
    return r, sc


# ---- frames -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which,sort", FRAME_SORTS, ids=[f"{case_id(c)}-{s}" for c, s in FRAME_SORTS])
def test_exact_frame_equals_the_oracle(oracle_mod, which, sort):
    """GS_RENDER_EXACT: element count, sorted tile / depth / id words, ranges, the covariance and colour of every splat the
    oracle keeps (GS_BUF_COLOR with the splats coloured on demand) and the pixels, np.array_equal against the oracle with the
    same params."""
    c = case(*which)
    r, sc = drawn(c, sort=SORTS[sort])
    img = r.draw(sc)
    assert_frame_equals_oracle(r, img, oracle_frame(*which))
    r.cleanup()


@pytest.mark.parametrize("name", CONFIGS)
def test_fast_frame_is_within_one_step(oracle_mod, name):
    """GS_RENDER_FAST on the ragged cloud: the list is the oracle's, every channel of every pixel within one 8-bit step."""
    which = (name, "ragged", None)
    r, sc = drawn(case(*which), mode=gs.GS_RENDER_FAST)
    img = r.draw(sc)
    assert_frame_equals_oracle(r, img, oracle_frame(*which), exact_pixels=False)
    r.cleanup()


@pytest.mark.parametrize("which", FRAME_CASES, ids=[case_id(c) for c in FRAME_CASES])
def test_float_outputs_equal_the_restatement(oracle_mod, tmp_path, which):
    """RGBA32F and depth bit for bit tests/host/blend_outputs_ref.c over the oracle's intermediates (reference_outputs)."""
    c = case(*which)
    ref = reference_outputs(tmp_path, c["p"], c["aos"], ref=oracle_frame(*which))
    r, sc = drawn(c)
    r.setOutputs(rgba32f=True, depth=True)
    img = r.draw(sc)
    f32, dep = outputs(r)
    r.cleanup()
    assert np.array_equal(img, ref["rgba"])
    assert np.array_equal(bits(f32), bits(ref["rgba32f"]))
    assert np.array_equal(bits(dep), bits(ref["depth"]))


# ---- bands ------------------------------------------------------------------------------------------------------------------
BAND_CASES = [(name, which, view, "radix4") for name in CONFIGS for which, view in BAND_RUNS] + \
    [(name, "A", "roll37", s) for name in ("pinhole", "tight") for s in ("splat_first", "bucket")]


@pytest.mark.parametrize("name,which,view,sort", BAND_CASES, ids=["-".join(c) for c in BAND_CASES])
def test_bands(oracle_mod, name, which, view, sort):
    """A context that owns the first, a middle or the ragged last tile row, or the interleaved rows 1, 4, 7, ..., under the
    configuration's constants and projection: every list in full against the oracle's run for those rows with the same
    constants.  This is where a wrong constant in radius_bound, box_misses_owned_rows or band_skip silently drops splats
    (test_camera_constants_cpu.test_the_constants_decide_the_band_culls: splats that emit into these bands and that the
    default constants would reject)."""
    cam, constants, refs = band_references(name, which, view)
    sc = scene_of(band_cloud(which), cam, W, H)
    r = make_renderer(sc, W, H, sort=SORTS[sort], **constants)
    for band, (rb, re, first, stride) in BAND_ROWS.items():
        assert refs[band]["e"] > 0
        if stride == 1:
            assert_band(r, sc, refs[band], rb, re, H, (name, which, view, band))
        else:
            r.setTileRowsInterleaved(first, stride)
            assert_rows(r, r.draw(sc), refs[band], GW, H, (name, which, view, band))
    r.cleanup()


# ---- gradients of the gaussians ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "no_depth"])
@pytest.mark.parametrize("which", GRAD_CASES, ids=[case_id(c) for c in GRAD_CASES])
def test_gradients_against_the_float64_reference(oracle_mod, tmp_path, which, with_depth):
    """gs_backward against reference_gradient with the comparison and tolerance of
    test_backward_gpu.test_against_the_float64_reference (per field |gpu - ref| <= 2e-2 |ref| + 2e-3 max|ref column|), with and
    without dL/dDEPTH; gs_backward_visible gives the same bits on the rasterised splats."""
    c = case(*which)
    aos, w, h = c["aos"], c["w"], c["h"]
    r, sc = drawn(c)
    r.draw(sc)
    wr, wd = weights(h, w, 1)
    got = r.backward(wr, wd if with_depth else None)
    r.draw(sc)
    ids, rows, count = r.backwardVisible(wr, wd if with_depth else None)
    r.cleanup()
    ref, flags = frame_decisions(tmp_path, c["p"], aos, ref=oracle_frame(*which))
    want = reference_gradient(c["p"], aos, ref, flags, wr.astype(np.float64), wd.astype(np.float64) if with_depth else None)
    assert np.all(np.isfinite(got)) and np.all(got[:, UNREAD] == 0)
    emitting = np.zeros(len(aos), bool)
    emitting[np.asarray(ref["id"])[:ref["e"]]] = True
    assert np.all(got[~emitting] == 0) and np.count_nonzero(np.abs(want).sum(1)) > 300
    bad = compare_with_reference(got, want, np.ones(len(aos), bool))
    assert not bad, bad[:10]
    touched, _ = list_offsets(ref)
    assert count == len(ids) and np.array_equal(ids, np.flatnonzero(touched != 0))
    assert np.array_equal(bits(rows), bits(got[ids]))


# ---- camera gradients -------------------------------------------------------------------------------------------------------
CAMERA_CASES = [c for c in GRAD_CASES if c[1] == "ragged"]


@pytest.mark.parametrize("which", CAMERA_CASES, ids=[case_id(c) for c in CAMERA_CASES])
def test_camera_gradients_against_the_float64_reference(oracle_mod, tmp_path, which):
    """All 35 floats of gs_backward_camera against the column sums of the float64 per-splat contributions
    (test_backward_camera_cpu.camera_reference) within test_backward_camera_gpu.TAU of S per component; the view's bottom row
    and the projection's clip-z row are exactly +0; under off_centre dL/dproj[8] and dL/dproj[9] -- zero entries of every
    other projection of the suite -- are live in the reference and on the GPU."""
    c = case(*which)
    w, h = c["w"], c["h"]
    r, sc = drawn(c)
    r.draw(sc)
    wr, wd = weights(h, w, 1)
    r.backward(wr, wd)
    got = r.backwardCamera()
    r.cleanup()
    want, S, _ = camera_reference(("camera constants",) + which, tmp_path, c["p"], c["aos"], wr, wd)
    assert np.count_nonzero(S) >= 20
    check_against(got, want, S, case_id(which))
    assert np.all(bits(got)[VIEW_BOTTOM_ROW] == 0) and np.all(bits(got)[PROJ_CLIP_Z] == 0)
    if which[0] == "off_centre":
        assert S[16 + 8] > 0 and S[16 + 9] > 0 and got[16 + 8] != 0 and got[16 + 9] != 0


def test_cam_pos_central_differences_under_split():
    """test_backward_camera_gpu.test_central_differences_for_cam_pos with proj at 90 degrees and fov_y = 1.2."""
    c = case("split", "ragged", "pose")
    r, sc = drawn(c)
    check_cam_pos_central_differences(r, sc, c["w"], c["h"], "split ragged@pose")


# ---- densification statistics -----------------------------------------------------------------------------------------------
STATS_CASES = [("pinhole", "ragged", "pose"), ("tight", "ragged", None)]


@pytest.mark.parametrize("which", STATS_CASES, ids=[case_id(c) for c in STATS_CASES])
def test_stats_after_one_step(oracle_mod, tmp_path, which):
    """test_densify_gpu.test_stats_after_one_step under pinhole and tight: seen is 1 exactly on the oracle's splats with a
    non-empty tile box, max_radius the radius NumPy computes from GS_BUF_COV bit for bit, grad_accum the norm of the float64
    screen gradient in NDC units within the gradient tolerance and exactly 0 elsewhere."""
    pytest.importorskip("torch")
    from test_densify_cpu import screen_gradient, screen_norm
    from test_densify_gpu import Frame, assert_norm, radius_of, zeros
    c = case(*which)
    aos, w, h = c["aos"], c["w"], c["h"]
    f = Frame(aos, w, h, sc=scene_of(aos, c["cam"], w, h), constants=c["constants"])
    accum, seen, radius = (a.copy() for a in f.stats(zeros(f.n)))
    cov = f.r.debugRead(gs.BUF_COV)
    V = f.visible()
    f.r.cleanup()
    ref, flags = frame_decisions(tmp_path, c["p"], aos, ref=oracle_frame(*which))
    touched, _ = list_offsets(ref)
    assert np.array_equal(V, np.flatnonzero(touched != 0)) and 500 < len(V) <= f.n
    inV = np.zeros(f.n, bool)
    inV[V] = True
    assert np.array_equal(seen, inV.astype(np.uint32))
    want_r = radius_of(cov)
    assert np.array_equal(bits(radius[inV]), bits(want_r[inV])) and not bits(radius[~inV]).any()
    assert radius[inV].min() >= 1 and len(np.unique(radius[inV])) > 5
    ds, _ = screen_gradient(c["p"], aos, ref, flags, f.wr.astype(np.float64), f.wd.astype(np.float64))
    want = screen_norm(ds, w, h)
    assert not bits(accum[~inV]).any() and np.all(np.isfinite(accum)) and np.all(accum >= 0)
    assert np.count_nonzero(want) > 100
    assert_norm(accum, want, np.ones(f.n, bool), case_id(which))


# ---- one trainer step -------------------------------------------------------------------------------------------------------

def test_one_trainer_step_under_pinhole():
    """Smoke tests on a renderer made with pinhole: a VisibleAdam(space="raw") step runs to finite numbers and moves the
    visible rows; a two-view step_batch leaves the bits that the same calls leave with a wait after each."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    from vk3dgaussiansplatting_amd.renderer import default_adam_params
    from test_train_chain_gpu import LAMBDA
    from test_camera_constants_cpu import configuration, view_camera
    c = case("pinhole", "dense", None)
    w, h, constants = c["w"], c["h"], c["constants"]
    aos = np.ascontiguousarray(c["aos"], np.float32)
    n = len(aos)
    # the second view: the generic pose with pinhole's projection at this size, looking at the same cloud from elsewhere
    cams = [c["cam"], view_camera("pose", w, h, configuration("pinhole", w, h)[1])]
    cameras = [(cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition()) for cam in cams]
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(3)
    targets = [torch.tensor(rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32), device=dev) for _ in cams]

    # one step
    rr = autograd.make_renderer(w, h, **constants)
    records = torch.tensor(aos, device=dev)
    opt = autograd.VisibleAdam(records, renderer=rr, space="raw")
    before = opt.records.clone()
    numbers = opt.step(*cameras[0], 0, targets[0], LAMBDA)
    opt.stream.synchronize()
    assert rr.cfg.fov_y == F(constants["fov_y"]) and rr.cfg.near_plane == F(constants["near_plane"])
    count = int(opt.count.cpu().numpy().view(np.uint32)[0])
    assert 500 < count < n and bool(torch.isfinite(numbers).all()) and float(numbers[0]) > 0
    assert bool(torch.isfinite(opt.records).all()) and bool(torch.isfinite(opt.raw).all())
    moved = (opt.records != before).any(dim=1).cpu().numpy()
    ids = opt.ids.cpu().numpy().view(np.uint32)[:count]
    # (most of the dense cloud's visible splats sit behind an early-out: zero gradient, zero moments, no move)
    assert moved.any() and not moved[np.setdiff1d(np.arange(n), ids)].any()
    rr.setStream(None)
    rr.cleanup()

    # a two-view batch, enqueued without waiting ...
    rr = autograd.make_renderer(w, h, **constants)
    opt = autograd.VisibleAdam(torch.tensor(aos, device=dev), renderer=rr, space="raw")
    batch_numbers = opt.step_batch(cameras, targets, 0, LAMBDA)
    opt.stream.synchronize()
    got = [t.cpu().numpy() for t in (batch_numbers, opt.records, opt.raw, opt.m, opt.v, opt.ids, opt.count)]
    rr.setStream(None)
    rr.cleanup()
    # ... and the same calls by hand on the context's own stream, a wait after each
    r = autograd.make_renderer(w, h, **constants)
    rec, raw = torch.tensor(aos, device=dev), torch.zeros(n, 84, device=dev)
    m, v = torch.zeros(n, 84, device=dev), torch.zeros(n, 84, device=dev)
    ids, rows = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, 84, device=dev)
    cnt, grad = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(h, w, 4, device=dev)
    acc, mark = torch.empty(n, 84, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    nums = torch.zeros(2, 3, device=dev)
    torch.cuda.synchronize()

    def each(call, *args):
        call(*args)
        r.synchronize()

    each(r.rawFromRecordsDevice, rec.data_ptr(), raw.data_ptr(), n)
    each(r.recordsFromRawDevice, raw.data_ptr(), rec.data_ptr(), n)
    each(r.uploadDevice, rec.data_ptr(), n)
    r.ensureOutputs(_lib.GS_OUTPUT_RGBA32F)
    for b in range(2):
        each(lambda: r.drawCamera(*cameras[b], 0, sync=False))
        each(r.photometricLossDevice, None, targets[b].data_ptr(), LAMBDA, None, nums[b].data_ptr(), grad.data_ptr())
        each(r.backwardVisibleDevice, grad.data_ptr(), None, ids.data_ptr(), rows.data_ptr(), n, cnt.data_ptr())
        each(r.rowsAccumulateDevice, acc.data_ptr(), mark.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), cnt.data_ptr(), n, 0.5)
    each(r.rowsCollectDevice, acc.data_ptr(), mark.data_ptr(), n, ids.data_ptr(), rows.data_ptr(), n, cnt.data_ptr())
    each(r.adamRowsRawDevice, raw.data_ptr(), rec.data_ptr(), m.data_ptr(), v.data_ptr(), n, ids.data_ptr(), rows.data_ptr(),
         cnt.data_ptr(), n, default_adam_params(space="raw", step=1))
    torch.cuda.synchronize()
    want = [t.cpu().numpy() for t in (nums, rec, raw, m, v, ids, cnt)]
    r.cleanup()
    union = int(want[6].view(np.uint32)[0])
    assert 500 < union <= n and np.all(np.isfinite(want[0])) and np.all(np.isfinite(want[1]))
    for name, a, b in zip(("numbers", "records", "raw", "m", "v"), got, want):
        assert np.array_equal(bits(a), bits(b)), name
    assert got[6].view(np.uint32)[0] == union and np.array_equal(got[5][:union], want[5][:union])
