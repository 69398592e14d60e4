"""The designs of tests/test_skipped_work_gpu.py, proven without a GPU.

A frame decides in three places NOT to do work, and no value of a frame shows whether it did: k_project stores the raster records
of a quarter wave only when one of its 16 splats emits (wave_wrote); k_band_cull and k_project's band_skip reject the waves and
splats that cannot reach a context's band of tile rows; k_tile_classes / k_tile_scatter / k_tile_order_small hand RenderGaussians
its tiles longest list first.  Each can fail towards doing too much with every pixel right.  gs_debug_read returns the three
decisions (GS_BUF_WAVE_WROTE, GS_BUF_BAND_BLOCKS, GS_BUF_TILE_ORDER); here is what they must read back, and why:

  records     expected_masks() from the oracle's classes, on the layout of test_project_records_cpu.py and on LAYOUT_B, whose
              N is no multiple of 16 and whose last wave stores its partial last quarter alone;
  band culls  cloud C of test_band_cull_cpu.py says which waves and splats are out; float64 restatements of
              box_misses_owned_rows and of k_project's band_skip show that the culls MUST reject them: the bound with all of the
              kernel's widening stays MARGIN_PX clear of the band, printed below;
  tile order  stacks of k coincident small splats on the tiles where the kernels have seams, k at both edges of every class
              of list lengths; tile_order_faults() is the whole specification of the table."""
import functools

import numpy as np
import pytest

from test_band_cull_cpu import (C_BAND, C_TAILS, H, NEAR, W, MatrixCamera, cameras, cloud_c, cloud_e, default_camera, emits_into,
                                oracle_run as band_oracle_run)
from test_band_cull_cpu import _world_of as world_at_pixel
from test_project_records_cpu import (CAMERA_1, CAMERA_2, CULLED, EMITS, FRAMES, LAYOUT, MARGIN, MARGIN_NDC_Y, N, QUARTER, WAVE,
                                      oracle_classes, scene)
from test_project_records_cpu import _world_of as world_at_ndc

# ---- stored raster records ------------------------------------------------------------------------------------------------------

# The second layout.  N_B % 16 == 5: the last wave is two whole quarters of margin splats and a partial third quarter of five --
# four culled splats (behind the camera under both cameras) and, last of all, the wave's only emitter.  Under CAMERA_1 the wave
# stores its partial quarter and nothing else (the `i < valid * 3` guard of k_project's store loop with something to store); under
# CAMERA_2 emitters and margin splats swap: the whole quarters are stored and the partial one holds a margin splat among culled ones.
LAYOUT_B = (
    ("all emitting", EMITS),
    ("all in the margin", MARGIN),
    ("a class per quarter: emitting, margin, culled, margin", "quarters"),
    ("one emitter at lane 31 among margin splats", (MARGIN, EMITS, (31,))),
    ("ragged: 32 margin splats, four culled ones, the only emitter last", "ragged"),
)
RAGGED_B = 37
N_B = (len(LAYOUT_B) - 1) * WAVE + RAGGED_B
MASKS_B = {"camera_1": [0xF, 0x0, 0x1, 0x2, 0x4], "camera_2": [0x0, 0xF, 0xA, 0xF, 0x3]}
MASKS_A_CAMERA_1 = [0xF, 0, 0, 1, 8, 1, 2, 4, 8, 0, 1, 0]          # test_waves_and_quarters_are_of_the_designed_kinds, as masks


def designed_classes_b():
    cls = np.empty(N_B, np.int64)
    for w, (_, what) in enumerate(LAYOUT_B):
        lanes = slice(w * WAVE, min((w + 1) * WAVE, N_B))
        if what == "quarters":
            cls[lanes] = np.repeat([EMITS, MARGIN, CULLED, MARGIN], QUARTER)
        elif what == "ragged":
            cls[lanes] = [MARGIN] * 32 + [CULLED] * 4 + [EMITS]
        elif isinstance(what, tuple):
            cls[lanes] = what[0]
            cls[w * WAVE + np.array(what[2])] = what[1]
        else:
            cls[lanes] = what
    return cls


@functools.lru_cache(maxsize=None)
def scene_b(w, h):
    """(aos [N_B][84], designed classes) for a w x h frame, never modified: the splats of test_project_records_cpu.scene (small,
    round, 16 non-zero SH coefficients; emitting ones mid-screen, margin ones at ndc x = 1.17 +- 0.04) in LAYOUT_B.  The culled
    splats of the last wave are behind the camera, so that they stay culled when the camera turns."""
    import oracle
    import vk3dgaussiansplatting_amd as gs
    view, proj = oracle.camera_matrices(np.zeros(3, np.float32), 0.0, 0.0, w / h)
    cls = designed_classes_b()
    rng = np.random.default_rng(w * 1000 + h + 7)
    aos = np.zeros((N_B, 84), np.float32)
    for g in range(N_B):
        depth = rng.uniform(3.0, 5.0)
        jx, jy = rng.uniform(-0.04, 0.04, 2)
        if cls[g] == EMITS:
            p = world_at_ndc(view, proj, 0.4 * jx, 0.4 * jy, depth)
        elif cls[g] == MARGIN:
            p = world_at_ndc(view, proj, 1.17 + jx, MARGIN_NDC_Y + jy, depth)
        elif g % 2 and g < 4 * WAVE:
            p = world_at_ndc(view, proj, 1.6 + jx, 4 * jy, depth)
        else:
            p = world_at_ndc(view, proj, 4 * jx, 4 * jy, -depth)          # behind the camera
        aos[g] = gs.makeGaussian(p, (0.04, 0.04, 0.04, 0.0), sh0=(0.0, 0.0, 0.0, rng.uniform(0.3, 0.9)))
    sh_rgb = np.array([12 + 4 * k + c for k in range(16) for c in range(3)])
    aos[:, sh_rgb] = (rng.uniform(0.1, 0.3, (N_B, 48)) * rng.choice([-1.0, 1.0], (N_B, 48))).astype(np.float32)
    aos.setflags(write=False)
    cls.setflags(write=False)
    return aos, cls


LAYOUTS = {"A": scene, "B": scene_b}
CAMERAS = {"camera_1": CAMERA_1, "camera_2": CAMERA_2}


def expected_masks(cls, band=False):
    """GS_BUF_WAVE_WROTE, uint8[ceil(N / 64)], from the class of every splat (EMITS = emits an element into the context's rows).
    Whole grid: bit q of wave w is set iff a splat of quarter q of the wave emits.  A contiguous band: 0xF iff a splat of the wave
    emits into the band, else 0."""
    emits = np.concatenate([np.asarray(cls) == EMITS, np.zeros(-len(cls) % WAVE, bool)])
    quarters = emits.reshape(-1, 4, QUARTER).any(axis=2)
    if band:
        return np.where(quarters.any(axis=1), 0xF, 0).astype(np.uint8)
    return (quarters * np.array([1, 2, 4, 8])).sum(axis=1).astype(np.uint8)


def band_classes(oracle, aos, w, h, cam, rb, re):
    """oracle_classes for a context that owns the tile rows [rb, re): EMITS = emits an element into those rows."""
    view, proj = oracle.camera_matrices(np.asarray(cam["pos"], np.float32), cam["yaw"], cam["pitch"], w / h)
    s = oracle.init_sort_list(oracle.make_params(w, h, view, proj, cam["pos"]), aos)["splats"]
    return np.where(emits_into(s, rb, re), EMITS, np.where(s["visible"] == 0, CULLED, MARGIN))


def test_expected_masks_on_hand_made_classes():
    cls = np.full(64 * 2 + 17, MARGIN)
    cls[[0, 31, 64 + 63, 128 + 16]] = EMITS
    assert expected_masks(cls).tolist() == [0b0011, 0b1000, 0b0010]
    assert expected_masks(cls, band=True).tolist() == [0xF, 0xF, 0xF]
    cls[128 + 16] = CULLED
    assert expected_masks(cls).tolist() == [0b0011, 0b1000, 0] and expected_masks(cls, band=True).tolist() == [0xF, 0xF, 0]


@pytest.mark.parametrize("w,h", FRAMES)
def test_layout_b_is_what_it_claims_under_both_cameras(oracle_mod, w, h):
    aos, want = scene_b(w, h)
    assert N_B == 293 and N_B % 16 == 5 and N_B > 256 and (N_B - 1) // 64 == 4
    first, _ = oracle_classes(oracle_mod, aos, w, h, CAMERA_1)
    assert np.array_equal(first, want)
    second, _ = oracle_classes(oracle_mod, aos, w, h, CAMERA_2)
    assert np.all(second[first == EMITS] == MARGIN) and np.all(second[first == MARGIN] == EMITS)
    last = slice(4 * WAVE, N_B)
    # the last wave: its only emitter is the last splat, in the partial quarter; turned, that quarter holds no emitter
    assert np.nonzero(first[last] == EMITS)[0].tolist() == [RAGGED_B - 1] and (RAGGED_B - 1) // QUARTER == 2
    assert second[last].tolist() == [EMITS] * 32 + [CULLED] * 4 + [MARGIN]
    assert expected_masks(first).tolist() == MASKS_B["camera_1"] and expected_masks(second).tolist() == MASKS_B["camera_2"]


@pytest.mark.parametrize("w,h", FRAMES)
def test_layout_a_masks_under_both_cameras(oracle_mod, w, h):
    """The layout of test_project_records_cpu.py: every single-bit mask, 0 and 0xF under CAMERA_1; its ragged last wave holds no
    emitter there (mask 0) and nothing but emitters under CAMERA_2 (a partial wave of 37: quarters 0, 1 and the partial 2)."""
    aos, _ = scene(w, h)
    first, _ = oracle_classes(oracle_mod, aos, w, h, CAMERA_1)
    second, _ = oracle_classes(oracle_mod, aos, w, h, CAMERA_2)
    a, b = expected_masks(first), expected_masks(second)
    assert a.size == b.size == (N + 63) // 64 == len(LAYOUT)
    assert a.tolist() == MASKS_A_CAMERA_1 and {0, 1, 2, 4, 8, 0xF} <= set(a.tolist())
    assert b[-1] == 0x7 and b[0] == 0 and b[1] == 0xF and not np.array_equal(a, b)
    # what the tuning builds store instead differs from the designed masks: whole waves (GS_PROJECT_RECORD_CHUNK=64), every
    # wave with a kept splat (GS_PROJECT_WRITE_KEPT), every wave (GS_PROJECT_WRITE_ALL)
    for cls, m in ((first, a), (second, b)):
        by_wave = np.where(m != 0, 0xF, 0)
        kept = np.where(expected_masks(np.where(cls != CULLED, EMITS, CULLED)) != 0, 0xF, 0)
        assert not np.array_equal(by_wave, m) and not np.array_equal(kept, m) and not np.array_equal(kept, by_wave) and (m != 0xF).any()


@pytest.mark.parametrize("rows", [(0, 1), (1, 3)])
@pytest.mark.parametrize("layout", ["A", "B"])
def test_band_masks_are_whole_waves(oracle_mod, layout, rows):
    """The band rule on the 64 x 48 frame (4 x 3 tiles): the two bands and the two cameras between them hold a wave that emits
    into the band and one that does not, and a wave whose whole-grid mask is not the band's."""
    w, h = FRAMES[0]
    aos, _ = LAYOUTS[layout](w, h)
    seen = set()
    for cam in CAMERAS.values():
        whole, _ = oracle_classes(oracle_mod, aos, w, h, cam)
        cls = band_classes(oracle_mod, aos, w, h, cam, *rows)
        m = expected_masks(cls, band=True)
        assert set(m.tolist()) <= {0, 0xF} and np.all((cls == EMITS) <= (whole == EMITS))
        seen |= set(m.tolist())
        if not np.array_equal(m, expected_masks(whole)):
            seen.add("differs")
    print(f"layout {layout} rows {rows}: band masks seen {sorted(map(str, seen))}")
    assert seen >= {0, "differs"}
    if rows == (1, 3):
        assert 0xF in seen


# ---- band culls -----------------------------------------------------------------------------------------------------------------

MARGIN_PX = 16.0        # what the bounds below, the kernel's widening included, must stay clear of the band's pixel rows by
FOV_Y = np.float32(3.1415) * np.float32(0.5)          # gs_default_config
IN_VIEW_LIMIT, NDC_CULL = 0.8, 1.3


def expected_band_records(tail):
    """GS_BUF_BAND_BLOCKS of cloud_c(tail), designed order, band C_BAND: wave w of block b is an in wave iff bit w of b is set, so
    block b survives with the skip mask ~b & 0xF and block 0 is rejected; the tail block holds ceil(tail / 64) waves of in splats
    and its waves past the last splat are skipped."""
    rec = [b | ((~b & 0xF) << 28) for b in range(1, 16)]
    if tail:
        waves = (tail + 63) // 64
        rec.append(16 | (((0xF << waves) & 0xF) << 28))
    return np.array(rec, np.uint32)


def _m(flat):
    return np.asarray(flat, np.float64).reshape(4, 4).T                  # the flat arrays are column-major


def sig2_of(aos):
    """store_record_planes (gs_upload.hip) in float64: |R|_2^2 max(scale)^2, |R|_2^2 <= min(Gershgorin, Frobenius) of R R^T."""
    a = np.asarray(aos, np.float64)
    r, x, y, z = a[:, 8], a[:, 9], a[:, 10], a[:, 11]
    R = np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * r * z, 2 * x * z + 2 * r * y,
                  2 * x * y + 2 * r * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * r * x,
                  2 * x * z - 2 * r * y, 2 * y * z + 2 * r * x, 1 - 2 * x * x - 2 * y * y], axis=1).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):
        rrt = R @ R.transpose(0, 2, 1)
        f2 = (R * R).sum(axis=(1, 2))
        gersh = np.abs(rrt).sum(axis=2).max(axis=1)
        r2 = np.where(gersh < f2, gersh, f2) * 1.0001
        return r2 * np.abs(a[:, 4:7]).max(axis=1) ** 2


def w_norm2_of(view):
    """make_frame_params (gs_ctx.h): min(trace, largest absolute row sum) of W^T W, times 1 + 1e-5."""
    wm = _m(view)[:3, :3]
    m = wm.T @ wm
    return min(np.trace(m), np.abs(m).sum(axis=1).max()) * (1.0 + 1e-5)


def radius_bound(w, h, tan_fov_y, w_norm2, tx, ty, vz, sig2):
    """radius_bound (gs_project.hip), the 2 % + 2 px of widening included."""
    tfx = tan_fov_y * w / h
    fx, fy = w / (2.0 * tfx), h / (2.0 * tan_fov_y)
    a, c, b = fx * fx * (1.0 + tx * tx), fy * fy * (1.0 + ty * ty), fx * fy * tx * ty
    j2 = (0.5 * (a + c) + np.sqrt(0.25 * (a - c) ** 2 + b * b)) / (vz * vz)
    return 3.0 * np.sqrt(j2 * w_norm2 * sig2 * 1.02 + 0.31) + 2.0


def clearance(ylo, yhi, rb, re):
    """Pixels between the pixel rows [ylo, yhi] and the tile rows [rb, re) -- negative when they meet, NaN for a NaN bound (kept).
    misses_owned_rows cuts rows as the reference does (int() truncates towards zero); the bands here lie below row 1, where that is
    floor."""
    assert rb >= 2
    return np.where(np.isnan(ylo) | np.isnan(yhi), np.nan, np.maximum(ylo - 16.0 * re, 16.0 * rb - yhi))


def wave_box_clearance(aos, cam, w, h, rb, re):
    """box_misses_owned_rows over the boxes k_block_bounds forms (min / max of the positions of 64 consecutive splats, their
    largest sig2), in float64: per wave, how far the bound -- widened as in the kernel by 0.01 % on the tangents, 2 % + 2 px on the
    radius and 1 px on the box -- stays from the rows [rb, re).  NaN: a corner at or behind the near plane or not finite (kept)."""
    a = np.asarray(aos, np.float64)
    n = a.shape[0]
    V, P = _m(cam.getViewMatrix()), _m(cam.getProjectionMatrix())
    tan_fov_y = np.tan(np.float64(FOV_Y * np.float32(0.5)))
    wn2, s2 = w_norm2_of(cam.getViewMatrix()), sig2_of(aos)
    out = np.full((n + 63) // 64, np.nan)
    for k in range(out.size):
        p, sig = a[k * 64:(k + 1) * 64, 0:3], s2[k * 64:(k + 1) * 64]
        if not (np.isfinite(p).all() and not np.isnan(sig).any()):
            continue
        lo, hi = p.min(axis=0), p.max(axis=0)
        corners = np.array([[(hi if c & 1 else lo)[0], (hi if c & 2 else lo)[1], (hi if c & 4 else lo)[2], 1.0] for c in range(8)])
        vp = corners @ V.T
        q = vp @ P.T
        sy = (1.0 - q[:, 1] / q[:, 3]) * 0.5 * h
        if not (np.all(-vp[:, 2] > NEAR) and np.all(q[:, 3] > 0) and np.isfinite(sy).all()):
            continue
        txm = min(np.abs(vp[:, 0] / vp[:, 2]).max() * 1.0001, tan_fov_y * w / h * IN_VIEW_LIMIT)
        tym = min(np.abs(vp[:, 1] / vp[:, 2]).max() * 1.0001, tan_fov_y * IN_VIEW_LIMIT)
        rmax = radius_bound(w, h, tan_fov_y, wn2, txm, tym, (-vp[:, 2]).min(), sig.max())
        out[k] = clearance(sy.min() - rmax - 1.0, sy.max() + rmax + 1.0, rb, re)
    return out


def splat_clearance(aos, cam, w, h, rb, re):
    """k_project's band_skip in float64: per splat that passes the near and the NDC cull, how far sy +- radius_bound stays from the
    rows [rb, re); NaN for the culled ones and for a NaN anywhere (both take the normal path)."""
    a = np.asarray(aos, np.float64)
    V, P = _m(cam.getViewMatrix()), _m(cam.getProjectionMatrix())
    tan_fov_y = np.tan(np.float64(FOV_Y * np.float32(0.5)))
    tfx = tan_fov_y * w / h
    with np.errstate(all="ignore"):
        vp = np.c_[a[:, 0:3], np.ones(a.shape[0])] @ V.T
        q = vp @ P.T
        ndc_x, ndc_y = q[:, 0] / q[:, 3], q[:, 1] / q[:, 3]
        passes = ~(-vp[:, 2] <= NEAR) & ~((np.abs(ndc_x) > NDC_CULL) | (np.abs(ndc_y) > NDC_CULL))
        tx = np.clip(vp[:, 0] / vp[:, 2], -tfx * IN_VIEW_LIMIT, tfx * IN_VIEW_LIMIT)
        ty = np.clip(vp[:, 1] / vp[:, 2], -tan_fov_y * IN_VIEW_LIMIT, tan_fov_y * IN_VIEW_LIMIT)
        rmax = radius_bound(w, h, tan_fov_y, w_norm2_of(cam.getViewMatrix()), tx, ty, vp[:, 2], sig2_of(aos))
        sy = (1.0 - ndc_y) * 0.5 * h
        return np.where(passes, clearance(sy - rmax, sy + rmax, rb, re), np.nan)


def blocks_the_restatement_keeps(aos, cam, w, h, rb, re):
    """Blocks of 256 splats with a wave whose box the float64 restatement does not put at least half a pixel clear of the band --
    the float32 kernel and its hardware reciprocals move a bound by a small fraction of that."""
    c = wave_box_clearance(aos, cam, w, h, rb, re)
    kept = np.concatenate([~(c >= 0.5), np.zeros(-c.size % 4, bool)]).reshape(-1, 4)
    return np.nonzero(kept.any(axis=1))[0]


def test_the_restatements_on_hand_made_splats():
    """One round splat of scale 0.1 straight ahead at depth 10 on the 640 x 360 frame: sig2 = 0.01 (+ 0.01 %), the radius bound is
    3 sqrt(1.02 (180 / 10)^2 0.01 (1 + 1e-5) + 0.31) + 2, and the splat at pixel row 180 is that far from a band."""
    cam = default_camera(W, H)
    aos = np.zeros((1, 84), np.float32)
    aos[0, 0:3] = world_at_pixel(cam, 320.0, 180.0, 10.0)
    aos[0, 4:7], aos[0, 8] = 0.1, 1.0
    assert abs(sig2_of(aos)[0] / (np.float64(np.float32(0.1)) ** 2 * 1.0001) - 1.0) < 1e-12
    assert abs(w_norm2_of(cam.getViewMatrix()) - (1.0 + 1e-5)) < 1e-6
    fy = H / (2.0 * np.tan(np.float64(FOV_Y * np.float32(0.5))))
    r = 3.0 * np.sqrt(1.02 * (fy / 10.0) ** 2 * sig2_of(aos)[0] * w_norm2_of(cam.getViewMatrix()) + 0.31) + 2.0
    assert abs(fy - 180.0) < 0.02 and 7.0 < r < 8.0
    got = splat_clearance(aos, cam, W, H, 15, 16)[0]                   # rows 240 .. 255
    assert abs(got - (240.0 - (180.0 + r))) < 1e-3
    assert abs(splat_clearance(aos, cam, W, H, 2, 11)[0] - ((180.0 - r) - 176.0)) < 1e-3
    assert splat_clearance(aos, cam, W, H, 11, 12)[0] < 0              # row 11 = pixel rows 176 .. 191: it is in
    assert abs(wave_box_clearance(aos, cam, W, H, 15, 16)[0] - (got - 1.0)) < 2e-2      # a box of one point: 1 px more, tangents 0.01 % up
    behind = aos.copy()
    behind[0, 0:3] = -behind[0, 0:3]
    assert np.isnan(splat_clearance(behind, cam, W, H, 15, 16)[0]) and np.isnan(wave_box_clearance(behind, cam, W, H, 15, 16)[0])
    assert expected_band_records(0).size == 15 and expected_band_records(65)[-1] == (16 | (0xC << 28))
    assert expected_band_records(1)[-1] == expected_band_records(63)[-1] == (16 | (0xE << 28)) and expected_band_records(1)[0] == (1 | (0xE << 28))


@pytest.mark.parametrize("tail", C_TAILS)
def test_cloud_c_culls_must_reject_what_they_are_expected_to(oracle_mod, tail):
    """Cloud C, designed order, `rigid`, band C_BAND.  Every out wave's box bound and the bound of every out splat of a stored wave,
    with all of the kernel's widening, stay MARGIN_PX clear of the band: a cull that keeps one of them is wrong by a tile row, not
    by a rounding.  Every in wave's box and every in splat's bound reach the band, as they must (nothing that emits is dropped)."""
    cam = cameras()["rigid"]
    aos, in_mask = cloud_c(tail)
    n = aos.shape[0]
    wave_in = np.array([in_mask[k:k + 64].any() for k in range(0, n, 64)])
    box = wave_box_clearance(aos, cam, W, H, *C_BAND)
    assert not np.isnan(box[~wave_in]).any() and not np.any(box[wave_in] >= 0)      # (an in wave's box may cross the near plane: NaN)
    stored = np.repeat(wave_in, 64)[:n]
    per = splat_clearance(aos, cam, W, H, *C_BAND)
    out_of_stored = stored & ~in_mask
    assert out_of_stored.sum() == 32 * 63 and not np.isnan(per[out_of_stored]).any() and not np.any(per[in_mask] >= 0)
    print(f"cloud C tail {tail}: clearance of the {np.count_nonzero(~wave_in)} out waves' boxes >= {box[~wave_in].min():.1f} px, "
          f"of the {out_of_stored.sum()} out splats of stored waves >= {per[out_of_stored].min():.1f} px (asserted: {MARGIN_PX} px)")
    assert box[~wave_in].min() >= MARGIN_PX and per[out_of_stored].min() >= MARGIN_PX
    # the out splats pass both culls: their covariance is not zero unless band_skip skips them
    s = band_oracle_run(("C", tail, False), aos, cam, W, H)
    assert np.all(s["splats"]["visible"][out_of_stored] == 1) and np.all(s["cov"][out_of_stored, 0] != 0)
    # hence the records: block b survives with the waves of ~b skipped
    kept = np.concatenate([wave_in, np.zeros(-wave_in.size % 4, bool)]).reshape(-1, 4)
    rec = [b | (int((~kept[b] * np.array([1, 2, 4, 8])).sum()) << 28) for b in range(kept.shape[0]) if kept[b].any()]
    assert np.array_equal(np.array(rec, np.uint32), expected_band_records(tail))
    assert np.array_equal(blocks_the_restatement_keeps(aos, cam, W, H, *C_BAND), np.nonzero(kept.any(axis=1))[0])


@pytest.mark.parametrize("tail", C_TAILS)
def test_cloud_c_permuted_bounds(oracle_mod, tail):
    """Permuted, nothing is designed: the blocks with an emitting splat are among the blocks the restatement keeps."""
    cam = cameras()["rigid"]
    aos, in_mask = cloud_c(tail, permuted=True)
    emitting = np.unique(np.nonzero(in_mask)[0] // 256)
    keeps = blocks_the_restatement_keeps(aos, cam, W, H, *C_BAND)
    assert np.isin(emitting, keeps).all() and emitting.size >= 8
    print(f"cloud C tail {tail} permuted: {emitting.size} blocks emit, the restatement keeps {keeps.size} of {(aos.shape[0] + 255) // 256}")


def test_cloud_e_poisoned_waves_have_no_bound(oracle_mod):
    """A NaN or an infinity in a position, a scale or a quaternion: the restatement has no clearance for the wave (NaN: kept)."""
    aos, poisoned = cloud_e()
    box = wave_box_clearance(aos, cameras()["rigid"], W, H, *C_BAND)
    for g, _, _ in poisoned:
        assert not box[g // 64] >= 0.5, g
    clean = wave_box_clearance(cloud_c(63)[0], cameras()["rigid"], W, H, *C_BAND)
    out_waves = {g // 64 for g, _, _ in poisoned if clean[g // 64] >= MARGIN_PX}
    assert len(out_waves) >= 10                      # waves the box test would drop but for the poison


# ---- tile dispatch order --------------------------------------------------------------------------------------------------------

STACK_SIZES = tuple(sorted({1} | {k for j in range(1, 12) for k in (2 ** j - 1, 2 ** j)}))       # 1, 2, 3, 4, 7, 8, ..., 2047, 2048
SEAMS = (0, 63, 64, 1023, 1024, 16383, 16384)        # first tile, wave, workgroup, second round of k_tile_scatter's loop


def bit_length(a):
    a = np.asarray(a, np.int64)
    out = np.zeros(a.shape, np.int64)
    nz = a > 0
    out[nz] = np.floor(np.log2(a[nz])).astype(np.int64) + 1
    return out


def designed_stacks(owned_tiles, first_size=0):
    """{global tile: k}: a stack on the first two and the last two OWNED tiles, on both tiles of every seam among them (compact
    indices, SEAMS) and on the tile before and the tile behind each seam; sizes dealt from STACK_SIZES from index first_size on."""
    owned = np.asarray(owned_tiles)
    t = owned.size
    at = sorted(c for c in {0, 1, t - 2, t - 1} | {s + d for s in SEAMS[1::2] for d in (-1, 0, 1, 2)} if 0 <= c < t)
    return {int(owned[c]): STACK_SIZES[(first_size + i) % len(STACK_SIZES)] for i, c in enumerate(at)}


def stack_cloud(w, h, stacks, seed=5):
    """aos: k coincident splats 8 px into every tile of `stacks` (radius 2 px: they touch that tile alone, also where the frame
    cuts the tile short), under
    default_camera(w, h); in a seeded random order, so that a tile's entries are spread over the project blocks."""
    cam = default_camera(w, h)
    gw = (w + 15) // 16
    rng = np.random.default_rng(seed)
    tiles = np.repeat(list(stacks.keys()), list(stacks.values()))
    tiles = tiles[rng.permutation(tiles.size)]
    sx, sy = (tiles % gw) * 16.0 + 8.0, (tiles // gw) * 16.0 + 8.0
    n = tiles.size
    aos = np.zeros((n, 84), np.float32)
    aos[:, 0:3] = world_at_pixel(cam, sx, sy, np.full(n, 5.0), w, h)
    aos[:, 4:7] = 1e-4
    aos[:, 8] = 1.0
    aos[:, 12:15] = rng.uniform(-1.0, 1.5, (n, 3))
    aos[:, 15] = rng.uniform(0.05, 0.3, n)
    aos.setflags(write=False)
    return aos, cam


def tile_order_faults(order, owned_tiles, lens):
    """The whole specification of GS_BUF_TILE_ORDER, from the ranges alone: a permutation of the owned tiles along which
    bit_length(end - start) never increases (the order inside a class is free).  lens: list length per GLOBAL tile.  -> a list of
    what is wrong, empty when nothing is."""
    order, owned = np.asarray(order, np.int64), np.asarray(owned_tiles, np.int64)
    faults = []
    if order.shape != owned.shape or not np.array_equal(np.sort(order), np.sort(owned)):
        return ["not a permutation of the owned tiles"]
    cls = bit_length(np.asarray(lens, np.int64)[order])
    if np.any(np.diff(cls) > 0):
        k = int(np.nonzero(np.diff(cls) > 0)[0][0])
        faults.append(f"class {cls[k + 1]} (tile {order[k + 1]}) dispatched behind class {cls[k]} (tile {order[k]}) at position {k + 1}")
    return faults


def test_stack_sizes_and_the_specification():
    assert STACK_SIZES[:6] == (1, 2, 3, 4, 7, 8) and STACK_SIZES[-2:] == (2047, 2048) and len(STACK_SIZES) == 22
    assert sorted(set(bit_length(STACK_SIZES).tolist())) == list(range(1, 13)) and bit_length([0, 1, 2 ** 31, 2 ** 32 - 1]).tolist() == [0, 1, 32, 32]
    assert sum(STACK_SIZES) == 8177                                    # the largest cloud: every size once
    owned = np.arange(5, 25)
    lens = np.zeros(30, np.int64)
    lens[[5, 9, 10, 24]] = [3, 2048, 2, 1]
    good = np.array([9, 10, 5, 24] + [t for t in owned if t not in (5, 9, 10, 24)])
    assert tile_order_faults(good, owned, lens) == []
    assert tile_order_faults(np.array([9, 5, 10, 24] + list(good[4:])), owned, lens) == []        # 2 and 3: one class
    assert tile_order_faults(good[::-1], owned, lens) != []                                        # shortest first
    assert tile_order_faults(owned, owned, lens) != []                                             # raster order
    assert tile_order_faults(np.r_[good[:-1], good[0]], owned, lens) == ["not a permutation of the owned tiles"]
    assert tile_order_faults(good - 5, owned, lens) == ["not a permutation of the owned tiles"]    # compact, not global, ids
    # the seams of every shape of the GPU file carry a stack, the largest shape every size
    for t, want in ((1, {0}), (1023, {0, 1, 62, 63, 64, 65, 1021, 1022}), (1025, {0, 1, 62, 63, 64, 65, 1022, 1023, 1024}),
                    (16385, {0, 1, 62, 63, 64, 65, 1022, 1023, 1024, 1025, 16382, 16383, 16384})):
        assert set(designed_stacks(np.arange(t))) == want, t
    assert len(designed_stacks(np.arange(16384))) == 12 and len(designed_stacks(np.arange(16385))) == 13


# owned tiles -> (width, height, index of the first stack size): one workgroup with room, full, and with one tile in a second one
# (k_tile_order_small up to 1024, k_tile_classes + k_tile_scatter above); three workgroups; sixteen, and a seventeenth that sends
# the waves of k_tile_scatter round their loop over the workgroups a second time.  The two largest carry the largest stacks.
SHAPES = {1: (13, 11, 2), 1023: (33 * 16 - 5, 31 * 16 - 9, 0), 1024: (512, 512, 6), 1025: (41 * 16 - 5, 25 * 16 - 7, 12),
          2049: (683 * 16, 48, 4), 16384: (2048, 2048, 10), 16385: (2320, 1808, 9)}
# a 48 x 60 grid: 30 rows of it (1440 tiles, the pair of launches) as a band and as every second row, and a band of 10 rows (480
# tiles, the single launch) -- the order table indexes the OWNED tiles and the kernels reach the ranges through the TileMap
ROWS = {"band 3..32": list(range(3, 33)), "interleaved 1/2": list(range(1, 60, 2)), "band 50..59": list(range(50, 60))}


def test_the_shapes_carry_every_stack_size():
    every = set()
    for tiles, (w, h, first) in SHAPES.items():
        assert ((w + 15) // 16) * ((h + 15) // 16) == tiles
        every |= set(designed_stacks(np.arange(tiles), first).values())
    assert every == set(STACK_SIZES)
    for tiles in (16384, 16385):
        assert {1023, 1024, 2047, 2048} <= set(designed_stacks(np.arange(tiles), SHAPES[tiles][2]).values())
    assert sum(designed_stacks(np.arange(16385), SHAPES[16385][2]).values()) == 8090
    assert all(r[0] >= 1 and r[-1] <= 59 for r in ROWS.values()) and sorted(len(r) * 48 for r in ROWS.values()) == [480, 1440, 1440]


@pytest.mark.parametrize("w,h,rows", [(16 * 13 - 3, 16 * 8 - 5, None), (16 * 13 - 3, 16 * 8 - 5, (1, 7)), (16 * 16, 16 * 10, (0, 10, 2))])
def test_stacks_touch_their_own_tile_alone(oracle_mod, w, h, rows):
    """On a small grid (13 x 8 tiles, ragged right and bottom edges; its rows 1 .. 6; every second row of 16 x 10), the oracle's ranges:
    each designed tile has exactly its k entries and every other tile none."""
    gw, gh = (w + 15) // 16, (h + 15) // 16
    own_rows = range(gh) if rows is None else range(*rows)
    owned = np.array([r * gw + x for r in own_rows for x in range(gw)])
    stacks = designed_stacks(owned, first_size=4)
    assert len(stacks) >= 8 and max(stacks.values()) >= 64
    aos, cam = stack_cloud(w, h, stacks)
    ref = band_oracle_run(("stacks", w, h, rows), aos, cam, w, h)
    lens = ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]
    want = np.zeros(gw * gh, np.int64)
    for t, k in stacks.items():
        want[t] = k
    assert np.array_equal(lens, want) and ref["e"] == aos.shape[0] == sum(stacks.values())
