"""Frames and gradients under camera constants other than the defaults, on the CPU.

gs_config carries five floats that stand in for the reference's compile-time constants -- near_plane, far_plane, ndc_cull,
in_view_limit, fov_y -- and every kernel that reads FrameParams reads some of them: the culls and the depth key of
k_project, get_covariance's focal lengths and clamp, radius_bound / box_misses_owned_rows / band_skip of a context that owns
a subset of the tile rows, bwd_chain, the densification statistics.  At the defaults tan(fov_y / 2) is 0.99995 and every
test camera's projection is gs_camera_matrices' 90 degrees, so a dropped tan_fov_y factor, a literal 0.1f or 1.3f, or a screen
position taken from the config's field of view instead of from proj changes nothing a test could see.  The four
configurations here are designed so that each constant decides; this file proves it on the oracle alone (the conditions
below are conditions, not measurements), shows that the references of the GPU tests honour the constants -- the C
restatement of the float outputs and the float64 frame -- and tests the refusals of gs_create and the Python keywords.
tests/test_camera_constants_gpu.py runs the library on the same inputs; the helpers are shared with it."""
import ctypes as C

import numpy as np
import pytest

from conftest import has_gpu

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_outputs_cpu import SCENES, assert_posed, camera, in_front_of, quantise, reference_outputs
from test_band_cull_cpu import GH, H, W, MatrixCamera, cameras, cloud_a, cloud_b, emits_into

F = np.float32
CONFIGS = ("pinhole", "split", "off_centre", "tight")
CONSTANTS = ("near_plane", "far_plane", "ndc_cull", "in_view_limit", "fov_y")
DEFAULTS = dict(near_plane=0.1, far_plane=100.0, ndc_cull=1.3, in_view_limit=0.8, fov_y=float(F(3.1415) * F(0.5)))


# ---- the designed configurations --------------------------------------------------------------------------------------------

def intrinsics_proj(fx, fy, cx, cy, w, h, near, far):
    """The column-major projection of a pinhole camera with focal lengths (fx, fy) and principal point (cx, cy) in pixels
    of a w x h frame, in the perspectiveRH_ZO shape of gs_camera_matrices (proj[11] = -1: clip w = -view z).  With sx = (ndc_x
    + 1) / 2 * w and sy = (1 - ndc_y) / 2 * h (Common.glsl:80-89) a view-space point (x, y, z) lands on sx = cx + fx x / -z,
    sy = cy - fy y / -z."""
    p = np.zeros(16, np.float64)
    p[0], p[5] = 2.0 * fx / w, 2.0 * fy / h
    p[8], p[9] = 1.0 - 2.0 * cx / w, 2.0 * cy / h - 1.0
    p[10], p[11], p[14] = far / (near - far), -1.0, -(far * near) / (far - near)
    return p.astype(F)


def default_proj(w, h):
    """gs_camera_matrices' fixed 90 degrees at this aspect."""
    import oracle
    return oracle.camera_matrices((0.0, 0.0, 0.0), 0.0, 0.0, w / h)[1]


def configuration(name, w, h):
    """(constants, proj) of a configuration at w x h: the keyword arguments of Renderer (and fields of the oracle's Params) that differ
    from the defaults, and the projection its frames are drawn with."""
    if name == "pinhole":
        # What a trainer sets: a per-dataset fov_y with the projection of the same angle, the INRIA clamp limit 1.3 (equal to
        # the NDC cull, so no visible splat clamps) and a near / far pair of its own.  Isolates every reader of tan_fov_y, of
        # near_plane and far_plane (the depth key), and the un-clamped Jacobian.
        fov_y = 0.9
        f = h / (2.0 * np.tan(fov_y / 2.0))
        return dict(fov_y=fov_y, in_view_limit=1.3, ndc_cull=1.3, near_plane=0.2, far_plane=40.0), \
            intrinsics_proj(f, f, w / 2.0, h / 2.0, w, h, 0.2, 40.0)
    if name == "split":
        # proj stays at 90 degrees, fov_y = 1.2: every reader of tan_fov_y now disagrees with every reader of proj by
        # tan(45 deg) / tan(0.6) = 1.46.  Isolates a screen position taken from the config's field of view, and a covariance
        # focal length taken from proj.
        return dict(fov_y=1.2), default_proj(w, h)
    if name == "off_centre":
        # Non-square pixels (fx = 1.15 fy) and a principal point moved by +7.5 % of the width and -5 % of the height:
        # proj[0] / proj[5] is not the aspect and proj[8], proj[9] are non-zero.  fov_y follows fy.  Isolates the projection's
        # third column in the forward and in dL/dproj, and a tan_fov_x used where tan_fov_y belongs.
        fov_y = 1.3
        fy = h / (2.0 * np.tan(fov_y / 2.0))
        return dict(fov_y=fov_y), intrinsics_proj(1.15 * fy, fy, w / 2.0 + 0.075 * w, h / 2.0 - 0.05 * h, w, h, 0.1, 100.0)
    if name == "tight":
        # The culls and the clamp pulled inside the frame: splats on the screen are culled (ndc_cull 0.9), most visible
        # splats clamp (in_view_limit 0.3), the near plane cuts the cloud (2.0) and the far plane saturates the depth key
        # of most of it (8.0).  The default 90 degree proj and fov_y are kept.  Isolates a literal 0.1f, 100.0f, 1.3f or 0.8f
        # and the clamp's derivative.
        return dict(ndc_cull=0.9, in_view_limit=0.3, near_plane=2.0, far_plane=8.0), default_proj(w, h)
    raise KeyError(name)


def view_camera(pose, w, h, proj):
    """The origin camera (pose None) or test_outputs_cpu.POSES[pose], with `proj` as its projection."""
    if pose is None:
        cam = gs.Camera(w / h)
        cam.setPosition((0.0, 0.0, 0.0))
        cam.setRotation(0.0, 0.0)
        cam.recalculate()
    else:
        cam = camera(pose, w, h)
    return MatrixCamera(cam.getViewMatrix(), proj, cam.getPosition())


def with_constants(p, constants):
    """The oracle's Params p with the constants written over gso_default_params' values (its struct has all five)."""
    for k, v in constants.items():
        assert k in CONSTANTS, k
        setattr(p, k, float(v))
    return p


def params_of(cam, w, h, constants, **kw):
    import oracle
    return with_constants(oracle.make_params(w, h, cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition(),
                                             sh_mode=cam.getShMode(), **kw), constants)


# (configuration, scene of test_outputs_cpu.SCENES, pose): the frames of both files ...
FRAME_CASES = [(c, "ragged", pose) for c in CONFIGS for pose in (None, "pose")] + [("pinhole", "dense", None), ("tight", "dense", "pose")]
# ... and the ones differentiated
GRAD_CASES = [("pinhole", "ragged", "pose"), ("split", "ragged", None), ("off_centre", "ragged", "pose"), ("tight", "ragged", None),
              ("tight", "dense", "pose")]
case_id = lambda c: f"{c[0]}-{c[1]}-{c[2] or 'origin'}"

_CASES = {}


def case(name, scene, pose):
    """dict(aos, w, h, cam, constants, p, p_default): a cloud of SCENES in front of the camera, the configuration's constants
    and projection, the oracle's params with them, and with the default constants under the same matrices.  Shared: do not
    write to the arrays."""
    key = (name, scene, pose)
    if key not in _CASES:
        aos, w, h = SCENES[scene]()
        if pose is not None:
            aos = in_front_of(aos, w, h, pose)
        constants, proj = configuration(name, w, h)
        cam = view_camera(pose, w, h, proj)
        aos.setflags(write=False)
        _CASES[key] = dict(aos=aos, w=w, h=h, cam=cam, constants=constants, p=params_of(cam, w, h, constants),
                           p_default=params_of(cam, w, h, {}))
    return _CASES[key]


_FRAMES = {}


def oracle_frame(name, scene, pose, default=False):
    """oracle.full_pipeline of a case (with the default constants instead: default=True), computed once."""
    key = (name, scene, pose, default)
    if key not in _FRAMES:
        import oracle
        c = case(name, scene, pose)
        _FRAMES[key] = oracle.full_pipeline(c["p_default"] if default else c["p"], c["aos"])
    return _FRAMES[key]


# ---- float32 restatements of what the kernels decide ------------------------------------------------------------------------

def mul44(m, v):
    """mat4_mul_vec4 on arrays: m column-major float32[16], v four float32 arrays; the products summed left to right."""
    m = np.asarray(m, F)
    out = []
    for r in range(4):
        acc = m[r] * v[0]
        for k in range(1, 4):
            acc = acc + m[k * 4 + r] * v[k]
        out.append(acc)
    return out


def projected(p, aos):
    """Per splat, in float32 as k_project computes them: view-space position vp[0..3], ndc_x, ndc_y, view depth."""
    a = np.asarray(aos, F)
    vp = mul44(p.view, [a[:, 0], a[:, 1], a[:, 2], np.ones(len(a), F)])
    q = mul44(p.proj, vp)
    with np.errstate(all="ignore"):
        return vp, q[0] / q[3], q[1] / q[3], -vp[2]


def tan_half(fov_y):
    """FrameParams::tan_fov_y (make_frame_params): tan in double of the float product, rounded to float."""
    return F(np.tan(np.float64(F(fov_y) * F(0.5))))


def clamp_limits(p):
    tan_y = tan_half(p.fov_y)
    tan_x = tan_y * F(p.width) / F(p.height)
    return tan_x * F(p.in_view_limit), tan_y * F(p.in_view_limit)


def clamp_masks(p, aos):
    """(clamp_x, clamp_y) per splat: x / z or y / z outside the limits of Common.glsl:60-61, as bwd_chain decides it."""
    vp, _, _, _ = projected(p, aos)
    lim_x, lim_y = clamp_limits(p)
    with np.errstate(all="ignore"):
        rx, ry = vp[0] / vp[2], vp[1] / vp[2]
    return (rx < -lim_x) | (rx > lim_x), (ry < -lim_y) | (ry > lim_y)


def sig2_of(aos):
    """store_record_planes' bound on the largest eigenvalue of a splat's 3-D covariance (gs_upload.hip)."""
    a = np.asarray(aos, F)
    r, x, y, z = (a[:, 8 + k] for k in range(4))
    two = F(2)
    e = [[F(1) - two * y * y - two * z * z, two * x * y - two * r * z, two * x * z + two * r * y],
         [two * x * y + two * r * z, F(1) - two * x * x - two * z * z, two * y * z - two * r * x],
         [two * x * z - two * r * y, two * y * z + two * r * x, F(1) - two * x * x - two * y * y]]
    with np.errstate(all="ignore"):
        f2 = sum(e[i][j] * e[i][j] for i in range(3) for j in range(3))
        gersh = np.zeros(len(a), F)
        for i in range(3):
            row = sum(np.abs(e[i][0] * e[j][0] + e[i][1] * e[j][1] + e[i][2] * e[j][2]) for j in range(3))
            gersh = np.where((row > gersh) | (row != row), row, gersh)
        r2 = np.where(gersh < f2, gersh, f2) * F(1.0001)
        sm = np.abs(a[:, 4:7]).max(axis=1)
        return (r2 * sm * sm).astype(F)


def w_norm2_of(view):
    """make_frame_params' bound on the squared spectral norm of the view's 3 x 3 block (gs_ctx.h)."""
    v = np.asarray(view, np.float64)
    m = np.array([[sum(v[i * 4 + k] * v[j * 4 + k] for k in range(3)) for j in range(3)] for i in range(3)])
    return F(min(np.trace(m), np.abs(m).sum(axis=1).max()) * (1.0 + 1e-5))


def radius_bound(p, tx, ty, vz, sig2):
    """radius_bound of gs_project.hip, expression by expression in float32."""
    wdt, hgt = F(p.width), F(p.height)
    tan_y = tan_half(p.fov_y)
    tfx = tan_y * wdt / hgt
    fx, fy = wdt / (F(2) * tfx), hgt / (F(2) * tan_y)
    a, c, b = fx * fx * (F(1) + tx * tx), fy * fy * (F(1) + ty * ty), fx * fy * tx * ty
    with np.errstate(all="ignore"):
        j2 = (F(0.5) * (a + c) + np.sqrt(F(0.25) * (a - c) * (a - c) + b * b)) / (vz * vz)
        lam = j2 * w_norm2_of(p.view) * sig2 * F(1.02) + F(0.31)
        return F(3) * np.sqrt(lam) + F(2)


def owned_rows_below(y, first, stride):
    y = np.asarray(y, np.int64)
    return np.where(y <= first, 0, (y - first + stride - 1) // stride)


def misses_owned_rows(ylo, yhi, row_begin, row_end, first, stride):
    """misses_owned_rows of gs_project.hip for the rows first, first + stride, ... inside [row_begin, row_end)."""
    with np.errstate(all="ignore"):
        ok = (ylo == ylo) & (yhi == yhi) & (ylo <= yhi)
        lo_row, hi_row = np.trunc(ylo * F(1.0 / 16.0)), np.trunc(yhi * F(1.0 / 16.0)) + F(1)
    lo_row, hi_row = np.where(ok, lo_row, 0.0), np.where(ok, hi_row, 0.0)
    y0 = np.where(lo_row < row_begin, row_begin, np.minimum(lo_row, 1e6)).astype(np.int64)
    y1 = np.where(hi_row > row_end, row_end, np.maximum(hi_row, -1e6)).astype(np.int64)
    miss = (y1 <= y0) | (owned_rows_below(y1, first, stride) - owned_rows_below(y0, first, stride) <= 0)
    return ok & miss


def band_state(p, aos, rows):
    """(passes, skipped) per splat for a context with the constants and matrices of p that owns `rows` = (row_begin, row_end,
    first_row, stride): passes both culls of k_project (:94, :100), and of those, rejected by k_project's band_skip -- the
    per-splat cull that reads tan_fov_y and in_view_limit through radius_bound and the clamp, and proj through the screen y.
    (The per-box cull of k_band_cull rejects a subset of what this rejects wave by wave: every splat of a rejected box is
    within the box's bound.)"""
    vp, ndc_x, ndc_y, depth = projected(p, aos)
    with np.errstate(all="ignore"):
        passes = ~(depth <= F(p.near_plane)) & ~((np.abs(ndc_x) > F(p.ndc_cull)) | (np.abs(ndc_y) > F(p.ndc_cull)))
        lim_x, lim_y = clamp_limits(p)
        tx = np.clip(vp[0] / vp[2], -lim_x, lim_x)
        ty = np.clip(vp[1] / vp[2], -lim_y, lim_y)
        rmax = radius_bound(p, tx, ty, vp[2], sig2_of(aos))
        sy_b = (F(1) - ndc_y) * F(0.5) * F(p.height)
        skipped = passes & misses_owned_rows(sy_b - rmax, sy_b + rmax, *rows)
    return passes, skipped


# ---- 1. the conditions, on the oracle alone ---------------------------------------------------------------------------------

def emitting_of(ref):
    s = ref["stage1"]["splats"]
    return (s["visible"] == 1) & (s["min_x"] < s["max_x"]) & (s["min_y"] < s["max_y"])


@pytest.mark.parametrize("name,scene,pose", FRAME_CASES, ids=[case_id(c) for c in FRAME_CASES])
def test_the_constants_decide_the_frame(oracle_mod, name, scene, pose):
    """Every frame of the GPU file differs from the frame of the same cloud and matrices under the default constants in its
    element count, in at least one pixel and -- where near or far moved -- in a sorted depth word of a (tile, id) pair both
    lists hold; at least 500 splats emit; a posed case is posed."""
    c = case(name, scene, pose)
    if pose is not None:
        assert_posed(c["p"])
    ref, dflt = oracle_frame(name, scene, pose), oracle_frame(name, scene, pose, default=True)
    assert ref["stage1"]["counter"] == ref["e"] and dflt["stage1"]["counter"] == dflt["e"]       # neither list overflows
    assert ref["e"] != dflt["e"], ref["e"]
    assert np.any(ref["image"] != dflt["image"])
    assert emitting_of(ref).sum() >= 500, emitting_of(ref).sum()
    key = lambda r: (r["tile"][:r["e"]].astype(np.uint64) << np.uint64(32)) | r["id"][:r["e"]]
    common, i, j = np.intersect1d(key(ref), key(dflt), return_indices=True)
    moved = int((ref["depth"][:ref["e"]][i] != dflt["depth"][:dflt["e"]][j]).sum())
    print(f"{case_id((name, scene, pose))}: e {ref['e']} (defaults {dflt['e']}), {emitting_of(ref).sum()} splats emit, "
          f"{len(common)} common (tile, id) pairs, {moved} with another depth word")
    assert len(common) > 1000
    if name in ("pinhole", "tight"):
        assert moved > 1000
    else:
        assert moved == 0                          # near and far are the defaults: the same key for the same splat


@pytest.mark.parametrize("name,scene,pose", FRAME_CASES, ids=[case_id(c) for c in FRAME_CASES])
def test_the_clamp_is_where_it_was_designed(oracle_mod, name, scene, pose):
    """pinhole: no visible splat takes the clamp of Common.glsl:60-61 (in_view_limit equals ndc_cull and proj is of fov_y's
    angle).  split, off_centre: it is taken and it is not.  tight: at least a quarter of the visible splats clamp in x, some
    in y, some not at all."""
    c = case(name, scene, pose)
    vis = oracle_frame(name, scene, pose)["stage1"]["splats"]["visible"] == 1
    cx, cy = clamp_masks(c["p"], c["aos"])
    nx, ny, none = int((vis & cx).sum()), int((vis & cy).sum()), int((vis & ~cx & ~cy).sum())
    print(f"{case_id((name, scene, pose))}: {vis.sum()} visible, clamp x {nx}, clamp y {ny}, neither {none}")
    if name == "pinhole":
        assert nx == 0 and ny == 0
    elif name == "tight":
        assert nx >= vis.sum() / 4 and ny >= 50 and none >= 50
    else:
        assert nx >= 50 and ny >= 50 and none >= 50


@pytest.mark.parametrize("scene,pose", [("ragged", None), ("ragged", "pose"), ("dense", "pose")])
def test_tight_culls_where_the_defaults_do_not(oracle_mod, scene, pose):
    """tight: at least 50 splats pass the default near cull and this NDC cull and fail this near cull; at least 50 visible
    splats saturate the depth key at far; at least 50 splats in front of the near plane lie inside |ndc| <= 1 -- on the
    screen -- and are culled."""
    c = case("tight", scene, pose)
    p = c["p"]
    s = oracle_frame("tight", scene, pose)["stage1"]["splats"]
    vis = s["visible"] == 1
    _, ndc_x, ndc_y, depth = projected(p, c["aos"])
    inside = lambda lim: (np.abs(ndc_x) <= F(lim)) & (np.abs(ndc_y) <= F(lim))
    near_only = (depth > F(DEFAULTS["near_plane"])) & (depth <= F(p.near_plane)) & inside(p.ndc_cull)
    saturated = vis & (s["depth_key"] == 0xFFFFFFFF)
    on_screen_culled = (depth > F(p.near_plane)) & inside(1.0) & ~inside(p.ndc_cull)
    print(f"tight {scene} {pose}: near-culled alone {near_only.sum()}, saturated {saturated.sum()}, on screen and culled "
          f"{on_screen_culled.sum()}")
    assert near_only.sum() >= 50 and not vis[near_only].any()
    assert saturated.sum() >= 50 and np.all(depth[saturated] >= F(p.far_plane) * F(0.999))
    assert on_screen_culled.sum() >= 50 and not vis[on_screen_culled].any()
    assert (vis & (s["depth_key"] != 0xFFFFFFFF) & (s["depth_key"] != 0)).sum() >= 50             # and some keys are live


# ---- the band runs ----------------------------------------------------------------------------------------------------------
BAND_RUNS = (("A", "rigid"), ("A", "roll37"), ("B", "rigid"))
BAND_ROWS = {"first": (0, 1, 0, 1), "middle": (11, 12, 11, 1), "last": (GH - 1, GH, GH - 1, 1), "interleaved": (0, GH, 1, 3)}


def band_cloud(which):
    return cloud_a() if which == "A" else cloud_b()[0]


def band_camera(name, view):
    """test_band_cull_cpu.cameras()[view] with the configuration's projection: (camera, constants)."""
    constants, proj = configuration(name, W, H)
    cam = cameras()[view]
    return MatrixCamera(cam.getViewMatrix(), proj, cam.getPosition()), constants


def band_key(name, which, view):
    """The cache key of test_band_cull_cpu.oracle_run / oracle_rows for a band run under a configuration."""
    return (which, view, "constants", name)


_BAND_REFS = {}


def band_references(name, which, view):
    """(camera, constants, refs) of a band run: refs[band name] = the oracle's run for that band with the configuration's
    constants -- oracle.full_pipeline on the rows of a contiguous band, the whole-frame list restricted to the rows for
    the interleaved one -- in the forms test_band_cull_gpu.assert_band and assert_rows take."""
    key = (name, which, view)
    if key not in _BAND_REFS:
        import oracle
        from vk3dgaussiansplatting_amd import dist as gsdist
        cam, constants = band_camera(name, view)
        aos = band_cloud(which)
        refs = {}
        for band, (rb, re, first, stride) in BAND_ROWS.items():
            if stride == 1:
                ref = oracle.full_pipeline(params_of(cam, W, H, constants, row_begin=rb, row_end=re), aos)
                e = ref["e"]
                assert ref["stage1"]["counter"] == e
                refs[band] = dict(e=e, tile=ref["tile"][:e], depth=ref["depth"][:e], id=ref["id"][:e], ranges=ref["ranges"],
                                  image=ref["image"])
            else:
                refs[band] = rows_reference(cam, constants, aos, gsdist.interleaved_rows(GH, first, stride))
        _BAND_REFS[key] = (cam, constants, refs)
    return _BAND_REFS[key]


def rows_reference(cam, constants, aos, rows):
    """test_band_cull_cpu.oracle_rows with the constants: the whole frame's elements restricted to the tile rows `rows`,
    sorted; the lengths of the tiles' ranges; the pixels of those rows."""
    import oracle
    p = params_of(cam, W, H, constants)
    s1 = oracle.init_sort_list(p, aos, want_splats=False)
    assert s1["counter"] <= s1["capacity"]
    gw, gh = oracle.grid(W, H)
    n_all = s1["counter"]
    mine = np.isin(s1["tile"][:n_all] // gw, rows)
    t, d, i = (np.ascontiguousarray(s1[k][:n_all][mine]) for k in ("tile", "depth", "id"))
    e = t.size
    t, d, i = oracle.sort_stable(t, d, i, e)
    ranges = oracle.find_ranges(t, e, gw * gh)
    image = np.zeros((H, W, 4), np.uint8)
    for row in rows:
        oracle.render(params_of(cam, W, H, constants, row_begin=row, row_end=row + 1), aos, s1["color"], s1["cov"], i, ranges, out=image)
    return dict(e=e, tile=t, depth=d, id=i, lens=ranges[:, 1].astype(np.int64) - ranges[:, 0], image=image, rows=list(rows))


@pytest.mark.parametrize("which,view", BAND_RUNS, ids=[f"{w}-{v}" for w, v in BAND_RUNS])
@pytest.mark.parametrize("name", CONFIGS)
def test_the_constants_decide_the_band_culls(oracle_mod, name, which, view):
    """For every band of the GPU file, with the restatement of k_project's band_skip (radius_bound and the clamp in float32):
    under the configuration's constants the cull rejects splats, and its decisions are not those of the default constants
    under the same matrices.

    radius_bound grows with the focal lengths and with the clamped |x / z|, |y / z|, so against the defaults a
    configuration moves every splat's bound one way: pinhole, split and off_centre (fov_y below 90 degrees: longer focal
    lengths) accept splats the default constants would reject -- the direction in which a wrong constant loses splats, and
    in every band of cloud A at least one such splat emits into the band, so a kernel that used a default there would show
    in the band's list -- and tight (in_view_limit 0.3) rejects splats the defaults would accept.  The opposite direction is empty by that
    monotonicity for every configuration of this file (asserted), and a cull that is merely more conservative than it
    need be changes no list: the GPU test cannot see it, and nothing is lost by it."""
    cam, constants = band_camera(name, view)
    aos = band_cloud(which)
    p, p_default = params_of(cam, W, H, constants), params_of(cam, W, H, {})
    import oracle
    s = oracle.init_sort_list(p, aos)["splats"]
    for band, rows in BAND_ROWS.items():
        passes, skipped = band_state(p, aos, rows)
        passes_d, skipped_d = band_state(p_default, aos, rows)
        assert np.array_equal(passes, s["visible"] == 1)                      # the restated culls are the oracle's
        both = passes & passes_d
        rejected_here = int((both & skipped & ~skipped_d).sum())              # the defaults would have accepted it
        accepted_here = both & ~skipped & skipped_d                           # the defaults would have rejected it
        own = np.arange(rows[2], rows[1], rows[3])
        emits = emits_into(s, rows[0], rows[1]) if rows[3] == 1 else \
            (s["visible"] == 1) & (s["min_x"] < s["max_x"]) & np.array([np.any((own >= a) & (own < b)) for a, b in zip(s["min_y"], s["max_y"])])
        assert not np.any(skipped & emits), (band, np.flatnonzero(skipped & emits)[:5])   # the cull loses nothing
        lost_by_defaults = int((accepted_here & emits).sum())
        print(f"{name} {which} {view} {band}: {passes.sum()} pass the culls, {skipped.sum()} rejected by the band cull, "
              f"{emits.sum()} emit; against the defaults: {rejected_here} rejected only here, {accepted_here.sum()} accepted only "
              f"here, {lost_by_defaults} of them emit")
        assert skipped.sum() >= 1 and emits.sum() >= 1
        if name == "tight":
            assert rejected_here >= 1 and accepted_here.sum() == 0
        else:
            assert accepted_here.sum() >= 1 and rejected_here == 0
            assert lost_by_defaults >= 1 or which == "B"          # the few hundred designed splats: not in every band


# ---- 2. the references honour the constants ---------------------------------------------------------------------------------

@pytest.mark.parametrize("name,scene,pose", FRAME_CASES, ids=[case_id(c) for c in FRAME_CASES])
def test_restatement_reproduces_the_oracle_frame(oracle_mod, tmp_path, name, scene, pose):
    """test_outputs_cpu.test_restatement_reproduces_the_oracle_frame under the four configurations: blend_outputs_ref.c gives
    the oracle's RGBA8 frame byte for byte, and the same bytes again from quantising its float colour -- the condition under
    which its RGBA32F and depth are the reference for the GPU's."""
    c = case(name, scene, pose)
    out = reference_outputs(tmp_path, c["p"], c["aos"], ref=oracle_frame(name, scene, pose))
    assert np.array_equal(out["rgba"], out["ref"]["image"])
    assert np.array_equal(quantise(out["rgba32f"]), out["rgba"])
    a, d = out["rgba32f"][..., 3], out["depth"]
    assert np.all((a >= 0) & (a <= 1)) and np.all(np.isfinite(d)) and np.all(d >= 0)
    assert np.count_nonzero(a) > c["w"] * c["h"] // 8
    if name == "tight":                             # nothing nearer than the near plane was blended: depth >= near * alpha
        assert np.all(d >= F(c["p"].near_plane) * a * F(0.9999))


@pytest.mark.parametrize("name,scene,pose", GRAD_CASES, ids=[case_id(c) for c in GRAD_CASES])
def test_reference_forward_matches_the_restatement(oracle_mod, tmp_path, name, scene, pose):
    """test_backward_cpu.test_reference_forward_matches_the_restatement under the configurations, at its tolerance (1e-5
    relative + 2e-5 absolute): the float64 frame reads fov_y, in_view_limit and proj as the float32 frame does, before the
    GPU's gradients are judged by it.  The culls and the depth key reach it through the frame's decisions."""
    torch = pytest.importorskip("torch")
    from frame64 import forward64, frame_decisions
    c = case(name, scene, pose)
    ref, flags = frame_decisions(tmp_path, c["p"], c["aos"], ref=oracle_frame(name, scene, pose))
    out = reference_outputs(tmp_path, c["p"], c["aos"], ref=ref)
    with torch.no_grad():
        rgba, dep = forward64(c["p"], torch.tensor(c["aos"].astype(np.float64)), ref, flags)
    assert np.count_nonzero(flags) > 1000
    np.testing.assert_allclose(rgba.numpy(), out["rgba32f"], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(dep.numpy(), out["depth"], rtol=1e-5, atol=2e-5 * max(1.0, float(np.abs(out["depth"]).max())))


def test_the_projection_helper(oracle_mod):
    """intrinsics_proj at 90 degrees, square pixels and a centred principal point is gs_camera_matrices' projection (to a
    float32 rounding of 1 / tan); off_centre's has the designed shape; a point on the optical axis lands on the principal
    point and one focal length off it per unit of x / -z."""
    for w, h in ((333, 190), (W, H)):
        f = h / (2.0 * np.tan(np.float64(F(90.0) * F(0.01745329251994329576923690768489)) / 2.0))
        np.testing.assert_allclose(intrinsics_proj(f, f, w / 2.0, h / 2.0, w, h, 0.1, 100.0), default_proj(w, h), rtol=3e-7, atol=0)
        constants, proj = configuration("off_centre", w, h)
        assert proj[11] == -1 and proj[8] == F(-0.15) and proj[9] == F(-0.1)
        np.testing.assert_allclose((proj[0] * w) / (proj[5] * h), 1.15, rtol=1e-6)
        np.testing.assert_allclose(proj[5], 1.0 / np.tan(constants["fov_y"] / 2.0), rtol=1e-6)
        fx, fy, cx, cy = proj[0] * w / 2.0, proj[5] * h / 2.0, w / 2.0 + 0.075 * w, h / 2.0 - 0.05 * h
        for x, y, z in ((0.0, 0.0, -3.0), (1.0, 0.0, -1.0), (0.0, 1.0, -1.0), (0.3, -0.2, -2.0)):
            q = np.asarray(mul44(proj, [F(x), F(y), F(z), F(1)]), np.float64)
            sx, sy = (q[0] / q[3] + 1.0) * 0.5 * w, (1.0 - q[1] / q[3]) * 0.5 * h
            np.testing.assert_allclose([sx, sy], [cx + fx * x / -z, cy - fy * y / -z], rtol=1e-5)


# ---- 3. the surface ---------------------------------------------------------------------------------------------------------

def _create(**fields):
    L = _lib.lib()
    cfg = _lib.GsConfig()
    L.gs_default_config(C.byref(cfg))
    for k, v in fields.items():
        setattr(cfg, k, v)
    h = C.c_void_p()
    rc = L.gs_create(C.byref(cfg), C.byref(h))
    msg = L.gs_last_error(None).decode()
    if h.value:
        L.gs_destroy(h)
    return rc, msg


PI32_BELOW = float(np.nextafter(F(np.pi), F(0)))          # the largest float32 below pi (float32(pi) itself is above it)
REFUSED = [(k, v) for k in CONSTANTS for v in (float("nan"), float("inf"), float("-inf"))] + \
    [("near_plane", 0.0), ("near_plane", -0.1), ("far_plane", 0.1), ("far_plane", 0.05), ("far_plane", -1.0),
     ("ndc_cull", 0.0), ("ndc_cull", -1.3), ("in_view_limit", 0.0), ("in_view_limit", -0.8),
     ("fov_y", 0.0), ("fov_y", -1.0), ("fov_y", float(F(np.pi))), ("fov_y", 4.0)]
ACCEPTED = [("near_plane", 1e-30), ("near_plane", float(np.nextafter(F(100.0), F(0)))), ("far_plane", float(np.nextafter(F(0.1), F(1)))),
            ("far_plane", 3.0e38), ("ndc_cull", 1e-30), ("ndc_cull", 3.0e38), ("in_view_limit", 1e-30), ("in_view_limit", 3.0e38),
            ("fov_y", 1e-30), ("fov_y", PI32_BELOW)]


@pytest.mark.parametrize("field,value", REFUSED, ids=[f"{k}={v}" for k, v in REFUSED])
def test_gs_create_refuses(field, value):
    """GS_ERR_INVALID with a message that names the field, before the device is asked for: a NaN or an infinity in any of
    the five, near_plane <= 0, far_plane <= near_plane, ndc_cull <= 0, in_view_limit <= 0, fov_y <= 0 or >= pi."""
    rc, msg = _create(**{field: value})
    assert rc == _lib.GS_ERR_INVALID, (field, value, rc, msg)
    assert msg.startswith("gs_create: ") and field in msg, msg


def test_gs_create_refuses_far_against_a_moved_near():
    rc, msg = _create(near_plane=2.0, far_plane=2.0)
    assert rc == _lib.GS_ERR_INVALID and "far_plane" in msg
    rc, msg = _create(near_plane=200.0)                      # beyond the default far plane
    assert rc == _lib.GS_ERR_INVALID and "far_plane" in msg


@pytest.mark.parametrize("field,value", ACCEPTED, ids=[f"{k}={v}" for k, v in ACCEPTED])
def test_gs_create_accepts_the_legal_neighbours(field, value):
    """The neighbours of every boundary that are legal pass the checks: GS_OK where a device exists, GS_ERR_NO_DEVICE (the
    check behind them) where none does."""
    rc, msg = _create(**{field: value})
    assert rc == (_lib.GS_OK if has_gpu() else _lib.GS_ERR_NO_DEVICE), (field, value, rc, msg)
    if field == "fov_y":
        assert np.isfinite(tan_half(value)) and tan_half(value) > 0


@pytest.mark.parametrize("name", CONFIGS)
def test_the_configurations_pass_gs_create(name):
    rc, msg = _create(**configuration(name, W, H)[0])
    assert rc == (_lib.GS_OK if has_gpu() else _lib.GS_ERR_NO_DEVICE), (rc, msg)


def test_renderer_keywords_land_in_cfg():
    """Renderer(...)'s five keywords are written into the gs_config it hands to gs_create and stay readable on Renderer.cfg;
    None keeps gs_default_config's value; autograd.make_renderer forwards them; the oracle's Params, through with_constants, holds the same values."""
    import oracle
    r = gs.Renderer(64, 48)
    for k in CONSTANTS:
        assert getattr(r.cfg, k) == F(DEFAULTS[k]), k
    for name in CONFIGS:
        constants, _ = configuration(name, 64, 48)
        r = gs.Renderer(64, 48, sort_algorithm=gs.GS_SORT_RADIX8, **constants)
        p = with_constants(oracle.make_params(64, 48), constants)
        for k in CONSTANTS:
            want = F(constants.get(k, DEFAULTS[k]))
            assert getattr(r.cfg, k) == want and getattr(p, k) == want, (name, k)
        assert r.cfg.sort_algorithm == gs.GS_SORT_RADIX8 and r.cfg.struct_size == C.sizeof(_lib.GsConfig)
    with pytest.raises(TypeError):
        gs.Renderer(64, 48, fov=1.0)
    r = gs.Renderer(64, 48, fov_y=0.0)    # the refusal reaches the caller, with or without a device
    with pytest.raises(gs.GsplatError) as ei:
        r.init(gs.ResourceManager())
    assert ei.value.code == _lib.GS_ERR_INVALID and "fov_y" in str(ei.value)
    pytest.importorskip("torch")
    import inspect
    from vk3dgaussiansplatting_amd import autograd
    assert inspect.signature(autograd.make_renderer).parameters["kw"].kind == inspect.Parameter.VAR_KEYWORD
