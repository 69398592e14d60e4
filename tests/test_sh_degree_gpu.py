"""SH degree 1 and 2 as frame modes (include/gsplat.h: GS_SH_DEGREE_1 = 5, GS_SH_DEGREE_2 = 4; the value 3 names no mode and
stays refused, as test_parity_gpu.test_c_abi_call_order_status_codes pins it): frames, gradients, the camera's gradients, the
torch surface and the trainer's degree schedule.

The reference for every value is the code that was there before the modes: for finite inputs mode m on records R equals
GS_SH_ALL_BANDS on Z_K(R), R with the rgb of the coefficients K..15 (K = 4 or 9) set to +0.0 -- x + 0 * b == x in value for a
finite b under the ascending sum.  Mode 0 is pinned to the oracle and the float64 reference by the rest of the suite, so the
comparison here is np.array_equal on values, no tolerance.  That the inactive planes are not read at all is shown with NaN and
1e30 in them."""
import ctypes as C
import functools

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib, synth
from test_parity_gpu import ALL_SORTS, make_renderer, make_scene
from test_outputs_cpu import POSES, SCENES, in_front_of, known_answer_scene
from frame64 import sh_basis, weights

pytestmark = pytest.mark.gpu

DEG1, DEG2 = _lib.GS_SH_DEGREE_1, _lib.GS_SH_DEGREE_2
K_OF_MODE = {DEG1: 4, DEG2: 9}
SH_RGB = np.array([12 + 4 * k + c for k in range(16) for c in range(3)])      # record floats of shCoeffs[k].rgb, k-major
NON_SH = np.setdiff1d(np.arange(84), SH_RGB)
P = lambda a: a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def inactive(K):
    return SH_RGB[3 * K:]


@functools.lru_cache(maxsize=None)
def scene(name):
    """'ragged' / 'dense' of test_outputs_cpu in front of the posed camera, all 16 coefficients non-zero: magnitudes 0.1-0.3,
    random signs.  Every tenth splat is pushed outwards by a fifth in x and y, so that some land beside the screen but inside
    the 1.3 NDC margin: they pass the culls, touch no tile, and GS_BUF_COLOR colours them on demand.  (aos, w, h, cam); never
    modified."""
    aos, w, h = SCENES[name]()
    aos = np.array(aos, np.float32, copy=True)
    aos[::10, 0:2] *= np.float32(1.2)
    aos = in_front_of(aos, w, h, "pose")
    pos, yaw, pitch = POSES["pose"]
    cam = dict(pos=pos, yaw=yaw, pitch=pitch)
    rng = np.random.default_rng(len(name))
    aos[:, SH_RGB] = (rng.uniform(0.1, 0.3, (len(aos), 48)) * rng.choice([-1.0, 1.0], (len(aos), 48))).astype(np.float32)
    aos.setflags(write=False)
    return aos, w, h, cam


def with_inactive(aos, K, value):
    """aos with the rgb of the coefficients K..15 set to value (0.0: Z_K)."""
    out = np.array(aos, np.float32, copy=True)
    out[:, inactive(K)] = np.float32(value)
    return out


def frame(aos, w, h, cam, sh_mode, rows=None, **kw):
    """One context: the RGBA8 frame and GS_BUF_COLOR without outputs (k_project without the depth store), then with both
    outputs.  rows: a tile-row band."""
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
    r = make_renderer(sc, w, h, **kw)
    if rows:
        r.setTileRows(*rows)
    out = {"plain": r.draw(sc).copy(), "plain_color": r.debugRead(gs.BUF_COLOR)}
    r.setOutputs(rgba32f=True, depth=True)
    out["image"] = r.draw(sc).copy()
    assert r.lastStatus == _lib.GS_OK
    out["rgba32f"], out["depth"] = r.readOutput(_lib.GS_OUTPUT_RGBA32F), r.readOutput(_lib.GS_OUTPUT_DEPTH)
    out["color"] = r.debugRead(gs.BUF_COLOR)
    # splats that passed the culls (a colour with their opacity) without an element in the list: coloured on demand
    listed = np.zeros(len(aos), bool)
    listed[r.debugRead(gs.BUF_SORTED_ID)] = True
    out["on_demand"] = np.array(np.count_nonzero((out["color"][:, 3] != 0) & ~listed))
    r.cleanup()
    return out


def assert_frames_equal(got, want, what):
    for key in want:
        assert np.isfinite(want[key]).all(), (what, key)
        assert np.array_equal(got[key], want[key]), (what, key)
    assert np.array_equal(got["plain"], got["image"]), what


# ---- 1. frames ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sort", ALL_SORTS)
@pytest.mark.parametrize("name", ["ragged", "dense"])
def test_frames_equal_all_bands_on_zeroed_records(name, sort):
    aos, w, h, cam = scene(name)
    for render_mode in (gs.GS_RENDER_EXACT, gs.GS_RENDER_FAST):
        for sh_mode, K in K_OF_MODE.items():
            want = frame(with_inactive(aos, K, 0.0), w, h, cam, 0, mode=render_mode, sort=sort)
            got = frame(aos, w, h, cam, sh_mode, mode=render_mode, sort=sort)
            assert_frames_equal(got, want, (name, sort, render_mode, sh_mode))
            # the colours filled in on demand are part of the comparison: some splats pass the culls and touch no tile
            assert want["on_demand"] > 0
            assert want["image"][..., :3].any()


@pytest.mark.parametrize("sh_mode", [DEG1, DEG2], ids=["degree1", "degree2"])
def test_frames_on_a_tile_row_band(sh_mode):
    aos, w, h, cam = scene("ragged")
    K = K_OF_MODE[sh_mode]
    want = frame(with_inactive(aos, K, 0.0), w, h, cam, 0, rows=(3, 8))
    got = frame(aos, w, h, cam, sh_mode, rows=(3, 8))
    assert_frames_equal(got, want, sh_mode)
    assert want["image"][48:128, :, :3].any() and not want["rgba32f"][:48].any()


# ---- 4. gradients (computed once, shared) ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gradients(name, sh_mode, with_depth, fill=None):
    """dense, (ids, rows, count) whole and with max_rows = |V| / 2, and the 35 camera floats of one context that drew scene
    `name` in sh_mode; fill: None = the scene as it is, else (K, value) = the coefficients K..15 set to value."""
    aos, w, h, cam = scene(name)
    if fill is not None:
        aos = with_inactive(aos, *fill)
    sc = make_scene(aos, w, h, sh_mode=sh_mode, **cam)
    r = make_renderer(sc, w, h)
    r.draw(sc)
    wr, wd = weights(h, w, 2)
    d = wd if with_depth else None
    dense = r.backward(wr, d)
    camera = r.backwardCamera()
    v = r.visibleCount()
    whole = r.backwardVisible(wr, d)
    half = r.backwardVisible(wr, d, max_rows=v // 2)
    assert r.lastStatus == _lib.GS_WARN_OVERFLOW and half[2] == v and len(half[0]) == v // 2
    again = (r.backward(wr, d), r.backwardVisible(wr, d), r.backwardCamera())
    r.cleanup()
    # bitwise the same from call to call
    assert np.array_equal(bits(again[0]), bits(dense)) and np.array_equal(bits(again[2]), bits(camera))
    assert np.array_equal(again[1][0], whole[0]) and np.array_equal(bits(again[1][1]), bits(whole[1]))
    for a in (dense, camera) + whole[:2] + half[:2]:
        a.setflags(write=False)
    return dense, whole, half, camera


@pytest.mark.parametrize("with_depth", [True, False], ids=["depth", "nodepth"])
@pytest.mark.parametrize("sh_mode", [DEG1, DEG2], ids=["degree1", "degree2"])
@pytest.mark.parametrize("name", ["ragged", "dense"])
def test_gradients_equal_all_bands_on_zeroed_records(name, sh_mode, with_depth):
    K = K_OF_MODE[sh_mode]
    dense, whole, half, _ = gradients(name, sh_mode, with_depth)
    want, want_whole, want_half, _ = gradients(name, 0, with_depth, (K, 0.0))
    keep = np.concatenate([NON_SH, SH_RGB[:3 * K]])
    off = inactive(K)
    for got, ref, what in ((dense, want, "dense"), (whole[1], want_whole[1], "visible"), (half[1], want_half[1], "half")):
        assert np.isfinite(ref).all(), what
        assert np.array_equal(got[:, keep], ref[:, keep]), what
        assert not bits(got[:, off]).any(), what                           # exactly +0.0f ...
        assert np.count_nonzero(ref[:, off]) > 0, what                     # ... where all 16 bands have gradients
        assert np.count_nonzero(got[:, SH_RGB[3:3 * K]]) > 0 and np.count_nonzero(got[:, 0:3]) > 0, what
    assert np.array_equal(whole[0], want_whole[0]) and whole[2] == want_whole[2] == len(whole[0])
    assert np.array_equal(half[0], want_half[0]) and np.array_equal(half[0], whole[0][:len(half[0])])
    assert np.array_equal(bits(whole[1]), bits(dense[whole[0]])) and np.array_equal(bits(half[1]), bits(whole[1][:len(half[0])]))


# ---- 2. inactive planes are not read ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("value", [float("nan"), 1e30], ids=["nan", "1e30"])
@pytest.mark.parametrize("sh_mode", [DEG1, DEG2], ids=["degree1", "degree2"])
def test_inactive_planes_are_not_read(sh_mode, value):
    K = K_OF_MODE[sh_mode]
    aos, w, h, cam = scene("ragged")
    want = frame(with_inactive(aos, K, 0.0), w, h, cam, sh_mode)
    got = frame(with_inactive(aos, K, value), w, h, cam, sh_mode)
    assert_frames_equal(got, want, (sh_mode, value))
    for with_depth in (True, False):
        clean = gradients("ragged", sh_mode, with_depth, (K, 0.0))
        dirty = gradients("ragged", sh_mode, with_depth, (K, value))
        assert np.array_equal(dirty[0], clean[0]) and np.isfinite(clean[0]).all()
        for a, b in ((dirty[1], clean[1]), (dirty[2], clean[2])):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert np.array_equal(dirty[3], clean[3]) and np.isfinite(clean[3]).all()
        assert not bits(dirty[0][:, inactive(K)]).any() and not bits(dirty[1][1][:, inactive(K)]).any()


# ---- 3. the degrees are four different things ---------------------------------------------------------------------------------------

def test_the_four_degrees_differ_pairwise():
    aos, w, h, cam = scene("ragged")
    frames = {m: frame(aos, w, h, cam, m) for m in (2, DEG1, DEG2, 0)}
    modes = list(frames)
    for i, a in enumerate(modes):
        for b in modes[i + 1:]:
            assert not np.array_equal(frames[a]["image"], frames[b]["image"]), (a, b)
            assert not np.array_equal(frames[a]["rgba32f"], frames[b]["rgba32f"]), (a, b)


@pytest.mark.parametrize("k", [0, 2, 6, 12])
def test_known_answer_one_coefficient_per_band(k):
    """One splat on the camera axis (direction (0, 0, 1) from the camera), only coefficient k set, to c: the zonal term of
    band 0, 1, 2, 3, whose basis does not vanish there.  Its colour is 0.5 + c * basis_k where the mode sums coefficient k and
    0.5 where it does not; the centre pixel (alpha = 0.5 there) holds half of it."""
    torch = pytest.importorskip("torch")
    c = 0.25
    aos, w, h = known_answer_scene((2.0,))
    aos[0, SH_RGB] = 0.0
    aos[0, 12 + 4 * k:15 + 4 * k] = c
    basis = sh_basis(torch.tensor([[0.0, 0.0, 1.0]], dtype=torch.float32))[0].numpy()
    assert basis.dtype == np.float32 and basis[k] != 0
    for sh_mode, K in ((2, 1), (DEG1, 4), (DEG2, 9), (0, 16)):
        sc = make_scene(aos, w, h, sh_mode=sh_mode)
        r = make_renderer(sc, w, h)
        r.setOutputs(rgba32f=True)
        r.draw(sc)
        col = r.debugRead(gs.BUF_COLOR)[0]
        px = r.readOutput(_lib.GS_OUTPUT_RGBA32F)[h // 2, w // 2]
        r.cleanup()
        want = np.float32(0.5) + np.float32(c) * basis[k] if k < K else np.float32(0.5)
        # two float32 roundings (the product, the + 0.5) on either side
        np.testing.assert_allclose(col[:3], want, rtol=3e-7, atol=0, err_msg=str((k, sh_mode)))
        if k >= K:
            assert np.all(col[:3] == np.float32(0.5))
        np.testing.assert_allclose(px[3], 0.5, rtol=1e-6)
        np.testing.assert_allclose(px[:3], 0.5 * want, rtol=2e-6, err_msg=str((k, sh_mode)))


# ---- 5. camera ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sh_mode", [DEG1, DEG2], ids=["degree1", "degree2"])
@pytest.mark.parametrize("name", ["ragged", "dense"])
def test_camera_gradients_equal_all_bands_on_zeroed_records(name, sh_mode):
    got = gradients(name, sh_mode, True)[3]
    want = gradients(name, 0, True, (K_OF_MODE[sh_mode], 0.0))[3]
    assert got.shape == (35,) and np.isfinite(want).all() and np.array_equal(got, want)
    assert np.count_nonzero(got) >= 20


def test_cam_pos_gradient_by_degree():
    assert np.all(gradients("ragged", DEG1, True)[3][32:35] != 0)
    assert not bits(gradients("ragged", 2, True)[3][32:35]).any()
    assert np.count_nonzero(gradients("ragged", 2, True)[3][:32]) >= 17


# ---- 6. torch and the trainer -----------------------------------------------------------------------------------------------------------

def test_torch_render_gradient():
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd import autograd
    aos, w, h, cam = scene("ragged")
    c = make_scene(aos, w, h, **cam).getCamera()
    rr = autograd.make_renderer(w, h)
    rec = torch.tensor(aos, device="cuda").requires_grad_(True)
    rgba, dep = autograd.render(rec, c.getViewMatrix(), c.getProjectionMatrix(), c.getPosition(), sh_mode=DEG1, depth=True, renderer=rr)
    wr, wd = weights(h, w, 2)
    (rgba * torch.tensor(wr, device="cuda")).sum().add((dep * torch.tensor(wd, device="cuda")).sum()).backward()
    rr.cleanup()
    assert np.array_equal(bits(rec.grad.cpu().numpy()), bits(gradients("ragged", DEG1, True)[0]))


def test_visible_adam_follows_the_degree_schedule():
    """A cloud from about 500 points has only its DC term.  Three raw-space steps at degree 0 leave the coefficients 1..15
    untouched in records, raw, m and v; after oneup_sh_degree() three more move 1..3 and leave 4..15 as they were.
    sh_mode=None drew with the mode of sh_degree: the explicit modes of degree 0, 0, 0, 1, 1, 1 from the same start gives the same bits."""
    torch = pytest.importorskip("torch")
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam, make_renderer as torch_renderer, records_from_points
    w, h, n = 96, 64, 500
    src = synth.generate(n, w, h, -3.0, seed=11)
    points = torch.tensor(np.ascontiguousarray(src[:, 0:3] * np.array([-1, -1, 1], np.float32)), device="cuda")
    colors = torch.tensor(np.random.default_rng(5).uniform(0.1, 0.9, (n, 3)).astype(np.float32), device="cuda")
    cam = make_scene(src, w, h).getCamera()
    view, proj, pos = cam.getViewMatrix(), cam.getProjectionMatrix(), cam.getPosition()
    targets = [torch.tensor(np.random.default_rng(s).uniform(0, 1, (h, w, 3)).astype(np.float32), device="cuda") for s in range(6)]
    rest, low, high = SH_RGB[3:], SH_RGB[3:12], SH_RGB[12:]

    def state(opt):
        opt.stream.synchronize()
        return [t.cpu().numpy() for t in (opt.records, opt.raw, opt.m, opt.v)]

    r = torch_renderer(w, h)
    records, _ = records_from_points(points, colors, renderer=r, max_scale=0.05)
    start = records.clone()
    opt = VisibleAdam(records, renderer=r, space="raw")
    assert opt.sh_degree == 3
    opt.sh_degree = 0
    for t in range(3):
        opt.step(view, proj, pos, None, targets[t])
    first = state(opt)
    assert int(opt.count.item()) > 100
    for a in first:
        assert not bits(a[:, rest]).any()
    assert np.count_nonzero(first[2][:, 12:15]) > 100               # the DC term's moments did move
    assert opt.oneup_sh_degree() == 1
    for t in range(3, 6):
        opt.step(view, proj, pos, sh_mode=None, target=targets[t])
    second = state(opt)
    r.cleanup()
    for a in second:
        assert np.count_nonzero(a[:, low]) > 100 and not bits(a[:, high]).any()

    r2 = torch_renderer(w, h)
    records2 = start.clone()
    explicit = VisibleAdam(records2, renderer=r2, space="raw")
    for t, mode in enumerate((2, 2, 2, DEG1, DEG1, DEG1)):
        explicit.step(view, proj, pos, mode, targets[t])
    want = state(explicit)
    r2.cleanup()
    for a, b in zip(second, want):
        assert np.array_equal(bits(a), bits(b))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------

def test_unknown_modes_are_refused():
    aos, w, h, cam = scene("ragged")
    sc = make_scene(aos, w, h, sh_mode=DEG2, **cam)
    r = make_renderer(sc, w, h)
    L, hdl = _lib.lib(), r._ctx.handle
    assert sorted((DEG1, DEG2)) == [4, 5]                           # 3 names no mode: refused as it always was, then 6 and up
    c = sc.getCamera()
    view, proj, pos = (np.ascontiguousarray(a, np.float32) for a in (c.getViewMatrix(), c.getProjectionMatrix(), c.getPosition()))
    before = r.draw(sc).copy()
    elements = r.timings().num_sort_elements
    out = np.full((h, w, 4), 7, np.uint8)
    for bad in (3, 6, 0xFFFFFFFF):
        for call, name in ((lambda: L.gs_render(hdl, P(view), P(proj), P(pos), bad, P(out)), "gs_render"),
                           (lambda: L.gs_render_device_async(hdl, P(view), P(proj), P(pos), bad, None), "gs_render"),
                           (lambda: L.gs_debug_init_sort_list(hdl, P(view), P(proj), P(pos), bad), "gs_debug_init_sort_list")):
            rc = call()
            msg = L.gs_last_error(hdl).decode()
            assert rc == _lib.GS_ERR_INVALID and name in msg and "sh_mode" in msg, (bad, rc, msg)
    r.synchronize()
    assert np.all(out == 7)                                         # nothing was drawn into the caller's image
    assert np.array_equal(r.debugRead(_lib.BUF_IMAGE), before)        # nor into the context's own
    for legal in (DEG1, DEG2):
        assert L.gs_debug_init_sort_list(hdl, P(view), P(proj), P(pos), legal) == _lib.GS_OK
    assert np.array_equal(r.draw(sc), before) and r.timings().num_sort_elements == elements
    r.cleanup()
