"""A cloud from points on the GPU (include/gsplat.h, gs_knn_mean_dist2_device / gs_records_from_points_device), bit for bit
against the NumPy float32 restatements of tests/test_init_cpu.py on its designed clouds; determinism across calls and
sorters, untouched memory, the call conventions, the refusals, and the way from points to a training step."""
import ctypes as C
import os

import numpy as np
import pytest

import vk3dgaussiansplatting_amd as gs
from vk3dgaussiansplatting_amd import _lib
from test_init_cpu import (F, KINDS, LARGE, LARGE_KINDS, SH_C0, SIZES, cloud, knn_mean_dist2_ref, records_from_points_ref,
                           reference)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
GUARD = 5                      # sentinel words / rows behind every output
SENT = F(-12345.5)
SENT_ID = -559038737           # 0xDEADBEEF as the int32 torch fills with
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def up(a):
    return torch.tensor(np.ascontiguousarray(a), device=DEV)


@pytest.fixture(scope="module")
def bare():
    """A context without a scene and without a resolution: all both calls need."""
    r = gs.Renderer(64, 64, record_timings=False)
    r.init(gs.ResourceManager())
    yield r
    r.cleanup()


def run_knn(r, points):
    """gs_knn_mean_dist2_device on a device copy -> dist2 [n]; the guard words behind it and the input keep their value."""
    n = len(points)
    d_p = up(points)
    out = torch.full((n + GUARD,), float(SENT), device=DEV)
    torch.cuda.synchronize()
    r.knnMeanDist2Device(d_p.data_ptr(), n, out.data_ptr())
    r.synchronize()
    got = out.cpu().numpy()
    assert np.all(got[n:] == SENT)
    assert np.array_equal(bits(d_p.cpu().numpy()), bits(points))
    return got[:n]


def run_records(r, points, colors=None, want_order=True, **params):
    """gs_records_from_points_device on device copies -> (records [n, 84], order [n] or None); guards and inputs checked."""
    n = len(points)
    d_p, d_c = up(points), None if colors is None else up(colors)
    rec = torch.full((n + GUARD, 84), float(SENT), device=DEV)
    order = torch.full((n + GUARD,), SENT_ID, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    r.recordsFromPointsDevice(d_p.data_ptr(), None if d_c is None else d_c.data_ptr(), n, gs.default_init_params(**params),
                              rec.data_ptr(), order.data_ptr() if want_order else None)
    r.synchronize()
    got, got_order = rec.cpu().numpy(), order.cpu().numpy()
    assert np.all(got[n:] == SENT) and np.all(got_order[n if want_order else 0:] == SENT_ID)
    assert np.array_equal(bits(d_p.cpu().numpy()), bits(points))
    if colors is not None:
        assert np.array_equal(bits(d_c.cpu().numpy()), bits(colors))
    return got[:n], got_order[:n].view(np.uint32) if want_order else None


def assert_same_rows(got, want, what):
    same = bits(got) == bits(want)
    assert same.all(), (what, np.argwhere(~same)[:5].tolist(), got[~same][:5], want[~same][:5])


# ---- against the restatements -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_knn_against_brute_force(bare, kind):
    for n in SIZES:
        got = run_knn(bare, cloud(kind, n)[0])
        assert_same_rows(got, reference(kind, n)[0], (kind, n))


@pytest.mark.parametrize("kind", LARGE_KINDS)
def test_knn_and_records_at_313_boxes(bare, kind):
    """n = 20 000: 313 boxes, five rounds of the 64-wide box test; one brute force serves both calls."""
    p, c = cloud(kind, LARGE)
    dist2, rec, order = reference(kind, LARGE)
    assert_same_rows(run_knn(bare, p), dist2, kind)
    got, got_order = run_records(bare, p, c)
    assert np.array_equal(got_order, order)
    assert_same_rows(got, rec, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_records_against_restatement(bare, kind):
    """order_out and all 84 floats of every row, with colours, under the defaults."""
    for n in SIZES:
        p, c = cloud(kind, n)
        _, rec, order = reference(kind, n)
        got, got_order = run_records(bare, p, c)
        assert np.array_equal(got_order, order), (kind, n)
        assert_same_rows(got, rec, (kind, n))


@pytest.mark.parametrize("kind,n", [("uniform", 257), ("lattice", 4097), ("identical", 65), ("outliers", 256)])
def test_records_parameters(bare, kind, n):
    """Without colours (SH DC +0), without order_out, a finite max_scale and a min_dist2 that both bite, another opacity."""
    p, c = cloud(kind, n)
    dist2 = reference(kind, n)[0]
    plain, order = records_from_points_ref(p, None, dist2)
    got, got_order = run_records(bare, p, None)
    assert np.array_equal(got_order, order)
    assert_same_rows(got, plain, "no colours")
    assert not bits(got[:, 12:15]).any()
    got, none = run_records(bare, p, c, want_order=False)
    assert none is None
    assert_same_rows(got, reference(kind, n)[1], "no order_out")
    s = np.sqrt(np.maximum(dist2, F(1e-7)))
    lo, hi = float(np.percentile(s, 30)), float(np.percentile(s, 70))
    if not lo < hi:                                            # every scale the same: the floor lifts it, then the cap cuts it
        lo, hi = float(s[0]) * 2, float(s[0]) * 1.5
    params = dict(opacity=0.37, min_dist2=lo * lo, max_scale=hi)
    want, _ = records_from_points_ref(p, c, dist2, **params)
    assert np.sum(want[:, 4] == F(hi)) > 0 and np.sum(dist2 < F(lo * lo)) > 0
    got, got_order = run_records(bare, p, c, **params)
    assert np.array_equal(got_order, order)
    assert_same_rows(got, want, params)
    assert np.all(got[:, 15] == F(0.37))


# ---- determinism, call behaviour ----------------------------------------------------------------------------------------------

def test_same_bits_from_call_to_call_and_for_every_sorter(bare):
    """Two calls give the same bits, and so do a GS_SORT_RADIX4 and a GS_SORT_RADIX8 context (4-bit passes with fed counts and
    with a Count launch per pass, 8-bit passes)."""
    for kind, n in (("seam", 4097), ("duplicates", 4097), ("uniform", 257)):
        p, c = cloud(kind, n)
        dist2, rec, order = reference(kind, n)
        for _ in range(2):
            assert_same_rows(run_knn(bare, p), dist2, kind)
        for sort, count in ((gs.GS_SORT_RADIX4, gs.GS_COUNT_PER_PASS), (gs.GS_SORT_RADIX8, gs.GS_COUNT_AUTO)):
            r = gs.Renderer(64, 64, record_timings=False, sort_algorithm=sort, count_launches=count)
            r.init(gs.ResourceManager())
            try:
                assert_same_rows(run_knn(r, p), dist2, (kind, sort))
                got, got_order = run_records(r, p, c)
                assert np.array_equal(got_order, order)
                assert_same_rows(got, rec, (kind, sort))
            finally:
                r.cleanup()


def test_unsynchronised_behind_other_work_and_scratch_growth(bare):
    """Both calls enqueued on a caller's stream right behind the work that writes their inputs, a small cloud after a large
    one and a larger one after that (the scratch grows), nothing waited for until the end."""
    stream = torch.cuda.Stream(device=DEV)
    bare.setStream(stream.cuda_stream)
    try:
        cases = [("uniform", 4097), ("seam", 257), ("outliers", 4097), ("lattice", 65)]
        host = [(up(cloud(k, n)[0]), up(cloud(k, n)[1])) for k, n in cases]
        torch.cuda.synchronize()
        outs = []
        with torch.cuda.stream(stream):
            busy = torch.ones(2048, 2048, device=DEV)
            for (kind, n), (src_p, src_c) in zip(cases, host):
                busy = busy @ busy * 0.0 + 1.0                                   # work in front, on the same stream
                p, c = torch.zeros_like(src_p), torch.zeros_like(src_c)
                p.copy_(src_p); c.copy_(src_c)                                   # the inputs are written by the stream itself
                d2 = torch.full((n + GUARD,), float(SENT), device=DEV)
                rec = torch.full((n + GUARD, 84), float(SENT), device=DEV)
                order = torch.full((n + GUARD,), SENT_ID, dtype=torch.int32, device=DEV)
                bare.knnMeanDist2Device(p.data_ptr(), n, d2.data_ptr())
                bare.recordsFromPointsDevice(p.data_ptr(), c.data_ptr(), n, gs.default_init_params(), rec.data_ptr(), order.data_ptr())
                outs.append((p, c, d2, rec, order))
        stream.synchronize()
        for (kind, n), (p, c, d2, rec, order) in zip(cases, outs):
            want_d2, want_rec, want_order = reference(kind, n)
            assert_same_rows(d2.cpu().numpy()[:n], want_d2, kind)
            assert_same_rows(rec.cpu().numpy()[:n], want_rec, kind)
            assert np.array_equal(order.cpu().numpy()[:n].view(np.uint32), want_order)
            assert np.all(d2.cpu().numpy()[n:] == SENT) and np.all(rec.cpu().numpy()[n:] == SENT)
    finally:
        bare.setStream(None)


def test_calls_beside_a_scene(bare):
    """A context that holds a scene and a resolution serves the calls too, and its next frame is what it was."""
    aos = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    rm = gs.ResourceManager(); rm.setGaussians(np.ascontiguousarray(aos["aos"], F))
    w, h = int(aos["width"]), int(aos["height"])
    r = gs.Renderer(w, h, record_timings=False, warmup_frames=0)
    r.init(rm); r.initForScene(gs.Scene(rm, aspect_ratio=w / h))
    try:
        cam = (aos["view"], aos["proj"], aos["cam_pos"], 0)
        r.drawCamera(*cam)
        before = r.debugRead(_lib.BUF_IMAGE).copy()
        assert_same_rows(run_knn(r, cloud("seam", 257)[0]), reference("seam", 257)[0], "beside a scene")
        r.drawCamera(*cam)
        assert np.array_equal(r.debugRead(_lib.BUF_IMAGE), before)
    finally:
        r.cleanup()


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(bare):
    """Every refusal of the header: GS_ERR_INVALID, its message, nothing written; valid calls afterwards work."""
    n = 40
    L, hdl = _lib.lib(), bare._ctx.handle
    p, c = cloud("uniform", 65)
    p, c = p[:n], c[:n]
    d = dict(p=up(p), c=up(c), d2=torch.full((n,), float(SENT), device=DEV), rec=torch.full((n, 84), float(SENT), device=DEV),
             o=torch.full((n,), SENT_ID, dtype=torch.int32, device=DEV))
    torch.cuda.synchronize()
    vp = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.data_ptr())

    def knn(n_=n, **swap):
        a = dict(d, **swap)
        return L.gs_knn_mean_dist2_device(hdl, vp(a["p"]), n_, vp(a["d2"]))

    def records(params=None, n_=n, null_params=False, **swap):
        a = dict(d, **swap)
        params = gs.default_init_params() if params is None else params
        return L.gs_records_from_points_device(hdl, vp(a["p"]), vp(a["c"]), n_, None if null_params else C.byref(params), vp(a["rec"]),
                                               vp(a["o"]))

    def refused(rc, word):
        msg = L.gs_last_error(hdl).decode()
        assert rc == _lib.GS_ERR_INVALID and word in msg, (rc, word, msg)

    refused(knn(p=None), "gs_knn_mean_dist2_device: null")
    refused(knn(d2=None), "gs_knn_mean_dist2_device: null")
    refused(records(p=None), "gs_records_from_points_device: null")
    refused(records(rec=None), "gs_records_from_points_device: null")
    for few in (0, 1, 3):
        refused(knn(n_=few), "fewer than four points have no three neighbours")
        refused(records(n_=few), "fewer than four points have no three neighbours")
    for many in (1 << 31, (1 << 32) - 1):
        refused(knn(n_=many), "below 2^31")
        refused(records(n_=many), "below 2^31")
    refused(records(null_params=True), "null gs_init_params")
    for size in (0, 12, 20):
        q = gs.default_init_params()
        q.struct_size = size
        refused(records(q), "struct_size")
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        refused(records(gs.default_init_params(opacity=bad)), "opacity")
    for bad in (-1e-9, float("inf"), float("nan")):
        refused(records(gs.default_init_params(min_dist2=bad)), "min_dist2")
    for bad in (0.0, -1.0, float("nan")):
        refused(records(gs.default_init_params(max_scale=bad)), "max_scale")
    refused(knn(d2=d["p"]), "aliases")
    refused(knn(d2=d["p"].data_ptr() + 12 * n - 4), "aliases")                             # the last input float only
    refused(knn(d2=d["p"].data_ptr() - 4 * n + 4), "aliases")                              # the first input float only
    refused(records(rec=d["p"]), "aliases an input")
    refused(records(rec=d["c"].data_ptr() - 336 * n + 4), "aliases an input")
    refused(records(o=d["p"]), "aliases an input")
    refused(records(o=d["c"].data_ptr() + 12 * n - 4), "aliases an input")
    refused(records(o=d["rec"]), "alias each other")
    refused(records(o=d["rec"].data_ptr() + 336 * n - 4), "alias each other")
    bare.synchronize()
    assert np.all(d["d2"].cpu().numpy() == SENT) and np.all(d["rec"].cpu().numpy() == SENT) and np.all(d["o"].cpu().numpy() == SENT_ID)
    # adjacent is not aliased; the boundary values of the parameters are parameters, not errors
    both = torch.full((n * 3 + n,), float(SENT), device=DEV)
    both[:n * 3] = d["p"].reshape(-1)
    torch.cuda.synchronize()
    assert knn(p=both.data_ptr(), d2=both.data_ptr() + 12 * n) == _lib.GS_OK
    assert records(gs.default_init_params(min_dist2=0.0, max_scale=float("inf"), opacity=1e-6)) == _lib.GS_OK
    assert records(c=None, o=None) == _lib.GS_OK
    assert knn() == _lib.GS_OK
    bare.synchronize()
    want = knn_mean_dist2_ref(p)
    assert_same_rows(d["d2"].cpu().numpy(), want, "after the refusals")
    assert_same_rows(both.cpu().numpy()[3 * n:], want, "adjacent arrays")
    assert_same_rows(d["rec"].cpu().numpy(), records_from_points_ref(p, None, want)[0], "after the refusals")
    assert np.array_equal(d["o"].cpu().numpy().view(np.uint32), records_from_points_ref(p, None, want)[1])   # of the first valid call


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def test_points_to_a_training_step():
    """The positions and DC colours of the small golden scene as an SfM cloud: records_from_points, the two raw conversion
    calls, an upload, a resolution and a frame -- GS_OK, splats visible, every record finite -- then one raw-space
    VisibleAdam step."""
    from vk3dgaussiansplatting_amd.autograd import VisibleAdam, make_renderer, records_from_points
    g = np.load(os.path.join(ROOT, "tests", "golden", "small_scene.npz"))
    aos = np.ascontiguousarray(g["aos"], F)
    n, w, h = len(aos), int(g["width"]), int(g["height"])
    points = np.ascontiguousarray(aos[:, 0:3] * np.array([-1, -1, 1], F))                   # back into the .ply's frame
    colors = np.ascontiguousarray(aos[:, 12:15] * SH_C0 + F(0.5))
    r = make_renderer(w, h)
    try:
        records, order = records_from_points(up(points), up(colors), renderer=r, max_scale=0.05)
        assert records.shape == (n, 84) and order.shape == (n,) and order.dtype == torch.int64
        want, want_order = records_from_points_ref(points, colors, max_scale=0.05)
        assert np.array_equal(order.cpu().numpy(), want_order)
        assert_same_rows(records.cpu().numpy(), want, "autograd.records_from_points")
        assert np.array_equal(records.cpu().numpy()[:, 0:3], aos[order.cpu().numpy(), 0:3])
        raw = torch.zeros_like(records)
        r.rawFromRecordsDevice(records.data_ptr(), raw.data_ptr(), n)
        r.recordsFromRawDevice(raw.data_ptr(), records.data_ptr(), n)
        r.uploadDevice(records.data_ptr(), n)                    # a new scene: sets the resolution again
        r.drawCamera(g["view"], g["proj"], g["cam_pos"], 0)
        assert r.lastStatus == _lib.GS_OK
        assert r.visibleCount() > 0
        rec = records.cpu().numpy()
        assert np.isfinite(rec).all() and np.all(rec[:, 4:7] > 0) and np.all(np.abs(rec[:, 15] - 0.1) < 1e-6)
        assert np.all(np.abs(rec[:, 4:7] - want[:, 4:7]) <= 2e-6 * want[:, 4:7])            # one log and one exp
        target = torch.rand(h, w, 3, device=DEV)
        opt = VisibleAdam(records, renderer=r, space="raw")
        numbers = opt.step(g["view"], g["proj"], g["cam_pos"], 0, target)
        opt.stream.synchronize()
        assert np.isfinite(numbers.cpu().numpy()).all() and int(opt.count.item()) > 0
        assert np.isfinite(opt.records.cpu().numpy()).all() and np.isfinite(opt.raw.cpu().numpy()).all()
        r.setStream(None)
    finally:
        r.cleanup()
